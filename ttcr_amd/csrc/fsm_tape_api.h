// ttcr_amd/csrc/fsm_tape_api.h -- the device-resident M tape (ttcr_fsm_raytrace_multi_tape, include/ttcr_amd.h): what the host side
// (fsm_capi.hip) sees of the kernels that turn the records of the compute_M walk (fsm_raypath3d_m<T, false>) into the rows of M on the
// device, index them by node and form M^T w.  The kernels live in a translation unit of their own (fsm_tape.hip, hipCUB sorts).
//
// Pipeline, per walk chunk (walk_m):  expand (each record -> its 8 contributions, keyed (row, node), in push order)
//                                     -> stable radix sort by key -> segmented sum from the FIRST contribution (mv[e] += v) -> drop
//                                     nodes >= n_nodes -> append (row, node, value) to the rows of the source.
// Once per tape:                      CSR row offsets; stable sort by node (rows stay ascending) -> per-node offsets.
// VJP:                                one thread per node, grad[n] = sum over its entries in ascending row order of fl(v * w[row]),
//                                     a serial chain from +0 (no atomics: the bits do not depend on arrival order).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace ttcr_amd {

// The eight terms of one walk record (mid[3], ds, s) as GridT::assemble_m forms them (Grid3Drn::getRaypath with m_data,
// ttcr/Grid3Drn.h:1503-1800): cell from (mid - min) / dx, weights WITHOUT the minimum (the reference's own formula), the weight
// product in double (1. is a double), cast to T, value -s^2 * ds * weight in T.  j[] may lie one node past the grid.  The one
// restatement of that arithmetic: host assembly and the expand kernel both call it.
template <typename T>
__host__ __device__ inline void m_record_terms(const T* sg, T xmin, T ymin, T zmin, T dx, size_t nnx, size_t nny, long long* j, T* v) {
    const T ds = sg[3];
    T sq = sg[4];
    sq *= sq;
    const size_t ix = (size_t)((sg[0] - xmin) / dx), iy = (size_t)((sg[1] - ymin) / dx), iz = (size_t)((sg[2] - zmin) / dx);
    int c = 0;
    for (size_t ii = 0; ii < 2; ++ii)
        for (size_t jj = 0; jj < 2; ++jj)
            for (size_t kk = 0; kk < 2; ++kk, ++c) {
                const size_t iv = ix + ii, jv = iy + jj, kv = iz + kk;
                const T dvdv = (T)((1. - std::abs(sg[0] - iv * dx) / dx) * (1. - std::abs(sg[1] - jv * dx) / dx) *
                                   (1. - std::abs(sg[2] - kv * dx) / dx));
                j[c] = (long long)((kv * nny + jv) * nnx + iv);
                v[c] = -sq * ds * dvdv;
            }
}

template <typename T>
struct MGeom {
    T xmin, ymin, zmin, dx;
    size_t nnx, nny;
    size_t nn;   // node count: entries with j >= nn are dropped
};

// A growable list of (row, node, value) entries on the current device; grow() keeps the contents.
struct TapeRows {
    int* row = nullptr;
    int* col = nullptr;
    void* val = nullptr;
    size_t n = 0, cap = 0, elem = 0;
    void grow(size_t need, hipStream_t stream);
    void release();
    TapeRows() = default;
    TapeRows(const TapeRows&) = delete;
    TapeRows& operator=(const TapeRows&) = delete;
    TapeRows(TapeRows&& o) noexcept { *this = std::move(o); }
    TapeRows& operator=(TapeRows&& o) noexcept {
        if (this != &o) {
            release();
            row = o.row; col = o.col; val = o.val; n = o.n; cap = o.cap; elem = o.elem;
            o.row = o.col = nullptr; o.val = nullptr; o.n = o.cap = 0;
        }
        return *this;
    }
    ~TapeRows() { release(); }
};

// Scratch of the chunk stages (contributions, sort buffers, scan), sized from the chunk being merged; reused between chunks.
class TapeChunk {
   public:
    // m rows whose records are roff[q] .. roff[q+1] (host array of m + 1 offsets, roff[0] = 0)
    void begin(const long long* h_roff, int m, size_t elem, hipStream_t stream);
    // contributions of rows q0 .. q0+mm-1: records of row q at recs + (q - q0) * row_stride * 5; rows whose status is not 0 skipped
    template <typename T>
    void expand(const T* recs, long row_stride, const int* d_status, int q0, int mm, const MGeom<T>& g, hipStream_t stream);
    // sort, merge, drop, append (row_base + q, node, value) to out
    template <typename T>
    void merge(int row_base, const MGeom<T>& g, TapeRows& out, hipStream_t stream);
    void release();
    ~TapeChunk() { release(); }

   private:
    int m_ = 0;
    size_t n_ = 0;   // contributions of the chunk
    std::vector<long long> h_roff_;
    long long* d_roff_ = nullptr;
    size_t roff_cap_ = 0;
    unsigned long long *key_ = nullptr, *key2_ = nullptr;
    void *v_ = nullptr, *v2_ = nullptr;
    int *keep_ = nullptr, *pos_ = nullptr;
    size_t cap_ = 0, vcap_ = 0;
    void* tmp_ = nullptr;
    size_t tmp_cap_ = 0;
    void reserve_tmp(size_t bytes);
};

// The finished tape on one device.
struct MTapeDev {
    int device = 0;
    size_t elem = 0, n_rows = 0, nn = 0, nnz = 0;
    long long* row_off = nullptr;    // n_rows + 1
    int* col = nullptr;              // nnz, row-major
    void* val = nullptr;             // nnz
    long long* node_off = nullptr;   // nn + 1
    int* trow = nullptr;             // nnz, node-major, rows ascending within a node
    void* tval = nullptr;            // nnz
    void* w_tmp = nullptr;           // n_rows (host w staged here)
    void* g_tmp = nullptr;           // nn (host grad staged here)
    hipStream_t stream = nullptr;
    size_t bytes() const;
    void release();
};

// rows (consumed: freed on return) -> t (device, n_rows, nn, elem set by the caller; the stream too)
template <typename T>
void tape_finish(MTapeDev& t, TapeRows& rows);
template <typename T>
void tape_vjp(const MTapeDev& t, const T* d_w, T* d_grad);
// row[i] += shift for i < n (the parts of a multi-device tape)
void tape_shift_rows(int* row, size_t n, int shift, hipStream_t stream);

}  // namespace ttcr_amd
