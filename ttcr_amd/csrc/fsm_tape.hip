// ttcr_amd/csrc/fsm_tape.hip -- translation unit of the M tape kernels (expand, merge, node index, M^T w); see fsm_tape_api.h.
#include "fsm_tape_api.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <limits>
#include <sstream>
#include <stdexcept>

#define TAPE_CHECK(expr)                                                                                          \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) {                                                                                   \
            std::ostringstream _m;                                                                                \
            _m << "HIP error " << hipGetErrorString(_e) << " at " << __FILE__ << ":" << __LINE__ << " (" #expr ")"; \
            throw std::runtime_error(_m.str());                                                                   \
        }                                                                                                         \
    } while (0)

namespace ttcr_amd {

namespace {

template <typename P>
void dev_alloc(P*& p, size_t count, size_t elem = sizeof(P)) {
    TAPE_CHECK(hipMalloc((void**)&p, std::max<size_t>(count, 1) * elem));
}
template <typename P>
void dev_free(P*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}
unsigned blocks_for(size_t n, unsigned b = 256) { return (unsigned)std::max<size_t>(1, (n + b - 1) / b); }
int bits_for(unsigned long long n) {   // bits of the largest key below n
    int b = 0;
    while (b < 64 && (n - 1) >> b) ++b;
    return std::max(b, 1);
}

// contributions of the records roff[q0] .. roff[q0+mm]: 8 per record, at 8 * record + term, key (row, node), node clamped to nn
template <typename T>
__global__ void tape_expand_kernel(const T* __restrict__ recs, long row_stride, const long long* __restrict__ roff,
                                   const int* __restrict__ status, int q0, int mm, MGeom<T> g, unsigned long long* __restrict__ key,
                                   T* __restrict__ val) {
    const long long i = roff[q0] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= roff[q0 + mm]) return;
    int lo = q0, hi = q0 + mm - 1;   // the last row q with roff[q] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (roff[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int q = lo;
    if (status[q] != 0) return;   // (a long walk: expanded from its own records once it has been walked again)
    const T* sg = recs + ((size_t)(q - q0) * row_stride + (size_t)(i - roff[q])) * 5;
    long long j[8];
    T v[8];
    m_record_terms<T>(sg, g.xmin, g.ymin, g.zmin, g.dx, g.nnx, g.nny, j, v);
    const unsigned long long base = (unsigned long long)q * (g.nn + 1);
    for (int c = 0; c < 8; ++c) {
        const unsigned long long jc = (unsigned long long)j[c] < g.nn ? (unsigned long long)j[c] : g.nn;
        key[8 * i + c] = base + jc;
        val[8 * i + c] = v[c];
    }
}

// first contribution of every (row, node) run whose node lies in the grid
__global__ void tape_keep_kernel(const unsigned long long* __restrict__ key, int n, unsigned long long nn1, int* __restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool head = i == 0 || key[i] != key[i - 1];
    keep[i] = head && key[i] % nn1 != nn1 - 1 ? 1 : 0;
}

// mv[e] += v in push order: the run's sum starts from its first contribution (not from +0: signed zeros are entries)
template <typename T>
__global__ void tape_write_kernel(const unsigned long long* __restrict__ key, const T* __restrict__ val, const int* __restrict__ keep,
                                  const int* __restrict__ pos, int n, unsigned long long nn1, int row_base, int* __restrict__ orow,
                                  int* __restrict__ ocol, T* __restrict__ oval) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const unsigned long long k = key[i];
    T s = val[i];
    for (int e = i + 1; e < n && key[e] == k; ++e) s += val[e];
    const int o = pos[i];
    orow[o] = row_base + (int)(k / nn1);
    ocol[o] = (int)(k % nn1);
    oval[o] = s;
}

// off[b] = first position whose key is >= b, for b = 0 .. n_bins (keys ascending, below n_bins)
__global__ void tape_offsets_kernel(const int* __restrict__ key, long long n, long long n_bins, long long* __restrict__ off) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const long long prev = i == 0 ? -1 : key[i - 1], cur = i == n ? n_bins : key[i];
    for (long long b = prev + 1; b <= cur; ++b) off[b] = i;
}

__global__ void tape_iota_kernel(int* __restrict__ a, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (int)i;
}

template <typename T>
__global__ void tape_gather_kernel(const int* __restrict__ perm, const int* __restrict__ row, const T* __restrict__ val, long long n,
                                   int* __restrict__ trow, T* __restrict__ tval) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int i = perm[k];
    trow[k] = row[i];
    tval[k] = val[i];
}

__global__ void tape_shift_kernel(int* __restrict__ row, long long n, int shift) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) row[i] += shift;
}

// grad[n] = sum over the node's entries, rows ascending, of fl(v * w[row]); one serial chain per node from +0, multiply and add
// rounded apart (the build has -ffp-contract=off)
template <typename T>
__global__ void tape_vjp_kernel(const long long* __restrict__ node_off, const int* __restrict__ trow, const T* __restrict__ tval,
                                const T* __restrict__ w, long long nn, T* __restrict__ grad) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nn) return;
    T acc = (T)0;
    for (long long k = node_off[n], e = node_off[n + 1]; k < e; ++k) {
        const T p = tval[k] * w[trow[k]];
        acc += p;
    }
    grad[n] = acc;
}

}  // namespace

void TapeRows::grow(size_t need, hipStream_t stream) {
    if (need <= cap) return;
    const size_t nc = std::max(need, 2 * cap);
    int *r = nullptr, *c = nullptr;
    char* v = nullptr;
    dev_alloc(r, nc);
    dev_alloc(c, nc);
    dev_alloc(v, nc, elem);
    if (n > 0) {
        TAPE_CHECK(hipMemcpyAsync(r, row, n * sizeof(int), hipMemcpyDeviceToDevice, stream));
        TAPE_CHECK(hipMemcpyAsync(c, col, n * sizeof(int), hipMemcpyDeviceToDevice, stream));
        TAPE_CHECK(hipMemcpyAsync(v, val, n * elem, hipMemcpyDeviceToDevice, stream));
        TAPE_CHECK(hipStreamSynchronize(stream));
    }
    const size_t keep_n = n, keep_elem = elem;
    release();
    row = r; col = c; val = v; cap = nc; n = keep_n; elem = keep_elem;
}

void TapeRows::release() {
    dev_free(row);
    dev_free(col);
    dev_free(val);
    n = cap = 0;
}

void TapeChunk::reserve_tmp(size_t bytes) {
    if (bytes <= tmp_cap_) return;
    dev_free(tmp_);
    dev_alloc(tmp_, bytes, 1);
    tmp_cap_ = bytes;
}

void TapeChunk::begin(const long long* h_roff, int m, size_t elem, hipStream_t stream) {
    m_ = m;
    h_roff_.assign(h_roff, h_roff + m + 1);
    const long long recs = h_roff[m];
    if (recs > (long long)(std::numeric_limits<int>::max() / 8)) throw std::runtime_error("M tape: too many walk records in one chunk");
    n_ = (size_t)recs * 8;
    if ((size_t)m + 1 > roff_cap_) {
        dev_free(d_roff_);
        dev_alloc(d_roff_, (size_t)m + 1);
        roff_cap_ = (size_t)m + 1;
    }
    TAPE_CHECK(hipMemcpyAsync(d_roff_, h_roff_.data(), sizeof(long long) * ((size_t)m + 1), hipMemcpyHostToDevice, stream));
    if (n_ > cap_ || elem > vcap_) {
        dev_free(key_); dev_free(key2_); dev_free(v_); dev_free(v2_); dev_free(keep_); dev_free(pos_);
        const size_t c = std::max(n_, cap_);
        dev_alloc(key_, c); dev_alloc(key2_, c); dev_alloc(v_, c, elem); dev_alloc(v2_, c, elem); dev_alloc(keep_, c); dev_alloc(pos_, c);
        cap_ = c;
        vcap_ = elem;
    }
}

template <typename T>
void TapeChunk::expand(const T* recs, long row_stride, const int* d_status, int q0, int mm, const MGeom<T>& g, hipStream_t stream) {
    if (mm <= 0) return;
    const long long n_recs = h_roff_[q0 + mm] - h_roff_[q0];
    if (n_recs <= 0) return;
    tape_expand_kernel<T><<<blocks_for((size_t)n_recs), 256, 0, stream>>>(recs, row_stride, d_roff_, d_status, q0, mm, g, key_, (T*)v_);
    TAPE_CHECK(hipGetLastError());
}

template <typename T>
void TapeChunk::merge(int row_base, const MGeom<T>& g, TapeRows& out, hipStream_t stream) {
    if (n_ == 0) return;
    const int n = (int)n_;
    const unsigned long long nn1 = (unsigned long long)g.nn + 1;
    const int end_bit = bits_for((unsigned long long)m_ * nn1);
    size_t sort_bytes = 0, scan_bytes = 0;
    TAPE_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, key_, key2_, (T*)v_, (T*)v2_, n, 0, end_bit, stream));
    TAPE_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, keep_, pos_, n, stream));
    reserve_tmp(std::max(sort_bytes, scan_bytes));
    // (radix sorts are stable: the contributions of one (row, node) keep their push order)
    TAPE_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp_, sort_bytes, key_, key2_, (T*)v_, (T*)v2_, n, 0, end_bit, stream));
    tape_keep_kernel<<<blocks_for(n_), 256, 0, stream>>>(key2_, n, nn1, keep_);
    TAPE_CHECK(hipGetLastError());
    TAPE_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp_, scan_bytes, keep_, pos_, n, stream));
    int tail[2] = {0, 0};
    TAPE_CHECK(hipMemcpyAsync(&tail[0], pos_ + (n - 1), sizeof(int), hipMemcpyDeviceToHost, stream));
    TAPE_CHECK(hipMemcpyAsync(&tail[1], keep_ + (n - 1), sizeof(int), hipMemcpyDeviceToHost, stream));
    TAPE_CHECK(hipStreamSynchronize(stream));
    const size_t count = (size_t)tail[0] + (size_t)tail[1];
    if (out.n + count > (size_t)std::numeric_limits<int>::max()) throw std::runtime_error("M tape: more than 2^31 - 1 entries");
    out.elem = sizeof(T);
    out.grow(out.n + count, stream);
    tape_write_kernel<T><<<blocks_for(n_), 256, 0, stream>>>(key2_, (const T*)v2_, keep_, pos_, n, nn1, row_base, out.row + out.n,
                                                             out.col + out.n, (T*)out.val + out.n);
    TAPE_CHECK(hipGetLastError());
    TAPE_CHECK(hipStreamSynchronize(stream));
    out.n += count;
}

void TapeChunk::release() {
    dev_free(d_roff_); dev_free(key_); dev_free(key2_); dev_free(v_); dev_free(v2_); dev_free(keep_); dev_free(pos_); dev_free(tmp_);
    roff_cap_ = cap_ = vcap_ = tmp_cap_ = 0;
}

size_t MTapeDev::bytes() const {
    return (n_rows + 1 + nn + 1) * sizeof(long long) + 2 * nnz * (sizeof(int) + elem) + (n_rows + nn) * elem;
}

void MTapeDev::release() {
    if (row_off || col || val || node_off || trow || tval || w_tmp || g_tmp || stream) (void)hipSetDevice(device);
    dev_free(row_off); dev_free(col); dev_free(val); dev_free(node_off); dev_free(trow); dev_free(tval); dev_free(w_tmp); dev_free(g_tmp);
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

template <typename T>
void tape_finish(MTapeDev& t, TapeRows& rows) {
    const hipStream_t s = t.stream;
    const size_t nnz = rows.n;
    t.nnz = nnz;
    dev_alloc(t.row_off, t.n_rows + 1);
    dev_alloc(t.node_off, t.nn + 1);
    dev_alloc(t.trow, nnz);
    dev_alloc(t.tval, nnz, sizeof(T));
    dev_alloc(t.w_tmp, t.n_rows, sizeof(T));
    dev_alloc(t.g_tmp, t.nn, sizeof(T));
    if (nnz > 0) {
        dev_alloc(t.col, nnz);
        dev_alloc(t.val, nnz, sizeof(T));
        TAPE_CHECK(hipMemcpyAsync(t.col, rows.col, nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
        TAPE_CHECK(hipMemcpyAsync(t.val, rows.val, nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
    } else {
        dev_alloc(t.col, 1);
        dev_alloc(t.val, 1, sizeof(T));
    }
    tape_offsets_kernel<<<blocks_for(nnz + 1), 256, 0, s>>>(rows.row, (long long)nnz, (long long)t.n_rows, t.row_off);
    TAPE_CHECK(hipGetLastError());
    // node index: entries sorted by node, stably (ascending rows within a node)
    int *perm0 = nullptr, *perm = nullptr, *keys = nullptr;
    void* tmp = nullptr;
    dev_alloc(perm0, nnz); dev_alloc(perm, nnz); dev_alloc(keys, nnz);
    try {
        if (nnz > 0) {
            const int n = (int)nnz;
            tape_iota_kernel<<<blocks_for(nnz), 256, 0, s>>>(perm0, (long long)nnz);
            TAPE_CHECK(hipGetLastError());
            const int end_bit = bits_for((unsigned long long)t.nn);
            size_t bytes = 0;
            const unsigned* kin = (const unsigned*)rows.col;
            TAPE_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, (unsigned*)keys, perm0, perm, n, 0, end_bit, s));
            dev_alloc(tmp, bytes, 1);
            TAPE_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, (unsigned*)keys, perm0, perm, n, 0, end_bit, s));
            tape_gather_kernel<T><<<blocks_for(nnz), 256, 0, s>>>(perm, rows.row, (const T*)rows.val, (long long)nnz, t.trow, (T*)t.tval);
            TAPE_CHECK(hipGetLastError());
        }
        tape_offsets_kernel<<<blocks_for(nnz + 1), 256, 0, s>>>(keys, (long long)nnz, (long long)t.nn, t.node_off);
        TAPE_CHECK(hipGetLastError());
        TAPE_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        dev_free(perm0); dev_free(perm); dev_free(keys); dev_free(tmp);
        throw;
    }
    dev_free(perm0); dev_free(perm); dev_free(keys); dev_free(tmp);
    rows.release();
}

template <typename T>
void tape_vjp(const MTapeDev& t, const T* d_w, T* d_grad) {
    tape_vjp_kernel<T><<<blocks_for(t.nn), 256, 0, t.stream>>>(t.node_off, t.trow, (const T*)t.tval, d_w, (long long)t.nn, d_grad);
    TAPE_CHECK(hipGetLastError());
}

void tape_shift_rows(int* row, size_t n, int shift, hipStream_t stream) {
    if (n == 0 || shift == 0) return;
    tape_shift_kernel<<<blocks_for(n), 256, 0, stream>>>(row, (long long)n, shift);
    TAPE_CHECK(hipGetLastError());
}

#define TAPE_INST(T)                                                                                                              \
    template void TapeChunk::expand<T>(const T*, long, const int*, int, int, const MGeom<T>&, hipStream_t);                       \
    template void TapeChunk::merge<T>(int, const MGeom<T>&, TapeRows&, hipStream_t);                                              \
    template void tape_finish<T>(MTapeDev&, TapeRows&);                                                                           \
    template void tape_vjp<T>(const MTapeDev&, const T*, T*);
TAPE_INST(float)
TAPE_INST(double)

}  // namespace ttcr_amd
