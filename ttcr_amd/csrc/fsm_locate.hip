// ttcr_amd/csrc/fsm_locate.hip -- translation unit of the field tape's grid-search hypocentre location (fsm_adjoint_api.h;
// tests/locate_reference.py restates the definition in numpy).  The fields of the tape are read, nothing is solved or relaxed.  Compiled
// with -ffp-contract=off like every other unit: each difference, product, quotient and sum below is rounded on its own, in float64
// whatever the tape's dtype (an fp32 field value converts exactly), in the order the definition writes them.
//
// For hypocentre q with picks k (field f_k, time t_k, weight w_k, ascending pick index) and node m:
//     sw = sum_k w_k (formed on the host, from +0)          r_k = fl(t_k - double(T[f_k][m]))        a = sum_k fl(w_k * r_k)
//     t0 = fl(a / sw)        d_k = fl(r_k - t0)             phi = sum_k fl(w_k * fl(d_k * d_k))      (sums from +0, ascending k)
// The result of q is the minimum of (phi, m) in lexicographic order over the nodes of the box, a NaN phi left out: associative and
// commutative, so no launch shape, tile order or chunking shows in the bits.  No atomics: partial minima, then one small kernel.
#include "fsm_adjoint_api.h"

#include <algorithm>
#include <sstream>
#include <string>

#define LOC_CHECK(expr)                                                                                           \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) {                                                                                   \
            std::ostringstream _m;                                                                                \
            _m << "HIP error " << hipGetErrorString(_e) << " at " << __FILE__ << ":" << __LINE__ << " (" #expr ")"; \
            throw AdjDeviceError(_m.str());                                                                       \
        }                                                                                                         \
    } while (0)

namespace ttcr_amd {

namespace {

constexpr int LOC_THREADS = 256;
constexpr int LOC_WAVE = 64;
constexpr int LOC_WAVES = LOC_THREADS / LOC_WAVE;
constexpr int LOC_CHUNK = 64;             // hypocentres per workgroup
constexpr size_t LOC_LDS = 48 * 1024;     // bytes of LDS for the staged field values of a node tile: three workgroups per CU
constexpr int LOC_MAX_GX = 1024;          // workgroups along the node tiles (each walks the tiles gx apart): rows of the partials
constexpr int LOC_MAX_SUB = 4;            // nodes per lane and tile

// nodes per lane (the node tile is LOC_THREADS times that) so that the values of n_fields fields at the tile's nodes fit LOC_LDS;
// 0: not even one node per lane fits, the kernel reads the fields from global memory
int loc_sub(size_t elem, size_t n_fields) {
    for (int sub = LOC_MAX_SUB; sub >= 1; sub /= 2)
        if (n_fields * elem * LOC_THREADS * sub <= LOC_LDS) return sub;
    return 0;
}

struct LocBox {
    int i0, j0, k0, ni, nj, nk;   // first node and node counts of the box
    int nnx, nny;
    long long nb;                 // nodes of the box
    size_t nn;                    // nodes of the grid
};

// is the candidate (p, n) before the best so far (bp, bn) in the order (phi, node)?  n < 0: no candidate; a NaN phi never wins
__device__ __forceinline__ bool loc_before(double p, long long n, double bp, long long bn) {
    return n >= 0 && p == p && (bn < 0 || p < bp || (p == bp && n < bn));
}

// One workgroup per (gx-strided set of node tiles, chunk of LOC_CHUNK hypocentres), lanes over the nodes of the box (x fastest), SUB nodes
// per lane and tile.  STAGED: the lane's values of every field sit in LDS as lds[field][node of the tile] -- stride 1 in the lane, no
// bank conflicts, and each lane reads back only what it wrote itself, so no barrier is needed around the staging.  The data of a pick
// (field, time, weight, offsets, sw) is the same for every lane: uniform addresses off kernel arguments, read through scalar loads.
// Per (tile, hypocentre) the lanes' minima are reduced inside the wavefront and merged into the wavefront's own slot in LDS; the slots
// become one partial (phi, node) per (workgroup, hypocentre) at the end.  vol (may be null): phi of every box node, n_hypo x nb.
template <typename T, int SUB, bool STAGED>
__global__ __launch_bounds__(LOC_THREADS) void loc_search_kernel(const T* __restrict__ fields, int n_fields, LocBox g, int n_hypo,
                                                                  const int* __restrict__ hyp_off, const double* __restrict__ hyp_sw,
                                                                  const int* __restrict__ pk_field, const double* __restrict__ pk_time,
                                                                  const double* __restrict__ pk_w, long long n_tiles,
                                                                  double* __restrict__ part_phi, long long* __restrict__ part_node,
                                                                  double* __restrict__ vol) {
    extern __shared__ unsigned char loc_smem[];
    T* lds = reinterpret_cast<T*>(loc_smem);
    __shared__ double best_phi[LOC_CHUNK * LOC_WAVES];
    __shared__ long long best_node[LOC_CHUNK * LOC_WAVES];
    constexpr int TILE = LOC_THREADS * SUB;
    const int lane = threadIdx.x;
    const int wave = lane / LOC_WAVE;
    const int q0 = blockIdx.y * LOC_CHUNK;
    const int nq = min(LOC_CHUNK, n_hypo - q0);
    for (int i = lane; i < LOC_CHUNK * LOC_WAVES; i += LOC_THREADS) {
        best_phi[i] = 0.0;
        best_node[i] = -1;
    }
    __syncthreads();
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long long b[SUB], m[SUB];
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            b[s] = tile * TILE + s * LOC_THREADS + lane;
            m[s] = -1;
            if (b[s] < g.nb) {
                const long long row = b[s] / g.ni;
                const int ib = (int)(b[s] - row * g.ni);
                const long long kb = row / g.nj;
                const int jb = (int)(row - kb * g.nj);
                m[s] = ((g.k0 + kb) * g.nny + (g.j0 + jb)) * g.nnx + (g.i0 + ib);
            }
        }
        if (STAGED) {
            for (int f = 0; f < n_fields; ++f) {
#pragma unroll
                for (int s = 0; s < SUB; ++s)
                    lds[(size_t)f * TILE + s * LOC_THREADS + lane] = m[s] >= 0 ? fields[(size_t)f * g.nn + (size_t)m[s]] : (T)0;
            }
        }
        for (int qi = 0; qi < nq; ++qi) {
            const int q = q0 + qi;
            const int k_lo = hyp_off[q], k_hi = hyp_off[q + 1];
            const double sw = hyp_sw[q];
            double phi[SUB];
            const bool live = sw != 0.0;   // (no picks or all weights zero: no winner, a volume row of +0)
            if (live) {
                double a[SUB];
#pragma unroll
                for (int s = 0; s < SUB; ++s) a[s] = 0.0;
                for (int k = k_lo; k < k_hi; ++k) {
                    const int f = pk_field[k];
                    const double t = pk_time[k], w = pk_w[k];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) {
                        const T v = STAGED ? lds[(size_t)f * TILE + s * LOC_THREADS + lane]
                                           : (m[s] >= 0 ? fields[(size_t)f * g.nn + (size_t)m[s]] : (T)0);
                        const double r = t - (double)v;
                        a[s] = a[s] + w * r;
                    }
                }
                double t0[SUB];
#pragma unroll
                for (int s = 0; s < SUB; ++s) {
                    t0[s] = a[s] / sw;
                    phi[s] = 0.0;
                }
                for (int k = k_lo; k < k_hi; ++k) {
                    const int f = pk_field[k];
                    const double t = pk_time[k], w = pk_w[k];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) {
                        const T v = STAGED ? lds[(size_t)f * TILE + s * LOC_THREADS + lane]
                                           : (m[s] >= 0 ? fields[(size_t)f * g.nn + (size_t)m[s]] : (T)0);
                        const double r = t - (double)v;
                        const double d = r - t0[s];
                        phi[s] = phi[s] + w * (d * d);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < SUB; ++s) phi[s] = 0.0;
            }
            if (vol) {
#pragma unroll
                for (int s = 0; s < SUB; ++s)
                    if (m[s] >= 0) vol[(size_t)q * (size_t)g.nb + (size_t)b[s]] = phi[s];
            }
            if (!live) continue;   // (the same for every lane)
            double bp = 0.0;
            long long bn = -1;
#pragma unroll
            for (int s = 0; s < SUB; ++s)
                if (loc_before(phi[s], m[s], bp, bn)) {
                    bp = phi[s];
                    bn = m[s];
                }
#pragma unroll
            for (int off = LOC_WAVE / 2; off >= 1; off /= 2) {
                const double op = __shfl_xor(bp, off, LOC_WAVE);
                const long long on = __shfl_xor(bn, off, LOC_WAVE);
                if (loc_before(op, on, bp, bn)) {
                    bp = op;
                    bn = on;
                }
            }
            if (lane % LOC_WAVE == 0) {
                const int slot = qi * LOC_WAVES + wave;
                if (loc_before(bp, bn, best_phi[slot], best_node[slot])) {
                    best_phi[slot] = bp;
                    best_node[slot] = bn;
                }
            }
        }
    }
    __syncthreads();
    if (lane < nq) {
        double bp = 0.0;
        long long bn = -1;
        for (int w = 0; w < LOC_WAVES; ++w) {
            const int slot = lane * LOC_WAVES + w;
            if (loc_before(best_phi[slot], best_node[slot], bp, bn)) {
                bp = best_phi[slot];
                bn = best_node[slot];
            }
        }
        const size_t o = (size_t)blockIdx.x * (size_t)n_hypo + (size_t)(q0 + lane);
        part_phi[o] = bp;
        part_node[o] = bn;
    }
}

// One thread per hypocentre: the minimum over the gx partials, then t0 at the winner by the definition.  No winner (sw == 0, or every
// phi NaN): node -1, t0 and misfit +0.
template <typename T>
__global__ void loc_finish_kernel(const T* __restrict__ fields, size_t nn, int n_hypo, int gx, const int* __restrict__ hyp_off,
                                  const double* __restrict__ hyp_sw, const int* __restrict__ pk_field, const double* __restrict__ pk_time,
                                  const double* __restrict__ pk_w, const double* __restrict__ part_phi,
                                  const long long* __restrict__ part_node, long long* __restrict__ node_out, double* __restrict__ t0_out,
                                  double* __restrict__ misfit_out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_hypo) return;
    double bp = 0.0;
    long long bn = -1;
    for (int x = 0; x < gx; ++x) {
        const size_t o = (size_t)x * (size_t)n_hypo + (size_t)q;
        const double p = part_phi[o];
        const long long n = part_node[o];
        if (loc_before(p, n, bp, bn)) {
            bp = p;
            bn = n;
        }
    }
    double t0 = 0.0;
    if (bn >= 0) {
        double a = 0.0;
        for (int k = hyp_off[q]; k < hyp_off[q + 1]; ++k) {
            const double r = pk_time[k] - (double)fields[(size_t)pk_field[k] * nn + (size_t)bn];
            a = a + pk_w[k] * r;
        }
        t0 = a / hyp_sw[q];
    } else {
        bp = 0.0;
    }
    node_out[q] = bn;
    t0_out[q] = t0;
    misfit_out[q] = bp;
}

void loc_grow(AdjTapeDev& t, void*& p, size_t& have, size_t bytes, const char* what) {
    if (p && bytes <= have) return;
    LOC_CHECK(hipSetDevice(t.device));
    if (p) (void)hipFree(p);
    p = nullptr;
    t.total_bytes -= have;
    have = 0;
    const size_t b = std::max<size_t>(bytes, 1);
    if (hipMalloc(&p, b) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        std::ostringstream m;
        m << "the grid search needs " << b << " bytes of device memory on device " << t.device << " for " << what
          << " (the allocation failed)";
        throw AdjDeviceError(m.str());
    }
    have = b;
    t.total_bytes += b;
}

template <typename T, int SUB, bool STAGED>
void loc_launch(AdjTapeDev& t, const LocWork& w, const LocBox& g, int n_hypo, long long n_tiles, double* d_vol) {
    const dim3 grid((unsigned)w.gx, (unsigned)((n_hypo + LOC_CHUNK - 1) / LOC_CHUNK));
    const size_t lds = STAGED ? t.n_events * sizeof(T) * LOC_THREADS * SUB : 0;
    loc_search_kernel<T, SUB, STAGED><<<grid, LOC_THREADS, lds, t.stream>>>((const T*)t.fields, (int)t.n_events, g, n_hypo, w.off, w.sw,
                                                                            w.field, w.time, w.weight, n_tiles, w.part_phi, w.part_node,
                                                                            d_vol);
    LOC_CHECK(hipGetLastError());
}

}  // namespace

void adj_loc_shape(const AdjTapeDev& t, int* node_tile, int* hypo_chunk, int* staged) {
    const int sub = loc_sub(t.elem, t.n_events);
    *node_tile = LOC_THREADS * std::max(sub, 1);
    *hypo_chunk = LOC_CHUNK;
    *staged = sub > 0 ? 1 : 0;
}

LocWork adj_loc_prepare(AdjTapeDev& t, size_t n_hypo, size_t n_picks, long long n_box) {
    const int sub = std::max(loc_sub(t.elem, t.n_events), 1);
    const long long n_tiles = (n_box + (long long)LOC_THREADS * sub - 1) / ((long long)LOC_THREADS * sub);
    const size_t gx = (size_t)std::min<long long>(std::max<long long>(n_tiles, 1), LOC_MAX_GX);
    // 8-byte values first, then the ints: sw, time, weight, partial phi and node, the three results; offsets and fields
    const size_t n8 = n_hypo + 2 * n_picks + 2 * gx * n_hypo + 3 * n_hypo;
    loc_grow(t, t.loc_work, t.loc_work_bytes, 8 * n8 + 4 * (n_hypo + 1 + n_picks), "its picks and partial minima");
    LocWork w;
    w.gx = (int)gx;
    w.sw = (double*)t.loc_work;
    w.time = w.sw + n_hypo;
    w.weight = w.time + n_picks;
    w.part_phi = w.weight + n_picks;
    w.part_node = (long long*)(w.part_phi + gx * n_hypo);
    w.node = w.part_node + gx * n_hypo;
    w.t0 = (double*)(w.node + n_hypo);
    w.misfit = w.t0 + n_hypo;
    w.off = (int*)(w.misfit + n_hypo);
    w.field = w.off + n_hypo + 1;
    return w;
}

double* adj_loc_volume(AdjTapeDev& t, size_t count) {
    loc_grow(t, t.loc_vol, t.loc_vol_bytes, count * sizeof(double), "the misfit volume");
    return (double*)t.loc_vol;
}

void adj_loc_release(AdjTapeDev& t) {
    if (!t.loc_work && !t.loc_vol) return;
    (void)hipSetDevice(t.device);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    if (t.loc_work) (void)hipFree(t.loc_work);
    if (t.loc_vol) (void)hipFree(t.loc_vol);
    t.loc_work = t.loc_vol = nullptr;
    t.total_bytes -= t.loc_work_bytes + t.loc_vol_bytes;
    t.loc_work_bytes = t.loc_vol_bytes = 0;
}

template <typename T>
void adj_loc_search(AdjTapeDev& t, const LocWork& w, size_t n_hypo, const int* box, double* d_vol) {
    if (n_hypo == 0) return;
    LOC_CHECK(hipSetDevice(t.device));
    LocBox g;
    g.i0 = box[0]; g.ni = box[1] - box[0];
    g.j0 = box[2]; g.nj = box[3] - box[2];
    g.k0 = box[4]; g.nk = box[5] - box[4];
    g.nnx = t.nnx; g.nny = t.nny;
    g.nb = (long long)g.ni * g.nj * g.nk;
    g.nn = t.nn;
    const int sub = loc_sub(sizeof(T), t.n_events);
    const long long tile = (long long)LOC_THREADS * std::max(sub, 1);
    const long long n_tiles = (g.nb + tile - 1) / tile;
    const int nh = (int)n_hypo;
    if (sub == 4) loc_launch<T, 4, true>(t, w, g, nh, n_tiles, d_vol);
    else if (sub == 2) loc_launch<T, 2, true>(t, w, g, nh, n_tiles, d_vol);
    else if (sub == 1) loc_launch<T, 1, true>(t, w, g, nh, n_tiles, d_vol);
    else loc_launch<T, 1, false>(t, w, g, nh, n_tiles, d_vol);
    loc_finish_kernel<T><<<(unsigned)((n_hypo + LOC_THREADS - 1) / LOC_THREADS), LOC_THREADS, 0, t.stream>>>(
        (const T*)t.fields, t.nn, nh, w.gx, w.off, w.sw, w.field, w.time, w.weight, w.part_phi, w.part_node, w.node, w.t0, w.misfit);
    LOC_CHECK(hipGetLastError());
}

template void adj_loc_search<float>(AdjTapeDev&, const LocWork&, size_t, const int*, double*);
template void adj_loc_search<double>(AdjTapeDev&, const LocWork&, size_t, const int*, double*);

}  // namespace ttcr_amd
