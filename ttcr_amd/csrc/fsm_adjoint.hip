// ttcr_amd/csrc/fsm_adjoint.hip -- translation unit of the field tape's kernels (coupling, seeds, relaxation, gradient; the forward-mode
// tangent: relaxation, receiver rows; cell tapes: the transpose of the cell-to-node averaging; block products: both relaxations, seeds and gradient
// for four columns at once); see fsm_adjoint_api.h and DESIGN.md 6b, 6c, 6e, 6g.  Compiled with -ffp-contract=off like every other unit: each product, difference, quotient and sum
// below is rounded on its own, in the order the definition writes them.
#include "fsm_adjoint_api.h"
#include "fsm_kernels.h"   // fsm_cells_to_nodes3d: the forward direction of a cell tape is set_slowness's own kernel

#include <hipcub/hipcub.hpp>   // the stable radix sort of a moved tape's seed list

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <sstream>
#include <string>

#define ADJ_CHECK(expr)                                                                                           \
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

constexpr int ADJ_THREADS = 256;
constexpr int ADJ_RING = 8;     // rows of the flag ring
constexpr int ADJ_CHECK_EVERY = 4;   // passes between two reads of the flags by the host (extra passes at the fixed point change nothing)
// interior edge of a relaxation tile: with its one-node halo, lam, T and D of a tile take 3 * (edge + 2)^3 * sizeof(T) bytes of LDS --
// 48 KiB (fp32, 16^3) and 40.5 KiB (fp64, 12^3), so three workgroups of 256 threads fit the 160 KiB of a CU
template <typename T> struct AdjTile;
template <> struct AdjTile<float> { static constexpr int edge = 14; };
template <> struct AdjTile<double> { static constexpr int edge = 10; };

template <typename T>
struct AdjGeom {
    int nnx, nny, nnz;
    size_t nn;
    T dx;
};

unsigned blocks_for(size_t n, unsigned b = ADJ_THREADS) { return (unsigned)std::max<size_t>(1, (n + b - 1) / b); }

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

template <typename T>
__global__ void adj_copy_field_kernel(const T* __restrict__ src, int ts, T* __restrict__ dst, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i * ts];
}

template <typename T>
__global__ void adj_mark_frozen_kernel(const long long* __restrict__ key, const T* __restrict__ d, size_t n, unsigned char* __restrict__ frozen,
                                       T* __restrict__ D) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    frozen[key[i]] = 1;
    D[key[i]] = d[i];
}

// Coupling pass, one thread per node, events in blockIdx.y.  For node m of field F (T = F[m]):
//   own side: per axis the smaller neighbour (outside the grid +inf, on a tie the lower index), active iff it is < T; D = sum of (T - a)
//             over the active axes in axis order (frozen nodes keep the d that adj_mark_frozen_kernel wrote);
//   inflow:   bit 2 * axis + side is set iff that neighbour n is not frozen, has m as its smaller neighbour along the axis and F[m] < F[n].
// A node that is not frozen and has no active axis cannot occur in a solved field: *err is raised.
template <typename T>
__global__ void adj_couple_kernel(const T* __restrict__ fields, AdjGeom<T> g, const unsigned char* __restrict__ frozen,
                                  unsigned char* __restrict__ inmask, T* __restrict__ D, int* __restrict__ err) {
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= g.nn) return;
    const size_t base = (size_t)blockIdx.y * g.nn;
    const T* F = fields + base;
    const unsigned char* fz = frozen + base;
    const T inf = std::numeric_limits<T>::infinity();
    const int pos[3] = {(int)(m % g.nnx), (int)((m / g.nnx) % g.nny), (int)(m / ((size_t)g.nnx * g.nny))};
    const int ext[3] = {g.nnx, g.nny, g.nnz};
    const size_t st[3] = {1, (size_t)g.nnx, (size_t)g.nnx * g.nny};
    const T t = F[m];
    const bool self_frozen = fz[m] != 0;
    unsigned in = 0;
    T Dm = 0;
    bool any = false;
    for (int ax = 0; ax < 3; ++ax) {
        const T lo = pos[ax] > 0 ? F[m - st[ax]] : inf;
        const T hi = pos[ax] < ext[ax] - 1 ? F[m + st[ax]] : inf;
        if (!self_frozen) {
            const T a = hi < lo ? hi : lo;
            if (a < t) {
                const T d = t - a;
                Dm = any ? Dm + d : d;
                any = true;
            }
        }
        if (pos[ax] > 0 && !fz[m - st[ax]]) {   // m is the upper neighbour of n = m - st: chosen iff strictly smaller than n's lower one
            const T other = pos[ax] > 1 ? F[m - 2 * st[ax]] : inf;
            if (t < other && t < lo) in |= 1u << (2 * ax);
        }
        if (pos[ax] < ext[ax] - 1 && !fz[m + st[ax]]) {   // m is the lower neighbour of n = m + st: chosen unless n's upper one is smaller
            const T other = pos[ax] < ext[ax] - 2 ? F[m + 2 * st[ax]] : inf;
            if (!(other < t) && t < hi) in |= 1u << (2 * ax + 1);
        }
    }
    inmask[base + m] = (unsigned char)in;
    if (!self_frozen) {
        D[base + m] = Dm;
        if (!any) atomicOr(err, 1);
    }
}

// g = field cotangent (or +0)
template <typename T>
__global__ void adj_seed_fill_kernel(const T* __restrict__ fc, T* __restrict__ g, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) g[i] = fc ? fc[i] : (T)0;
}

// receiver part: the entries are sorted by (event, node) and keep row order, then stencil order, within a node; the first entry of a node
// adds the whole run, left to right -- the bits of one serial chain over the rows of the event
template <typename T>
__global__ void adj_seed_rows_kernel(const long long* __restrict__ key, const int* __restrict__ row, const T* __restrict__ wt, size_t n,
                                     const T* __restrict__ w, T* __restrict__ g) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long k = key[i];
    if (i > 0 && key[i - 1] == k) return;
    T a = g[k];
    for (size_t r = i; r < n && key[r] == k; ++r) a = a + w[row[r]] * wt[r];
    g[k] = a;
}

// lam[j] = g[j] + sum over the flagged neighbours, order x-, x+, y-, y+, z-, z+, of fl(fl(lam[n] * (T[n] - T[j])) / D[n])
#define ADJ_TERM(bit, off)                                              \
    if (in & (1u << (bit))) acc = acc + (L[(off)] * (F[(off)] - tj)) / Dn[(off)];

// Global Jacobi pass (the correctness baseline): out = gather(in) for every node of every event that still changed in the previous pass.
template <typename T>
__global__ void adj_jacobi_kernel(const T* __restrict__ fields, const T* __restrict__ D, const unsigned char* __restrict__ inmask,
                                  const T* __restrict__ g, const T* __restrict__ lam_in, T* __restrict__ lam_out, AdjGeom<T> geo,
                                  const int* __restrict__ prev, int* __restrict__ cur) {
    const int e = blockIdx.y;
    if (prev && prev[e] == 0) return;   // (both buffers of the event hold the fixed point already)
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    int changed = 0;
    if (m < geo.nn) {
        const size_t idx = (size_t)e * geo.nn + m;
        const long long sy = geo.nnx, sz = (long long)geo.nnx * geo.nny;
        const T* L = lam_in + idx;
        const T* F = fields + idx;
        const T* Dn = D + idx;
        const unsigned in = inmask[idx];
        const T tj = F[0];
        T acc = g[idx];
        ADJ_TERM(0, -1) ADJ_TERM(1, 1) ADJ_TERM(2, -sy) ADJ_TERM(3, sy) ADJ_TERM(4, -sz) ADJ_TERM(5, sz)
        changed = !same_bits(acc, L[0]);
        lam_out[idx] = acc;
    }
    if (__syncthreads_or(changed) && threadIdx.x == 0) cur[e] = 1;
}

// Tiled relaxation: one workgroup per tile and event.  lam, T and D of the tile and its one-node halo are staged in LDS, the interior is
// relaxed there (Jacobi steps between barriers) until no value of it changes, then written back in place.  A tile runs in pass p > 0 only
// if one of its six face neighbours changed in pass p - 1 or later (stamps).  Tiles of one pass may read a neighbour's values of this pass
// or of the previous one: both are intermediate values of the same relaxation, the fixed point is the same, and a pass in which no tile
// changed a bit has read final values everywhere.
template <typename T, int TI>
__global__ __launch_bounds__(ADJ_THREADS) void adj_tiled_kernel(const T* __restrict__ fields, const T* __restrict__ D,
                                                                 const unsigned char* __restrict__ inmask, const T* __restrict__ g,
                                                                 T* lam, AdjGeom<T> geo, int ntx, int nty, int ntz, int* stamps, int pass,
                                                                 int* __restrict__ cur) {
    constexpr int TH = TI + 2, NH = TH * TH * TH, NI = TI * TI * TI, NPT = (NI + ADJ_THREADS - 1) / ADJ_THREADS;
    __shared__ T sL[NH], sF[NH], sD[NH];
    const int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
    int* st = stamps + (size_t)e * ntx * nty * ntz;
    if (pass > 0) {
        const int since = pass - 1;
        bool run = false;
        if (tx > 0) run |= st[tile - 1] >= since;
        if (tx < ntx - 1) run |= st[tile + 1] >= since;
        if (ty > 0) run |= st[tile - ntx] >= since;
        if (ty < nty - 1) run |= st[tile + ntx] >= since;
        if (tz > 0) run |= st[tile - ntx * nty] >= since;
        if (tz < ntz - 1) run |= st[tile + ntx * nty] >= since;
        if (!__syncthreads_or(run)) return;   // (one decision for the workgroup: neighbours stamp during this pass, so the threads' own reads may differ)
    }
    const size_t base = (size_t)e * geo.nn;
    const int x0 = tx * TI - 1, y0 = ty * TI - 1, z0 = tz * TI - 1;
    for (int h = tid; h < NH; h += ADJ_THREADS) {
        const int x = x0 + h % TH, y = y0 + (h / TH) % TH, z = z0 + h / (TH * TH);
        const bool inside = x >= 0 && x < geo.nnx && y >= 0 && y < geo.nny && z >= 0 && z < geo.nnz;
        const size_t idx = base + ((size_t)(inside ? z : 0) * geo.nny + (inside ? y : 0)) * geo.nnx + (inside ? x : 0);
        sL[h] = inside ? lam[idx] : (T)0;
        sF[h] = inside ? fields[idx] : (T)0;
        sD[h] = inside ? D[idx] : (T)1;
    }
    // the interior nodes of this thread: LDS index, seed, inflow mask (0 for nodes outside the grid: they stay as loaded)
    int hq[NPT];
    T gq[NPT];
    unsigned inq[NPT];
    size_t mq[NPT];
    for (int q = 0; q < NPT; ++q) {
        const int n = tid + q * ADJ_THREADS;
        hq[q] = -1; gq[q] = 0; inq[q] = 0; mq[q] = 0;
        if (n >= NI) continue;
        const int lx = n % TI, ly = (n / TI) % TI, lz = n / (TI * TI);
        const int x = x0 + 1 + lx, y = y0 + 1 + ly, z = z0 + 1 + lz;
        if (x >= geo.nnx || y >= geo.nny || z >= geo.nnz) continue;
        hq[q] = ((lz + 1) * TH + ly + 1) * TH + lx + 1;
        mq[q] = base + ((size_t)z * geo.nny + y) * geo.nnx + x;
        gq[q] = g[mq[q]];
        inq[q] = inmask[mq[q]];
    }
    __syncthreads();
    bool tile_changed = false;
    for (int it = 0; it <= NI; ++it) {
        T nv[NPT];
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const T* L = sL + hq[q];
            const T* F = sF + hq[q];
            const T* Dn = sD + hq[q];
            const unsigned in = inq[q];
            const T tj = F[0];
            T acc = gq[q];
            ADJ_TERM(0, -1) ADJ_TERM(1, 1) ADJ_TERM(2, -TH) ADJ_TERM(3, TH) ADJ_TERM(4, -TH * TH) ADJ_TERM(5, TH * TH)
            nv[q] = acc;
        }
        __syncthreads();   // every read of this step is done
        int ch = 0;
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            if (!same_bits(nv[q], sL[hq[q]])) { sL[hq[q]] = nv[q]; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        tile_changed = true;
    }
    if (!tile_changed) return;
    for (int q = 0; q < NPT; ++q)
        if (hq[q] >= 0) lam[mq[q]] = sL[hq[q]];
    if (tid == 0) { st[tile] = pass; cur[e] = 1; }
}
#undef ADJ_TERM

// grad[m] = sum over the events, ascending, from +0, of  d * lam (frozen)  or  fl(fl(lam * fl(dx * fl(s * dx))) / D)
template <typename T>
__global__ void adj_grad_kernel(const T* __restrict__ lam, const T* __restrict__ D, const unsigned char* __restrict__ frozen,
                                const T* __restrict__ s, AdjGeom<T> geo, size_t n_events, T* __restrict__ grad) {
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= geo.nn) return;
    const T c = geo.dx * (s[m] * geo.dx);
    T acc = 0;
    for (size_t e = 0; e < n_events; ++e) {
        const size_t idx = e * geo.nn + m;
        const T l = lam[idx];
        const T v = frozen[idx] ? D[idx] * l : (l * c) / D[idx];
        acc = acc + v;
    }
    grad[m] = acc;
}

// ---- forward mode: mu = dT/ds . ds per event, the same triangular system run the other way.
// interior edge of a tangent tile: mu and T of a tile with its one-node halo take 2 * (edge + 2)^3 * sizeof(T) bytes of LDS (13.5 KiB fp32,
// 15.6 KiB fp64).  Smaller than the adjoint's tile (a step re-evaluates every node of the tile, and a tile needs about 3 * edge steps), so
// the forward mode keeps stamps of its own.
template <typename T> struct TanTile;
template <> struct TanTile<float> { static constexpr int edge = 10; };
template <> struct TanTile<double> { static constexpr int edge = 8; };

// Global Jacobi pass of the tangent (the correctness baseline): out = gather(in).  The upwind choice is recomputed from the field:
//   mu[m] = fl(d_m * ds[m])                                                           m frozen
//   mu[m] = fl(acc / D_m), acc = fl(fl(dx * fl(s[m] * dx)) * ds[m]), then per active axis x, y, z: acc = fl(acc + fl(mu[u] * fl(T[m] - a)))
// JOINT: a frozen node keeps what joint_seed_kernel wrote (in both buffers), as in src_jacobi_kernel.
template <typename T, bool JOINT = false>
__global__ void tan_jacobi_kernel(const T* __restrict__ fields, const T* __restrict__ D, const unsigned char* __restrict__ frozen,
                                  const T* __restrict__ s, const T* __restrict__ ds, const T* __restrict__ mu_in, T* __restrict__ mu_out,
                                  AdjGeom<T> geo, const int* __restrict__ prev, int* __restrict__ cur) {
    const int e = blockIdx.y;
    if (prev && prev[e] == 0) return;   // (both buffers of the event hold the fixed point already)
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    int changed = 0;
    if (m < geo.nn && !(JOINT && frozen[(size_t)e * geo.nn + m])) {
        const size_t idx = (size_t)e * geo.nn + m;
        const T inf = std::numeric_limits<T>::infinity();
        const int pos[3] = {(int)(m % geo.nnx), (int)((m / geo.nnx) % geo.nny), (int)(m / ((size_t)geo.nnx * geo.nny))};
        const int ext[3] = {geo.nnx, geo.nny, geo.nnz};
        const long long st[3] = {1, (long long)geo.nnx, (long long)geo.nnx * geo.nny};
        const T* F = fields + idx;
        const T* L = mu_in + idx;
        const T t = F[0];
        T v;
        if (!JOINT && frozen[idx]) {
            v = D[idx] * ds[m];
        } else {
            T acc = (geo.dx * (s[m] * geo.dx)) * ds[m];
            for (int ax = 0; ax < 3; ++ax) {
                const T lo = pos[ax] > 0 ? F[-st[ax]] : inf;
                const T hi = pos[ax] < ext[ax] - 1 ? F[st[ax]] : inf;
                const bool up = hi < lo;
                const T a = up ? hi : lo;
                if (a < t) acc = acc + (up ? L[st[ax]] : L[-st[ax]]) * (t - a);
            }
            v = acc / D[idx];
        }
        changed = !same_bits(v, L[0]);
        mu_out[idx] = v;
    }
    if (__syncthreads_or(changed) && threadIdx.x == 0) cur[e] = 1;
}

// Tiled relaxation of the tangent: one workgroup per tile and event.  mu and T of the tile and its one-node halo are staged in LDS (+inf
// for T outside the grid, so that the upwind choice of 6b falls out of the staged values); every thread keeps, for its interior nodes, the
// own term, D, the upwind choice (2 bits per axis: active, upper) and the differences T[m] - a in registers, so a Jacobi step reads mu only.
// Frozen nodes: own term d * ds, no axis, divisor 1 (exact).  Stamps and passes as in adj_tiled_kernel.
// JOINT: the slowness term and the source seeds in one relaxation -- frozen nodes hold what joint_seed_kernel wrote and are
// staged like halo nodes, read and never rewritten (src_tiled_kernel's treatment); every other node is the one above.
template <typename T, int TI, bool JOINT = false>
__global__ __launch_bounds__(ADJ_THREADS) void tan_tiled_kernel(const T* __restrict__ fields, const T* __restrict__ D,
                                                                 const unsigned char* __restrict__ frozen, const T* __restrict__ s,
                                                                 const T* __restrict__ ds, T* mu, AdjGeom<T> geo, int ntx, int nty, int ntz,
                                                                 int* stamps, int pass, int* __restrict__ cur) {
    constexpr int TH = TI + 2, NH = TH * TH * TH, NI = TI * TI * TI, NPT = (NI + ADJ_THREADS - 1) / ADJ_THREADS;
    __shared__ T sL[NH], sF[NH];
    const int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
    int* st = stamps + (size_t)e * ntx * nty * ntz;
    if (pass > 0) {
        const int since = pass - 1;
        bool run = false;
        if (tx > 0) run |= st[tile - 1] >= since;
        if (tx < ntx - 1) run |= st[tile + 1] >= since;
        if (ty > 0) run |= st[tile - ntx] >= since;
        if (ty < nty - 1) run |= st[tile + ntx] >= since;
        if (tz > 0) run |= st[tile - ntx * nty] >= since;
        if (tz < ntz - 1) run |= st[tile + ntx * nty] >= since;
        if (!__syncthreads_or(run)) return;   // (one decision for the workgroup: neighbours stamp during this pass, so the threads' own reads may differ)
    }
    const T inf = std::numeric_limits<T>::infinity();
    const size_t base = (size_t)e * geo.nn;
    const int x0 = tx * TI - 1, y0 = ty * TI - 1, z0 = tz * TI - 1;
    for (int h = tid; h < NH; h += ADJ_THREADS) {
        const int x = x0 + h % TH, y = y0 + (h / TH) % TH, z = z0 + h / (TH * TH);
        const bool inside = x >= 0 && x < geo.nnx && y >= 0 && y < geo.nny && z >= 0 && z < geo.nnz;
        const size_t idx = base + ((size_t)(inside ? z : 0) * geo.nny + (inside ? y : 0)) * geo.nnx + (inside ? x : 0);
        sL[h] = inside ? mu[idx] : (T)0;
        sF[h] = inside ? fields[idx] : inf;
    }
    __syncthreads();
    // the interior nodes of this thread (hq < 0: outside the grid)
    int hq[NPT];
    unsigned cq[NPT];
    T bq[NPT], dq[NPT], c0[NPT], c1[NPT], c2[NPT];
    for (int q = 0; q < NPT; ++q) {
        const int n = tid + q * ADJ_THREADS;
        hq[q] = -1; cq[q] = 0; bq[q] = 0; dq[q] = 1; c0[q] = 0; c1[q] = 0; c2[q] = 0;
        if (n >= NI) continue;
        const int lx = n % TI, ly = (n / TI) % TI, lz = n / (TI * TI);
        const int x = x0 + 1 + lx, y = y0 + 1 + ly, z = z0 + 1 + lz;
        if (x >= geo.nnx || y >= geo.nny || z >= geo.nnz) continue;
        const int h = ((lz + 1) * TH + ly + 1) * TH + lx + 1;
        const size_t m = ((size_t)z * geo.nny + y) * geo.nnx + x;
        if (JOINT && frozen[base + m]) continue;
        hq[q] = h;
        if (!JOINT && frozen[base + m]) {
            bq[q] = D[base + m] * ds[m];
            continue;
        }
        bq[q] = (geo.dx * (s[m] * geo.dx)) * ds[m];
        dq[q] = D[base + m];
        const T t = sF[h];
        unsigned code = 0;
        {
            const T lo = sF[h - 1], hi = sF[h + 1];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 3u : 1u; c0[q] = t - a; }
        }
        {
            const T lo = sF[h - TH], hi = sF[h + TH];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 12u : 4u; c1[q] = t - a; }
        }
        {
            const T lo = sF[h - TH * TH], hi = sF[h + TH * TH];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 48u : 16u; c2[q] = t - a; }
        }
        cq[q] = code;
    }
    bool tile_changed = false;
    for (int it = 0; it <= NI; ++it) {
        T nv[NPT];
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const T* L = sL + hq[q];
            const unsigned code = cq[q];
            T acc = bq[q];
            if (code & 1u) acc = acc + L[(code & 2u) ? 1 : -1] * c0[q];
            if (code & 4u) acc = acc + L[(code & 8u) ? TH : -TH] * c1[q];
            if (code & 16u) acc = acc + L[(code & 32u) ? TH * TH : -TH * TH] * c2[q];
            nv[q] = acc / dq[q];
        }
        __syncthreads();   // every read of this step is done
        int ch = 0;
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            if (!same_bits(nv[q], sL[hq[q]])) { sL[hq[q]] = nv[q]; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        tile_changed = true;
    }
    if (!tile_changed) return;
    for (int q = 0; q < NPT; ++q) {
        if (hq[q] < 0) continue;
        const int n = tid + q * ADJ_THREADS;
        const int x = x0 + 1 + n % TI, y = y0 + 1 + (n / TI) % TI, z = z0 + 1 + n / (TI * TI);
        mu[base + ((size_t)z * geo.nny + y) * geo.nnx + x] = sL[hq[q]];
    }
    if (tid == 0) { st[tile] = pass; cur[e] = 1; }
}

// dtt[row] = from +0, over the row's stencil entries in interp3d_stencil order: acc = fl(acc + fl(weight * mu[node])); one thread per row
template <typename T>
__global__ void tan_rows_kernel(const int* __restrict__ off, const long long* __restrict__ key, const T* __restrict__ wt, size_t n_rows,
                                const T* __restrict__ mu, T* __restrict__ dtt) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    T acc = 0;
    for (int c = off[r]; c < off[r + 1]; ++c) acc = acc + wt[c] * mu[key[c]];
    dtt[r] = acc;
}

// w[row] = fl(rw[row] * w[row])
template <typename T>
__global__ void tan_scale_rows_kernel(const T* __restrict__ rw, T* __restrict__ w, size_t n_rows) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r < n_rows) w[r] = rw[r] * w[r];
}

// ---- double-difference rows: the data operator B = diag(rw) + Q^T diag(pw) Q in a pair-major pass and one serial chain
// per row.  out[p] = fl(x[a_p] - x[b_p]), times pw[p] (rounded on its own) if pw is given; one thread per pair, a, b, pw and out
// coalesced, the two reads of x gathered
template <typename T>
__global__ void dd_pairs_kernel(const int* __restrict__ a, const int* __restrict__ b, const T* __restrict__ pw, const T* __restrict__ x,
                                size_t n_pairs, T* __restrict__ out) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const T d = x[a[p]] - x[b[p]];
    out[p] = pw ? pw[p] * d : d;
}

// out[row] = a chain over the row's entries (ent[c] = 2 p + sign, ascending p): acc = fl(acc + u[p]), or fl(acc - u[p]) for sign 1.  It
// starts from +0 (x null), from x[row] (rw null) or from fl(rw[row] * x[row]); one thread per row
template <typename T>
__global__ void dd_rows_kernel(const int* __restrict__ off, const int* __restrict__ ent, const T* __restrict__ u, const T* __restrict__ rw,
                               const T* __restrict__ x, size_t n_rows, T* __restrict__ out) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    T acc = x ? (rw ? rw[r] * x[r] : x[r]) : T(0);
    for (int c = off[r]; c < off[r + 1]; ++c) {
        const int e = ent[c];
        const T v = u[e >> 1];
        acc = (e & 1) ? acc - v : acc + v;
    }
    out[r] = acc;
}

// ---- derivatives with respect to the source points: mu = dT/d(t0, x, y, z) . dsrc per event, K columns at once.  A source
// enters the scheme through its frozen nodes only, T[m] = t0 + d_m s[m]: there mu is set by src_seed_kernel and left alone by the
// relaxation; everywhere else mu obeys the tangent's triangular system with the slowness term switched off.  The K values of a node are
// adjacent in memory and in LDS: one 16-byte access per node for fp32, K = 4 (two for fp64).
template <typename T, int K>
struct alignas(sizeof(T) * K) SrcVec {
    T v[K];
};

// mu[m][k] = dsrc[k][q][0], then for a = x, y, z: acc = fl(acc + fl(fl(s[m] * c[m][a]) * dsrc[k][q][1 + a])), q the point that wrote m last;
// +0 in the columns past n_cols.  One thread per frozen entry.
template <typename T, int K>
__global__ void src_seed_kernel(const long long* __restrict__ key, const int* __restrict__ node, const int* __restrict__ pt,
                                const T* __restrict__ c, size_t n, const T* __restrict__ s, const T* __restrict__ dsrc, int n_cols,
                                size_t n_points, SrcVec<T, K>* __restrict__ mu) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T sm = s[node[i]];
    const T sc0 = sm * c[3 * i], sc1 = sm * c[3 * i + 1], sc2 = sm * c[3 * i + 2];
    SrcVec<T, K> v;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T acc = 0;
        if (k < n_cols) {
            const T* d = dsrc + ((size_t)k * n_points + pt[i]) * 4;
            acc = d[0];
            acc = acc + sc0 * d[1];
            acc = acc + sc1 * d[2];
            acc = acc + sc2 * d[3];
        }
        v.v[k] = acc;
    }
    mu[key[i]] = v;
}

// ---- joint hypocentre-velocity tangent: mu[m] = fl(fl(d_m * ds[m]) + sigma[m]) at the frozen node m, sigma the expression of
// src_seed_kernel (K = 1) for the point that wrote m last and d_m what D holds there.  One thread per frozen entry; mu2 (may be null) is the
// second buffer of the Jacobi schedule.  Every other node starts from +0.
template <typename T>
__global__ void joint_seed_kernel(const long long* __restrict__ key, const int* __restrict__ node, const int* __restrict__ pt,
                                  const T* __restrict__ c, size_t n, const T* __restrict__ s, const T* __restrict__ D,
                                  const T* __restrict__ ds, const T* __restrict__ dsrc, T* __restrict__ mu, T* __restrict__ mu2) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T sm = s[node[i]];
    const T* d = dsrc + (size_t)pt[i] * 4;
    T sigma = d[0];
    sigma = sigma + (sm * c[3 * i]) * d[1];
    sigma = sigma + (sm * c[3 * i + 1]) * d[2];
    sigma = sigma + (sm * c[3 * i + 2]) * d[3];
    const T v = D[key[i]] * ds[node[i]] + sigma;
    mu[key[i]] = v;
    if (mu2) mu2[key[i]] = v;
}

// out[i] = fl(c[i] * in[i]): the column scaling of the source block (in and out may be the same array)
template <typename T>
__global__ void joint_scale_kernel(const T* __restrict__ c, const T* in, T* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = c[i] * in[i];
}

// ---- derivatives with respect to the receiver points
template <typename T>
struct RcvGeom {
    int nn[3];
    size_t nodes;
    T dx, cmin[3], shift[3];
};

// G[a] = d interp3d_pt / d p_a with the cell and the on flags held fixed: +0 on an axis the point lies on; otherwise fl(I_a / dx), I_a the
// nested interpolation of interp3d_pt over the remaining axes that are not on (z, then y, then x; the same w1, w2;
// fl(fl(t1 * w1) + fl(t2 * w2))) applied to the differences fl(T[hi_a] - T[lo_a]).  lo, on, w1, w2 as interp3d_stencil computes them, node
// indices clamped as TT clamps them: a clamped upper node reads the lower one again and the difference is +0.
template <typename T>
__device__ __forceinline__ void rcv_grad_pt(const T* __restrict__ Tn, const T* p, const RcvGeom<T>& g, T* G) {
    const double small2 = 1.e-4 * 1.e-4;
    uint32_t c0[3], c1[3];
    bool on[3];
    T w1[3], w2[3];
    for (int a = 0; a < 3; ++a) {
        const uint32_t lo = idx_u32(small2 + (double)((p[a] - g.cmin[a]) / g.dx));
        const T off = p[a] - (g.cmin[a] + (T)lo * g.dx);
        on[a] = (double)(off < 0 ? -off : off) < small2;
        w1[a] = (g.cmin[a] + (T)(lo + 1) * g.dx - p[a]) / g.dx;
        w2[a] = (p[a] - (g.cmin[a] + (T)lo * g.dx)) / g.dx;
        const uint32_t last = (uint32_t)g.nn[a] - 1u;
        c0[a] = lo < last ? lo : last;
        c1[a] = lo + 1u < (uint32_t)g.nn[a] ? lo + 1u : last;
    }
    const size_t stride[3] = {1, (size_t)g.nn[0], (size_t)g.nn[0] * g.nn[1]};
    for (int a = 0; a < 3; ++a) {
        if (on[a]) {
            G[a] = 0;
            continue;
        }
        const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;   // the other two axes, b < c: c is interpolated first
        const int nb = on[b] ? 1 : 2, nc = on[c] ? 1 : 2;
        T e[2];
        for (int ib = 0; ib < nb; ++ib) {
            T d[2];
            for (int ic = 0; ic < nc; ++ic) {
                const size_t rest = (ib ? c1[b] : c0[b]) * stride[b] + (ic ? c1[c] : c0[c]) * stride[c];
                d[ic] = Tn[rest + c1[a] * stride[a]] - Tn[rest + c0[a] * stride[a]];
            }
            e[ib] = on[c] ? d[0] : d[0] * w1[c] + d[1] * w2[c];
        }
        const T i_a = on[b] ? e[0] : e[0] * w1[b] + e[1] * w2[b];
        G[a] = i_a / g.dx;
    }
}

// one thread per query (point, event): tt = interp3d_pt of the event's field, the three G values behind it.  pts and event are never
// null (the tape's own rows are evaluated by passing rcv_p and rcv_event with shift = 0: they are held as the solver sees them);
// shift: the origin of a translated grid is subtracted first, as the solver's entries do
template <typename T>
__global__ void rcv_eval_kernel(const T* __restrict__ fields, const T* __restrict__ pts, const int* __restrict__ event, size_t n,
                                RcvGeom<T> g, int shift, T* __restrict__ tt, T* __restrict__ grad) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    T p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    if (shift)
        for (int a = 0; a < 3; ++a) p[a] = p[a] - g.shift[a];
    const T* Tn = fields + (size_t)event[i] * g.nodes;
    if (tt) tt[i] = interp3d_pt<T>(Tn, 1, p[0], p[1], p[2], g.nn[0], g.nn[1], g.nn[2], g.dx, g.cmin[0], g.cmin[1], g.cmin[2]);
    if (grad) {
        T G[3];
        rcv_grad_pt<T>(Tn, p, g, G);
        grad[3 * i] = G[0];
        grad[3 * i + 1] = G[1];
        grad[3 * i + 2] = G[2];
    }
}

// the forward chain, one thread per row: acc = drcv[q][0], then per axis x, y, z acc = fl(acc + fl(G[r][a] * drcv[q][1 + a])), q the point
// of the row; dtt[r] = acc, or fl(base[r] + acc) in the joint tangent (base may be dtt)
template <typename T>
__global__ void rcv_rows_kernel(const int* __restrict__ pt, const T* __restrict__ G, const T* __restrict__ drcv, size_t n_rows,
                                const T* base, T* dtt) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const T* d = drcv + (size_t)pt[r] * 4;
    T acc = d[0];
    acc = acc + G[3 * r] * d[1];
    acc = acc + G[3 * r + 1] * d[2];
    acc = acc + G[3 * r + 2] * d[3];
    dtt[r] = base ? base[r] + acc : acc;
}

// the reverse chains, one thread per (receiver point, parameter): over the rows of the point in ascending row order, from +0,
// acc = fl(acc + w[r]) for t0 and acc = fl(acc + fl(w[r] * G[r][a])) for x, y, z
template <typename T>
__global__ void rcv_grad_kernel(const int* __restrict__ off, const int* __restrict__ rows, const T* __restrict__ G,
                                const T* __restrict__ w, size_t n_points, T* __restrict__ grcv) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= 4 * n_points) return;
    const size_t q = i / 4;
    const int k = (int)(i % 4);
    T acc = 0;
    for (int j = off[q]; j < off[q + 1]; ++j) {
        const int r = rows[j];
        acc = k == 0 ? acc + w[r] : acc + w[r] * G[3 * (size_t)r + k - 1];
    }
    grcv[i] = acc;
}

// ---- moving the receiver points.  One thread per row r of receiver point q = pt[r]: the point as the solver sees it
// (p = fl(pts[q] - shift) per axis, the arithmetic of the raytrace entry; a grid that is not translated has shift +0), its stencil
// (interp3d_stencil) written into the row-order list at off[r] -- the host formed the offsets from the same function; a count that
// differs raises *err and nothing is written past the row's room --, with the row and the place of every entry for the sort that follows;
// then tt (interp3d_pt on the event's field) and G (rcv_grad_pt), as rcv_eval_kernel computes them.
template <typename T>
__global__ void rcv_move_kernel(const T* __restrict__ fields, const T* __restrict__ pts, const int* __restrict__ pt,
                                const int* __restrict__ event, const int* __restrict__ off, size_t n_rows, RcvGeom<T> g,
                                T* __restrict__ rcv_p, T* __restrict__ tt, T* __restrict__ grad, long long* __restrict__ rw_key,
                                T* __restrict__ rw_w, int* __restrict__ ent_row, int* __restrict__ ent_idx, int* __restrict__ err) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const size_t q = (size_t)pt[r];
    T p[3];
    for (int a = 0; a < 3; ++a) {
        p[a] = pts[3 * q + a] - g.shift[a];
        rcv_p[3 * r + a] = p[a];
    }
    long long nd[8];
    T wt[8];
    const int cnt = interp3d_stencil<T>(p[0], p[1], p[2], g.nn[0], g.nn[1], g.nn[2], g.dx, g.cmin[0], g.cmin[1], g.cmin[2], nd, wt);
    const int o = off[r], room = off[r + 1] - o;
    if (cnt != room) atomicOr(err, 1);
    const long long base = (long long)((size_t)event[r] * g.nodes);
    for (int c = 0; c < room; ++c) {   // (every place of the row's room is written, so the sort never sees a stale entry)
        const bool real = c < cnt;
        rw_key[o + c] = base + (real ? nd[c] : 0);
        rw_w[o + c] = real ? wt[c] : (T)0;
        ent_row[o + c] = (int)r;
        ent_idx[o + c] = o + c;
    }
    const T* Tn = fields + (size_t)event[r] * g.nodes;
    tt[r] = interp3d_pt<T>(Tn, 1, p[0], p[1], p[2], g.nn[0], g.nn[1], g.nn[2], g.dx, g.cmin[0], g.cmin[1], g.cmin[2]);
    T G[3];
    rcv_grad_pt<T>(Tn, p, g, G);
    grad[3 * r] = G[0];
    grad[3 * r + 1] = G[1];
    grad[3 * r + 2] = G[2];
}

// the seed list behind the sorted keys: place i holds entry perm[i] of the row-order list
template <typename T>
__global__ void rcv_move_gather_kernel(const int* __restrict__ perm, const int* __restrict__ ent_row, const T* __restrict__ rw_w, size_t n,
                                       int* __restrict__ sd_row, T* __restrict__ sd_w) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e = perm[i];
    sd_row[i] = ent_row[e];
    sd_w[i] = rw_w[e];
}

// Global Jacobi pass of the K-column relaxation (the correctness baseline): for a node that is not frozen
//   mu[m][k] = fl(acc / D_m), acc = +0, then per active axis x, y, z: acc = fl(acc + fl(mu[u][k] * fl(T[m] - a)))
// with the upwind choice recomputed from the field once for the K columns.  Frozen nodes keep what src_seed_kernel wrote (in both buffers).
template <typename T, int K>
__global__ void src_jacobi_kernel(const T* __restrict__ fields, const T* __restrict__ D, const unsigned char* __restrict__ frozen,
                                  const SrcVec<T, K>* __restrict__ mu_in, SrcVec<T, K>* __restrict__ mu_out, AdjGeom<T> geo,
                                  const int* __restrict__ prev, int* __restrict__ cur) {
    const int e = blockIdx.y;
    if (prev && prev[e] == 0) return;   // (both buffers of the event hold the fixed point already)
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    int changed = 0;
    if (m < geo.nn && !frozen[(size_t)e * geo.nn + m]) {
        const size_t idx = (size_t)e * geo.nn + m;
        const T inf = std::numeric_limits<T>::infinity();
        const int pos[3] = {(int)(m % geo.nnx), (int)((m / geo.nnx) % geo.nny), (int)(m / ((size_t)geo.nnx * geo.nny))};
        const int ext[3] = {geo.nnx, geo.nny, geo.nnz};
        const long long st[3] = {1, (long long)geo.nnx, (long long)geo.nnx * geo.nny};
        const T* F = fields + idx;
        const SrcVec<T, K>* L = mu_in + idx;
        const T t = F[0];
        SrcVec<T, K> acc;
#pragma unroll
        for (int k = 0; k < K; ++k) acc.v[k] = 0;
        for (int ax = 0; ax < 3; ++ax) {
            const T lo = pos[ax] > 0 ? F[-st[ax]] : inf;
            const T hi = pos[ax] < ext[ax] - 1 ? F[st[ax]] : inf;
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) {
                const T d = t - a;
                const SrcVec<T, K> u = up ? L[st[ax]] : L[-st[ax]];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * d;
            }
        }
        const T Dm = D[idx];
        const SrcVec<T, K> old = L[0];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            acc.v[k] = acc.v[k] / Dm;
            changed |= !same_bits(acc.v[k], old.v[k]);
        }
        mu_out[idx] = acc;
    }
    if (__syncthreads_or(changed) && threadIdx.x == 0) cur[e] = 1;
}

// Tiled K-column relaxation: tan_tiled_kernel's tiles, stamps and passes.  T of the tile and its halo is staged once (+inf outside the grid),
// the upwind choice, D and the differences T[m] - a are computed once per node and kept in registers for the K columns; a Jacobi step reads
// the K adjacent values of each upwind neighbour in one access.  LDS: (K + 1) (edge + 2)^3 elements -- 34.5 KiB (fp32) and 39 KiB (fp64)
// for K = 4.  Frozen nodes are staged like halo nodes: read, never written.
template <typename T, int K, int TI>
__global__ __launch_bounds__(ADJ_THREADS) void src_tiled_kernel(const T* __restrict__ fields, const T* __restrict__ D,
                                                                 const unsigned char* __restrict__ frozen, SrcVec<T, K>* mu, AdjGeom<T> geo,
                                                                 int ntx, int nty, int ntz, int* stamps, int pass, int* __restrict__ cur) {
    constexpr int TH = TI + 2, NH = TH * TH * TH, NI = TI * TI * TI, NPT = (NI + ADJ_THREADS - 1) / ADJ_THREADS;
    __shared__ SrcVec<T, K> sL[NH];
    __shared__ T sF[NH];
    const int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
    int* st = stamps + (size_t)e * ntx * nty * ntz;
    if (pass > 0) {
        const int since = pass - 1;
        bool run = false;
        if (tx > 0) run |= st[tile - 1] >= since;
        if (tx < ntx - 1) run |= st[tile + 1] >= since;
        if (ty > 0) run |= st[tile - ntx] >= since;
        if (ty < nty - 1) run |= st[tile + ntx] >= since;
        if (tz > 0) run |= st[tile - ntx * nty] >= since;
        if (tz < ntz - 1) run |= st[tile + ntx * nty] >= since;
        if (!__syncthreads_or(run)) return;   // (one decision for the workgroup, as in tan_tiled_kernel)
    }
    const T inf = std::numeric_limits<T>::infinity();
    const size_t base = (size_t)e * geo.nn;
    const int x0 = tx * TI - 1, y0 = ty * TI - 1, z0 = tz * TI - 1;
    SrcVec<T, K> zero;
#pragma unroll
    for (int k = 0; k < K; ++k) zero.v[k] = 0;
    for (int h = tid; h < NH; h += ADJ_THREADS) {
        const int x = x0 + h % TH, y = y0 + (h / TH) % TH, z = z0 + h / (TH * TH);
        const bool inside = x >= 0 && x < geo.nnx && y >= 0 && y < geo.nny && z >= 0 && z < geo.nnz;
        const size_t idx = base + ((size_t)(inside ? z : 0) * geo.nny + (inside ? y : 0)) * geo.nnx + (inside ? x : 0);
        SrcVec<T, K> v = zero;
        if (inside) v = mu[idx];
        sL[h] = v;
        sF[h] = inside ? fields[idx] : inf;
    }
    __syncthreads();
    // the interior nodes of this thread that the relaxation owns (hq < 0: outside the grid, or frozen)
    int hq[NPT];
    unsigned cq[NPT];
    T dq[NPT], c0[NPT], c1[NPT], c2[NPT];
    for (int q = 0; q < NPT; ++q) {
        const int n = tid + q * ADJ_THREADS;
        hq[q] = -1; cq[q] = 0; dq[q] = 1; c0[q] = 0; c1[q] = 0; c2[q] = 0;
        if (n >= NI) continue;
        const int lx = n % TI, ly = (n / TI) % TI, lz = n / (TI * TI);
        const int x = x0 + 1 + lx, y = y0 + 1 + ly, z = z0 + 1 + lz;
        if (x >= geo.nnx || y >= geo.nny || z >= geo.nnz) continue;
        const int h = ((lz + 1) * TH + ly + 1) * TH + lx + 1;
        const size_t m = ((size_t)z * geo.nny + y) * geo.nnx + x;
        if (frozen[base + m]) continue;
        hq[q] = h;
        dq[q] = D[base + m];
        const T t = sF[h];
        unsigned code = 0;
        {
            const T lo = sF[h - 1], hi = sF[h + 1];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 3u : 1u; c0[q] = t - a; }
        }
        {
            const T lo = sF[h - TH], hi = sF[h + TH];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 12u : 4u; c1[q] = t - a; }
        }
        {
            const T lo = sF[h - TH * TH], hi = sF[h + TH * TH];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 48u : 16u; c2[q] = t - a; }
        }
        cq[q] = code;
    }
    bool tile_changed = false;
    for (int it = 0; it <= NI; ++it) {
        SrcVec<T, K> nv[NPT];
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const SrcVec<T, K>* L = sL + hq[q];
            const unsigned code = cq[q];
            SrcVec<T, K> acc = zero;
            if (code & 1u) {
                const SrcVec<T, K> u = L[(code & 2u) ? 1 : -1];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * c0[q];
            }
            if (code & 4u) {
                const SrcVec<T, K> u = L[(code & 8u) ? TH : -TH];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * c1[q];
            }
            if (code & 16u) {
                const SrcVec<T, K> u = L[(code & 32u) ? TH * TH : -TH * TH];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * c2[q];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) nv[q].v[k] = acc.v[k] / dq[q];
        }
        __syncthreads();   // every read of this step is done
        int ch = 0;
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const SrcVec<T, K> old = sL[hq[q]];
            bool diff = false;
#pragma unroll
            for (int k = 0; k < K; ++k) diff |= !same_bits(nv[q].v[k], old.v[k]);
            if (diff) { sL[hq[q]] = nv[q]; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        tile_changed = true;
    }
    if (!tile_changed) return;
    for (int q = 0; q < NPT; ++q) {
        if (hq[q] < 0) continue;
        const int n = tid + q * ADJ_THREADS;
        const int x = x0 + 1 + n % TI, y = y0 + 1 + (n / TI) % TI, z = z0 + 1 + n / (TI * TI);
        mu[base + ((size_t)z * geo.nny + y) * geo.nnx + x] = sL[hq[q]];
    }
    if (tid == 0) { st[tile] = pass; cur[e] = 1; }
}

// dtt[k][row] = from +0, over the row's stencil entries in interp3d_stencil order: acc = fl(acc + fl(weight * mu[node][k])); one thread per
// (row, column)
template <typename T, int K>
__global__ void src_rows_kernel(const int* __restrict__ off, const long long* __restrict__ key, const T* __restrict__ wt, size_t n_rows,
                                int n_cols, const T* __restrict__ mu, T* __restrict__ dtt) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n_rows * (size_t)n_cols) return;
    const size_t r = i % n_rows;
    const int k = (int)(i / n_rows);
    T acc = 0;
    for (int c = off[r]; c < off[r + 1]; ++c) acc = acc + wt[c] * mu[(size_t)key[c] * K + k];
    dtt[i] = acc;
}

// dfields[k][i] = mu[i][k]
template <typename T, int K>
__global__ void src_unpack_kernel(const T* __restrict__ mu, size_t en, int n_cols, T* __restrict__ out) {
    const size_t n = en * (size_t)n_cols;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = mu[(i % en) * K + i / en];
}

// ---- block products: K model vectors per relaxation, the K values of a node adjacent (SrcVec) in memory and in LDS.  What a
// step computes once per node -- masks, upwind choice, differences, D -- serves the K columns; per column the expressions and their order are
// those of the one-column kernels above, so every column has the bits of the one-column call.

// g[j][k] = from +0, over the stencil entries of node j in row order: acc = fl(acc + fl(w[k][row] * weight)): adj_seed_rows_kernel's serial
// chain, K chains per thread (+0 in the columns past n_cols).  g is +0 everywhere before the launch.
template <typename T, int K>
__global__ void adjk_seed_rows_kernel(const long long* __restrict__ key, const int* __restrict__ row, const T* __restrict__ wt, size_t n,
                                      const T* __restrict__ w, size_t n_rows, int n_cols, SrcVec<T, K>* __restrict__ g) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long j = key[i];
    if (i > 0 && key[i - 1] == j) return;
    SrcVec<T, K> a;
#pragma unroll
    for (int k = 0; k < K; ++k) a.v[k] = 0;
    for (size_t r = i; r < n && key[r] == j; ++r) {
        const T wr = wt[r];
        const size_t rr = (size_t)row[r];
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k < n_cols) a.v[k] = a.v[k] + w[(size_t)k * n_rows + rr] * wr;
    }
    g[j] = a;
}

// lam[j][k] = g[j][k] + sum over the flagged neighbours, order x-, x+, y-, y+, z-, z+, of fl(fl(lam[n][k] * (T[n] - T[j])) / D[n])
#define ADJK_TERM(bit, off)                                                  \
    if (in & (1u << (bit))) {                                                \
        const T c = F[(off)] - tj;                                           \
        const T dn = Dn[(off)];                                              \
        const SrcVec<T, K> u = L[(off)];                                     \
        _Pragma("unroll") for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + (u.v[k] * c) / dn; \
    }

// Tiled K-column relaxation of the adjoint: adj_tiled_kernel with the tangent's tile edge (lam of K columns, T and D of a tile with its
// halo take (K + 2) (edge + 2)^3 elements of LDS: 40.5 KiB fp32, 46.9 KiB fp64 for K = 4), its stamps, run decision and passes.  The
// in-mask, T[n] - T[j] and D[n] are read and formed once per coupling, the K values of lam[n] come in one access.
template <typename T, int K, int TI>
__global__ __launch_bounds__(ADJ_THREADS) void adjk_tiled_kernel(const T* __restrict__ fields, const T* __restrict__ D,
                                                                  const unsigned char* __restrict__ inmask,
                                                                  const SrcVec<T, K>* __restrict__ g, SrcVec<T, K>* lam, AdjGeom<T> geo, int ntx,
                                                                  int nty, int ntz, int* stamps, int pass, int* __restrict__ cur) {
    constexpr int TH = TI + 2, NH = TH * TH * TH, NI = TI * TI * TI, NPT = (NI + ADJ_THREADS - 1) / ADJ_THREADS;
    __shared__ SrcVec<T, K> sL[NH];
    __shared__ T sF[NH], sD[NH];
    const int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
    int* st = stamps + (size_t)e * ntx * nty * ntz;
    if (pass > 0) {
        const int since = pass - 1;
        bool run = false;
        if (tx > 0) run |= st[tile - 1] >= since;
        if (tx < ntx - 1) run |= st[tile + 1] >= since;
        if (ty > 0) run |= st[tile - ntx] >= since;
        if (ty < nty - 1) run |= st[tile + ntx] >= since;
        if (tz > 0) run |= st[tile - ntx * nty] >= since;
        if (tz < ntz - 1) run |= st[tile + ntx * nty] >= since;
        if (!__syncthreads_or(run)) return;   // (one decision for the workgroup, as in adj_tiled_kernel)
    }
    const size_t base = (size_t)e * geo.nn;
    const int x0 = tx * TI - 1, y0 = ty * TI - 1, z0 = tz * TI - 1;
    SrcVec<T, K> zero;
#pragma unroll
    for (int k = 0; k < K; ++k) zero.v[k] = 0;
    for (int h = tid; h < NH; h += ADJ_THREADS) {
        const int x = x0 + h % TH, y = y0 + (h / TH) % TH, z = z0 + h / (TH * TH);
        const bool inside = x >= 0 && x < geo.nnx && y >= 0 && y < geo.nny && z >= 0 && z < geo.nnz;
        const size_t idx = base + ((size_t)(inside ? z : 0) * geo.nny + (inside ? y : 0)) * geo.nnx + (inside ? x : 0);
        SrcVec<T, K> v = zero;
        if (inside) v = lam[idx];
        sL[h] = v;
        sF[h] = inside ? fields[idx] : (T)0;
        sD[h] = inside ? D[idx] : (T)1;
    }
    // the interior nodes of this thread: LDS index, seeds, inflow mask (hq < 0: outside the grid)
    int hq[NPT];
    SrcVec<T, K> gq[NPT];
    unsigned inq[NPT];
    size_t mq[NPT];
    for (int q = 0; q < NPT; ++q) {
        const int n = tid + q * ADJ_THREADS;
        hq[q] = -1; gq[q] = zero; inq[q] = 0; mq[q] = 0;
        if (n >= NI) continue;
        const int lx = n % TI, ly = (n / TI) % TI, lz = n / (TI * TI);
        const int x = x0 + 1 + lx, y = y0 + 1 + ly, z = z0 + 1 + lz;
        if (x >= geo.nnx || y >= geo.nny || z >= geo.nnz) continue;
        hq[q] = ((lz + 1) * TH + ly + 1) * TH + lx + 1;
        mq[q] = base + ((size_t)z * geo.nny + y) * geo.nnx + x;
        gq[q] = g[mq[q]];
        inq[q] = inmask[mq[q]];
    }
    __syncthreads();
    bool tile_changed = false;
    for (int it = 0; it <= NI; ++it) {
        SrcVec<T, K> nv[NPT];
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const SrcVec<T, K>* L = sL + hq[q];
            const T* F = sF + hq[q];
            const T* Dn = sD + hq[q];
            const unsigned in = inq[q];
            const T tj = F[0];
            SrcVec<T, K> acc = gq[q];
            ADJK_TERM(0, -1) ADJK_TERM(1, 1) ADJK_TERM(2, -TH) ADJK_TERM(3, TH) ADJK_TERM(4, -TH * TH) ADJK_TERM(5, TH * TH)
            nv[q] = acc;
        }
        __syncthreads();   // every read of this step is done
        int ch = 0;
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const SrcVec<T, K> old = sL[hq[q]];
            bool diff = false;
#pragma unroll
            for (int k = 0; k < K; ++k) diff |= !same_bits(nv[q].v[k], old.v[k]);
            if (diff) { sL[hq[q]] = nv[q]; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        tile_changed = true;
    }
    if (!tile_changed) return;
    for (int q = 0; q < NPT; ++q)
        if (hq[q] >= 0) lam[mq[q]] = sL[hq[q]];
    if (tid == 0) { st[tile] = pass; cur[e] = 1; }
}
#undef ADJK_TERM

// grad[k][m] = sum over the events, ascending, from +0, of  d * lam[.][k] (frozen)  or  fl(fl(lam[.][k] * fl(dx * fl(s * dx))) / D):
// adj_grad_kernel per column, D, the frozen mark and the own factor read once
template <typename T, int K>
__global__ void adjk_grad_kernel(const SrcVec<T, K>* __restrict__ lam, const T* __restrict__ D, const unsigned char* __restrict__ frozen,
                                 const T* __restrict__ s, AdjGeom<T> geo, size_t n_events, int n_cols, T* __restrict__ grad) {
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= geo.nn) return;
    const T c = geo.dx * (s[m] * geo.dx);
    SrcVec<T, K> acc;
#pragma unroll
    for (int k = 0; k < K; ++k) acc.v[k] = 0;
    for (size_t e = 0; e < n_events; ++e) {
        const size_t idx = e * geo.nn + m;
        const SrcVec<T, K> l = lam[idx];
        const T d = D[idx];
        const bool fz = frozen[idx] != 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T v = fz ? d * l.v[k] : (l.v[k] * c) / d;
            acc.v[k] = acc.v[k] + v;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (k < n_cols) grad[(size_t)k * geo.nn + m] = acc.v[k];
}

// Tiled K-column relaxation of the tangent with its slowness term: src_tiled_kernel's tiles, staging and registers plus tan_tiled_kernel's
// own term per column -- fl(d_m * ds[k][m]) for a frozen node (no axis, divisor 1: exact), fl(fl(dx * fl(s[m] * dx)) * ds[k][m]) for every
// other one, the start of the chain over the active axes (never +0: +0 + (-0) is +0).  ds holds n_cols columns of nn values; the columns
// past n_cols are +0.
template <typename T, int K, int TI>
__global__ __launch_bounds__(ADJ_THREADS) void tank_tiled_kernel(const T* __restrict__ fields, const T* __restrict__ D,
                                                                  const unsigned char* __restrict__ frozen, const T* __restrict__ s,
                                                                  const T* __restrict__ ds, int n_cols, SrcVec<T, K>* mu, AdjGeom<T> geo,
                                                                  int ntx, int nty, int ntz, int* stamps, int pass, int* __restrict__ cur) {
    constexpr int TH = TI + 2, NH = TH * TH * TH, NI = TI * TI * TI, NPT = (NI + ADJ_THREADS - 1) / ADJ_THREADS;
    __shared__ SrcVec<T, K> sL[NH];
    __shared__ T sF[NH];
    const int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
    int* st = stamps + (size_t)e * ntx * nty * ntz;
    if (pass > 0) {
        const int since = pass - 1;
        bool run = false;
        if (tx > 0) run |= st[tile - 1] >= since;
        if (tx < ntx - 1) run |= st[tile + 1] >= since;
        if (ty > 0) run |= st[tile - ntx] >= since;
        if (ty < nty - 1) run |= st[tile + ntx] >= since;
        if (tz > 0) run |= st[tile - ntx * nty] >= since;
        if (tz < ntz - 1) run |= st[tile + ntx * nty] >= since;
        if (!__syncthreads_or(run)) return;   // (one decision for the workgroup, as in tan_tiled_kernel)
    }
    const T inf = std::numeric_limits<T>::infinity();
    const size_t base = (size_t)e * geo.nn;
    const int x0 = tx * TI - 1, y0 = ty * TI - 1, z0 = tz * TI - 1;
    SrcVec<T, K> zero;
#pragma unroll
    for (int k = 0; k < K; ++k) zero.v[k] = 0;
    for (int h = tid; h < NH; h += ADJ_THREADS) {
        const int x = x0 + h % TH, y = y0 + (h / TH) % TH, z = z0 + h / (TH * TH);
        const bool inside = x >= 0 && x < geo.nnx && y >= 0 && y < geo.nny && z >= 0 && z < geo.nnz;
        const size_t idx = base + ((size_t)(inside ? z : 0) * geo.nny + (inside ? y : 0)) * geo.nnx + (inside ? x : 0);
        SrcVec<T, K> v = zero;
        if (inside) v = mu[idx];
        sL[h] = v;
        sF[h] = inside ? fields[idx] : inf;
    }
    __syncthreads();
    // the interior nodes of this thread (hq < 0: outside the grid)
    int hq[NPT];
    unsigned cq[NPT];
    SrcVec<T, K> bq[NPT];
    T dq[NPT], c0[NPT], c1[NPT], c2[NPT];
    for (int q = 0; q < NPT; ++q) {
        const int n = tid + q * ADJ_THREADS;
        hq[q] = -1; cq[q] = 0; bq[q] = zero; dq[q] = 1; c0[q] = 0; c1[q] = 0; c2[q] = 0;
        if (n >= NI) continue;
        const int lx = n % TI, ly = (n / TI) % TI, lz = n / (TI * TI);
        const int x = x0 + 1 + lx, y = y0 + 1 + ly, z = z0 + 1 + lz;
        if (x >= geo.nnx || y >= geo.nny || z >= geo.nnz) continue;
        const int h = ((lz + 1) * TH + ly + 1) * TH + lx + 1;
        const size_t m = ((size_t)z * geo.nny + y) * geo.nnx + x;
        hq[q] = h;
        const bool fz = frozen[base + m] != 0;
        const T own = fz ? D[base + m] : geo.dx * (s[m] * geo.dx);
#pragma unroll
        for (int k = 0; k < K; ++k) bq[q].v[k] = own * (k < n_cols ? ds[(size_t)k * geo.nn + m] : (T)0);
        if (fz) continue;
        dq[q] = D[base + m];
        const T t = sF[h];
        unsigned code = 0;
        {
            const T lo = sF[h - 1], hi = sF[h + 1];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 3u : 1u; c0[q] = t - a; }
        }
        {
            const T lo = sF[h - TH], hi = sF[h + TH];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 12u : 4u; c1[q] = t - a; }
        }
        {
            const T lo = sF[h - TH * TH], hi = sF[h + TH * TH];
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) { code |= up ? 48u : 16u; c2[q] = t - a; }
        }
        cq[q] = code;
    }
    bool tile_changed = false;
    for (int it = 0; it <= NI; ++it) {
        SrcVec<T, K> nv[NPT];
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const SrcVec<T, K>* L = sL + hq[q];
            const unsigned code = cq[q];
            SrcVec<T, K> acc = bq[q];
            if (code & 1u) {
                const SrcVec<T, K> u = L[(code & 2u) ? 1 : -1];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * c0[q];
            }
            if (code & 4u) {
                const SrcVec<T, K> u = L[(code & 8u) ? TH : -TH];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * c1[q];
            }
            if (code & 16u) {
                const SrcVec<T, K> u = L[(code & 32u) ? TH * TH : -TH * TH];
#pragma unroll
                for (int k = 0; k < K; ++k) acc.v[k] = acc.v[k] + u.v[k] * c2[q];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) nv[q].v[k] = acc.v[k] / dq[q];
        }
        __syncthreads();   // every read of this step is done
        int ch = 0;
        for (int q = 0; q < NPT; ++q) {
            if (hq[q] < 0) continue;
            const SrcVec<T, K> old = sL[hq[q]];
            bool diff = false;
#pragma unroll
            for (int k = 0; k < K; ++k) diff |= !same_bits(nv[q].v[k], old.v[k]);
            if (diff) { sL[hq[q]] = nv[q]; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        tile_changed = true;
    }
    if (!tile_changed) return;
    for (int q = 0; q < NPT; ++q) {
        if (hq[q] < 0) continue;
        const int n = tid + q * ADJ_THREADS;
        const int x = x0 + 1 + n % TI, y = y0 + 1 + (n / TI) % TI, z = z0 + 1 + n / (TI * TI);
        mu[base + ((size_t)z * geo.nny + y) * geo.nnx + x] = sL[hq[q]];
    }
    if (tid == 0) { st[tile] = pass; cur[e] = 1; }
}

// gsrc[q][0] = from +0, over the frozen nodes of point q in ascending node index: acc = fl(acc + lam[m]);
// gsrc[q][1 + a] = the same chain of fl(lam[m] * fl(s[m] * c[m][a])).  One thread per point; no atomics.
template <typename T>
__global__ void src_grad_kernel(const int* __restrict__ off, const long long* __restrict__ key, const int* __restrict__ node,
                                const T* __restrict__ c, size_t n_points, const T* __restrict__ s, const T* __restrict__ lam,
                                T* __restrict__ gsrc) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= n_points) return;
    T a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = off[q]; i < off[q + 1]; ++i) {
        const T l = lam[key[i]];
        const T sm = s[node[i]];
        a0 = a0 + l;
        a1 = a1 + l * (sm * c[3 * (size_t)i]);
        a2 = a2 + l * (sm * c[3 * (size_t)i + 1]);
        a3 = a3 + l * (sm * c[3 * (size_t)i + 2]);
    }
    gsrc[4 * q] = a0; gsrc[4 * q + 1] = a1; gsrc[4 * q + 2] = a2; gsrc[4 * q + 3] = a3;
}

// ---- second-order products: the derivative of the vjp in a direction v, for a cotangent whose lam is held on the tape.
// Three streaming passes around the relaxations above; every value is one fixed expression of final values.
// dD[n] = sum over the active axes, order x, y, z, the first term assigned, of fl(mu[n] - mu[u_axis(n)]); +0 for a frozen node.  One thread
// per node, events in blockIdx.y; the upwind choice is recomputed from the field as tan_jacobi_kernel does.
template <typename T>
__global__ void hess_dd_kernel(const T* __restrict__ fields, const unsigned char* __restrict__ frozen, const T* __restrict__ mu,
                               AdjGeom<T> geo, T* __restrict__ dD) {
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= geo.nn) return;
    const size_t idx = (size_t)blockIdx.y * geo.nn + m;
    T acc = 0;
    if (!frozen[idx]) {
        const T inf = std::numeric_limits<T>::infinity();
        const int pos[3] = {(int)(m % geo.nnx), (int)((m / geo.nnx) % geo.nny), (int)(m / ((size_t)geo.nnx * geo.nny))};
        const int ext[3] = {geo.nnx, geo.nny, geo.nnz};
        const long long st[3] = {1, (long long)geo.nnx, (long long)geo.nnx * geo.nny};
        const T* F = fields + idx;
        const T* M = mu + idx;
        const T t = F[0], mm = M[0];
        bool any = false;
        for (int ax = 0; ax < 3; ++ax) {
            const T lo = pos[ax] > 0 ? F[-st[ax]] : inf;
            const T hi = pos[ax] < ext[ax] - 1 ? F[st[ax]] : inf;
            const bool up = hi < lo;
            const T a = up ? hi : lo;
            if (a < t) {
                const T p = mm - (up ? M[st[ax]] : M[-st[ax]]);
                acc = any ? acc + p : p;
                any = true;
            }
        }
    }
    dD[idx] = acc;
}

// q[j] = +0, then over the neighbours n flagged in j's in-mask, order x-, x+, y-, y+, z-, z+:
//   q[j] = fl(q[j] + fl(lam[n] * fl(fl(fl(mu[n] - mu[j]) - fl(fl(fl(T[n] - T[j]) / D[n]) * dD[n])) / D[n])))
#define HESS_TERM(bit, off)                                                                          \
    if (in & (1u << (bit))) {                                                                         \
        const T dn = Dn[(off)];                                                                       \
        acc = acc + L[(off)] * (((M[(off)] - mj) - ((F[(off)] - tj) / dn) * dDn[(off)]) / dn);        \
    }
template <typename T>
__global__ void hess_q_kernel(const T* __restrict__ fields, const T* __restrict__ D, const unsigned char* __restrict__ inmask,
                              const T* __restrict__ lam, const T* __restrict__ mu, const T* __restrict__ dD, AdjGeom<T> geo,
                              T* __restrict__ q) {
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= geo.nn) return;
    const size_t idx = (size_t)blockIdx.y * geo.nn + m;
    const long long sy = geo.nnx, sz = (long long)geo.nnx * geo.nny;
    const unsigned in = inmask[idx];
    T acc = 0;
    if (in) {
        const T* L = lam + idx;
        const T* F = fields + idx;
        const T* M = mu + idx;
        const T* Dn = D + idx;
        const T* dDn = dD + idx;
        const T tj = F[0], mj = M[0];
        HESS_TERM(0, -1) HESS_TERM(1, 1) HESS_TERM(2, -sy) HESS_TERM(3, sy) HESS_TERM(4, -sz) HESS_TERM(5, sz)
    }
    q[idx] = acc;
}
#undef HESS_TERM

// out[m] = sum over the events, ascending, from +0, of  fl(d * lam2) (frozen)  or  fl(fl(fl(lam2 * c) / D) + r),
//   c = fl(dx * fl(s * dx)),  r = fl(fl(lam * fl(fl(dx * fl(v * dx)) - fl(fl(c / D) * dD))) / D)
// adj_grad_kernel with the direct term added.  v and out may be the same array (a thread reads v[m] before it writes out[m]).
template <typename T>
__global__ void hess_grad_kernel(const T* __restrict__ lam2, const T* __restrict__ lam, const T* __restrict__ D, const T* __restrict__ dD,
                                 const unsigned char* __restrict__ frozen, const T* __restrict__ s, const T* v, AdjGeom<T> geo,
                                 size_t n_events, T* out) {
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= geo.nn) return;
    const T c = geo.dx * (s[m] * geo.dx);
    const T cv = geo.dx * (v[m] * geo.dx);
    T acc = 0;
    for (size_t e = 0; e < n_events; ++e) {
        const size_t idx = e * geo.nn + m;
        const T l2 = lam2[idx];
        const T d = D[idx];
        T o;
        if (frozen[idx]) {
            o = d * l2;
        } else {
            const T r = (lam[idx] * (cv - (c / d) * dD[idx])) / d;
            o = (l2 * c) / d + r;
        }
        acc = acc + o;
    }
    out[m] = acc;
}

// ---- cell tapes: gc = A^T g, A the averaging of fsm_cells_to_nodes3d.  One thread per cell c = (ck * ncy + cj) * ncx + ci:
// the eight products fl(f(n) * g[n]) over the corner nodes n = (ci + a, cj + b, ck + d), f(n) = 1 / (cells touching n) = 1, 1/2, 1/4 or 1/8
// (a product of exact per-axis factors), added left to right from the first product, a innermost, d outermost.  No atomics.
template <typename T>
__global__ void adj_nodes_to_cells_kernel(const T* __restrict__ g, T* __restrict__ gc, int ncx, int ncy, int ncz) {
    const size_t nc = (size_t)ncx * ncy * ncz;
    const size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int ci = (int)(c % ncx), cj = (int)((c / ncx) % ncy), ck = (int)(c / ((size_t)ncx * ncy));
    const size_t nnx = (size_t)ncx + 1, nny = (size_t)ncy + 1;
    T acc = 0;
    for (int d = 0; d < 2; ++d) {
        const int k = ck + d;
        const T fz = (k == 0 || k == ncz) ? (T)1 : (T)0.5;
        for (int b = 0; b < 2; ++b) {
            const int j = cj + b;
            const T fy = (j == 0 || j == ncy) ? fz : fz * (T)0.5;
            for (int a = 0; a < 2; ++a) {
                const int i = ci + a;
                const T f = (i == 0 || i == ncx) ? fy : fy * (T)0.5;
                const T p = f * g[((size_t)k * nny + j) * nnx + i];
                acc = (a | b | d) == 0 ? p : acc + p;
            }
        }
    }
    gc[c] = acc;
}

struct Alloc {
    AdjTapeDev& t;
    size_t planned;
    template <typename P>
    void operator()(P*& p, size_t bytes) {
        const size_t b = std::max<size_t>(bytes, 1);
        void* raw = nullptr;
        if (hipMalloc(&raw, b) != hipSuccess) {
            (void)hipGetLastError();
            std::ostringstream m;
            m << "the field tape needs " << planned << " bytes of device memory on device " << t.device << " (an allocation of " << b
              << " bytes failed)";
            throw AdjDeviceError(m.str());
        }
        p = (P*)raw;
        t.total_bytes += b;
    }
};

template <typename P>
void dev_free(P*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

size_t tiles_of(const AdjTapeDev& t, int ed) { return (size_t)((t.nnx + ed - 1) / ed) * ((t.nny + ed - 1) / ed) * ((t.nnz + ed - 1) / ed); }
size_t tiles_of(const AdjTapeDev& t) { return tiles_of(t, adj_tile_edge(t.elem)); }

// every byte the finished tape holds (the figure an allocation failure names): fields, D, g, lam, lam2; inmask, frozen; slowness and the
// staged gradient; the staged w; the seed entries (8 per row at most); flags, stamps, error flag; a cell or model tape's staged model
// vector; a model tape's axis tables and the two intermediates of P^T
size_t model_map_planned(const AdjTapeDev& t) {
    if (!t.model) return 0;
    const int n[3] = {t.nnx, t.nny, t.nnz};
    return model_map_bytes(n, t.elem) + (t.map.n_stage_z() + t.map.n_stage_y()) * t.elem;
}
size_t planned_bytes(const AdjTapeDev& t) {
    const size_t en = t.n_events * t.nn;
    return 5 * en * t.elem + 2 * en + 2 * t.nn * t.elem + t.n_rows * t.elem + 8 * t.n_rows * (8 + 4 + t.elem) +
           (t.mapped() ? t.n_model() * t.elem : 0) + model_map_planned(t) +
           (ADJ_RING * t.n_events + t.n_events * tiles_of(t) + 1) * sizeof(int);
}

}  // namespace

int adj_tile_edge(size_t elem) { return elem == 4 ? AdjTile<float>::edge : AdjTile<double>::edge; }
int adj_tan_tile_edge(size_t elem) { return elem == 4 ? TanTile<float>::edge : TanTile<double>::edge; }

void AdjTapeDev::release() {
    if (!fields && !stream) return;
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    dev_free(fields); dev_free(slowness); dev_free(D); dev_free(inmask); dev_free(frozen); dev_free(g); dev_free(lam); dev_free(lam2);
    dev_free(sd_key); dev_free(sd_row); dev_free(sd_w); dev_free(flags); dev_free(stamps); dev_free(err); dev_free(w_tmp); dev_free(grad_tmp);
    dev_free(rw_off); dev_free(rw_key); dev_free(rw_w); dev_free(rw_tmp); dev_free(tan_stamps);
    dev_free(src_off); dev_free(src_pt); dev_free(src_key); dev_free(src_node); dev_free(src_c); dev_free(src_io); dev_free(src_rows);
    dev_free(mu4); dev_free(mu4b); dev_free(cell_tmp); dev_free(hold_lam); dev_free(hess_dd);
    dev_free(map_a); dev_free(map_b);
    model_map_free(map);
    dev_free(g4); dev_free(blk_model); dev_free(blk_nodes); dev_free(blk_rows); dev_free(blk_rw);
    for (CgSystem sys : {CG_MODEL, CG_SOURCE, CG_RECEIVER, CG_RELOC}) adj_cg_release(*this, sys);
    dev_free(mv_row); dev_free(mv_idx); dev_free(mv_perm); dev_free(mv_sort);
    mv_cap = 0;
    mv_sort_bytes = 0;
    dev_free(rcv_p); dev_free(rcv_event); dev_free(rcv_pt); dev_free(rcv_rows); dev_free(rcv_off); dev_free(rcv_G); dev_free(rcv_tt);
    dev_free(rcv_io); dev_free(rcv_stage);
    adj_loc_release(*this);
    adj_dd_release(*this);
    rcv_stage_bytes = 0;
    rcv_bytes = 0;
    blk_owns_mu4 = false;
    blk_bytes = 0;
    held = false;
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    total_bytes = 0;
}

void adj_alloc_fields(AdjTapeDev& t) {
    ADJ_CHECK(hipSetDevice(t.device));
    Alloc alloc{t, planned_bytes(t)};
    alloc(t.fields, t.n_events * t.nn * t.elem);
    alloc(t.slowness, t.nn * t.elem);
}

template <typename T>
void adj_copy_field(const T* src, int ts, T* dst, size_t n, hipStream_t stream) {
    if (n == 0) return;
    adj_copy_field_kernel<T><<<std::min(blocks_for(n), 16384u), ADJ_THREADS, 0, stream>>>(src, ts, dst, n);
    ADJ_CHECK(hipGetLastError());
}

template <typename T>
void adj_finish(AdjTapeDev& t, const AdjSink& sink) {
    ADJ_CHECK(hipSetDevice(t.device));
    const size_t en = t.n_events * t.nn;
    if (t.n_events > 65535) throw std::runtime_error("the field tape takes at most 65535 events per call");
    // frozen nodes: one entry per (event, node), the last writer's d
    std::vector<long long> fk;
    std::vector<T> fd;
    for (size_t e = 0; e < t.n_events; ++e)
        for (size_t q = 0; q < sink.fr_node[e].size(); ++q) {
            fk.push_back((long long)(e * t.nn) + sink.fr_node[e][q]);
            fd.push_back((T)sink.fr_d[e][q]);
        }
    // seed entries: row order, then stencil order, kept within a node by the stable sort
    std::vector<long long> key;
    std::vector<int> row;
    std::vector<T> wt;
    for (size_t r = 0; r < t.n_rows; ++r)
        for (int c = 0; c < sink.st_cnt[r]; ++c) {
            key.push_back((long long)((size_t)sink.st_event[r] * t.nn) + sink.st_node[8 * r + c]);
            row.push_back((int)r);
            wt.push_back((T)sink.st_w[8 * r + c]);
        }
    std::vector<size_t> ord(key.size());
    std::iota(ord.begin(), ord.end(), (size_t)0);
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return key[a] < key[b]; });
    std::vector<long long> key2(key.size());
    std::vector<int> row2(key.size());
    std::vector<T> wt2(key.size());
    for (size_t q = 0; q < ord.size(); ++q) { key2[q] = key[ord[q]]; row2[q] = row[ord[q]]; wt2[q] = wt[ord[q]]; }
    t.n_seed = key2.size();
    t.n_tiles = tiles_of(t);
    // the same entries in row order, for the forward mode: kept on the host until the first jvp uploads them
    t.h_rw_off.assign(t.n_rows + 1, 0);
    for (size_t r = 0; r < t.n_rows; ++r) t.h_rw_off[r + 1] = t.h_rw_off[r] + sink.st_cnt[r];
    t.h_rw_key = key;
    t.h_rw_w.assign(wt.begin(), wt.end());
    // the frozen entries by (point, node), for the source derivative: kept on the host until the first call that needs them
    {
        t.n_points = sink.pt_off.empty() ? 0 : (size_t)sink.pt_off[t.n_events];
        t.h_pt_event.assign(t.n_points, 0);
        struct Ent { int pt; long long key; const double* c; };
        std::vector<Ent> ent;
        for (size_t e = 0; e < t.n_events; ++e) {
            for (int q = sink.pt_off[e]; q < sink.pt_off[e + 1]; ++q) t.h_pt_event[q] = (int)e;
            for (size_t q = 0; q < sink.fr_node[e].size(); ++q)
                ent.push_back({sink.pt_off[e] + sink.fr_pt[e][q], (long long)(e * t.nn) + sink.fr_node[e][q], &sink.fr_c[e][3 * q]});
        }
        std::sort(ent.begin(), ent.end(), [](const Ent& a, const Ent& b) { return a.pt != b.pt ? a.pt < b.pt : a.key < b.key; });
        t.h_src_off.assign(t.n_points + 1, 0);
        t.h_src_key.clear();
        t.h_src_c.clear();
        for (const Ent& en_ : ent) {
            t.h_src_off[en_.pt + 1] += 1;
            t.h_src_key.push_back(en_.key);
            t.h_src_c.insert(t.h_src_c.end(), en_.c, en_.c + 3);
        }
        for (size_t q = 0; q < t.n_points; ++q) t.h_src_off[q + 1] += t.h_src_off[q];
    }
    // the receivers of the rows, for the receiver derivative: kept on the host until the first call that needs them; one
    // receiver point per row until adj_rcv_set_points says otherwise
    {
        t.h_rcv_p = sink.st_p;
        t.h_rcv_p.resize(3 * t.n_rows, 0.0);
        t.h_rcv_event.assign(sink.st_event.begin(), sink.st_event.end());
        std::copy(sink.rcv_min, sink.rcv_min + 3, t.rcv_min);
        std::copy(sink.rcv_shift, sink.rcv_shift + 3, t.rcv_shift);
        std::copy(sink.rcv_max, sink.rcv_max + 3, t.rcv_max);
        std::vector<int> one(t.n_rows);
        std::iota(one.begin(), one.end(), 0);
        adj_rcv_set_points(t, one.data(), t.n_rows);
    }

    Alloc alloc{t, planned_bytes(t)};
    alloc(t.D, en * t.elem);
    alloc(t.g, en * t.elem);
    alloc(t.lam, en * t.elem);
    alloc(t.lam2, en * t.elem);
    alloc(t.inmask, en);
    alloc(t.frozen, en);
    alloc(t.sd_key, t.n_seed * sizeof(long long));
    alloc(t.sd_row, t.n_seed * sizeof(int));
    alloc(t.sd_w, t.n_seed * t.elem);
    alloc(t.flags, ADJ_RING * t.n_events * sizeof(int));
    alloc(t.stamps, t.n_events * t.n_tiles * sizeof(int));
    alloc(t.err, sizeof(int));
    alloc(t.w_tmp, t.n_rows * t.elem);
    alloc(t.grad_tmp, t.nn * t.elem);
    if (t.mapped()) alloc(t.cell_tmp, t.n_model() * t.elem);
    if (t.model) {   // the intermediates of P^T and the axis tables of P (the sizes of t.map were set with the tape)
        alloc(t.map_a, t.map.n_stage_z() * t.elem);
        alloc(t.map_b, t.map.n_stage_y() * t.elem);
        const int n[3] = {t.nnx, t.nny, t.nnz};
        const int m[3] = {t.map.m[0], t.map.m[1], t.map.m[2]};
        model_map_create<T>(t.map, n, m);
        t.total_bytes += t.map.bytes;
    }
    long long* d_fk = nullptr;
    T* d_fd = nullptr;
    hipStream_t s = t.stream;
    try {
        if (t.n_seed > 0) {
            ADJ_CHECK(hipMemcpyAsync(t.sd_key, key2.data(), t.n_seed * sizeof(long long), hipMemcpyHostToDevice, s));
            ADJ_CHECK(hipMemcpyAsync(t.sd_row, row2.data(), t.n_seed * sizeof(int), hipMemcpyHostToDevice, s));
            ADJ_CHECK(hipMemcpyAsync(t.sd_w, wt2.data(), t.n_seed * sizeof(T), hipMemcpyHostToDevice, s));
        }
        ADJ_CHECK(hipMemsetAsync(t.err, 0, sizeof(int), s));
        if (en > 0) {
            ADJ_CHECK(hipMemsetAsync(t.frozen, 0, en, s));
            if (!fk.empty()) {
                ADJ_CHECK(hipMalloc((void**)&d_fk, fk.size() * sizeof(long long)));
                ADJ_CHECK(hipMalloc((void**)&d_fd, fd.size() * sizeof(T)));
                ADJ_CHECK(hipMemcpyAsync(d_fk, fk.data(), fk.size() * sizeof(long long), hipMemcpyHostToDevice, s));
                ADJ_CHECK(hipMemcpyAsync(d_fd, fd.data(), fd.size() * sizeof(T), hipMemcpyHostToDevice, s));
                adj_mark_frozen_kernel<T><<<blocks_for(fk.size()), ADJ_THREADS, 0, s>>>(d_fk, d_fd, fk.size(), t.frozen, (T*)t.D);
                ADJ_CHECK(hipGetLastError());
            }
            const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
            adj_couple_kernel<T><<<dim3(blocks_for(t.nn), (unsigned)t.n_events), ADJ_THREADS, 0, s>>>((const T*)t.fields, geo, t.frozen, t.inmask,
                                                                                                   (T*)t.D, t.err);
            ADJ_CHECK(hipGetLastError());
        }
        int h_err = 0;
        ADJ_CHECK(hipMemcpyAsync(&h_err, t.err, sizeof(int), hipMemcpyDeviceToHost, s));
        ADJ_CHECK(hipStreamSynchronize(s));
        dev_free(d_fk);
        dev_free(d_fd);
        if (h_err) throw std::runtime_error("adjoint: internal error, a node that is not frozen has no upwind neighbour (the field is not a solved one)");
    } catch (...) {
        dev_free(d_fk);
        dev_free(d_fd);
        throw;
    }
}

// Passes until one changes nothing in any event: launch(pass, prev, cur) enqueues pass `pass`, which raises cur[e] if it changed a value of
// event e (prev: the flags of the pass before, null for pass 0).  The host reads the flags every ADJ_CHECK_EVERY passes.  Returns the
// passes launched.
template <typename Launch>
int relax_to_fixed_point(AdjTapeDev& t, const char* what, Launch launch) {
    hipStream_t s = t.stream;
    const size_t E = t.n_events;
    std::vector<int> h_flags((size_t)ADJ_RING * E);
    const size_t max_passes = t.nn + ADJ_CHECK_EVERY + 1;   // (the depth of the DAG is below the node count)
    int passes = 0;
    for (;;) {
        for (int k = 0; k < ADJ_CHECK_EVERY; ++k, ++passes) {
            int* cur = t.flags + (size_t)(passes % ADJ_RING) * E;
            const int* prev = passes > 0 ? t.flags + (size_t)((passes - 1) % ADJ_RING) * E : nullptr;
            ADJ_CHECK(hipMemsetAsync(cur, 0, E * sizeof(int), s));
            launch(passes, prev, cur);
            ADJ_CHECK(hipGetLastError());
        }
        ADJ_CHECK(hipMemcpyAsync(h_flags.data(), t.flags, h_flags.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        ADJ_CHECK(hipStreamSynchronize(s));
        const int* last = h_flags.data() + (size_t)((passes - 1) % ADJ_RING) * E;
        bool any = false;
        for (size_t e = 0; e < E; ++e) any = any || last[e] != 0;
        if (!any) return passes;
        if ((size_t)passes > max_passes)
            throw std::runtime_error(std::string(what) + ": internal error, the relaxation did not reach its fixed point");
    }
}

// the vjp; d_grad may be null (no gradient kernel); *lam_final (may be null) receives the buffer that holds the fixed point
template <typename T>
static int adj_vjp_impl(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, int schedule, const T** lam_final) {
    ADJ_CHECK(hipSetDevice(t.device));
    hipStream_t s = t.stream;
    const size_t E = t.n_events, en = E * t.nn;
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    T* g = (T*)t.g;
    T* lam = (T*)t.lam;
    int passes = 0;
    if (en > 0) {
        if (d_fc != g) {   // (a caller that formed the field cotangent in g itself: hess_q_kernel)
            adj_seed_fill_kernel<T><<<std::min(blocks_for(en), 65536u), ADJ_THREADS, 0, s>>>(d_fc, g, en);
            ADJ_CHECK(hipGetLastError());
        }
        if (d_w && t.n_seed > 0) {
            adj_seed_rows_kernel<T><<<blocks_for(t.n_seed), ADJ_THREADS, 0, s>>>(t.sd_key, t.sd_row, (const T*)t.sd_w, t.n_seed, d_w, g);
            ADJ_CHECK(hipGetLastError());
        }
        ADJ_CHECK(hipMemcpyAsync(lam, g, en * sizeof(T), hipMemcpyDeviceToDevice, s));
        if (schedule == 0) ADJ_CHECK(hipMemsetAsync(t.stamps, 0xFF, E * t.n_tiles * sizeof(int), s));
        const int ed = adj_tile_edge(sizeof(T));
        const int ntx = (t.nnx + ed - 1) / ed, nty = (t.nny + ed - 1) / ed, ntz = (t.nnz + ed - 1) / ed;
        T* in = lam;
        T* out = (T*)t.lam2;
        passes = relax_to_fixed_point(t, "adjoint", [&](int pass, const int* prev, int* cur) {
            if (schedule == 0) {
                adj_tiled_kernel<T, AdjTile<T>::edge><<<dim3((unsigned)t.n_tiles, (unsigned)E), ADJ_THREADS, 0, s>>>(
                    (const T*)t.fields, (const T*)t.D, t.inmask, g, lam, geo, ntx, nty, ntz, t.stamps, pass, cur);
            } else {
                adj_jacobi_kernel<T><<<dim3(blocks_for(t.nn), (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.inmask, g,
                                                                                                in, out, geo, prev, cur);
                std::swap(in, out);
            }
        });
        if (schedule != 0) lam = in;   // (the buffer the last pass wrote; both hold the fixed point)
    }
    if (d_grad && t.nn > 0) {
        adj_grad_kernel<T><<<blocks_for(t.nn), ADJ_THREADS, 0, s>>>(lam, (const T*)t.D, t.frozen, (const T*)t.slowness, geo, E, d_grad);
        ADJ_CHECK(hipGetLastError());
    }
    if (lam_final) *lam_final = lam;
    return passes;
}

// The map between the model vector and the node vector of a tape whose model vector is not the node vector, on the tape's stream -- the
// one place that knows the parameterisation.  Cell tape: d_nodes = A d_cells (fsm_cells_to_nodes3d), d_cells = A^T d_nodes (one thread
// per cell).  Model tape: d_nodes = P d_model, d_model = P^T d_nodes (fsm_model.hip).
template <typename T>
void adj_model_to_nodes(AdjTapeDev& t, const T* d_cells, T* d_nodes) {
    if (!t.mapped()) throw std::logic_error("adj_model_to_nodes: a node tape has no map");
    if (t.nn == 0) return;
    if (t.model) return model_prolong<T>(t.map, d_cells, d_nodes, t.stream);
    const unsigned blocks = std::min(blocks_for(t.nn), 4096u);   // (the launch of set_slowness)
    fsm_cells_to_nodes3d<T><<<blocks, ADJ_THREADS, 0, t.stream>>>(d_cells, d_nodes, t.nnx - 1, t.nny - 1, t.nnz - 1);
    ADJ_CHECK(hipGetLastError());
}

template <typename T>
void adj_nodes_to_model(AdjTapeDev& t, const T* d_nodes, T* d_cells) {
    if (!t.mapped()) throw std::logic_error("adj_nodes_to_model: a node tape has no map");
    if (t.model) return model_restrict<T>(t.map, d_nodes, (T*)t.map_a, (T*)t.map_b, d_cells, t.stream);
    if (t.nc == 0) return;
    adj_nodes_to_cells_kernel<T><<<blocks_for(t.nc), ADJ_THREADS, 0, t.stream>>>(d_nodes, d_cells, t.nnx - 1, t.nny - 1, t.nnz - 1);
    ADJ_CHECK(hipGetLastError());
}

// the vjp with respect to the model vector: on a cell or model tape the node gradient of 6b is formed in grad_tmp, then d_grad = the
// transposed map of grad_tmp
template <typename T>
static int adj_vjp_model(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, int schedule, const T** lam_final) {
    if (!t.mapped() || !d_grad) return adj_vjp_impl<T>(t, d_w, d_fc, d_grad, schedule, lam_final);
    const int passes = adj_vjp_impl<T>(t, d_w, d_fc, (T*)t.grad_tmp, schedule, lam_final);
    adj_nodes_to_model<T>(t, (const T*)t.grad_tmp, d_grad);
    return passes;
}

template <typename T>
int adj_vjp(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, int schedule) {
    return adj_vjp_model<T>(t, d_w, d_fc, d_grad, schedule, nullptr);
}

// what the first jvp adds to the tape: the stencil in row order (offsets, keys, weights), a staging row for a host row_weight and the
// stamps of the tangent tiles
size_t adj_jvp_extra_bytes(const AdjTapeDev& t) {
    return (t.n_rows + 1) * sizeof(int) + t.n_seed * (sizeof(long long) + t.elem) + t.n_rows * t.elem +
           t.n_events * tiles_of(t, adj_tan_tile_edge(t.elem)) * sizeof(int);
}

template <typename T>
void adj_jvp_prepare(AdjTapeDev& t) {
    if (t.rw_off) return;
    ADJ_CHECK(hipSetDevice(t.device));
    Alloc alloc{t, adj_jvp_extra_bytes(t)};
    const size_t before = t.total_bytes;
    try {
        alloc(t.rw_off, (t.n_rows + 1) * sizeof(int));
        alloc(t.rw_key, t.n_seed * sizeof(long long));
        alloc(t.rw_w, t.n_seed * sizeof(T));
        alloc(t.rw_tmp, t.n_rows * sizeof(T));
        t.n_tan_tiles = tiles_of(t, TanTile<T>::edge);
        alloc(t.tan_stamps, t.n_events * t.n_tan_tiles * sizeof(int));
        const std::vector<T> wt(t.h_rw_w.begin(), t.h_rw_w.end());
        ADJ_CHECK(hipMemcpyAsync(t.rw_off, t.h_rw_off.data(), (t.n_rows + 1) * sizeof(int), hipMemcpyHostToDevice, t.stream));
        if (t.n_seed > 0) {
            ADJ_CHECK(hipMemcpyAsync(t.rw_key, t.h_rw_key.data(), t.n_seed * sizeof(long long), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.rw_w, wt.data(), t.n_seed * sizeof(T), hipMemcpyHostToDevice, t.stream));
        }
        ADJ_CHECK(hipStreamSynchronize(t.stream));   // (wt leaves scope)
    } catch (...) {
        dev_free(t.rw_off); dev_free(t.rw_key); dev_free(t.rw_w); dev_free(t.rw_tmp); dev_free(t.tan_stamps);
        t.total_bytes = before;
        throw;
    }
}

// the jvp; *mu_final (may be null) receives the buffer that holds the relaxed tangent, *ds_nodes (may be null) the node perturbation
template <typename T>
static int adj_jvp_impl(AdjTapeDev& t, const T* d_ds, T* d_dtt, T* d_dfields, int schedule, const T** mu_final, const T** ds_nodes) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_jvp_prepare<T>(t);
    hipStream_t s = t.stream;
    const size_t E = t.n_events, en = E * t.nn;
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    if (t.mapped()) {   // the node perturbation: what set_slowness would compute from the cell perturbation, or P d_ds
        adj_model_to_nodes<T>(t, d_ds, (T*)t.grad_tmp);
        d_ds = (const T*)t.grad_tmp;
    }
    T* mu = (T*)t.lam;
    int passes = 0;
    if (en > 0) {
        ADJ_CHECK(hipMemsetAsync(mu, 0, en * sizeof(T), s));   // (+0: any start reaches the fixed point)
        if (schedule == 0) ADJ_CHECK(hipMemsetAsync(t.tan_stamps, 0xFF, E * t.n_tan_tiles * sizeof(int), s));
        constexpr int ed = TanTile<T>::edge;
        const int ntx = (t.nnx + ed - 1) / ed, nty = (t.nny + ed - 1) / ed, ntz = (t.nnz + ed - 1) / ed;
        const unsigned tiles = (unsigned)t.n_tan_tiles;
        T* in = mu;
        T* out = (T*)t.lam2;
        passes = relax_to_fixed_point(t, "tangent", [&](int pass, const int* prev, int* cur) {
            if (schedule == 0) {
                tan_tiled_kernel<T, ed><<<dim3(tiles, (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.frozen,
                                                                                        (const T*)t.slowness, d_ds, mu, geo, ntx, nty, ntz,
                                                                                        t.tan_stamps, pass, cur);
            } else {
                tan_jacobi_kernel<T><<<dim3(blocks_for(t.nn), (unsigned)E), ADJ_THREADS, 0, s>>>(
                    (const T*)t.fields, (const T*)t.D, t.frozen, (const T*)t.slowness, d_ds, in, out, geo, prev, cur);
                std::swap(in, out);
            }
        });
        if (schedule != 0) mu = in;   // (the buffer the last pass wrote; both hold the fixed point)
    }
    if (d_dtt && t.n_rows > 0) {
        tan_rows_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, s>>>(t.rw_off, t.rw_key, (const T*)t.rw_w, t.n_rows, mu, d_dtt);
        ADJ_CHECK(hipGetLastError());
    }
    if (d_dfields && en > 0) ADJ_CHECK(hipMemcpyAsync(d_dfields, mu, en * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (mu_final) *mu_final = mu;
    if (ds_nodes) *ds_nodes = d_ds;
    return passes;
}

template <typename T>
int adj_jvp(AdjTapeDev& t, const T* d_ds, T* d_dtt, T* d_dfields, int schedule) {
    return adj_jvp_impl<T>(t, d_ds, d_dtt, d_dfields, schedule, nullptr, nullptr);
}

// ---- double-difference rows
void adj_dd_set_pairs(AdjTapeDev& t, const int* row_a, const int* row_b, size_t n_pairs) {
    adj_dd_release(t);   // (what is on the device belongs to the old list)
    t.h_dd_a.assign(row_a, row_a + n_pairs);
    t.h_dd_b.assign(row_b, row_b + n_pairs);
    t.n_pairs = n_pairs;
    t.dd_set = true;
    t.h_dd_off.assign(t.n_rows + 1, 0);
    for (size_t p = 0; p < n_pairs; ++p) {
        t.h_dd_off[row_a[p] + 1] += 1;
        t.h_dd_off[row_b[p] + 1] += 1;
    }
    for (size_t r = 0; r < t.n_rows; ++r) t.h_dd_off[r + 1] += t.h_dd_off[r];
    t.h_dd_ent.assign(2 * n_pairs, 0);
    std::vector<int> fill(t.h_dd_off.begin(), t.h_dd_off.end() - 1);
    for (size_t p = 0; p < n_pairs; ++p) {   // (ascending p within a row)
        t.h_dd_ent[fill[row_a[p]]++] = (int)(2 * p);
        t.h_dd_ent[fill[row_b[p]]++] = (int)(2 * p + 1);
    }
}

size_t adj_dd_bytes(const AdjTapeDev& t) {
    auto at_least_1 = [](size_t b) { return std::max<size_t>(b, 1); };
    return 2 * at_least_1(t.n_pairs * sizeof(int)) + at_least_1((t.n_rows + 1) * sizeof(int)) + at_least_1(2 * t.n_pairs * sizeof(int)) +
           2 * at_least_1(t.n_pairs * t.elem) + at_least_1(t.n_rows * t.elem);
}

void adj_dd_prepare(AdjTapeDev& t) {
    if (t.dd_off) return;
    ADJ_CHECK(hipSetDevice(t.device));
    Alloc alloc{t, adj_dd_bytes(t)};
    const size_t before = t.total_bytes;
    try {
        alloc(t.dd_a, t.n_pairs * sizeof(int));
        alloc(t.dd_b, t.n_pairs * sizeof(int));
        alloc(t.dd_off, (t.n_rows + 1) * sizeof(int));
        alloc(t.dd_ent, 2 * t.n_pairs * sizeof(int));
        alloc(t.dd_u, t.n_pairs * t.elem);
        alloc(t.dd_pw, t.n_pairs * t.elem);
        alloc(t.dd_rows, t.n_rows * t.elem);
        ADJ_CHECK(hipMemcpyAsync(t.dd_off, t.h_dd_off.data(), (t.n_rows + 1) * sizeof(int), hipMemcpyHostToDevice, t.stream));
        if (t.n_pairs > 0) {
            ADJ_CHECK(hipMemcpyAsync(t.dd_a, t.h_dd_a.data(), t.n_pairs * sizeof(int), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.dd_b, t.h_dd_b.data(), t.n_pairs * sizeof(int), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.dd_ent, t.h_dd_ent.data(), 2 * t.n_pairs * sizeof(int), hipMemcpyHostToDevice, t.stream));
        }
    } catch (...) {
        dev_free(t.dd_a); dev_free(t.dd_b); dev_free(t.dd_off); dev_free(t.dd_ent); dev_free(t.dd_u); dev_free(t.dd_pw); dev_free(t.dd_rows);
        t.total_bytes = before;
        throw;
    }
    t.dd_bytes = t.total_bytes - before;
}

void adj_dd_release(AdjTapeDev& t) {
    if (!t.dd_off) return;
    (void)hipSetDevice(t.device);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    dev_free(t.dd_a); dev_free(t.dd_b); dev_free(t.dd_off); dev_free(t.dd_ent); dev_free(t.dd_u); dev_free(t.dd_pw); dev_free(t.dd_rows);
    t.total_bytes -= t.dd_bytes;
    t.dd_bytes = 0;
}

template <typename T>
void adj_dd_apply(AdjTapeDev& t, int mode, const T* d_x, const T* d_rw, const T* d_pw, T* d_out) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_dd_prepare(t);
    hipStream_t s = t.stream;
    if (mode != 1 && t.n_pairs > 0) {
        dd_pairs_kernel<T><<<blocks_for(t.n_pairs), ADJ_THREADS, 0, s>>>(t.dd_a, t.dd_b, mode == 2 ? d_pw : nullptr, d_x, t.n_pairs,
                                                                         mode == 0 ? d_out : (T*)t.dd_u);
        ADJ_CHECK(hipGetLastError());
    }
    if (mode != 0 && t.n_rows > 0) {
        dd_rows_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, s>>>(t.dd_off, t.dd_ent, mode == 1 ? d_x : (const T*)t.dd_u,
                                                                       mode == 2 ? d_rw : nullptr, mode == 2 ? d_x : nullptr, t.n_rows, d_out);
        ADJ_CHECK(hipGetLastError());
    }
}

template <typename T>
const T* adj_row_operator(AdjTapeDev& t, const RowOp<T>& op, T* d_w) {
    if (!op.pw) {
        if (op.rw && t.n_rows > 0) {
            tan_scale_rows_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, t.stream>>>(op.rw, d_w, t.n_rows);
            ADJ_CHECK(hipGetLastError());
        }
        return d_w;
    }
    adj_dd_apply<T>(t, 2, d_w, op.rw, op.pw, (T*)t.dd_rows);
    return (const T*)t.dd_rows;
}

template <typename T>
void adj_gn(AdjTapeDev& t, const T* d_v, const RowOp<T>& op, T* d_out, int schedule, int* passes_jvp, int* passes_vjp) {
    T* w = (T*)t.w_tmp;
    *passes_jvp = adj_jvp<T>(t, d_v, w, nullptr, schedule);
    *passes_vjp = adj_vjp<T>(t, adj_row_operator<T>(t, op, w), nullptr, d_out, schedule);
}

// ---- second-order products
size_t adj_hold_bytes(const AdjTapeDev& t) { return 2 * t.n_events * t.nn * t.elem; }

void adj_release_hold(AdjTapeDev& t) {
    if (!t.hold_lam && !t.hess_dd) return;
    (void)hipSetDevice(t.device);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    const size_t each = std::max<size_t>(t.n_events * t.nn * t.elem, 1);
    if (t.hold_lam) { dev_free(t.hold_lam); t.total_bytes -= each; }
    if (t.hess_dd) { dev_free(t.hess_dd); t.total_bytes -= each; }
    t.held = false;
}

template <typename T>
int adj_hold(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, int schedule) {
    ADJ_CHECK(hipSetDevice(t.device));
    const size_t en = t.n_events * t.nn;
    t.held = false;
    if (!t.hold_lam || !t.hess_dd) {
        Alloc alloc{t, adj_hold_bytes(t)};
        try {
            if (!t.hold_lam) alloc(t.hold_lam, en * sizeof(T));
            if (!t.hess_dd) alloc(t.hess_dd, en * sizeof(T));
        } catch (...) {
            adj_release_hold(t);
            throw;
        }
    }
    const T* lam = nullptr;
    const int passes = adj_vjp_model<T>(t, d_w, d_fc, d_grad, schedule, &lam);
    if (en > 0) ADJ_CHECK(hipMemcpyAsync(t.hold_lam, lam, en * sizeof(T), hipMemcpyDeviceToDevice, t.stream));
    t.held = true;
    return passes;
}

// tangent relaxation of v -> dD and q from final values (q written into g, the seeds of the relaxation that follows) -> adjoint relaxation
// of lam2 for the field cotangent q (newton: and the rows rw * J v) -> gradient with the direct term; a cell or model tape ends with
// the transposed map
template <typename T>
void adj_hess(AdjTapeDev& t, const T* d_v, const RowOp<T>& op, bool newton, T* d_out, int schedule, int* passes_jvp, int* passes_vjp) {
    if (!t.held) throw std::invalid_argument("no held cotangent: call hold first");
    hipStream_t s = t.stream;
    const size_t E = t.n_events, en = E * t.nn;
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    T* w = (T*)t.w_tmp;
    const T* mu = nullptr;
    const T* v_nodes = nullptr;
    *passes_jvp = adj_jvp_impl<T>(t, d_v, newton ? w : nullptr, nullptr, schedule, &mu, &v_nodes);
    const T* rows = newton ? adj_row_operator<T>(t, op, w) : nullptr;
    if (en > 0) {
        const dim3 grid(blocks_for(t.nn), (unsigned)E);
        hess_dd_kernel<T><<<grid, ADJ_THREADS, 0, s>>>((const T*)t.fields, t.frozen, mu, geo, (T*)t.hess_dd);
        ADJ_CHECK(hipGetLastError());
        hess_q_kernel<T><<<grid, ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.inmask, (const T*)t.hold_lam, mu,
                                                     (const T*)t.hess_dd, geo, (T*)t.g);
        ADJ_CHECK(hipGetLastError());
    }
    const T* lam2 = nullptr;
    *passes_vjp = adj_vjp_impl<T>(t, rows, (const T*)t.g, nullptr, schedule, &lam2);
    if (t.nn > 0) {
        T* out_nodes = t.mapped() ? (T*)t.grad_tmp : d_out;   // (a cell or model tape: v_nodes is grad_tmp, overwritten in place)
        hess_grad_kernel<T><<<blocks_for(t.nn), ADJ_THREADS, 0, s>>>(lam2, (const T*)t.hold_lam, (const T*)t.D, (const T*)t.hess_dd, t.frozen,
                                                                    (const T*)t.slowness, v_nodes, geo, E, out_nodes);
        ADJ_CHECK(hipGetLastError());
        if (t.mapped()) adj_nodes_to_model<T>(t, (const T*)t.grad_tmp, d_out);
    }
}

// ---- derivatives with respect to the source points
size_t adj_src_extra_bytes(const AdjTapeDev& t) {
    const size_t n_ent = t.h_src_key.size();
    return (t.n_points + 1) * sizeof(int) + n_ent * (2 * sizeof(int) + sizeof(long long) + 3 * t.elem) + 16 * t.n_points * t.elem +
           4 * t.n_rows * t.elem;
}
size_t adj_src_column_bytes(const AdjTapeDev& t) { return 4 * t.n_events * t.nn * t.elem; }

template <typename T>
void adj_src_prepare(AdjTapeDev& t) {
    if (t.src_off) return;
    ADJ_CHECK(hipSetDevice(t.device));
    Alloc alloc{t, adj_src_extra_bytes(t)};
    const size_t before = t.total_bytes;
    const size_t n_ent = t.h_src_key.size();
    try {
        alloc(t.src_off, (t.n_points + 1) * sizeof(int));
        alloc(t.src_pt, n_ent * sizeof(int));
        alloc(t.src_key, n_ent * sizeof(long long));
        alloc(t.src_node, n_ent * sizeof(int));
        alloc(t.src_c, 3 * n_ent * sizeof(T));
        alloc(t.src_io, 16 * t.n_points * sizeof(T));
        alloc(t.src_rows, 4 * t.n_rows * sizeof(T));
        std::vector<int> pt(n_ent), node(n_ent);
        for (size_t q = 0; q < t.n_points; ++q)
            for (int i = t.h_src_off[q]; i < t.h_src_off[q + 1]; ++i) {
                pt[i] = (int)q;
                node[i] = (int)(t.h_src_key[i] - (long long)((size_t)t.h_pt_event[q] * t.nn));
            }
        const std::vector<T> c(t.h_src_c.begin(), t.h_src_c.end());
        ADJ_CHECK(hipMemcpyAsync(t.src_off, t.h_src_off.data(), (t.n_points + 1) * sizeof(int), hipMemcpyHostToDevice, t.stream));
        if (n_ent > 0) {
            ADJ_CHECK(hipMemcpyAsync(t.src_pt, pt.data(), n_ent * sizeof(int), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.src_key, t.h_src_key.data(), n_ent * sizeof(long long), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.src_node, node.data(), n_ent * sizeof(int), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.src_c, c.data(), 3 * n_ent * sizeof(T), hipMemcpyHostToDevice, t.stream));
        }
        ADJ_CHECK(hipStreamSynchronize(t.stream));   // (the host vectors leave scope)
    } catch (...) {
        dev_free(t.src_off); dev_free(t.src_pt); dev_free(t.src_key); dev_free(t.src_node); dev_free(t.src_c); dev_free(t.src_io);
        dev_free(t.src_rows);
        t.total_bytes = before;
        throw;
    }
}

template <typename T, int K>
static int adj_jvp_source_k(AdjTapeDev& t, const T* d_dsrc, int n_cols, T* d_dtt, T* d_dfields, int schedule, const T** mu_out) {
    using V = SrcVec<T, K>;
    hipStream_t s = t.stream;
    const size_t E = t.n_events, en = E * t.nn, n_ent = t.h_src_key.size();
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    V* mu = (V*)(K == 1 ? t.lam : t.mu4);
    V* mu2 = (V*)(K == 1 ? t.lam2 : t.mu4b);
    const V* fin = mu;
    int passes = 0;
    if (en > 0) {
        ADJ_CHECK(hipMemsetAsync(mu, 0, en * sizeof(V), s));   // (+0: any start reaches the fixed point)
        if (schedule != 0) ADJ_CHECK(hipMemsetAsync(mu2, 0, en * sizeof(V), s));
        if (n_ent > 0)
            for (V* buf : {mu, schedule != 0 ? mu2 : (V*)nullptr}) {
                if (!buf) continue;
                src_seed_kernel<T, K><<<blocks_for(n_ent), ADJ_THREADS, 0, s>>>(t.src_key, t.src_node, t.src_pt, (const T*)t.src_c, n_ent,
                                                                               (const T*)t.slowness, d_dsrc, n_cols, t.n_points, buf);
                ADJ_CHECK(hipGetLastError());
            }
        if (schedule == 0) ADJ_CHECK(hipMemsetAsync(t.tan_stamps, 0xFF, E * t.n_tan_tiles * sizeof(int), s));
        constexpr int ed = TanTile<T>::edge;
        const int ntx = (t.nnx + ed - 1) / ed, nty = (t.nny + ed - 1) / ed, ntz = (t.nnz + ed - 1) / ed;
        const unsigned tiles = (unsigned)t.n_tan_tiles;
        V* in = mu;
        V* out = mu2;
        passes = relax_to_fixed_point(t, "source tangent", [&](int pass, const int* prev, int* cur) {
            if (schedule == 0) {
                src_tiled_kernel<T, K, ed><<<dim3(tiles, (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.frozen, mu, geo,
                                                                                           ntx, nty, ntz, t.tan_stamps, pass, cur);
            } else {
                src_jacobi_kernel<T, K><<<dim3(blocks_for(t.nn), (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.frozen,
                                                                                                   in, out, geo, prev, cur);
                std::swap(in, out);
            }
        });
        if (schedule != 0) fin = in;   // (the buffer the last pass wrote; both hold the fixed point)
    }
    if (d_dtt && t.n_rows > 0) {
        src_rows_kernel<T, K><<<blocks_for(t.n_rows * (size_t)n_cols), ADJ_THREADS, 0, s>>>(t.rw_off, t.rw_key, (const T*)t.rw_w, t.n_rows,
                                                                                           n_cols, (const T*)fin, d_dtt);
        ADJ_CHECK(hipGetLastError());
    }
    if (d_dfields && en > 0) {
        src_unpack_kernel<T, K><<<std::min(blocks_for(en * (size_t)n_cols), 65536u), ADJ_THREADS, 0, s>>>((const T*)fin, en, n_cols, d_dfields);
        ADJ_CHECK(hipGetLastError());
    }
    if (mu_out) *mu_out = (const T*)fin;
    return passes;
}

template <typename T>
int adj_jvp_source(AdjTapeDev& t, const T* d_dsrc, int n_cols, T* d_dtt, T* d_dfields, int schedule, const T** mu_out, int* k_out) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_jvp_prepare<T>(t);   // (the stencil in row order and the stamps of the tangent tiles)
    adj_src_prepare<T>(t);
    const int K = n_cols > 1 ? 4 : 1;
    if (k_out) *k_out = K;
    if (K == 1) return adj_jvp_source_k<T, 1>(t, d_dsrc, n_cols, d_dtt, d_dfields, schedule, mu_out);
    for (void** buf : {&t.mu4, schedule != 0 ? &t.mu4b : (void**)nullptr}) {
        if (!buf || *buf) continue;
        Alloc alloc{t, adj_src_column_bytes(t)};
        alloc(*buf, adj_src_column_bytes(t));
    }
    return adj_jvp_source_k<T, 4>(t, d_dsrc, n_cols, d_dtt, d_dfields, schedule, mu_out);
}

template <typename T>
int adj_vjp_source(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, T* d_gsrc, int schedule) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_src_prepare<T>(t);
    const T* lam = nullptr;
    const int passes = adj_vjp_model<T>(t, d_w, d_fc, d_grad, schedule, &lam);
    if (t.n_points > 0) {
        if (t.n_events * t.nn == 0) {
            ADJ_CHECK(hipMemsetAsync(d_gsrc, 0, 4 * t.n_points * sizeof(T), t.stream));
        } else {
            src_grad_kernel<T><<<blocks_for(t.n_points), ADJ_THREADS, 0, t.stream>>>(t.src_off, t.src_key, t.src_node, (const T*)t.src_c,
                                                                                    t.n_points, (const T*)t.slowness, lam, d_gsrc);
            ADJ_CHECK(hipGetLastError());
        }
    }
    return passes;
}

// ---- joint hypocentre-velocity products
template <typename T>
int adj_jvp_joint(AdjTapeDev& t, const T* d_ds, const T* d_dsrc, T* d_dtt, T* d_dfields, int schedule, const T** mu_out) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_jvp_prepare<T>(t);
    adj_src_prepare<T>(t);
    hipStream_t s = t.stream;
    const size_t E = t.n_events, en = E * t.nn, n_ent = t.h_src_key.size();
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    if (t.mapped()) {   // the node perturbation: what set_slowness would compute from the cell perturbation, or P d_ds
        adj_model_to_nodes<T>(t, d_ds, (T*)t.grad_tmp);
        d_ds = (const T*)t.grad_tmp;
    }
    T* mu = (T*)t.lam;
    T* mu2 = schedule != 0 ? (T*)t.lam2 : nullptr;
    int passes = 0;
    if (en > 0) {
        ADJ_CHECK(hipMemsetAsync(mu, 0, en * sizeof(T), s));
        if (mu2) ADJ_CHECK(hipMemsetAsync(mu2, 0, en * sizeof(T), s));
        if (n_ent > 0) {
            joint_seed_kernel<T><<<blocks_for(n_ent), ADJ_THREADS, 0, s>>>(t.src_key, t.src_node, t.src_pt, (const T*)t.src_c, n_ent,
                                                                          (const T*)t.slowness, (const T*)t.D, d_ds, d_dsrc, mu, mu2);
            ADJ_CHECK(hipGetLastError());
        }
        if (schedule == 0) ADJ_CHECK(hipMemsetAsync(t.tan_stamps, 0xFF, E * t.n_tan_tiles * sizeof(int), s));
        constexpr int ed = TanTile<T>::edge;
        const int ntx = (t.nnx + ed - 1) / ed, nty = (t.nny + ed - 1) / ed, ntz = (t.nnz + ed - 1) / ed;
        const unsigned tiles = (unsigned)t.n_tan_tiles;
        T* in = mu;
        T* out = (T*)t.lam2;
        passes = relax_to_fixed_point(t, "joint tangent", [&](int pass, const int* prev, int* cur) {
            if (schedule == 0) {
                tan_tiled_kernel<T, ed, true><<<dim3(tiles, (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.frozen,
                                                                                              (const T*)t.slowness, d_ds, mu, geo, ntx, nty,
                                                                                              ntz, t.tan_stamps, pass, cur);
            } else {
                tan_jacobi_kernel<T, true><<<dim3(blocks_for(t.nn), (unsigned)E), ADJ_THREADS, 0, s>>>(
                    (const T*)t.fields, (const T*)t.D, t.frozen, (const T*)t.slowness, d_ds, in, out, geo, prev, cur);
                std::swap(in, out);
            }
        });
        if (schedule != 0) mu = in;   // (the buffer the last pass wrote; both hold the fixed point)
    }
    if (d_dtt && t.n_rows > 0) {
        tan_rows_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, s>>>(t.rw_off, t.rw_key, (const T*)t.rw_w, t.n_rows, mu, d_dtt);
        ADJ_CHECK(hipGetLastError());
    }
    if (d_dfields && en > 0) ADJ_CHECK(hipMemcpyAsync(d_dfields, mu, en * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (mu_out) *mu_out = mu;
    return passes;
}

template <typename T>
void adj_gn_joint(AdjTapeDev& t, const T* d_vs, const T* d_ve, const T* d_scale, T* d_ve_scaled, const RowOp<T>& op, T* d_gs, T* d_ge,
                  int schedule, int* passes_jvp, int* passes_vjp) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_src_prepare<T>(t);
    if (d_scale) {
        adj_scale<T>(t, d_scale, d_ve, d_ve_scaled, 4 * t.n_points);
        d_ve = d_ve_scaled;
    }
    T* w = (T*)t.w_tmp;
    *passes_jvp = adj_jvp_joint<T>(t, d_vs, d_ve, w, nullptr, schedule, nullptr);
    *passes_vjp = adj_vjp_source<T>(t, adj_row_operator<T>(t, op, w), nullptr, d_gs, d_ge, schedule);
    if (d_scale) adj_scale<T>(t, d_scale, d_ge, d_ge, 4 * t.n_points);
}

// ---- derivatives with respect to the receiver points
void adj_rcv_set_points(AdjTapeDev& t, const int* point_of_row, size_t n_points) {
    adj_rcv_release(t);   // (what is on the device belongs to the old map)
    t.h_mv_pts.clear();   // (... and the points of the last move to the old points)
    t.h_rcv_pt.assign(point_of_row, point_of_row + t.n_rows);
    t.n_rcv_points = n_points;
    t.h_rcv_off.assign(n_points + 1, 0);
    for (size_t r = 0; r < t.n_rows; ++r) t.h_rcv_off[t.h_rcv_pt[r] + 1] += 1;
    for (size_t q = 0; q < n_points; ++q) t.h_rcv_off[q + 1] += t.h_rcv_off[q];
    t.h_rcv_rows.assign(t.n_rows, 0);
    std::vector<int> fill(t.h_rcv_off.begin(), t.h_rcv_off.end() - 1);
    for (size_t r = 0; r < t.n_rows; ++r) t.h_rcv_rows[fill[t.h_rcv_pt[r]]++] = (int)r;   // (rows ascending within a point)
}

size_t adj_rcv_extra_bytes(const AdjTapeDev& t) {
    auto at_least_1 = [](size_t b) { return std::max<size_t>(b, 1); };
    return at_least_1(3 * t.n_rows * t.elem) + 3 * at_least_1(t.n_rows * sizeof(int)) + at_least_1((t.n_rcv_points + 1) * sizeof(int)) +
           at_least_1(3 * t.n_rows * t.elem) + at_least_1(t.n_rows * t.elem) + at_least_1(16 * t.n_rcv_points * t.elem);
}

template <typename T>
static RcvGeom<T> rcv_geom(const AdjTapeDev& t) {
    RcvGeom<T> g;
    g.nn[0] = t.nnx; g.nn[1] = t.nny; g.nn[2] = t.nnz;
    g.nodes = t.nn;
    g.dx = (T)t.dx;
    for (int a = 0; a < 3; ++a) { g.cmin[a] = (T)t.rcv_min[a]; g.shift[a] = (T)t.rcv_shift[a]; }
    return g;
}

template <typename T>
void adj_rcv_prepare(AdjTapeDev& t) {
    if (t.rcv_p) return;
    ADJ_CHECK(hipSetDevice(t.device));
    Alloc alloc{t, adj_rcv_extra_bytes(t)};
    const size_t before = t.total_bytes;
    try {
        alloc(t.rcv_p, 3 * t.n_rows * sizeof(T));
        alloc(t.rcv_event, t.n_rows * sizeof(int));
        alloc(t.rcv_pt, t.n_rows * sizeof(int));
        alloc(t.rcv_rows, t.n_rows * sizeof(int));
        alloc(t.rcv_off, (t.n_rcv_points + 1) * sizeof(int));
        alloc(t.rcv_G, 3 * t.n_rows * sizeof(T));
        alloc(t.rcv_tt, t.n_rows * sizeof(T));
        alloc(t.rcv_io, 16 * t.n_rcv_points * sizeof(T));
        const std::vector<T> p(t.h_rcv_p.begin(), t.h_rcv_p.end());
        ADJ_CHECK(hipMemcpyAsync(t.rcv_off, t.h_rcv_off.data(), (t.n_rcv_points + 1) * sizeof(int), hipMemcpyHostToDevice, t.stream));
        if (t.n_rows > 0) {
            ADJ_CHECK(hipMemcpyAsync(t.rcv_p, p.data(), 3 * t.n_rows * sizeof(T), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.rcv_event, t.h_rcv_event.data(), t.n_rows * sizeof(int), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.rcv_pt, t.h_rcv_pt.data(), t.n_rows * sizeof(int), hipMemcpyHostToDevice, t.stream));
            ADJ_CHECK(hipMemcpyAsync(t.rcv_rows, t.h_rcv_rows.data(), t.n_rows * sizeof(int), hipMemcpyHostToDevice, t.stream));
            // G (and tt) of the tape's rows: computed once, kept with the receiver arrays
            rcv_eval_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, t.stream>>>((const T*)t.fields, (const T*)t.rcv_p, t.rcv_event, t.n_rows,
                                                                                  rcv_geom<T>(t), 0, (T*)t.rcv_tt, (T*)t.rcv_G);
            ADJ_CHECK(hipGetLastError());
        }
        ADJ_CHECK(hipStreamSynchronize(t.stream));   // (p leaves scope)
    } catch (...) {
        dev_free(t.rcv_p); dev_free(t.rcv_event); dev_free(t.rcv_pt); dev_free(t.rcv_rows); dev_free(t.rcv_off); dev_free(t.rcv_G);
        dev_free(t.rcv_tt); dev_free(t.rcv_io);
        t.total_bytes = before;
        throw;
    }
    t.rcv_bytes = t.total_bytes - before;
}

void* adj_rcv_stage(AdjTapeDev& t, size_t bytes) {
    if (bytes <= t.rcv_stage_bytes && t.rcv_stage) return t.rcv_stage;
    ADJ_CHECK(hipSetDevice(t.device));
    dev_free(t.rcv_stage);
    t.total_bytes -= t.rcv_stage_bytes;
    t.rcv_stage_bytes = 0;
    Alloc alloc{t, bytes};
    alloc(t.rcv_stage, bytes);
    t.rcv_stage_bytes = std::max<size_t>(bytes, 1);
    return t.rcv_stage;
}

void adj_rcv_release(AdjTapeDev& t) {
    adj_cg_release(t, CG_RECEIVER);
    adj_cg_release(t, CG_RELOC);
    if (!t.rcv_p && !t.rcv_stage) return;
    (void)hipSetDevice(t.device);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    dev_free(t.rcv_stage);
    t.total_bytes -= t.rcv_stage_bytes;
    t.rcv_stage_bytes = 0;
    if (!t.rcv_p) return;
    dev_free(t.rcv_p); dev_free(t.rcv_event); dev_free(t.rcv_pt); dev_free(t.rcv_rows); dev_free(t.rcv_off); dev_free(t.rcv_G);
    dev_free(t.rcv_tt); dev_free(t.rcv_io);
    t.total_bytes -= t.rcv_bytes;
    t.rcv_bytes = 0;
}

template <typename T>
void adj_rcv_eval(AdjTapeDev& t, size_t n, const T* d_pts, const int* d_event, bool shift, T* d_tt, T* d_grad) {
    ADJ_CHECK(hipSetDevice(t.device));
    if (!d_pts) {   // the tape's own rows: evaluated by adj_rcv_prepare
        adj_rcv_prepare<T>(t);
        if (d_tt && t.n_rows > 0) ADJ_CHECK(hipMemcpyAsync(d_tt, t.rcv_tt, t.n_rows * sizeof(T), hipMemcpyDeviceToDevice, t.stream));
        if (d_grad && t.n_rows > 0) ADJ_CHECK(hipMemcpyAsync(d_grad, t.rcv_G, 3 * t.n_rows * sizeof(T), hipMemcpyDeviceToDevice, t.stream));
        return;
    }
    if (n == 0) return;
    rcv_eval_kernel<T><<<blocks_for(n), ADJ_THREADS, 0, t.stream>>>((const T*)t.fields, d_pts, d_event, n, rcv_geom<T>(t), shift ? 1 : 0, d_tt,
                                                                   d_grad);
    ADJ_CHECK(hipGetLastError());
}

template <typename T>
void adj_jvp_rcv(AdjTapeDev& t, const T* d_drcv, const T* d_base, T* d_dtt) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_rcv_prepare<T>(t);
    if (t.n_rows == 0) return;
    rcv_rows_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, t.stream>>>(t.rcv_pt, (const T*)t.rcv_G, d_drcv, t.n_rows, d_base, d_dtt);
    ADJ_CHECK(hipGetLastError());
}

template <typename T>
void adj_vjp_rcv(AdjTapeDev& t, const T* d_w, T* d_grcv) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_rcv_prepare<T>(t);
    if (t.n_rcv_points == 0) return;
    rcv_grad_kernel<T><<<blocks_for(4 * t.n_rcv_points), ADJ_THREADS, 0, t.stream>>>(t.rcv_off, t.rcv_rows, (const T*)t.rcv_G, d_w,
                                                                                    t.n_rcv_points, d_grcv);
    ADJ_CHECK(hipGetLastError());
}

// ---- moving the receiver points, and the relocation-only product
template <typename T>
const char* adj_rcv_move_error(const AdjTapeDev& t, const T* h_pts) {
    for (size_t q = 0; q < t.n_rcv_points; ++q)
        for (int a = 0; a < 3; ++a) {
            const T v = h_pts[3 * q + a];
            if (!std::isfinite((double)v)) return "xyz: a coordinate that is not finite";
            const T p = v - (T)t.rcv_shift[a];
            if (p < (T)t.rcv_min[a] || p > (T)t.rcv_max[a]) return "Receiver outside grid";
        }
    return nullptr;
}

namespace {
int mv_end_bit(const AdjTapeDev& t) {   // the bits of the largest key, event * nn + node
    unsigned long long top = (unsigned long long)t.n_events * t.nn;
    int bits = 1;
    while (bits < 64 && (top >> bits) != 0) ++bits;
    return bits;
}
size_t mv_sort_need(const AdjTapeDev& t, size_t n) {
    size_t bytes = 0;
    ADJ_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const long long*)nullptr, (long long*)nullptr, (const int*)nullptr,
                                                 (int*)nullptr, n, 0, mv_end_bit(t), t.stream));
    return std::max<size_t>(bytes, 1);
}
}  // namespace

size_t adj_rcv_move_bytes(const AdjTapeDev& t) {
    const size_t cap = 8 * t.n_rows;
    auto at_least_1 = [](size_t b) { return std::max<size_t>(b, 1); };
    return 2 * at_least_1(cap * sizeof(long long)) + 2 * at_least_1(cap * t.elem) + 4 * at_least_1(cap * sizeof(int)) + mv_sort_need(t, cap);
}

// the first move: room for 8 entries per row in the seed list and the row-order list (the old arrays, sized by the first stencils,
// leave), the three index arrays and the sort's workspace.  The stream is idle (every entry waits for it before it returns).
static void mv_prepare(AdjTapeDev& t) {
    if (t.mv_row) return;
    const size_t cap = 8 * t.n_rows;
    Alloc alloc{t, adj_rcv_move_bytes(t)};
    const size_t before = t.total_bytes;
    long long *k1 = nullptr, *k2 = nullptr;
    int* r1 = nullptr;
    void *w1 = nullptr, *w2 = nullptr;
    try {
        alloc(k1, cap * sizeof(long long));
        alloc(r1, cap * sizeof(int));
        alloc(w1, cap * t.elem);
        alloc(k2, cap * sizeof(long long));
        alloc(w2, cap * t.elem);
        alloc(t.mv_row, cap * sizeof(int));
        alloc(t.mv_idx, cap * sizeof(int));
        alloc(t.mv_perm, cap * sizeof(int));
        t.mv_sort_bytes = mv_sort_need(t, cap);
        alloc(t.mv_sort, t.mv_sort_bytes);
    } catch (...) {
        dev_free(k1); dev_free(r1); dev_free(w1); dev_free(k2); dev_free(w2);
        dev_free(t.mv_row); dev_free(t.mv_idx); dev_free(t.mv_perm); dev_free(t.mv_sort);
        t.mv_sort_bytes = 0;
        t.total_bytes = before;
        throw;
    }
    auto was = [](size_t b) { return std::max<size_t>(b, 1); };   // (what Alloc counted for the arrays that leave)
    t.total_bytes -= 2 * was(t.n_seed * sizeof(long long)) + was(t.n_seed * sizeof(int)) + 2 * was(t.n_seed * t.elem);
    dev_free(t.sd_key); dev_free(t.sd_row); dev_free(t.sd_w); dev_free(t.rw_key); dev_free(t.rw_w);
    t.sd_key = k1; t.sd_row = r1; t.sd_w = w1; t.rw_key = k2; t.rw_w = w2;
    t.mv_cap = cap;
}

template <typename T>
void adj_rcv_move(AdjTapeDev& t, const T* h_pts, const T* d_pts, T* d_tt) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_rcv_prepare<T>(t);
    adj_jvp_prepare<T>(t);   // (the row-order list lives on the device from here on)
    mv_prepare(t);
    adj_release_hold(t);     // (the held adjoint belongs to the old stencils)
    hipStream_t s = t.stream;
    const size_t n_pts = t.n_rcv_points;
    // host: the stencil of every point as the kernel will compute it -- the offsets of the row-order list come from its counts --, and
    // the mirrors of what the device rebuilds
    std::vector<int> cnt(n_pts);
    std::vector<long long> nd(8 * n_pts);
    std::vector<T> wt(8 * n_pts), ps(3 * n_pts);
    for (size_t q = 0; q < n_pts; ++q) {
        for (int a = 0; a < 3; ++a) ps[3 * q + a] = h_pts[3 * q + a] - (T)t.rcv_shift[a];
        cnt[q] = interp3d_stencil<T>(ps[3 * q], ps[3 * q + 1], ps[3 * q + 2], t.nnx, t.nny, t.nnz, (T)t.dx, (T)t.rcv_min[0], (T)t.rcv_min[1],
                                     (T)t.rcv_min[2], &nd[8 * q], &wt[8 * q]);
    }
    for (size_t r = 0; r < t.n_rows; ++r) t.h_rw_off[r + 1] = t.h_rw_off[r] + cnt[t.h_rcv_pt[r]];
    const size_t n_seed = t.n_rows > 0 ? (size_t)t.h_rw_off[t.n_rows] : 0;
    t.h_rw_key.resize(n_seed);
    t.h_rw_w.resize(n_seed);
    for (size_t r = 0; r < t.n_rows; ++r) {
        const size_t q = (size_t)t.h_rcv_pt[r], o = (size_t)t.h_rw_off[r];
        for (int c = 0; c < cnt[q]; ++c) {
            t.h_rw_key[o + c] = (long long)((size_t)t.h_rcv_event[r] * t.nn) + nd[8 * q + c];
            t.h_rw_w[o + c] = (double)wt[8 * q + c];
        }
        for (int a = 0; a < 3; ++a) t.h_rcv_p[3 * r + a] = (double)ps[3 * q + a];
    }
    t.h_mv_pts.assign(h_pts, h_pts + 3 * n_pts);
    t.n_seed = n_seed;
    if (t.n_rows > 0) {
        ADJ_CHECK(hipMemcpyAsync(t.rw_off, t.h_rw_off.data(), (t.n_rows + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (!d_pts) {
            ADJ_CHECK(hipMemcpyAsync(t.rcv_io, h_pts, 3 * n_pts * sizeof(T), hipMemcpyHostToDevice, s));
            d_pts = (const T*)t.rcv_io;
        }
        ADJ_CHECK(hipMemsetAsync(t.err, 0, sizeof(int), s));
        rcv_move_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, s>>>((const T*)t.fields, d_pts, t.rcv_pt, t.rcv_event, t.rw_off, t.n_rows,
                                                                      rcv_geom<T>(t), (T*)t.rcv_p, (T*)t.rcv_tt, (T*)t.rcv_G, t.rw_key,
                                                                      (T*)t.rw_w, t.mv_row, t.mv_idx, t.err);
        ADJ_CHECK(hipGetLastError());
        if (n_seed > 0) {
            size_t bytes = mv_sort_need(t, n_seed);
            if (bytes > t.mv_sort_bytes) throw std::logic_error("move_receiver_points: the sort asks for more workspace than at its capacity");
            bytes = t.mv_sort_bytes;
            ADJ_CHECK(hipcub::DeviceRadixSort::SortPairs(t.mv_sort, bytes, (const long long*)t.rw_key, t.sd_key, (const int*)t.mv_idx,
                                                         t.mv_perm, n_seed, 0, mv_end_bit(t), s));
            rcv_move_gather_kernel<T><<<blocks_for(n_seed), ADJ_THREADS, 0, s>>>(t.mv_perm, t.mv_row, (const T*)t.rw_w, n_seed, t.sd_row,
                                                                                (T*)t.sd_w);
            ADJ_CHECK(hipGetLastError());
        }
        if (d_tt) ADJ_CHECK(hipMemcpyAsync(d_tt, t.rcv_tt, t.n_rows * sizeof(T), hipMemcpyDeviceToDevice, s));
        int h_err = 0;
        ADJ_CHECK(hipMemcpyAsync(&h_err, t.err, sizeof(int), hipMemcpyDeviceToHost, s));
        ADJ_CHECK(hipStreamSynchronize(s));
        if (h_err) throw std::runtime_error("move_receiver_points: internal error, the stencil of a row differs between the host and the device");
    }
}

template <typename T>
void adj_gn_reloc(AdjTapeDev& t, const T* d_ve, const T* d_scale, T* d_ve_scaled, const RowOp<T>& op, T* d_ge) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_rcv_prepare<T>(t);
    const size_t blk = 4 * t.n_rcv_points;
    if (d_scale) {
        adj_scale<T>(t, d_scale, d_ve, d_ve_scaled, blk);
        d_ve = d_ve_scaled;
    }
    T* w = (T*)t.w_tmp;
    adj_jvp_rcv<T>(t, d_ve, nullptr, w);
    const T* rows = adj_row_operator<T>(t, op, w);
    adj_vjp_rcv<T>(t, rows, d_ge);
    if (d_scale) adj_scale<T>(t, d_scale, d_ge, d_ge, blk);
}

template <typename T>
void adj_scale(AdjTapeDev& t, const T* d_c, const T* d_in, T* d_out, size_t n) {
    if (n == 0) return;
    joint_scale_kernel<T><<<blocks_for(n), ADJ_THREADS, 0, t.stream>>>(d_c, d_in, d_out, n);
    ADJ_CHECK(hipGetLastError());
}

template <typename T>
int adj_jvp_rjoint(AdjTapeDev& t, const T* d_ds, const T* d_drcv, T* d_dtt, T* d_dfields, int schedule) {
    const int passes = adj_jvp<T>(t, d_ds, d_dtt, d_dfields, schedule);
    if (d_dtt) adj_jvp_rcv<T>(t, d_drcv, d_dtt, d_dtt);
    return passes;
}

template <typename T>
void adj_gn_rjoint(AdjTapeDev& t, const T* d_vs, const T* d_ve, const T* d_scale, T* d_ve_scaled, const RowOp<T>& op, T* d_gs, T* d_ge,
                   int schedule, int* passes_jvp, int* passes_vjp) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_rcv_prepare<T>(t);
    const size_t blk = 4 * t.n_rcv_points;
    if (d_scale) {
        adj_scale<T>(t, d_scale, d_ve, d_ve_scaled, blk);
        d_ve = d_ve_scaled;
    }
    T* w = (T*)t.w_tmp;
    *passes_jvp = adj_jvp_rjoint<T>(t, d_vs, d_ve, w, nullptr, schedule);
    const T* rows = adj_row_operator<T>(t, op, w);
    adj_vjp_rcv<T>(t, rows, d_ge);
    *passes_vjp = adj_vjp<T>(t, rows, nullptr, d_gs, schedule);
    if (d_scale) adj_scale<T>(t, d_scale, d_ge, d_ge, blk);
}


// ---- block products
size_t adj_block_bytes(const AdjTapeDev& t) {
    return (t.mu4 ? 1 : 2) * adj_src_column_bytes(t) + 4 * t.n_model() * t.elem + (t.mapped() ? 4 * t.nn * t.elem : 0) + 8 * t.n_rows * t.elem;
}

template <typename T>
void adj_block_prepare(AdjTapeDev& t) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_jvp_prepare<T>(t);   // (the stencil in row order and the stamps of the tangent tiles)
    if (t.g4) return;
    Alloc alloc{t, adj_block_bytes(t)};
    const size_t before = t.total_bytes;
    const bool had_mu4 = t.mu4 != nullptr;
    try {
        alloc(t.g4, adj_src_column_bytes(t));
        if (!had_mu4) alloc(t.mu4, adj_src_column_bytes(t));
        alloc(t.blk_model, 4 * t.n_model() * t.elem);
        if (t.mapped()) alloc(t.blk_nodes, 4 * t.nn * t.elem);
        alloc(t.blk_rows, 4 * t.n_rows * t.elem);
        alloc(t.blk_rw, 4 * t.n_rows * t.elem);
    } catch (...) {
        dev_free(t.g4); dev_free(t.blk_model); dev_free(t.blk_nodes); dev_free(t.blk_rows); dev_free(t.blk_rw);
        if (!had_mu4) dev_free(t.mu4);
        t.total_bytes = before;
        throw;
    }
    t.blk_owns_mu4 = !had_mu4;
    t.blk_bytes = t.total_bytes - before;
}

void adj_block_release(AdjTapeDev& t) {
    if (!t.g4) return;
    (void)hipSetDevice(t.device);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    dev_free(t.g4); dev_free(t.blk_model); dev_free(t.blk_nodes); dev_free(t.blk_rows); dev_free(t.blk_rw);
    if (t.blk_owns_mu4) dev_free(t.mu4);
    t.blk_owns_mu4 = false;
    t.total_bytes -= t.blk_bytes;
    t.blk_bytes = 0;
}

template <typename T>
int adj_jvp_block(AdjTapeDev& t, const T* d_ds, int n_cols, T* d_dtt, T* d_dfields, int schedule) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_block_prepare<T>(t);
    const size_t E = t.n_events, en = E * t.nn;
    if (schedule != 0) {   // the Jacobi baseline, column by column
        int passes = 0;
        for (int k = 0; k < n_cols; ++k)
            passes += adj_jvp<T>(t, d_ds + (size_t)k * t.n_model(), d_dtt ? d_dtt + (size_t)k * t.n_rows : nullptr,
                                 d_dfields ? d_dfields + (size_t)k * en : nullptr, schedule);
        return passes;
    }
    constexpr int K = 4;
    using V = SrcVec<T, K>;
    hipStream_t s = t.stream;
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    if (t.mapped()) {   // column by column, the node perturbation: set_slowness's from the cell perturbation, or P of the column
        for (int k = 0; k < n_cols; ++k) adj_model_to_nodes<T>(t, d_ds + (size_t)k * t.n_model(), (T*)t.blk_nodes + (size_t)k * t.nn);
        d_ds = (const T*)t.blk_nodes;
    }
    V* mu = (V*)t.mu4;
    int passes = 0;
    if (en > 0) {
        ADJ_CHECK(hipMemsetAsync(mu, 0, en * sizeof(V), s));   // (+0: any start reaches the fixed point)
        ADJ_CHECK(hipMemsetAsync(t.tan_stamps, 0xFF, E * t.n_tan_tiles * sizeof(int), s));
        constexpr int ed = TanTile<T>::edge;
        const int ntx = (t.nnx + ed - 1) / ed, nty = (t.nny + ed - 1) / ed, ntz = (t.nnz + ed - 1) / ed;
        const unsigned tiles = (unsigned)t.n_tan_tiles;
        passes = relax_to_fixed_point(t, "block tangent", [&](int pass, const int*, int* cur) {
            tank_tiled_kernel<T, K, ed><<<dim3(tiles, (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.frozen,
                                                                                        (const T*)t.slowness, d_ds, n_cols, mu, geo, ntx, nty,
                                                                                        ntz, t.tan_stamps, pass, cur);
        });
    }
    if (d_dtt && t.n_rows > 0) {
        src_rows_kernel<T, K><<<blocks_for(t.n_rows * (size_t)n_cols), ADJ_THREADS, 0, s>>>(t.rw_off, t.rw_key, (const T*)t.rw_w, t.n_rows,
                                                                                           n_cols, (const T*)mu, d_dtt);
        ADJ_CHECK(hipGetLastError());
    }
    if (d_dfields && en > 0) {
        src_unpack_kernel<T, K><<<std::min(blocks_for(en * (size_t)n_cols), 65536u), ADJ_THREADS, 0, s>>>((const T*)mu, en, n_cols, d_dfields);
        ADJ_CHECK(hipGetLastError());
    }
    return passes;
}

template <typename T>
int adj_vjp_block(AdjTapeDev& t, const T* d_w, int n_cols, T* d_grad, int schedule) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_block_prepare<T>(t);
    const size_t E = t.n_events, en = E * t.nn;
    if (schedule != 0) {   // the Jacobi baseline, column by column
        int passes = 0;
        for (int k = 0; k < n_cols; ++k)
            passes += adj_vjp<T>(t, d_w + (size_t)k * t.n_rows, nullptr, d_grad + (size_t)k * t.n_model(), schedule);
        return passes;
    }
    constexpr int K = 4;
    using V = SrcVec<T, K>;
    hipStream_t s = t.stream;
    const AdjGeom<T> geo{t.nnx, t.nny, t.nnz, t.nn, (T)t.dx};
    V* g = (V*)t.g4;
    V* lam = (V*)t.mu4;
    int passes = 0;
    if (en > 0) {
        ADJ_CHECK(hipMemsetAsync(g, 0, en * sizeof(V), s));
        if (t.n_seed > 0) {
            adjk_seed_rows_kernel<T, K><<<blocks_for(t.n_seed), ADJ_THREADS, 0, s>>>(t.sd_key, t.sd_row, (const T*)t.sd_w, t.n_seed, d_w,
                                                                                    t.n_rows, n_cols, g);
            ADJ_CHECK(hipGetLastError());
        }
        ADJ_CHECK(hipMemcpyAsync(lam, g, en * sizeof(V), hipMemcpyDeviceToDevice, s));
        ADJ_CHECK(hipMemsetAsync(t.tan_stamps, 0xFF, E * t.n_tan_tiles * sizeof(int), s));
        constexpr int ed = TanTile<T>::edge;
        const int ntx = (t.nnx + ed - 1) / ed, nty = (t.nny + ed - 1) / ed, ntz = (t.nnz + ed - 1) / ed;
        const unsigned tiles = (unsigned)t.n_tan_tiles;
        passes = relax_to_fixed_point(t, "block adjoint", [&](int pass, const int*, int* cur) {
            adjk_tiled_kernel<T, K, ed><<<dim3(tiles, (unsigned)E), ADJ_THREADS, 0, s>>>((const T*)t.fields, (const T*)t.D, t.inmask, g, lam, geo,
                                                                                        ntx, nty, ntz, t.tan_stamps, pass, cur);
        });
    }
    if (t.nn > 0) {
        // a cell or model tape forms the node gradients of the group in blk_nodes, then d_grad = the transposed map of each
        T* gn = t.mapped() ? (T*)t.blk_nodes : d_grad;
        adjk_grad_kernel<T, K><<<blocks_for(t.nn), ADJ_THREADS, 0, s>>>(lam, (const T*)t.D, t.frozen, (const T*)t.slowness, geo, E, n_cols, gn);
        ADJ_CHECK(hipGetLastError());
        if (t.mapped())
            for (int k = 0; k < n_cols; ++k) adj_nodes_to_model<T>(t, gn + (size_t)k * t.nn, d_grad + (size_t)k * t.n_model());
    }
    return passes;
}

template <typename T>
void adj_gn_block(AdjTapeDev& t, const T* d_v, const T* d_rw, size_t rw_stride, int n_cols, T* d_out, int schedule, int* passes_jvp,
                  int* passes_vjp) {
    ADJ_CHECK(hipSetDevice(t.device));
    adj_block_prepare<T>(t);
    T* w = (T*)t.blk_rows;
    *passes_jvp = adj_jvp_block<T>(t, d_v, n_cols, w, nullptr, schedule);
    if (d_rw && t.n_rows > 0)
        for (int k = 0; k < n_cols; ++k) {
            tan_scale_rows_kernel<T><<<blocks_for(t.n_rows), ADJ_THREADS, 0, t.stream>>>(d_rw + (size_t)k * rw_stride, w + (size_t)k * t.n_rows,
                                                                                        t.n_rows);
            ADJ_CHECK(hipGetLastError());
        }
    *passes_vjp = adj_vjp_block<T>(t, w, n_cols, d_out, schedule);
}

template void adj_copy_field<float>(const float*, int, float*, size_t, hipStream_t);
template void adj_copy_field<double>(const double*, int, double*, size_t, hipStream_t);
template void adj_finish<float>(AdjTapeDev&, const AdjSink&);
template void adj_finish<double>(AdjTapeDev&, const AdjSink&);
template void adj_model_to_nodes<float>(AdjTapeDev&, const float*, float*);
template void adj_model_to_nodes<double>(AdjTapeDev&, const double*, double*);
template void adj_nodes_to_model<float>(AdjTapeDev&, const float*, float*);
template void adj_nodes_to_model<double>(AdjTapeDev&, const double*, double*);
template int adj_vjp<float>(AdjTapeDev&, const float*, const float*, float*, int);
template int adj_vjp<double>(AdjTapeDev&, const double*, const double*, double*, int);
template void adj_jvp_prepare<float>(AdjTapeDev&);
template void adj_jvp_prepare<double>(AdjTapeDev&);
template int adj_jvp<float>(AdjTapeDev&, const float*, float*, float*, int);
template int adj_jvp<double>(AdjTapeDev&, const double*, double*, double*, int);
template void adj_dd_apply<float>(AdjTapeDev&, int, const float*, const float*, const float*, float*);
template void adj_dd_apply<double>(AdjTapeDev&, int, const double*, const double*, const double*, double*);
template const float* adj_row_operator<float>(AdjTapeDev&, const RowOp<float>&, float*);
template const double* adj_row_operator<double>(AdjTapeDev&, const RowOp<double>&, double*);
template void adj_gn<float>(AdjTapeDev&, const float*, const RowOp<float>&, float*, int, int*, int*);
template void adj_gn<double>(AdjTapeDev&, const double*, const RowOp<double>&, double*, int, int*, int*);
template int adj_hold<float>(AdjTapeDev&, const float*, const float*, float*, int);
template int adj_hold<double>(AdjTapeDev&, const double*, const double*, double*, int);
template void adj_hess<float>(AdjTapeDev&, const float*, const RowOp<float>&, bool, float*, int, int*, int*);
template void adj_hess<double>(AdjTapeDev&, const double*, const RowOp<double>&, bool, double*, int, int*, int*);

template void adj_src_prepare<float>(AdjTapeDev&);
template void adj_src_prepare<double>(AdjTapeDev&);
template int adj_jvp_source<float>(AdjTapeDev&, const float*, int, float*, float*, int, const float**, int*);
template int adj_jvp_source<double>(AdjTapeDev&, const double*, int, double*, double*, int, const double**, int*);
template int adj_vjp_source<float>(AdjTapeDev&, const float*, const float*, float*, float*, int);
template int adj_vjp_source<double>(AdjTapeDev&, const double*, const double*, double*, double*, int);

template int adj_jvp_joint<float>(AdjTapeDev&, const float*, const float*, float*, float*, int, const float**);
template int adj_jvp_joint<double>(AdjTapeDev&, const double*, const double*, double*, double*, int, const double**);
template void adj_gn_joint<float>(AdjTapeDev&, const float*, const float*, const float*, float*, const RowOp<float>&, float*, float*, int, int*,
                                  int*);
template void adj_gn_joint<double>(AdjTapeDev&, const double*, const double*, const double*, double*, const RowOp<double>&, double*, double*, int, int*,
                                   int*);

template void adj_rcv_prepare<float>(AdjTapeDev&);
template void adj_rcv_prepare<double>(AdjTapeDev&);
template void adj_rcv_eval<float>(AdjTapeDev&, size_t, const float*, const int*, bool, float*, float*);
template void adj_rcv_eval<double>(AdjTapeDev&, size_t, const double*, const int*, bool, double*, double*);
template void adj_jvp_rcv<float>(AdjTapeDev&, const float*, const float*, float*);
template void adj_jvp_rcv<double>(AdjTapeDev&, const double*, const double*, double*);
template void adj_vjp_rcv<float>(AdjTapeDev&, const float*, float*);
template void adj_vjp_rcv<double>(AdjTapeDev&, const double*, double*);
template const char* adj_rcv_move_error<float>(const AdjTapeDev&, const float*);
template const char* adj_rcv_move_error<double>(const AdjTapeDev&, const double*);
template void adj_rcv_move<float>(AdjTapeDev&, const float*, const float*, float*);
template void adj_rcv_move<double>(AdjTapeDev&, const double*, const double*, double*);
template void adj_gn_reloc<float>(AdjTapeDev&, const float*, const float*, float*, const RowOp<float>&, float*);
template void adj_gn_reloc<double>(AdjTapeDev&, const double*, const double*, double*, const RowOp<double>&, double*);
template void adj_scale<float>(AdjTapeDev&, const float*, const float*, float*, size_t);
template void adj_scale<double>(AdjTapeDev&, const double*, const double*, double*, size_t);
template int adj_jvp_rjoint<float>(AdjTapeDev&, const float*, const float*, float*, float*, int);
template int adj_jvp_rjoint<double>(AdjTapeDev&, const double*, const double*, double*, double*, int);
template void adj_gn_rjoint<float>(AdjTapeDev&, const float*, const float*, const float*, float*, const RowOp<float>&, float*, float*, int, int*,
                                   int*);
template void adj_gn_rjoint<double>(AdjTapeDev&, const double*, const double*, const double*, double*, const RowOp<double>&, double*, double*, int, int*,
                                    int*);

template void adj_block_prepare<float>(AdjTapeDev&);
template void adj_block_prepare<double>(AdjTapeDev&);
template int adj_jvp_block<float>(AdjTapeDev&, const float*, int, float*, float*, int);
template int adj_jvp_block<double>(AdjTapeDev&, const double*, int, double*, double*, int);
template int adj_vjp_block<float>(AdjTapeDev&, const float*, int, float*, int);
template int adj_vjp_block<double>(AdjTapeDev&, const double*, int, double*, int);
template void adj_gn_block<float>(AdjTapeDev&, const float*, const float*, size_t, int, float*, int, int*, int*);
template void adj_gn_block<double>(AdjTapeDev&, const double*, const double*, size_t, int, double*, int, int*, int*);

}  // namespace ttcr_amd
