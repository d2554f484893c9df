// ttcr_amd/csrc/fsm_model.hip -- the coarse model grid of a field tape (tests/model_reference.py restates it): the trilinear
// prolongation P from mx x my x mz model nodes onto the nx x ny x nz nodes of the grid, and its transpose.
//
// Per axis and fine index i (64-bit integers): q = i (m - 1), I = q div (n - 1), r = q mod (n - 1); the last fine node takes I = m - 2,
// r = n - 1; wl = T((n - 1 - r) / (n - 1)), wh = T(r / (n - 1)), each quotient taken in double and rounded to T once.  m = 1: I = 0, wl = 1
// and no upper term (wh = 0).  The three axes' I, wl and wh are formed on the host and uploaded once (ModelMap): n_x + n_y + n_z entries.
// A term whose weight is exactly 0 is left out of every sum, so m = n gives the identity bit for bit.
//
// P:    one thread per fine node: lerp_x over the four x-pairs of the eight surrounding model nodes, lerp_y over the two pairs of results,
//       lerp_z; lerp(a, b) = the sum, lower index first, of the non-zero-weight terms fl(wl a), fl(wh b).
// P^T:  three stages, z first (stage z reads the node-sized array coalesced along x; the other two run on small arrays).  One thread per
//       output element; its support on the axis is a contiguous index range, found in O(1); a serial sum over it in ascending order,
//       starting from the first term.  No atomics.
// Compiled with -ffp-contract=off: every product and sum is rounded in T.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <sstream>
#include <vector>

#include "fsm_adjoint_api.h"

#define MDL_CHECK(expr)                                                                                           \
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

constexpr int MDL_THREADS = 256;

unsigned mdl_blocks(size_t n) { return (unsigned)((n + MDL_THREADS - 1) / MDL_THREADS); }

// the tables of one axis as the kernels see them: lower model index and the two weights of every fine index
template <typename T>
struct MdlAxis {
    const int* idx;
    const T* wl;
    const T* wh;
    int n, m;
};

template <typename T>
struct MdlAxes {
    MdlAxis<T> x, y, z;
};

template <typename T>
MdlAxes<T> mdl_axes(const ModelMap& map) {
    MdlAxes<T> a;
    MdlAxis<T>* ax[3] = {&a.x, &a.y, &a.z};
    const size_t tot = (size_t)map.n[0] + map.n[1] + map.n[2];
    size_t off = 0;
    for (int d = 0; d < 3; ++d) {
        ax[d]->idx = map.idx + off;
        ax[d]->wl = (const T*)map.w + off;
        ax[d]->wh = (const T*)map.w + tot + off;
        ax[d]->n = map.n[d];
        ax[d]->m = map.m[d];
        off += (size_t)map.n[d];
    }
    return a;
}

// the sum, lower index first, of the non-zero-weight terms fl(wl a), fl(wh b)
template <typename T>
__device__ __forceinline__ T mdl_lerp(T wl, T wh, T a, T b) {
    if (wh == T(0)) return wl * a;
    if (wl == T(0)) return wh * b;
    return wl * a + wh * b;
}

// s = P v: one thread per fine node.  The upper model node of an axis is read only where its weight is not 0 (m = 1 has none).
template <typename T>
__global__ __launch_bounds__(MDL_THREADS) void mdl_prolong_kernel(const T* __restrict__ v, T* __restrict__ s, MdlAxes<T> ax) {
    const size_t nn = (size_t)ax.x.n * ax.y.n * ax.z.n;
    const size_t node = blockIdx.x * (size_t)MDL_THREADS + threadIdx.x;
    if (node >= nn) return;
    const int i = (int)(node % ax.x.n), j = (int)((node / ax.x.n) % ax.y.n), k = (int)(node / ((size_t)ax.x.n * ax.y.n));
    const int I = ax.x.idx[i], J = ax.y.idx[j], K = ax.z.idx[k];
    const T xl = ax.x.wl[i], xh = ax.x.wh[i], yl = ax.y.wl[j], yh = ax.y.wh[j], zl = ax.z.wl[k], zh = ax.z.wh[k];
    const size_t mx = (size_t)ax.x.m, mxy = mx * ax.y.m;
    T cz[2] = {T(0), T(0)};
    for (int c = 0; c < 2; ++c) {
        if (c == 1 && zh == T(0)) break;
        T cy[2] = {T(0), T(0)};
        for (int b = 0; b < 2; ++b) {
            if (b == 1 && yh == T(0)) break;
            const T* row = v + (size_t)(K + c) * mxy + (size_t)(J + b) * mx + I;
            cy[b] = mdl_lerp<T>(xl, xh, row[0], xh == T(0) ? T(0) : row[1]);
        }
        cz[c] = mdl_lerp<T>(yl, yh, cy[0], cy[1]);
    }
    s[node] = mdl_lerp<T>(zl, zh, cz[0], cz[1]);
}

// One stage of P^T along an axis of n fine and m model indices.  The input is [outer][n][inner], the output [outer][m][inner] (inner the
// product of the faster extents, outer of the slower ones); one thread per output element.  Model index K gathers the fine k with
// I(k) == K (weight wl) or I(k) + 1 == K (weight wh): k (m - 1) / (n - 1) in [K - 1, K + 1), a contiguous range.  Ascending k, the sum
// starts from its first non-zero-weight term.
template <typename T>
__global__ __launch_bounds__(MDL_THREADS) void mdl_restrict_kernel(const T* __restrict__ g, T* __restrict__ out, MdlAxis<T> ax, size_t inner,
                                                                   size_t outer) {
    const size_t total = inner * (size_t)ax.m * outer;
    const size_t o = blockIdx.x * (size_t)MDL_THREADS + threadIdx.x;
    if (o >= total) return;
    const size_t in = o % inner, hi_part = o / inner;
    const int K = (int)(hi_part % (size_t)ax.m);
    const size_t ou = hi_part / (size_t)ax.m;
    int lo = 0, hi = ax.n - 1;
    if (ax.m > 1) {
        const long long n1 = ax.n - 1, m1 = ax.m - 1;
        const long long a = ((long long)(K - 1) * n1 + m1 - 1) / m1;   // ceil((K - 1) (n - 1) / (m - 1)) for K >= 1
        const long long b = ((long long)(K + 1) * n1 + m1 - 1) / m1 - 1;
        lo = K >= 1 ? (int)a : 0;
        hi = (int)(b < n1 ? b : n1);
    }
    const T* col = g + ou * (size_t)ax.n * inner + in;
    T acc = T(0);
    bool first = true;
    for (int k = lo; k <= hi; ++k) {
        const int I = ax.idx[k];
        T w = T(0);
        if (I == K) w = ax.wl[k];
        else if (I + 1 == K) w = ax.wh[k];
        if (w == T(0)) continue;
        const T p = w * col[(size_t)k * inner];
        acc = first ? p : acc + p;
        first = false;
    }
    out[o] = acc;
}

}  // namespace

size_t model_map_bytes(const int n[3], size_t elem) {
    const size_t tot = (size_t)n[0] + n[1] + n[2];
    return std::max<size_t>(tot * sizeof(int), 1) + std::max<size_t>(2 * tot * elem, 1);
}

void model_axis_stencil(int i, int n, int m, int* I, double* wl, double* wh) {
    if (m == 1) {
        *I = 0; *wl = 1.0; *wh = 0.0;
        return;
    }
    const long long q = (long long)i * (m - 1);
    long long lo = q / (n - 1), r = q % (n - 1);
    if (lo == m - 1) { lo = m - 2; r = n - 1; }
    *I = (int)lo;
    *wl = (double)(n - 1 - r) / (double)(n - 1);
    *wh = (double)r / (double)(n - 1);
}

template <typename T>
void model_map_create(ModelMap& map, const int n[3], const int m[3]) {
    const size_t tot = (size_t)n[0] + n[1] + n[2];
    std::vector<int> idx(tot);
    std::vector<T> w(2 * tot);
    size_t off = 0;
    for (int d = 0; d < 3; ++d) {
        map.n[d] = n[d];
        map.m[d] = m[d];
        for (int i = 0; i < n[d]; ++i) {
            double wl, wh;
            model_axis_stencil(i, n[d], m[d], &idx[off + i], &wl, &wh);
            w[off + i] = (T)wl;
            w[tot + off + i] = (T)wh;
        }
        off += (size_t)n[d];
    }
    const size_t planned = model_map_bytes(n, sizeof(T));
    void* raw[2] = {nullptr, nullptr};
    const size_t want[2] = {std::max<size_t>(tot * sizeof(int), 1), std::max<size_t>(2 * tot * sizeof(T), 1)};
    for (int a = 0; a < 2; ++a)
        if (hipMalloc(&raw[a], want[a]) != hipSuccess) {
            (void)hipGetLastError();
            if (raw[0]) (void)hipFree(raw[0]);
            std::ostringstream msg;
            msg << "the model grid's axis tables need " << planned << " bytes of device memory (an allocation of " << want[a]
                << " bytes failed)";
            throw AdjDeviceError(msg.str());
        }
    map.idx = (int*)raw[0];
    map.w = raw[1];
    map.bytes = want[0] + want[1];
    try {
        if (tot > 0) {
            MDL_CHECK(hipMemcpy(map.idx, idx.data(), tot * sizeof(int), hipMemcpyHostToDevice));
            MDL_CHECK(hipMemcpy(map.w, w.data(), 2 * tot * sizeof(T), hipMemcpyHostToDevice));
        }
    } catch (...) {
        model_map_free(map);
        throw;
    }
}

void model_map_free(ModelMap& map) {
    if (map.idx) (void)hipFree(map.idx);
    if (map.w) (void)hipFree(map.w);
    map.idx = nullptr;
    map.w = nullptr;
    map.bytes = 0;
}

template <typename T>
void model_prolong(const ModelMap& map, const T* d_v, T* d_s, hipStream_t stream) {
    const size_t nn = map.n_fine();
    if (nn == 0) return;
    mdl_prolong_kernel<T><<<mdl_blocks(nn), MDL_THREADS, 0, stream>>>(d_v, d_s, mdl_axes<T>(map));
    MDL_CHECK(hipGetLastError());
}

template <typename T>
void model_restrict(const ModelMap& map, const T* d_g, T* d_a, T* d_b, T* d_gm, hipStream_t stream) {
    if (map.n_fine() == 0) return;
    const MdlAxes<T> ax = mdl_axes<T>(map);
    const size_t nx = map.n[0], ny = map.n[1], my = map.m[1], mz = map.m[2];
    // stage z: [1][nz][nx ny] -> [1][mz][nx ny];  stage y: [mz][ny][nx] -> [mz][my][nx];  stage x: [my mz][nx][1] -> [my mz][mx][1]
    mdl_restrict_kernel<T><<<mdl_blocks(nx * ny * mz), MDL_THREADS, 0, stream>>>(d_g, d_a, ax.z, nx * ny, 1);
    MDL_CHECK(hipGetLastError());
    mdl_restrict_kernel<T><<<mdl_blocks(nx * my * mz), MDL_THREADS, 0, stream>>>(d_a, d_b, ax.y, nx, mz);
    MDL_CHECK(hipGetLastError());
    mdl_restrict_kernel<T><<<mdl_blocks(map.n_model()), MDL_THREADS, 0, stream>>>(d_b, d_gm, ax.x, 1, my * mz);
    MDL_CHECK(hipGetLastError());
}

template void model_map_create<float>(ModelMap&, const int[3], const int[3]);
template void model_map_create<double>(ModelMap&, const int[3], const int[3]);
template void model_prolong<float>(const ModelMap&, const float*, float*, hipStream_t);
template void model_prolong<double>(const ModelMap&, const double*, double*, hipStream_t);
template void model_restrict<float>(const ModelMap&, const float*, float*, float*, float*, hipStream_t);
template void model_restrict<double>(const ModelMap&, const double*, double*, double*, double*, hipStream_t);

}  // namespace ttcr_amd
