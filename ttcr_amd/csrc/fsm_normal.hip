// ttcr_amd/csrc/fsm_normal.hip -- translation unit of the field tape's normal-equation solver: the smoothing operator
// R v = sum_d a_d K_d^T (K_d v) on the tape's model vector, the inner product with a fixed summation order, and conjugate gradients on
// (H + lam R + mu I) x = b with H the tape's Gauss-Newton (or Newton) product; see fsm_adjoint_api.h.  tests/normal_reference.py restates
// all of it in numpy.  The same solver runs the joint hypocentre-velocity system (6j) and the receiver joint system (6k), whose vectors
// carry an extra block behind the model vector (tests/joint_reference.py, tests/receiver_reference.py), and the relocation-only system
// (6o), whose vector is the receiver block alone (tests/relocation_reference.py).  Compiled with -ffp-contract=off like every other unit: each product, difference, quotient and sum below is
// rounded on its own, in the order the definition writes them.  No floating-point atomics.
#include "fsm_adjoint_api.h"

#include <algorithm>
#include <cmath>
#include <sstream>
#include <string>
#include <type_traits>

#define NRM_CHECK(expr)                                                                                           \
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

constexpr int NRM_THREADS = 256;
constexpr int NRM_CHUNK = 1024;   // elements of a chunk partial: one workgroup, four elements per thread
// interior edge of a smoothing tile: with its two-node halo the tile of v takes (edge + 4)^3 * sizeof(T) bytes of LDS -- 31.25 KiB
// (fp32, 20^3) and 32 KiB (fp64, 16^3)
template <typename T> struct NrmTile;
template <> struct NrmTile<float> { static constexpr int edge = 16; };
template <> struct NrmTile<double> { static constexpr int edge = 12; };

// what the update kernels read from device memory, and what the host reads once per iteration
struct NrmCtl {
    double rho;      // <r, r> of the current residual
    double pq;       // <p, q> of the running iteration
    double alpha;    // T(rho / pq), held exactly
    double beta;     // T(rho_new / rho), held exactly
    double sum;      // the last plain inner product (rho0; adj_dot)
    int ok;          // pq > 0 and finite: the update kernels of the iteration run
};

enum NrmClose { NRM_PLAIN, NRM_RR0, NRM_PQ, NRM_RR };

struct NrmDims {
    int mx, my, mz;   // parameters along x, y, z (x fastest)
};

// one axis of K^T K v at the parameter whose value is c[0]: c[o * sd] is the parameter o steps along the axis (|o| <= 2, inside the
// grid), i its index on the axis and n the length of the axis (>= 3).  Rows in ascending order, the sum starts from its first term.
template <typename T>
__device__ __forceinline__ T nrm_axis(const T* c, int sd, int i, int n, T ih2, T m2ih2) {
    auto y = [&](int r) {
        const int o = min(max(r, 1), n - 2) - i;
        return ((c[(o - 1) * sd] + c[(o + 1) * sd]) - T(2) * c[o * sd]) * ih2;
    };
    T z = T(0);
    bool first = true;
    auto add = [&](T term) {
        z = first ? term : z + term;
        first = false;
    };
    if (i <= 2) add((i == 1 ? m2ih2 : ih2) * y(0));
    for (int r = max(i - 1, 1); r <= min(i + 1, n - 2); ++r) add((r == i ? m2ih2 : ih2) * y(r));
    if (i >= n - 3) add((i == n - 2 ? m2ih2 : ih2) * y(n - 1));
    return z;
}

template <typename T>
struct NrmSmooth {
    NrmDims g;
    T ihx, ihy, ihz;   // T(1 / h_d^2) per axis, h_d the spacing of the parameters along it (node and cell tapes: dx on all three)
    T ax, ay, az;      // the weights of the axes
    int ex, ey, ez;    // the axis is evaluated (node and cell tapes: all three; a model tape leaves out an axis with fewer than 3 nodes)
};

// (R v) at the parameter (gx, gy, gz) whose value is c[0]; sx, sy, sz are the strides of the three axes in the array c points into
template <typename T>
__device__ __forceinline__ T nrm_smooth_at(const T* c, int sx, int sy, int sz, int gx, int gy, int gz, const NrmSmooth<T>& sm) {
    // the left-to-right sum over the evaluated axes in x, y, z order, starting from its first term: (ax zx + ay zy) + az zz with all three
    T z = T(0);
    bool first = true;
    auto add = [&](T term) {
        z = first ? term : z + term;
        first = false;
    };
    if (sm.ex) add(sm.ax * nrm_axis<T>(c, sx, gx, sm.g.mx, sm.ihx, T(-2) * sm.ihx));
    if (sm.ey) add(sm.ay * nrm_axis<T>(c, sy, gy, sm.g.my, sm.ihy, T(-2) * sm.ihy));
    if (sm.ez) add(sm.az * nrm_axis<T>(c, sz, gz, sm.g.mz, sm.ihz, T(-2) * sm.ihz));
    return z;
}

// out = R v: one workgroup per tile of TI^3 parameters; the tile of v with a two-node halo (cut at the faces of the grid) sits in LDS,
// y is recomputed from it.  Thread t owns the interior parameters t + 256 q, x fastest.
template <typename T, int TI>
__global__ __launch_bounds__(NRM_THREADS) void nrm_smooth_kernel(const T* __restrict__ v, T* __restrict__ out, NrmSmooth<T> sm, int ntx,
                                                                 int nty) {
    const NrmDims g = sm.g;
    constexpr int P = TI + 4;   // pitch of a row, rows of a plane
    __shared__ T tile[P * P * P];
    const int tx = blockIdx.x % ntx, ty = (blockIdx.x / ntx) % nty, tz = blockIdx.x / (ntx * nty);
    const int x0 = tx * TI, y0 = ty * TI, z0 = tz * TI;
    for (int l = threadIdx.x; l < P * P * P; l += NRM_THREADS) {
        const int gx = x0 - 2 + l % P, gy = y0 - 2 + (l / P) % P, gz = z0 - 2 + l / (P * P);
        const bool in = gx >= 0 && gx < g.mx && gy >= 0 && gy < g.my && gz >= 0 && gz < g.mz;
        tile[l] = in ? v[((size_t)gz * g.my + gy) * g.mx + gx] : T(0);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < TI * TI * TI; q += NRM_THREADS) {
        const int lx = q % TI, ly = (q / TI) % TI, lz = q / (TI * TI);
        const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
        if (gx >= g.mx || gy >= g.my || gz >= g.mz) continue;
        const T* c = tile + ((lz + 2) * P + (ly + 2)) * P + (lx + 2);
        out[((size_t)gz * g.my + gy) * g.mx + gx] = nrm_smooth_at<T>(c, 1, P, P * P, gx, gy, gz, sm);
    }
}

// the chunk partial of a workgroup from the four elements e0 .. e3 of thread t (elements t, t + 256, t + 512, t + 768 of the chunk):
// ((e0 + e1) + e2) + e3, then s[t] += s[t + stride] for stride = 128 .. 1
__device__ __forceinline__ void nrm_chunk_partial(double e0, double e1, double e2, double e3, double* __restrict__ partial) {
    __shared__ double s[NRM_THREADS];
    const int t = threadIdx.x;
    s[t] = ((e0 + e1) + e2) + e3;
    __syncthreads();
    for (int stride = NRM_THREADS / 2; stride >= 1; stride >>= 1) {
        if (t < stride) s[t] += s[t + stride];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = s[0];
}

__device__ __forceinline__ double nrm_prod(float a, float b) { return (double)a * (double)b; }
__device__ __forceinline__ double nrm_prod(double a, double b) { return a * b; }

// chunk partials of <a, b>
template <typename T>
__global__ __launch_bounds__(NRM_THREADS) void nrm_dot_kernel(const T* __restrict__ a, const T* __restrict__ b, size_t n,
                                                              double* __restrict__ partial) {
    double e[4];
    for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)blockIdx.x * NRM_CHUNK + threadIdx.x + (size_t)k * NRM_THREADS;
        e[k] = i < n ? nrm_prod(a[i], b[i]) : 0.0;
    }
    nrm_chunk_partial(e[0], e[1], e[2], e[3], partial);
}

// kernel 1 of an iteration at a parameter of the model vector: q = fl(fl(hp + fl(lam * (R p))) + fl(mu * p)) (the smoothing term only if
// with_smooth, the damping term only if with_damp).  A workgroup owns a chunk of the flat vector, as the partials demand, so the smoothing
// gather reads p around each of its parameters from global memory (the expression is nrm_smooth_kernel's: nrm_smooth_at on other strides)
template <typename T>
__device__ __forceinline__ T nrm_combine_at(const T* __restrict__ hp, const T* __restrict__ p, size_t i, T pi, const NrmSmooth<T>& sm, T lam,
                                            T mu, int with_smooth, int with_damp) {
    T a = hp[i];
    if (with_smooth) {
        const int gx = (int)(i % sm.g.mx), gy = (int)((i / sm.g.mx) % sm.g.my), gz = (int)(i / ((size_t)sm.g.mx * sm.g.my));
        a = a + lam * nrm_smooth_at<T>(p + i, 1, sm.g.mx, sm.g.mx * sm.g.my, gx, gy, gz, sm);
    }
    if (with_damp) a = a + mu * pi;
    return a;
}

// kernel 1 over the n_joint elements of the flat vector of a system: below n_model the expression above, in the block behind it (DESIGN.md
// 6j) q = fl(hp + fl(delta * p)) (delta null: q = hp); the chunk partials of <p, q> with the block seam wherever it falls in a chunk.  The
// model system has no block: n_joint == n_model and a null delta.
template <typename T>
__global__ __launch_bounds__(NRM_THREADS) void jnt_combine_kernel(const T* __restrict__ hp, const T* __restrict__ p, T* __restrict__ q,
                                                                  size_t n_model, size_t n_joint, NrmSmooth<T> sm, T lam, T mu,
                                                                  int with_smooth, int with_damp, const T* __restrict__ delta,
                                                                  double* __restrict__ partial) {
    double e[4];
    for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)blockIdx.x * NRM_CHUNK + threadIdx.x + (size_t)k * NRM_THREADS;
        e[k] = 0.0;
        if (i < n_joint) {
            const T pi = p[i];
            T a;
            if (i < n_model) {
                a = nrm_combine_at<T>(hp, p, i, pi, sm, lam, mu, with_smooth, with_damp);
            } else {
                a = hp[i];
                if (delta) a = a + delta[i - n_model] * pi;
            }
            q[i] = a;
            e[k] = nrm_prod(pi, a);
        }
    }
    nrm_chunk_partial(e[0], e[1], e[2], e[3], partial);
}

// the start of a solve: r = rhs (in r on entry), or fl(rhs - q) with q = A x0 if with_x0; p = r; chunk partials of <r, r>
template <typename T>
__global__ __launch_bounds__(NRM_THREADS) void nrm_start_kernel(T* __restrict__ r, const T* __restrict__ q, T* __restrict__ p, size_t n,
                                                                int with_x0, double* __restrict__ partial) {
    double e[4];
    for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)blockIdx.x * NRM_CHUNK + threadIdx.x + (size_t)k * NRM_THREADS;
        e[k] = 0.0;
        if (i < n) {
            T ri = r[i];
            if (with_x0) {
                ri = ri - q[i];
                r[i] = ri;
            }
            p[i] = ri;
            e[k] = nrm_prod(ri, ri);
        }
    }
    nrm_chunk_partial(e[0], e[1], e[2], e[3], partial);
}

// kernel 2: x = fl(x + fl(aT * p)), r = fl(r - fl(aT * q)), chunk partials of <r, r>; nothing at all if the iteration broke down
template <typename T>
__global__ __launch_bounds__(NRM_THREADS) void nrm_update_kernel(T* __restrict__ x, T* __restrict__ r, const T* __restrict__ p,
                                                                 const T* __restrict__ q, size_t n, const NrmCtl* __restrict__ ctl,
                                                                 double* __restrict__ partial) {
    if (!ctl->ok) return;
    const T aT = (T)ctl->alpha;
    double e[4];
    for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)blockIdx.x * NRM_CHUNK + threadIdx.x + (size_t)k * NRM_THREADS;
        e[k] = 0.0;
        if (i < n) {
            x[i] = x[i] + aT * p[i];
            const T ri = r[i] - aT * q[i];
            r[i] = ri;
            e[k] = nrm_prod(ri, ri);
        }
    }
    nrm_chunk_partial(e[0], e[1], e[2], e[3], partial);
}

// kernel 3: p = fl(r + fl(bT * p))
template <typename T>
__global__ __launch_bounds__(NRM_THREADS) void nrm_direction_kernel(const T* __restrict__ r, T* __restrict__ p, size_t n,
                                                                    const NrmCtl* __restrict__ ctl) {
    if (!ctl->ok) return;
    const T bT = (T)ctl->beta;
    const size_t i = (size_t)blockIdx.x * NRM_THREADS + threadIdx.x;
    if (i < n) p[i] = r[i] + bT * p[i];
}

// the finishing reduction, one workgroup: thread t adds the chunk partials t, t + 256, ... ascending from +0, then the halving of the
// chunk rule.  Thread 0 then closes the inner product: the scalars of the recurrence are formed here, on the device, in fp64, and
// alpha / beta are rounded to T.  After a breakdown the <r, r> of the iteration is not closed: rho stays what it was.
template <typename T>
__global__ __launch_bounds__(NRM_THREADS) void nrm_finish_kernel(const double* __restrict__ partial, size_t n_partials, int what,
                                                                 NrmCtl* __restrict__ ctl) {
    if (what == NRM_RR && !ctl->ok) return;
    __shared__ double s[NRM_THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (size_t j = t; j < n_partials; j += NRM_THREADS) acc += partial[j];
    s[t] = acc;
    __syncthreads();
    for (int stride = NRM_THREADS / 2; stride >= 1; stride >>= 1) {
        if (t < stride) s[t] += s[t + stride];
        __syncthreads();
    }
    if (t != 0) return;
    const double sum = s[0];
    if (what == NRM_PLAIN) {
        ctl->sum = sum;
    } else if (what == NRM_RR0) {
        ctl->rho = sum;
    } else if (what == NRM_PQ) {
        ctl->pq = sum;
        ctl->ok = (sum > 0.0 && sum <= 1.7976931348623157e308) ? 1 : 0;
        ctl->alpha = (double)(T)(ctl->rho / sum);
    } else {
        ctl->beta = (double)(T)(sum / ctl->rho);
        ctl->rho = sum;
    }
}

void nrm_free(void*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

void cg_free_all(CgWork& w) {
    nrm_free(w.x); nrm_free(w.r); nrm_free(w.p); nrm_free(w.q); nrm_free(w.hp); nrm_free(w.scale);
    nrm_free(w.damp); nrm_free(w.ve); nrm_free(w.partial); nrm_free(w.ctl);
}

size_t nrm_chunks(size_t n) { return std::max<size_t>(1, (n + NRM_CHUNK - 1) / NRM_CHUNK); }

NrmDims nrm_dims(const AdjTapeDev& t) {
    if (t.model) return NrmDims{t.map.m[0], t.map.m[1], t.map.m[2]};
    const int c = t.cells ? 1 : 0;
    return NrmDims{t.nnx - c, t.nny - c, t.nnz - c};
}

// closes the inner product whose chunk partials a kernel of the system has just written
template <typename T>
void nrm_close(AdjTapeDev& t, CgSystem sys, int what) {
    const CgWork& w = t.cg[sys];
    nrm_finish_kernel<T><<<1, NRM_THREADS, 0, t.stream>>>((const double*)w.partial, nrm_chunks(t.cg_len(sys)), what, (NrmCtl*)w.ctl);
    NRM_CHECK(hipGetLastError());
}

template <typename T>
NrmSmooth<T> nrm_smooth_args(const AdjTapeDev& t, const double* weights) {
    const NrmDims g = nrm_dims(t);
    const T ih2 = (T)(1.0 / (t.dx * t.dx));
    if (!t.model) return NrmSmooth<T>{g, ih2, ih2, ih2, (T)weights[0], (T)weights[1], (T)weights[2], 1, 1, 1};
    // a model tape: spacing h_d = dx (n_d - 1) / (m_d - 1) in double; an axis with fewer than 3 model nodes is not evaluated
    const int n[3] = {t.nnx, t.nny, t.nnz}, m[3] = {g.mx, g.my, g.mz};
    T ih[3];
    int ev[3];
    for (int d = 0; d < 3; ++d) {
        ev[d] = m[d] >= 3 ? 1 : 0;
        const double h = ev[d] ? t.dx * (double)(n[d] - 1) / (double)(m[d] - 1) : t.dx;
        ih[d] = (T)(1.0 / (h * h));
    }
    return NrmSmooth<T>{g, ih[0], ih[1], ih[2], (T)weights[0], (T)weights[1], (T)weights[2], ev[0], ev[1], ev[2]};
}

}  // namespace

const char* adj_smooth_error(const AdjTapeDev& t, const double* weights) {
    const NrmDims g = nrm_dims(t);
    const int m[3] = {g.mx, g.my, g.mz};
    if (!t.model)
        return std::min({m[0], m[1], m[2]}) < 3 ? "smooth: second-order smoothing needs at least 3 parameters along every axis" : nullptr;
    for (int d = 0; d < 3; ++d)
        if (m[d] < 3 && weights[d] != 0.0)
            return "smooth: a model axis with fewer than 3 nodes is left out of the smoothing operator and takes weight 0";
    return nullptr;
}

int adj_smooth_tile_edge(size_t elem) { return elem == 4 ? NrmTile<float>::edge : NrmTile<double>::edge; }

size_t adj_cg_bytes(const AdjTapeDev& t, CgSystem sys) {
    const size_t n = t.cg_len(sys);
    return 5 * std::max<size_t>(n * t.elem, 1) + (sys == CG_MODEL ? 0 : 3 * std::max<size_t>(t.cg_block(sys) * t.elem, 1)) +
           nrm_chunks(n) * sizeof(double) + sizeof(NrmCtl);
}

void adj_cg_prepare(AdjTapeDev& t, CgSystem sys) {
    CgWork& w = t.cg[sys];
    if (w.x) return;
    NRM_CHECK(hipSetDevice(t.device));
    static const char* const what[CG_SYSTEMS] = {"the normal-equation solver", "the joint solver", "the receiver joint solver",
                                                 "the relocation solver"};
    const size_t planned = adj_cg_bytes(t, sys);
    size_t got = 0;
    auto alloc = [&](void*& p, size_t bytes) {
        const size_t b = std::max<size_t>(bytes, 1);
        if (hipMalloc(&p, b) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            std::ostringstream m;
            m << what[sys] << " of the field tape needs " << planned << " bytes of device memory on device " << t.device
              << " (an allocation of " << b << " bytes failed)";
            throw AdjDeviceError(m.str());
        }
        got += b;
    };
    try {
        const size_t vec = t.cg_len(sys) * t.elem, blk = t.cg_block(sys) * t.elem;
        alloc(w.x, vec);
        alloc(w.r, vec);
        alloc(w.p, vec);
        alloc(w.q, vec);
        alloc(w.hp, vec);
        if (sys != CG_MODEL) {
            alloc(w.scale, blk);
            alloc(w.damp, blk);
            alloc(w.ve, blk);
        }
        alloc(w.partial, nrm_chunks(t.cg_len(sys)) * sizeof(double));
        alloc(w.ctl, sizeof(NrmCtl));
    } catch (...) {
        cg_free_all(w);
        throw;
    }
    w.bytes = got;
    t.total_bytes += got;
}

void adj_cg_release(AdjTapeDev& t, CgSystem sys) {
    CgWork& w = t.cg[sys];
    if (!w.x) return;
    (void)hipSetDevice(t.device);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    cg_free_all(w);
    t.total_bytes -= w.bytes;
    w.bytes = 0;
}

template <typename T>
void adj_smooth(AdjTapeDev& t, const T* d_v, const double* weights, T* d_out) {
    const NrmDims g = nrm_dims(t);
    if (const char* bad = adj_smooth_error(t, weights)) throw std::invalid_argument(bad);
    constexpr int ed = NrmTile<T>::edge;
    const int ntx = (g.mx + ed - 1) / ed, nty = (g.my + ed - 1) / ed, ntz = (g.mz + ed - 1) / ed;
    nrm_smooth_kernel<T, ed><<<(unsigned)((size_t)ntx * nty * ntz), NRM_THREADS, 0, t.stream>>>(d_v, d_out, nrm_smooth_args<T>(t, weights), ntx,
                                                                                              nty);
    NRM_CHECK(hipGetLastError());
}

template <typename T>
double adj_dot(AdjTapeDev& t, const T* d_a, const T* d_b) {
    adj_cg_prepare(t, CG_MODEL);
    const CgWork& w = t.cg[CG_MODEL];
    nrm_dot_kernel<T><<<(unsigned)nrm_chunks(t.n_model()), NRM_THREADS, 0, t.stream>>>(d_a, d_b, t.n_model(), (double*)w.partial);
    NRM_CHECK(hipGetLastError());
    nrm_close<T>(t, CG_MODEL, NRM_PLAIN);
    NrmCtl h;
    NRM_CHECK(hipMemcpyAsync(&h, w.ctl, sizeof(h), hipMemcpyDeviceToHost, t.stream));
    NRM_CHECK(hipStreamSynchronize(t.stream));
    return h.sum;
}

template <typename T>
void adj_solve(AdjTapeDev& t, CgSystem sys, const RowOp<T>& rop, const NormalOperator& op, bool with_x0, bool with_scale, bool with_damp,
               int maxiter, double rtol, int schedule, NormalResult& res) {
    if (sys != CG_MODEL && (with_x0 || op.newton))
        throw std::invalid_argument("solve: x0 and the Newton product are offered for the model system only");
    NRM_CHECK(hipSetDevice(t.device));
    adj_cg_prepare(t, sys);
    const CgWork& wk = t.cg[sys];
    hipStream_t s = t.stream;
    const size_t nm = t.cg_model(sys), n = t.cg_len(sys), blk = t.cg_block(sys);   // (nm = 0: the relocation-only system)
    const unsigned chunks = (unsigned)nrm_chunks(n);
    T* x = (T*)wk.x;
    T* r = (T*)wk.r;
    T* p = (T*)wk.p;
    T* q = (T*)wk.q;
    T* hp = (T*)wk.hp;
    const T* c = with_scale ? (const T*)wk.scale : nullptr;
    const T* delta = with_damp ? (const T*)wk.damp : nullptr;
    double* partial = (double*)wk.partial;
    NrmCtl* ctl = (NrmCtl*)wk.ctl;
    // q = A v (v is p of an iteration or x0) and the chunk partials of <v, q>: the product of the system into hp, then kernel 1
    auto apply = [&](const T* v, int* pj, int* pv) {
        if (sys == CG_SOURCE) adj_gn_joint<T>(t, v, v + nm, c, (T*)wk.ve, rop, hp, hp + nm, schedule, pj, pv);
        else if (sys == CG_RECEIVER) adj_gn_rjoint<T>(t, v, v + nm, c, (T*)wk.ve, rop, hp, hp + nm, schedule, pj, pv);
        else if (sys == CG_RELOC) adj_gn_reloc<T>(t, v, c, (T*)wk.ve, rop, hp);   // (no relaxation: the passes stay 0)
        else if (op.newton) adj_hess<T>(t, v, rop, true, hp, schedule, pj, pv);
        else adj_gn<T>(t, v, rop, hp, schedule, pj, pv);
        jnt_combine_kernel<T><<<chunks, NRM_THREADS, 0, s>>>(hp, v, q, nm, n, nrm_smooth_args<T>(t, op.weights), (T)op.smooth, (T)op.damp,
                                                            op.smooth != 0.0, op.damp != 0.0, delta, partial);
        NRM_CHECK(hipGetLastError());
    };
    res = NormalResult();
    // rho0 = <rhs, rhs> (rhs is in r; its block scaled first: (b_s, fl(c * b_e))), then the starting residual, p and rho
    NRM_CHECK(hipMemsetAsync(ctl, 0, sizeof(NrmCtl), s));
    if (c) adj_scale<T>(t, c, r + nm, r + nm, blk);
    nrm_dot_kernel<T><<<chunks, NRM_THREADS, 0, s>>>(r, r, n, partial);
    NRM_CHECK(hipGetLastError());
    nrm_close<T>(t, sys, NRM_PLAIN);
    if (with_x0) apply(x, &res.passes0[0], &res.passes0[1]);
    else if (n > 0) NRM_CHECK(hipMemsetAsync(x, 0, n * sizeof(T), s));
    nrm_start_kernel<T><<<chunks, NRM_THREADS, 0, s>>>(r, q, p, n, with_x0 ? 1 : 0, partial);
    NRM_CHECK(hipGetLastError());
    nrm_close<T>(t, sys, NRM_RR0);
    NrmCtl h;
    NRM_CHECK(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, s));
    NRM_CHECK(hipStreamSynchronize(s));
    const double rho0 = h.sum;
    double rho = h.rho;
    res.rho.push_back(rho0);
    res.rho.push_back(rho);
    res.status = 1;
    for (int k = 1; k <= maxiter; ++k) {
        if (rho <= rtol * rtol * rho0) {
            res.status = 0;
            break;
        }
        int pj = 0, pv = 0;
        apply(p, &pj, &pv);
        res.passes.push_back(pj);
        res.passes.push_back(pv);
        nrm_close<T>(t, sys, NRM_PQ);
        nrm_update_kernel<T><<<chunks, NRM_THREADS, 0, s>>>(x, r, p, q, n, ctl, partial);
        NRM_CHECK(hipGetLastError());
        nrm_close<T>(t, sys, NRM_RR);
        nrm_direction_kernel<T><<<(unsigned)std::max<size_t>(1, (n + NRM_THREADS - 1) / NRM_THREADS), NRM_THREADS, 0, s>>>(r, p, n, ctl);
        NRM_CHECK(hipGetLastError());
        NRM_CHECK(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, s));   // the one host read of the iteration: (rho, pq)
        NRM_CHECK(hipStreamSynchronize(s));
        res.pq.push_back(h.pq);
        if (!h.ok) {   // (the update kernels saw the same flag and left x, r and p alone)
            res.status = 2;
            break;
        }
        rho = h.rho;
        res.rho.push_back(rho);
        ++res.iterations;
    }
    if (c) adj_scale<T>(t, c, x + nm, x + nm, blk);   // x_e = fl(c * z_e)
}

template void adj_smooth<float>(AdjTapeDev&, const float*, const double*, float*);
template void adj_smooth<double>(AdjTapeDev&, const double*, const double*, double*);
template double adj_dot<float>(AdjTapeDev&, const float*, const float*);
template double adj_dot<double>(AdjTapeDev&, const double*, const double*);
template void adj_solve<float>(AdjTapeDev&, CgSystem, const RowOp<float>&, const NormalOperator&, bool, bool, bool, int, double, int, NormalResult&);
template void adj_solve<double>(AdjTapeDev&, CgSystem, const RowOp<double>&, const NormalOperator&, bool, bool, bool, int, double, int, NormalResult&);

}  // namespace ttcr_amd
