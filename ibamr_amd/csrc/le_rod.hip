// le_rod.hip -- Kirchhoff rods on the device: the force and torque of
// IBKirchhoffRodForceGen::computeLagrangianForceAndTorque (IBKirchhoffRodForceGen.cpp:
// 326-527) and the director update of GeneralizedIBMethod::eulerStep / trapezoidalStep
// (GeneralizedIBMethod.cpp:326-447), with their C ABI (ibtk_le_rodgen_*,
// ibtk_le_director_update; include/ibtk_le.h).
//
// Force and torque: one gather kernel, one lane per node, no global atomics -- the
// reason is le_force.hip's: a node's sum has a fixed order.  The reference evaluates rod
// k = 0, 1, ... serially into four scratch vectors and adds them with two
// VecSetValuesBlocked(ADD_VALUES) calls per vector: every curr contribution in ascending
// k, then every next contribution in ascending k (:489-515).  The plan (set_rods, below)
// stores exactly that list per node (CSR, 64-bit row offsets), each entry carrying the
// whole rod, so a lane re-evaluates every rod it touches from the same operands with the
// same instructions: the two ends of a rod see the identical F_half and N_half.  X_next
// and D_next are plain gathers (the reference's MatMult rows hold a single 1.0).
//
// The principal square root of A = sum_i D_next_i D_i^T is a Denman-Beavers iteration on a
// general 3x3 matrix (the triads drift, A is not assumed to be a rotation), with explicit
// inverses, stopped when an iterate moves by less than 2^-40 of its size (the convergence
// is quadratic: the iterate returned is then converged to rounding) and after
// ROD_SQRT_ITERS iterations at the latest -- a compile-time constant, so no input
// lengthens the loop.  sqrt(I) is I exactly.  The reference uses Eigen's Schur route: the
// result agrees to rounding, not bit for bit.
//
// Arithmetic: one rounded operation per reference operation (-ffp-contract=off), Eigen's
// evaluation order for the fixed-size products and sums (left to right).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ibtk_le.h"
#include "le_rod.h"

namespace ibtk_le {

namespace {

constexpr int ROD_BLOCK = 256;
constexpr int ROD_SQRT_ITERS = 20;       // Denman-Beavers cap (3 rad between neighbours needs 10)
constexpr double ROD_SQRT_TOL = 0x1p-40;  // an iterate that moved less than this (relative) ends the loop

__device__ __forceinline__ double dot3(const double* a, const double* b) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// o = m^-1 (row-major 3x3): the adjugate times 1 / det.  The identity maps to itself exactly.
__device__ __forceinline__ void inv3(const double (&m)[9], double (&o)[9]) {
    const double c0 = m[4] * m[8] - m[5] * m[7];
    const double c1 = m[5] * m[6] - m[3] * m[8];
    const double c2 = m[3] * m[7] - m[4] * m[6];
    const double r = 1.0 / ((m[0] * c0 + m[1] * c1) + m[2] * c2);
    o[0] = c0 * r;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * r;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    o[3] = c1 * r;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * r;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    o[6] = c2 * r;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * r;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * r;
}

// Y = the principal square root of A: Y_0 = A, Z_0 = I, Y' = (Y + Z^-1) / 2, Z' = (Z + Y^-1) / 2.
// An A with an eigenvalue on the closed negative real axis has none: Y is then whatever the
// capped loop leaves (it may hold inf or NaN).
__device__ __forceinline__ void sqrt3(const double (&A)[9], double (&Y)[9]) {
    double Z[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int j = 0; j < 9; ++j) Y[j] = A[j];
#pragma unroll 1
    for (int it = 0; it < ROD_SQRT_ITERS; ++it) {
        double Yi[9], Zi[9];
        inv3(Y, Yi);
        inv3(Z, Zi);
        double moved = 0.0, size = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const double y = 0.5 * (Y[j] + Zi[j]);
            moved = fmax(moved, fabs(y - Y[j]));
            size = fmax(size, fabs(y));
            Y[j] = y;
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) Z[j] = 0.5 * (Z[j] + Yi[j]);
        if (moved <= ROD_SQRT_TOL * size) break;
    }
}

// Rod *rp at (X, D): F_half, N_half and c = 0.5 (X_next - X) x F_half
// (IBKirchhoffRodForceGen.cpp:401-469).  Nothing of the rod is live across the root's
// iteration: the triads, the positions and the parameters are read (again) after it, in
// stages -- the compiler barriers keep those loads there --, which holds the kernel under 128
// VGPRs with no scratch.
__device__ __forceinline__ void rod_eval(const RodRec* __restrict__ rp, int curr, int next,
                                         const double* __restrict__ X, const double* __restrict__ D,
                                         double (&Fh)[3], double (&Nh)[3], double (&c)[3]) {
    const long bc = (long)curr, bn = (long)next;
    double S[9];
    {
        // A = sum_i D_next_i D_i^T, added to a zero matrix in i order
        double A[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) v = v + D[bn * 9 + 3 * i + a] * D[bc * 9 + 3 * i + b];
                A[3 * a + b] = v;
            }
        sqrt3(A, S);
    }
    asm volatile("" ::: "memory");
    double Dc[9], Dh[9];  // Dh: rows D1_half, D2_half, D3_half = sqrt_A D_i
#pragma unroll
    for (int j = 0; j < 9; ++j) Dc[j] = D[bc * 9 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) Dh[3 * i + a] = dot3(&S[3 * a], &Dc[3 * i]);
    asm volatile("" ::: "memory");
    const double ds = rp->p[0];
    double dX[3], dX_ds[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        dX[d] = X[bn * 3 + d] - X[bc * 3 + d];
        dX_ds[d] = dX[d] / ds;
    }
    const double F1 = rp->p[4] * dot3(&Dh[0], dX_ds);
    const double F2 = rp->p[5] * dot3(&Dh[3], dX_ds);
    const double F3 = rp->p[6] * (dot3(&Dh[6], dX_ds) - 1.0);
#pragma unroll
    for (int d = 0; d < 3; ++d) Fh[d] = (F1 * Dh[d] + F2 * Dh[3 + d]) + F3 * Dh[6 + d];

    asm volatile("" ::: "memory");
    double dD[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) dD[j] = (D[bn * 9 + j] - Dc[j]) / ds;
    const double N1 = rp->p[1] * (dot3(&dD[3], &Dh[6]) - rp->p[7]);
    const double N2 = rp->p[2] * (dot3(&dD[6], &Dh[0]) - rp->p[8]);
    const double N3 = rp->p[3] * (dot3(&dD[0], &Dh[3]) - rp->p[9]);
#pragma unroll
    for (int d = 0; d < 3; ++d) Nh[d] = (N1 * Dh[d] + N2 * Dh[3 + d]) + N3 * Dh[6 + d];

    const double h[3] = {0.5 * dX[0], 0.5 * dX[1], 0.5 * dX[2]};
    c[0] = h[1] * Fh[2] - h[2] * Fh[1];
    c[1] = h[2] * Fh[0] - h[0] * Fh[2];
    c[2] = h[0] * Fh[1] - h[1] * Fh[0];
}

__global__ __launch_bounds__(ROD_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void k_rodgen(RodGenParams p) {
    __shared__ double sF[ROD_BLOCK * 3];
    __shared__ double sN[ROD_BLOCK * 3];
    const int t = threadIdx.x;
    const long i0 = (long)blockIdx.x * ROD_BLOCK;
    const long i = i0 + t;
    if (i < p.n) {
        const int node = (int)i;
        // the lane's sums live in its LDS row, not in registers: twelve fewer VGPRs across
        // the root's iteration; the order of the adds is the list's all the same
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            sF[t * 3 + d] = 0.0;
            sN[t * 3 + d] = 0.0;
        }
        const RodRec* __restrict__ rp = p.rec + p.off[i];
        const RodRec* const rend = p.rec + p.off[i + 1];
        for (; rp != rend; ++rp) {
            const int curr = rp->curr, next = rp->next;
            double Fh[3], Nh[3], c[3];
            rod_eval(rp, curr, next, p.X, p.D, Fh, Nh, c);
            if (curr == node) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    sF[t * 3 + d] += Fh[d];
                    sN[t * 3 + d] += Nh[d] + c[d];
                }
            } else {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    sF[t * 3 + d] += -Fh[d];
                    sN[t * 3 + d] += -Nh[d] + c[d];
                }
            }
        }
    }
    __syncthreads();
    // the block's rows of F (and of N) are one contiguous run of doubles: every lane stores
    // (and, when accumulating, loads) consecutive 8-byte words, whatever the view's alignment
    const long rows = p.n - i0 < ROD_BLOCK ? p.n - i0 : ROD_BLOCK;
    const int cnt = (int)rows * 3;
    double* __restrict__ Fb = p.F + i0 * 3;
    double* __restrict__ Nb = p.N + i0 * 3;
    for (int j = t; j < cnt; j += ROD_BLOCK) {
        Fb[j] = p.accumulate_F ? Fb[j] + sF[j] : sF[j];
        Nb[j] = p.accumulate_N ? Nb[j] + sN[j] : sN[j];
    }
}

// GeneralizedIBMethod.cpp:344-378 / :410-444, one lane per node.  D_new may be D_cur: a
// lane reads its nine values before it writes them.
template <bool TRAPEZOIDAL>
__global__ __launch_bounds__(ROD_BLOCK) void k_director_update(long n, double dt, const double* D_cur,
                                                               const double* __restrict__ W0,
                                                               const double* __restrict__ W1, double* D_new) {
    const long l = (long)blockIdx.x * ROD_BLOCK + threadIdx.x;
    if (l >= n) return;
    double e[3], D[9];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if constexpr (TRAPEZOIDAL) e[d] = 0.5 * (W0[l * 3 + d] + W1[l * 3 + d]);
        else e[d] = W0[l * 3 + d];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) D[j] = D_cur[l * 9 + j];
    const double norm_e = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    if (norm_e > DBL_EPSILON) {
        const double theta = norm_e * dt;
#pragma unroll
        for (int d = 0; d < 3; ++d) e[d] = e[d] / norm_e;
        const double c_t = cos(theta);
        const double s_t = sin(theta);
        const double R[9] = {c_t + (1.0 - c_t) * e[0] * e[0],        (1.0 - c_t) * e[0] * e[1] - s_t * e[2],
                             (1.0 - c_t) * e[0] * e[2] + s_t * e[1], (1.0 - c_t) * e[1] * e[0] + s_t * e[2],
                             c_t + (1.0 - c_t) * e[1] * e[1],        (1.0 - c_t) * e[1] * e[2] - s_t * e[0],
                             (1.0 - c_t) * e[2] * e[0] - s_t * e[1], (1.0 - c_t) * e[2] * e[1] + s_t * e[0],
                             c_t + (1.0 - c_t) * e[2] * e[2]};
#pragma unroll
        for (int alpha = 0; alpha < 3; ++alpha)
#pragma unroll
            for (int a = 0; a < 3; ++a) D_new[l * 9 + 3 * alpha + a] = dot3(&R[3 * a], &D[3 * alpha]);
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) D_new[l * 9 + j] = D[j];
    }
}

}  // namespace

hipError_t launch_rodgen(const RodGenParams& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const long grid = (p.n + ROD_BLOCK - 1) / ROD_BLOCK;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rodgen, dim3((unsigned)grid), dim3(ROD_BLOCK), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_director_update(long n, double dt, const double* D_cur, const double* W0, const double* W1,
                                  double* D_new, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const long grid = (n + ROD_BLOCK - 1) / ROD_BLOCK;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(ROD_BLOCK);
    if (W1) hipLaunchKernelGGL((k_director_update<true>), g, b, 0, s, n, dt, D_cur, W0, W1, D_new);
    else hipLaunchKernelGGL((k_director_update<false>), g, b, 0, s, n, dt, D_cur, W0, W1, D_new);
    return hipGetLastError();
}

}  // namespace ibtk_le

// ---------------------------------------------------------------------------
// The C ABI.  set_rods builds the per-node lists on the host (a stable counting sort: a
// node's curr entries in ascending k, then its next entries in ascending k) and uploads
// them once; compute is one launch on the context stream.
// ---------------------------------------------------------------------------
using namespace ibtk_le;

#define ROD_HIP_TRY(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return abi_fail(IBTK_LE_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct ibtk_le_rodgen_s {
    ibtk_le_ctx ctx = nullptr;  // NULL: the handle only validates
    int n = 0;                  // nodes
    long long nrods = 0;        // rods in the plan
    long long* off = nullptr;   // device: n + 1 row offsets
    RodRec* rec = nullptr;      // device: 2 nrods records
};

namespace {

// the device and stream of a plan's context
void rg_where(ibtk_le_ctx ctx, int& device, hipStream_t& stream) { abi_ctx_device_stream(ctx, &device, &stream); }

// [a, a + na) and [b, b + nb) bytes share a byte
bool rg_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

}  // namespace

extern "C" int ibtk_le_rodgen_create(ibtk_le_ctx ctx, int n_nodes, ibtk_le_rodgen* out) {
    if (!out) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_create: null out");
    if (n_nodes < 0) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_create: negative node count %d", n_nodes);
    auto* rg = new ibtk_le_rodgen_s();
    rg->ctx = ctx;
    rg->n = n_nodes;
    *out = rg;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_rodgen_destroy(ibtk_le_rodgen rg) {
    if (!rg) return IBTK_LE_OK;
    if (rg->ctx) {
        int device;
        hipStream_t stream;
        rg_where(rg->ctx, device, stream);
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        if (rg->off) (void)hipFree(rg->off);
        if (rg->rec) (void)hipFree(rg->rec);
    }
    delete rg;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_rodgen_set_rods(ibtk_le_rodgen rg, int n, const int* curr, const int* next,
                                       const double* params) {
    if (!rg) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_set_rods: null rod force generator");
    if (n < 0) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_set_rods: negative rod count %d", n);
    if (n > 0 && (!curr || !next || !params)) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_set_rods: null array");
    static const char* const kParam[10] = {"ds", "a1", "a2", "a3", "b1", "b2", "b3", "kappa1", "kappa2", "tau"};
    for (int k = 0; k < n; ++k) {
        if (curr[k] < 0 || curr[k] >= rg->n)
            return abi_fail(IBTK_LE_ERR_ARG, "rod %d: curr node index %d is out of range [0, %d)", k, curr[k], rg->n);
        if (next[k] < 0 || next[k] >= rg->n)
            return abi_fail(IBTK_LE_ERR_ARG, "rod %d: next node index %d is out of range [0, %d)", k, next[k], rg->n);
        if (curr[k] == next[k]) return abi_fail(IBTK_LE_ERR_ARG, "rod %d: curr and next are both node %d", k, curr[k]);
        for (int j = 0; j < 10; ++j)
            if (!std::isfinite(params[(size_t)k * 10 + j]))
                return abi_fail(IBTK_LE_ERR_ARG, "rod %d: parameter %s is not finite", k, kParam[j]);
    }
    if (n == 0) {
        rg->nrods = 0;
        return IBTK_LE_OK;
    }
    if (!rg->ctx)
        return abi_fail(IBTK_LE_ERR_ARG, "rodgen_set_rods: the handle was created without a context: nothing to upload to");
    // a node's row: its curr entries (ascending k), then its next entries (ascending k)
    std::vector<int> nc(rg->n, 0), nn(rg->n, 0);
    for (int k = 0; k < n; ++k) {
        ++nc[curr[k]];
        ++nn[next[k]];
    }
    std::vector<long long> off((size_t)rg->n + 1, 0), pc(rg->n), pn(rg->n);
    for (int i = 0; i < rg->n; ++i) {
        pc[i] = off[i];
        pn[i] = off[i] + nc[i];
        off[i + 1] = pn[i] + nn[i];
    }
    std::vector<RodRec> rec((size_t)off.back());
    for (int k = 0; k < n; ++k) {
        RodRec r;
        r.curr = curr[k];
        r.next = next[k];
        for (int j = 0; j < 10; ++j) r.p[j] = params[(size_t)k * 10 + j];
        rec[(size_t)pc[r.curr]++] = r;
        rec[(size_t)pn[r.next]++] = r;
    }
    int device;
    hipStream_t stream;
    rg_where(rg->ctx, device, stream);
    ROD_HIP_TRY(hipSetDevice(device));
    ROD_HIP_TRY(hipStreamSynchronize(stream));  // an earlier compute may still read the old plan
    // into fresh buffers, swapped in once both copies are done: a failure leaves the old plan
    long long* noff = nullptr;
    RodRec* nrec = nullptr;
    const size_t off_bytes = off.size() * sizeof(long long), rec_bytes = rec.size() * sizeof(RodRec);
    if (hipMalloc((void**)&noff, off_bytes) != hipSuccess || hipMalloc((void**)&nrec, rec_bytes) != hipSuccess) {
        if (noff) (void)hipFree(noff);
        return abi_fail(IBTK_LE_ERR_NOMEM, "rodgen_set_rods: hipMalloc(%zu + %zu) failed", off_bytes, rec_bytes);
    }
    hipError_t e = hipMemcpy(noff, off.data(), off_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(nrec, rec.data(), rec_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(noff);
        (void)hipFree(nrec);
        return abi_fail(IBTK_LE_ERR_DEVICE, "rodgen_set_rods: upload: %s", hipGetErrorString(e));
    }
    if (rg->off) (void)hipFree(rg->off);
    if (rg->rec) (void)hipFree(rg->rec);
    rg->off = noff;
    rg->rec = nrec;
    rg->nrods = n;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_rodgen_compute(ibtk_le_ctx ctx, ibtk_le_rodgen rg, const double* X_dev, const double* D_dev,
                                      double* F_dev, double* N_dev, int accumulate_F, int accumulate_N) {
    if (!ctx) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_compute: null context");
    if (!rg) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_compute: null rod force generator");
    if (!rg->ctx) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_compute: the handle was created without a context");
    // set_rods and destroy wait for the plan's own context before they free its buffers, so
    // no other context may have a compute in flight on them
    if (ctx != rg->ctx)
        return abi_fail(IBTK_LE_ERR_ARG, "rodgen_compute: the plan was created on another context");
    int device;
    hipStream_t stream;
    rg_where(ctx, device, stream);
    if (rg->n == 0) return IBTK_LE_OK;
    if (!X_dev || !D_dev || !F_dev || !N_dev) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_compute: null array");
    const size_t b3 = sizeof(double) * 3 * (size_t)rg->n, b9 = 3 * b3;
    if (rg_overlap(F_dev, b3, N_dev, b3) || rg_overlap(F_dev, b3, X_dev, b3) || rg_overlap(F_dev, b3, D_dev, b9) ||
        rg_overlap(N_dev, b3, X_dev, b3) || rg_overlap(N_dev, b3, D_dev, b9))
        return abi_fail(IBTK_LE_ERR_ARG, "rodgen_compute: F and N must not overlap each other, X or D");
    ROD_HIP_TRY(hipSetDevice(device));
    if (rg->nrods == 0) {
        if (!accumulate_F) ROD_HIP_TRY(hipMemsetAsync(F_dev, 0, b3, stream));
        if (!accumulate_N) ROD_HIP_TRY(hipMemsetAsync(N_dev, 0, b3, stream));
        return IBTK_LE_OK;
    }
    RodGenParams p{};
    p.n = rg->n;
    p.off = rg->off;
    p.rec = rg->rec;
    p.X = X_dev;
    p.D = D_dev;
    p.F = F_dev;
    p.N = N_dev;
    p.accumulate_F = accumulate_F ? 1 : 0;
    p.accumulate_N = accumulate_N ? 1 : 0;
    ROD_HIP_TRY(launch_rodgen(p, stream));
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_rodgen_plan_size(ibtk_le_rodgen rg, long long* n_entries) {
    if (!rg || !n_entries) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_plan_size: null argument");
    *n_entries = 2 * rg->nrods;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_rodgen_plan_read(ibtk_le_rodgen rg, long long* off_host, void* rec_host, long long rec_bytes) {
    if (!rg || !off_host) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_plan_read: null argument");
    const long long want = 2 * rg->nrods * (long long)sizeof(RodRec);
    if (rec_bytes != want)
        return abi_fail(IBTK_LE_ERR_ARG, "rodgen_plan_read: rec_bytes %lld, the plan's records take %lld", rec_bytes, want);
    if (rg->nrods == 0) {
        for (int i = 0; i <= rg->n; ++i) off_host[i] = 0;
        return IBTK_LE_OK;
    }
    if (!rec_host) return abi_fail(IBTK_LE_ERR_ARG, "rodgen_plan_read: null records");
    int device;
    hipStream_t stream;
    rg_where(rg->ctx, device, stream);
    ROD_HIP_TRY(hipSetDevice(device));
    ROD_HIP_TRY(hipMemcpy(off_host, rg->off, ((size_t)rg->n + 1) * sizeof(long long), hipMemcpyDeviceToHost));
    ROD_HIP_TRY(hipMemcpy(rec_host, rg->rec, (size_t)want, hipMemcpyDeviceToHost));
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_director_update(ibtk_le_ctx ctx, int scheme, long long n, double dt, const double* D_cur_dev,
                                       const double* W0_dev, const double* W1_dev, double* D_new_dev) {
    if (scheme == IBTK_LE_MIDPOINT)
        return abi_fail(IBTK_LE_ERR_ARG,
                        "director_update: time-stepping type MIDPOINT_RULE is not supported for the directors; use "
                        "TRAPEZOIDAL_RULE instead");
    if (scheme != IBTK_LE_EULER && scheme != IBTK_LE_TRAPEZOIDAL)
        return abi_fail(IBTK_LE_ERR_ARG, "director_update: unknown update scheme %d", scheme);
    if (!ctx) return abi_fail(IBTK_LE_ERR_ARG, "director_update: null context");
    if (n < 0) return abi_fail(IBTK_LE_ERR_ARG, "director_update: negative node count %lld", n);
    if (n == 0) return IBTK_LE_OK;
    const bool trap = scheme == IBTK_LE_TRAPEZOIDAL;
    if (!D_cur_dev || !W0_dev || !D_new_dev || (trap && !W1_dev))
        return abi_fail(IBTK_LE_ERR_ARG, "director_update: null array");
    const size_t b3 = sizeof(double) * 3 * (size_t)n, b9 = 3 * b3;
    if ((D_new_dev != D_cur_dev && rg_overlap(D_new_dev, b9, D_cur_dev, b9)) || rg_overlap(D_new_dev, b9, W0_dev, b3) ||
        (trap && rg_overlap(D_new_dev, b9, W1_dev, b3)))
        return abi_fail(IBTK_LE_ERR_ARG, "director_update: D_new may be D_cur itself; it overlaps D_cur, W0 or W1 otherwise");
    int device;
    hipStream_t stream;
    rg_where(ctx, device, stream);
    ROD_HIP_TRY(hipSetDevice(device));
    ROD_HIP_TRY(launch_director_update((long)n, dt, D_cur_dev, W0_dev, trap ? W1_dev : nullptr, D_new_dev, stream));
    return IBTK_LE_OK;
}
