// le_force_jac.hip -- the force Jacobian of IBStandardForceGen on the device
// (computeLagrangianForceJacobianNonzeroStructure and computeLagrangianForceJacobian,
// IBStandardForceGen.cpp:315-496, 498-665; the default Hookean law and its derivative,
// IBSpringForceFunctions.h:117-131), read from the force plan of le_force.hip.
//
// The pattern (symbolic phase).  Row i of the plan names the block columns the reference's
// MatSetValuesBlocked calls touch in block row i: the other end of each of its springs, the
// {prev, next, master} of each of its beams, and i itself (the preallocated diagonal, :351).
// Those are the row's "candidates", in a fixed place each:
//   cand(i) = i + soff[i] + 3 boff[i]          the diagonal
//   cand(i) + 1 + q                            spring entry q of the row
//   cand(i) + 1 + ns_i + 3 q + {0, 1, 2}       beam entry q: prev, next, master
// One stable radix sort of the (row, col) keys with the candidates' indices as values, a
// head flag per sorted key and a scan give the block-CSR arrays and, for every block, its
// row and its run of the sorted candidates.  A row's candidates ascend in the order of the
// reference's calls (springs by k, then beams by k) and the sort is stable, so a block's
// run lists its contributions in the order the reference adds them: the numeric phase
// searches nothing.
//
// The values (numeric phase).  One lane per block forms the block in registers from +0.0:
// the contributions of its run in order; on a diagonal block first -dF of every spring of
// the row (they have no candidate of their own), then the run's beam candidates, then the
// row's target points.  Every block is written once, through LDS, as part of the
// workgroup's contiguous run of val: no zeroing pass, no read-modify-write, no atomics, and
// bit for bit the serial assembly.
//
// The product Y = J V streams the blocks of a row as one run of doubles through a group of
// 16 lanes (k_forcejac_apply); the linearized force (k_forcegen_linearized) is the walk of
// the assembly with every block applied to V at once; the preallocation counts
// (k_forcegen_nnz) are the same walk in integers.
//
// Arithmetic: one rounded operation per reference operation (-ffp-contract=off), IEEE
// sqrt and divide.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "le_internal.h"

namespace ibtk_le {

namespace {

constexpr int FJ_BLOCK = 256;

inline unsigned fj_grid(long n) { return (unsigned)((n + FJ_BLOCK - 1) / FJ_BLOCK); }

__device__ __forceinline__ long long fj_off(const long long* __restrict__ off, long i) { return off ? off[i] : 0; }

// the first candidate of row i (see the top of the file)
__device__ __forceinline__ long long fj_cand(const ForceJacPlan& p, long i) {
    return i + fj_off(p.soff, i) + 3 * fj_off(p.boff, i);
}

// ---------------------------------------------------------------------------------------
// symbolic phase
// ---------------------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(FJ_BLOCK) void k_fj_keys(ForceJacPlan p, unsigned long long* __restrict__ keys,
                                                      int* __restrict__ vals) {
    const long i = (long)blockIdx.x * FJ_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    const unsigned long long row = (unsigned long long)i << 32;
    long long c = fj_cand(p, i);
    keys[c] = row | (unsigned)i;
    vals[c] = (int)c;
    ++c;
    if (p.soff) {
        const long long e1 = p.soff[i + 1];
        for (long long e = p.soff[i]; e < e1; ++e, ++c) {
            const FgSpring r = p.srec[e];
            keys[c] = row | (unsigned)(r.m == (int)i ? r.s : r.m);
            vals[c] = (int)c;
        }
    }
    if (p.boff) {
        const FgBeam<ND>* __restrict__ rec = static_cast<const FgBeam<ND>*>(p.brec);
        const long long e1 = p.boff[i + 1];
        for (long long e = p.boff[i]; e < e1; ++e, c += 3) {
            const FgBeam<ND> r = rec[e];
            keys[c] = row | (unsigned)r.pv;
            keys[c + 1] = row | (unsigned)r.nx;
            keys[c + 2] = row | (unsigned)r.m;
            vals[c] = (int)c;
            vals[c + 1] = (int)c + 1;
            vals[c + 2] = (int)c + 2;
        }
    }
}

__global__ __launch_bounds__(FJ_BLOCK) void k_fj_heads(const unsigned long long* __restrict__ skeys, int C,
                                                       int* __restrict__ head) {
    const long j = (long)blockIdx.x * FJ_BLOCK + threadIdx.x;
    if (j >= C) return;
    head[j] = (j == 0 || skeys[j] != skeys[j - 1]) ? 1 : 0;
}

// incl[j] = the heads among the sorted keys 0 .. j: key j's block is incl[j] - 1, and a head
// starts that block's run of the sorted candidates
__global__ __launch_bounds__(FJ_BLOCK) void k_fj_scatter(const unsigned long long* __restrict__ skeys,
                                                         const int* __restrict__ incl, int C, long n,
                                                         long long* __restrict__ rowptr, int* __restrict__ col,
                                                         int* __restrict__ brow, int* __restrict__ bstart) {
    const long j = (long)blockIdx.x * FJ_BLOCK + threadIdx.x;
    if (j >= C) return;
    const unsigned long long k = skeys[j];
    const int sl = incl[j] - 1;
    if (j == 0 || skeys[j - 1] != k) {
        col[sl] = (int)(unsigned)k;
        brow[sl] = (int)(k >> 32);
        bstart[sl] = (int)j;
        // every row holds its diagonal, so every row has a first key
        if (j == 0 || (skeys[j - 1] >> 32) != (k >> 32)) rowptr[k >> 32] = sl;
    }
    if (j == C - 1) {
        rowptr[n] = incl[j];
        bstart[incl[j]] = C;
    }
}

// ---------------------------------------------------------------------------------------
// the contributions, shared by the assembly and the linearized force
// ---------------------------------------------------------------------------------------
template <int ND, bool HAS_DX>
__device__ __forceinline__ void fj_pos(const double* __restrict__ X, const double* __restrict__ dX, int j,
                                       double (&x)[ND]) {
    const long b = (long)j * ND;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if constexpr (HAS_DX) x[d] = X[b + d] + dX[b + d];
        else x[d] = X[b + d];
    }
}

// The block MatSetValuesBlocked stores for spring r (:541-565): D.norm() is Eigen's unrolled
// reduction, x^2 + (y^2 + z^2); no guard for R = 0 (0 / 0 = NaN, as in the reference);
// dF_dX.data() is column-major and read row-major, so the stored (row, c) is the
// expression at i = c, j = row.
template <int ND, bool HAS_DX>
__device__ __forceinline__ void fj_spring_block(const FgSpring& r, const double* __restrict__ X,
                                                const double* __restrict__ dX, double X_coef, double (&B)[ND * ND]) {
    double xm[ND], xs[ND], D[ND];
    fj_pos<ND, HAS_DX>(X, dX, r.m, xm);
    fj_pos<ND, HAS_DX>(X, dX, r.s, xs);
#pragma unroll
    for (int d = 0; d < ND; ++d) D[d] = xs[d] - xm[d];
    double R2;
    if constexpr (ND == 3) R2 = D[0] * D[0] + (D[1] * D[1] + D[2] * D[2]);
    else R2 = D[0] * D[0] + D[1] * D[1];
    const double R = sqrt(R2);
    const double T = r.kappa * (R - r.rest);
    const double dT_dR = r.kappa;
    const double T_R = T / R;
    const double RR = R * R;
    const double G = dT_dR - T_R;
#pragma unroll
    for (int row = 0; row < ND; ++row) {
#pragma unroll
        for (int c = 0; c < ND; ++c) {
            // i = c, j = row
            B[row * ND + c] = X_coef * ((T_R * (c == row ? 1.0 : 0.0)) + ((G * D[c]) * D[row]) / RR);
        }
    }
}

// the diagonal value a beam entry of the given role puts into column j (0 prev, 1 next,
// 2 master) of its row (:604-635)
__device__ __forceinline__ double fj_beam_value(int role, int j, double bend, double X_coef) {
    if (role == 0) return j == 2 ? (-4.0 * bend) * X_coef : (2.0 * bend) * X_coef;
    return j == 2 ? (2.0 * bend) * X_coef : (-1.0 * bend) * X_coef;
}

// ---------------------------------------------------------------------------------------
// numeric phase: a lane per block (see the top of the file)
// ---------------------------------------------------------------------------------------
template <int ND, bool HAS_DX>
__global__ __launch_bounds__(FJ_BLOCK) void k_forcejac_assemble(ForceJacParams p) {
    constexpr int BS = ND * ND;
    __shared__ double sB[FJ_BLOCK * BS];
    const int t = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * FJ_BLOCK;
    const long long b = b0 + t;
    if (b < p.nblocks) {
        const long i = p.brow[b];
        const long long base = fj_cand(p.plan, i);
        const long long s0 = fj_off(p.plan.soff, i);
        const long long ns_i = p.plan.soff ? p.plan.soff[i + 1] - s0 : 0;
        double acc[BS];
#pragma unroll
        for (int x = 0; x < BS; ++x) acc[x] = 0.0;
        int q = p.bstart[b];
        const int q1 = p.bstart[b + 1];
        const bool diagonal = p.scand[q] == base;  // the row's first candidate heads its diagonal block
        if (diagonal) {
            for (long long e = s0; e < s0 + ns_i; ++e) {
                const FgSpring r = p.plan.srec[e];
                double B[BS];
                fj_spring_block<ND, HAS_DX>(r, p.X, p.dX, p.X_coef, B);
#pragma unroll
                for (int x = 0; x < BS; ++x) acc[x] = acc[x] + B[x] * -1.0;
            }
            ++q;
        }
        for (; q < q1; ++q) {
            const long long c = p.scand[q] - base - 1;
            if (c < ns_i) {
                const FgSpring r = p.plan.srec[s0 + c];
                double B[BS];
                fj_spring_block<ND, HAS_DX>(r, p.X, p.dX, p.X_coef, B);
#pragma unroll
                for (int x = 0; x < BS; ++x) acc[x] = acc[x] + B[x];
            } else {
                const long long cb = c - ns_i, eb = cb / 3;
                const FgBeam<ND>* __restrict__ rec = static_cast<const FgBeam<ND>*>(p.plan.brec);
                const long long e = p.plan.boff[i] + eb;
                const double a = fj_beam_value(rec[e].role, (int)(cb - 3 * eb), rec[e].bend, p.X_coef);
#pragma unroll
                for (int x = 0; x < BS; ++x) acc[x] = acc[x] + (x % (ND + 1) == 0 ? a : 0.0);
            }
        }
        if (diagonal && p.plan.toff) {
            const FgTarget<ND>* __restrict__ rec = static_cast<const FgTarget<ND>*>(p.plan.trec);
            const long long e1 = p.plan.toff[i + 1];
            for (long long e = p.plan.toff[i]; e < e1; ++e) {
                const double a = ((-p.X_coef) * rec[e].kappa) - (p.U_coef * rec[e].eta);
#pragma unroll
                for (int x = 0; x < BS; ++x) acc[x] = acc[x] + (x % (ND + 1) == 0 ? a : 0.0);
            }
        }
#pragma unroll
        for (int x = 0; x < BS; ++x) sB[t * BS + x] = acc[x];
    }
    __syncthreads();
    // the workgroup's blocks are one contiguous run of val
    const long long left = p.nblocks - b0;
    const int cnt = (int)(left < FJ_BLOCK ? left : FJ_BLOCK) * BS;
    double* __restrict__ vb = p.val + b0 * BS;
    for (int j = t; j < cnt; j += FJ_BLOCK) vb[j] = sB[j];
}

// ---------------------------------------------------------------------------------------
// Y (+)= J V.  A group of FJ_GROUP lanes takes FJ_ROWS consecutive block rows, one after
// the other.  A row's blocks are one run of doubles, e = 0 .. BS (rowptr[i+1] - rowptr[i]):
// lane l multiplies e = l, l + 16, ... by V[col[e / BS]][e % ND] and adds the products, in
// that order, to the partial sum of component (e % BS) / ND; the 16 partial sums of a
// component are then combined by a butterfly at lane distances 8, 4, 2, 1.  The order is
// fixed by the pattern alone.  Y leaves through LDS as the workgroup's contiguous run.
// ---------------------------------------------------------------------------------------
constexpr int FJ_GROUP = 16;
constexpr int FJ_ROWS = 4;
constexpr int FJ_UNROLL = 4;
constexpr int FJ_WG_ROWS = FJ_BLOCK / FJ_GROUP * FJ_ROWS;

template <int ND>
__global__ __launch_bounds__(FJ_BLOCK) void k_forcejac_apply(ForceJacApplyParams p) {
    constexpr int BS = ND * ND;
    __shared__ double sY[FJ_WG_ROWS * ND];
    const int t = threadIdx.x;
    const int g = t / FJ_GROUP, l = t % FJ_GROUP;
    const long i0 = (long)blockIdx.x * FJ_WG_ROWS;
#pragma unroll 1
    for (int k = 0; k < FJ_ROWS; ++k) {
        const int lr = g * FJ_ROWS + k;
        const long i = i0 + lr;
        double acc[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = 0.0;
        if (i < p.n) {
            const long long b0 = p.rowptr[i];
            const long long len = (p.rowptr[i + 1] - b0) * BS;
            const double* __restrict__ v = p.val + b0 * BS;
            const int* __restrict__ cl = p.col + b0;
            // e = b BS + w without a division in the loop; FJ_UNROLL steps' loads are issued
            // together (a step past the row's end reads the row's first double and is dropped)
            long long b = l / BS;
            int w = l % BS;
            for (long long e = l; e < len; e += FJ_GROUP * FJ_UNROLL) {
                double a[FJ_UNROLL], x[FJ_UNROLL];
                int r[FJ_UNROLL];
                bool on[FJ_UNROLL];
#pragma unroll
                for (int u = 0; u < FJ_UNROLL; ++u) {
                    const long long eu = e + u * FJ_GROUP;
                    on[u] = eu < len;
                    r[u] = w / ND;
                    a[u] = v[on[u] ? eu : 0];
                    x[u] = p.V[(long long)cl[on[u] ? b : 0] * ND + (w - r[u] * ND)];
                    b += FJ_GROUP / BS;
                    w += FJ_GROUP % BS;
                    if (w >= BS) {
                        w -= BS;
                        ++b;
                    }
                }
#pragma unroll
                for (int u = 0; u < FJ_UNROLL; ++u) {
                    const double prod = a[u] * x[u];
#pragma unroll
                    for (int d = 0; d < ND; ++d)
                        if (on[u] && d == r[u]) acc[d] = acc[d] + prod;
                }
            }
        }
#pragma unroll
        for (int off = FJ_GROUP / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int d = 0; d < ND; ++d) acc[d] = acc[d] + __shfl_xor(acc[d], off, FJ_GROUP);
        }
        if (l == 0) {
#pragma unroll
            for (int d = 0; d < ND; ++d) sY[lr * ND + d] = acc[d];
        }
    }
    __syncthreads();
    const long rows = p.n - i0 < FJ_WG_ROWS ? p.n - i0 : FJ_WG_ROWS;
    const int cnt = (int)rows * ND;
    double* __restrict__ Yb = p.Y + i0 * ND;
    for (int j = t; j < cnt; j += FJ_BLOCK) Yb[j] = p.accumulate ? Yb[j] + sY[j] : sY[j];
}

// ---------------------------------------------------------------------------------------
// Y (+)= J(X + dX) V straight from the plan: the assembly's walk, every block applied to
// V[col] as it is formed, row by row of the block and left to right within a row
// ---------------------------------------------------------------------------------------
template <int ND, bool HAS_DX>
__global__ __launch_bounds__(FJ_BLOCK) void k_forcegen_linearized(ForceJacParams p, const double* __restrict__ V,
                                                                  double* __restrict__ Y, int accumulate) {
    constexpr int BS = ND * ND;
    __shared__ double sY[FJ_BLOCK * ND];
    const int t = threadIdx.x;
    const long i0 = (long)blockIdx.x * FJ_BLOCK;
    const long i = i0 + t;
    if (i < p.plan.n) {
        const int node = (int)i;
        double acc[ND], vi[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            acc[d] = 0.0;
            vi[d] = V[i * ND + d];
        }
        if (p.plan.soff) {
            const long long e1 = p.plan.soff[i + 1];
            for (long long e = p.plan.soff[i]; e < e1; ++e) {
                const FgSpring r = p.plan.srec[e];
                double B[BS];
                fj_spring_block<ND, HAS_DX>(r, p.X, p.dX, p.X_coef, B);
                const long o = (long)(r.m == node ? r.s : r.m) * ND;
#pragma unroll
                for (int row = 0; row < ND; ++row) {
#pragma unroll
                    for (int c = 0; c < ND; ++c) acc[row] = acc[row] + B[row * ND + c] * V[o + c];
                }
#pragma unroll
                for (int row = 0; row < ND; ++row) {
#pragma unroll
                    for (int c = 0; c < ND; ++c) acc[row] = acc[row] + (B[row * ND + c] * -1.0) * vi[c];
                }
            }
        }
        if (p.plan.boff) {
            const FgBeam<ND>* __restrict__ rec = static_cast<const FgBeam<ND>*>(p.plan.brec);
            const long long e1 = p.plan.boff[i + 1];
            for (long long e = p.plan.boff[i]; e < e1; ++e) {
                const FgBeam<ND> r = rec[e];
                const int cols[3] = {r.pv, r.nx, r.m};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double a = fj_beam_value(r.role, j, r.bend, p.X_coef);
                    const long o = (long)cols[j] * ND;
#pragma unroll
                    for (int d = 0; d < ND; ++d) acc[d] = acc[d] + a * V[o + d];
                }
            }
        }
        if (p.plan.toff) {
            const FgTarget<ND>* __restrict__ rec = static_cast<const FgTarget<ND>*>(p.plan.trec);
            const long long e1 = p.plan.toff[i + 1];
            for (long long e = p.plan.toff[i]; e < e1; ++e) {
                const double a = ((-p.X_coef) * rec[e].kappa) - (p.U_coef * rec[e].eta);
#pragma unroll
                for (int d = 0; d < ND; ++d) acc[d] = acc[d] + a * vi[d];
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) sY[t * ND + d] = acc[d];
    }
    __syncthreads();
    const long rows = p.plan.n - i0 < FJ_BLOCK ? p.plan.n - i0 : FJ_BLOCK;
    const int cnt = (int)rows * ND;
    double* __restrict__ Yb = Y + i0 * ND;
    for (int j = t; j < cnt; j += FJ_BLOCK) Yb[j] = accumulate ? Yb[j] + sY[j] : sY[j];
}

// ---------------------------------------------------------------------------------------
// the preallocation counts (:351-457) per block row: a node is local iff its index is
// below n_local.  Every plan entry adds what the reference adds at the entry's node.
// ---------------------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(FJ_BLOCK) void k_forcegen_nnz(ForceJacPlan p, int n_local, int* __restrict__ d_nnz,
                                                           int* __restrict__ o_nnz) {
    const long i = (long)blockIdx.x * FJ_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    int dn = 1, on = 0;
    if (p.soff) {
        const long long e1 = p.soff[i + 1];
        for (long long e = p.soff[i]; e < e1; ++e) {
            if (p.srec[e].s < n_local) ++dn;
            else ++on;
        }
    }
    if (p.boff) {
        const FgBeam<ND>* __restrict__ rec = static_cast<const FgBeam<ND>*>(p.brec);
        const long long e1 = p.boff[i + 1];
        for (long long e = p.boff[i]; e < e1; ++e) {
            const int role = rec[e].role;  // 0 master, 1 next, 2 prev
            const bool nl = rec[e].nx < n_local, pl = rec[e].pv < n_local;
            if (nl && pl) {
                dn += 2;
            } else if (nl) {
                dn += role == 2 ? 0 : 1;
                on += role == 2 ? 2 : 1;
            } else if (pl) {
                dn += role == 1 ? 0 : 1;
                on += role == 1 ? 2 : 1;
            } else {
                dn += role == 0 ? 0 : 2;
                on += 2;
            }
        }
    }
    d_nnz[i] = dn;
    o_nnz[i] = on;
}

}  // namespace

hipError_t launch_fj_keys(int ndim, const ForceJacPlan& p, unsigned long long* keys, int* vals, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    if (ndim == 2) hipLaunchKernelGGL((k_fj_keys<2>), dim3(fj_grid(p.n)), dim3(FJ_BLOCK), 0, s, p, keys, vals);
    else hipLaunchKernelGGL((k_fj_keys<3>), dim3(fj_grid(p.n)), dim3(FJ_BLOCK), 0, s, p, keys, vals);
    return hipGetLastError();
}

// radix_sort_pairs is stable, and the numeric phase depends on it: candidates with equal keys
// stay in ascending index order, the order of the reference's calls (k_forcejac_assemble)
hipError_t launch_fj_sort(void* temp, size_t& temp_bytes, const unsigned long long* kin, unsigned long long* kout,
                          const int* vin, int* vout, int n, int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)end_bit, s,
                                     false);
}

hipError_t launch_fj_heads(const unsigned long long* skeys, int C, int* head, hipStream_t s) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fj_heads, dim3(fj_grid(C)), dim3(FJ_BLOCK), 0, s, skeys, C, head);
    return hipGetLastError();
}

hipError_t launch_fj_scan(void* temp, size_t& temp_bytes, const int* in, int* out, int n, hipStream_t s) {
    return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)n, rocprim::plus<int>(), s, false);
}

hipError_t launch_fj_scatter(const unsigned long long* skeys, const int* incl, int C, long n, long long* rowptr,
                             int* col, int* brow, int* bstart, hipStream_t s) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fj_scatter, dim3(fj_grid(C)), dim3(FJ_BLOCK), 0, s, skeys, incl, C, n, rowptr, col, brow,
                       bstart);
    return hipGetLastError();
}

hipError_t launch_forcejac_assemble(int ndim, const ForceJacParams& p, hipStream_t s) {
    if (p.plan.n <= 0 || p.nblocks <= 0) return hipSuccess;
    const dim3 g(fj_grid(p.nblocks)), b(FJ_BLOCK);
    if (ndim == 2) {
        if (p.dX) hipLaunchKernelGGL((k_forcejac_assemble<2, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((k_forcejac_assemble<2, false>), g, b, 0, s, p);
    } else {
        if (p.dX) hipLaunchKernelGGL((k_forcejac_assemble<3, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((k_forcejac_assemble<3, false>), g, b, 0, s, p);
    }
    return hipGetLastError();
}

hipError_t launch_forcejac_apply(int ndim, const ForceJacApplyParams& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const dim3 g((unsigned)((p.n + FJ_WG_ROWS - 1) / FJ_WG_ROWS)), b(FJ_BLOCK);
    if (ndim == 2) hipLaunchKernelGGL((k_forcejac_apply<2>), g, b, 0, s, p);
    else hipLaunchKernelGGL((k_forcejac_apply<3>), g, b, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_forcegen_linearized(int ndim, const ForceJacParams& p, const double* V, double* Y, int accumulate,
                                      hipStream_t s) {
    if (p.plan.n <= 0) return hipSuccess;
    const dim3 g(fj_grid(p.plan.n)), b(FJ_BLOCK);
    if (ndim == 2) {
        if (p.dX) hipLaunchKernelGGL((k_forcegen_linearized<2, true>), g, b, 0, s, p, V, Y, accumulate);
        else hipLaunchKernelGGL((k_forcegen_linearized<2, false>), g, b, 0, s, p, V, Y, accumulate);
    } else {
        if (p.dX) hipLaunchKernelGGL((k_forcegen_linearized<3, true>), g, b, 0, s, p, V, Y, accumulate);
        else hipLaunchKernelGGL((k_forcegen_linearized<3, false>), g, b, 0, s, p, V, Y, accumulate);
    }
    return hipGetLastError();
}

hipError_t launch_forcegen_nnz(int ndim, const ForceJacPlan& p, int n_local, int* d_nnz, int* o_nnz, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const dim3 g(fj_grid(p.n)), b(FJ_BLOCK);
    if (ndim == 2) hipLaunchKernelGGL((k_forcegen_nnz<2>), g, b, 0, s, p, n_local, d_nnz, o_nnz);
    else hipLaunchKernelGGL((k_forcegen_nnz<3>), g, b, 0, s, p, n_local, d_nnz, o_nnz);
    return hipGetLastError();
}

}  // namespace ibtk_le
