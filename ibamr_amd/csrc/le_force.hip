// le_force.hip -- the Lagrangian force of IBStandardForceGen on the device: springs,
// beams and target points (IBStandardForceGen.cpp:265-313, 778-892, 990-1099,
// 1150-1216; the default Hookean law, IBSpringForceFunctions.h:117-120).
//
// One fused gather kernel per NDIM, one lane per node.  The reference adds the
// contributions into F_ghost in three serial loops over k (springs, beams, target
// points), so a node's sum has a fixed order: its springs by k, then its beams by k
// (master, next, prev within one k), then its target points.  The plan
// (ibtk_le_forcegen_set_*, le_abi.cpp) stores exactly that list per node (CSR, 64-bit
// row offsets), each entry carrying the whole spring / beam record, so every lane
// recomputes the reference's f from the same operands in the same orientation and
// adds or subtracts it as the reference statement for its role does.  No atomics: the
// result is the serial loop's, bit for bit, run to run.  A node with a very long list
// (a hub) runs serially in its lane; that is the price of the fixed order.
//
// Arithmetic: one rounded operation per reference operation (-ffp-contract=off), IEEE
// sqrt and divide.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "le_internal.h"

namespace ibtk_le {

namespace {

constexpr int FG_BLOCK = 256;

// the position the reference reads: X_ghost = X + dX (IBStandardForceGen.cpp:289), one
// rounded add per use
template <int ND, bool HAS_DX>
__device__ __forceinline__ void fg_pos(const double* __restrict__ X, const double* __restrict__ dX, int j,
                                       double (&x)[ND]) {
    const long b = (long)j * ND;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if constexpr (HAS_DX) x[d] = X[b + d] + dX[b + d];
        else x[d] = X[b + d];
    }
}

template <int ND, bool HAS_DX>
__global__ __launch_bounds__(FG_BLOCK) void k_forcegen(ForceGenParams p) {
    __shared__ double sF[FG_BLOCK * ND];
    const int t = threadIdx.x;
    const long i0 = (long)blockIdx.x * FG_BLOCK;
    const long i = i0 + t;
    if (i < p.n) {
        const int node = (int)i;
        double acc[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = 0.0;

        if (p.soff) {
            const FgSpring* __restrict__ rec = p.srec;
            const long long e1 = p.soff[i + 1];
            for (long long e = p.soff[i]; e < e1; ++e) {
                const FgSpring r = rec[e];
                double xm[ND], xs[ND], D[ND];
                fg_pos<ND, HAS_DX>(p.X, p.dX, r.m, xm);
                fg_pos<ND, HAS_DX>(p.X, p.dX, r.s, xs);
#pragma unroll
                for (int d = 0; d < ND; ++d) D[d] = xs[d] - xm[d];
                double R2 = D[0] * D[0] + D[1] * D[1];
                if constexpr (ND == 3) R2 = R2 + D[2] * D[2];
                const double R = sqrt(R2);
                if (R < DBL_EPSILON) continue;
                const double T_over_R = (r.kappa * (R - r.rest)) / R;
                if (r.m == node) {
#pragma unroll
                    for (int d = 0; d < ND; ++d) acc[d] += T_over_R * D[d];
                } else {
#pragma unroll
                    for (int d = 0; d < ND; ++d) acc[d] -= T_over_R * D[d];
                }
            }
        }

        if (p.boff) {
            const FgBeam<ND>* __restrict__ rec = static_cast<const FgBeam<ND>*>(p.brec);
            const long long e1 = p.boff[i + 1];
            for (long long e = p.boff[i]; e < e1; ++e) {
                const FgBeam<ND> r = rec[e];
                double xm[ND], xn[ND], xp[ND];
                fg_pos<ND, HAS_DX>(p.X, p.dX, r.m, xm);
                fg_pos<ND, HAS_DX>(p.X, p.dX, r.nx, xn);
                fg_pos<ND, HAS_DX>(p.X, p.dX, r.pv, xp);
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const double f = r.bend * (((xn[d] + xp[d]) - 2.0 * xm[d]) - r.curv[d]);
                    if (r.role == 0) acc[d] += 2.0 * f;
                    else acc[d] -= f;
                }
            }
        }

        if (p.toff) {
            const FgTarget<ND>* __restrict__ rec = static_cast<const FgTarget<ND>*>(p.trec);
            const long long e1 = p.toff[i + 1];
            for (long long e = p.toff[i]; e < e1; ++e) {
                const FgTarget<ND> r = rec[e];
                double x[ND];
                fg_pos<ND, HAS_DX>(p.X, p.dX, node, x);
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const double u = p.U ? p.U[i * ND + d] : 0.0;
                    acc[d] += r.kappa * (r.X0[d] - x[d]) - r.eta * u;
                }
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) sF[t * ND + d] = acc[d];
    }
    __syncthreads();
    // the block's F rows are one contiguous run of doubles: every lane stores (and, when
    // accumulating, loads) consecutive 8-byte words, whatever the alignment of the view
    const long rows = p.n - i0 < FG_BLOCK ? p.n - i0 : FG_BLOCK;
    const int cnt = (int)rows * ND;
    double* __restrict__ Fb = p.F + i0 * ND;
    for (int j = t; j < cnt; j += FG_BLOCK) Fb[j] = p.accumulate ? Fb[j] + sF[j] : sF[j];
}

}  // namespace

hipError_t launch_forcegen(int ndim, const ForceGenParams& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const long grid = (p.n + FG_BLOCK - 1) / FG_BLOCK;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(FG_BLOCK);
    if (ndim == 2) {
        if (p.dX) hipLaunchKernelGGL((k_forcegen<2, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((k_forcegen<2, false>), g, b, 0, s, p);
    } else {
        if (p.dX) hipLaunchKernelGGL((k_forcegen<3, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((k_forcegen<3, false>), g, b, 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace ibtk_le
