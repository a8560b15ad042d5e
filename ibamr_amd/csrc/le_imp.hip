// le_imp.hip -- the device stages of IMPMethod, the immersed material point method
// (src/IB/IMPMethod.cpp), for one patch of side-centred data in 2-D and 3-D:
//
//   k_imp_interp   U and Grad U at the points        IMPMethod::interpolateVelocity :460-536
//   k_imp_spread   f_c += sum_k tau(c,k) d_k delta_h wgt / dV     ::spreadForce  :848-921
//   k_imp_update   F_new = inv(I - a dt Gb)(I + a dt Ga) F_cur    ::eulerStep .. :547-716
//   k_imp_stress   tau = PP FF^T, the law of examples/IMP/explicit/ex0/main.cpp:68-89
//
// IMPMethod carries its own IB_6 kernel with the derivative (:119-171); imp_kernel below
// restates it operation by operation.  It is NOT closed_weights<K_IB_6> (le_stencil.h):
// the powers here are the running products r2 = r r, r3 = r r2, ... r6 = r r5 where the
// Fortran path uses binary powering (r4 = (r r)(r r)), so the weights differ in the last
// bits, and there are six derivative values besides.  The anchor is the same NINT, so the
// markers' IB_6 bins bound this stencil.
//
// Interp: one lane per list entry in the markers' sorted order (neighbouring lanes read
// neighbouring grid lines); per component the 36 weights sit in registers, the 6^NDIM
// loop is unrolled and the sums run in the reference's order, dimension 0 fastest, so U
// and Grad U equal the reference's bit for bit.  A stencil point outside the component's
// ghost box is not read and contributes u = 0: a sum that starts at +0 is never -0, and
// adding or subtracting a zero leaves every other value as it is.
//
// Spread: owner gathers.  A workgroup owns a tile of side points of one component and
// walks the entries whose cell-frame anchor lies within IMP_REACH cells of the tile, row
// of anchor cells by row, each row in list order: a fixed order, so the result is the
// same from run to run, with no atomics.  The entry ranges come from a sort of the list
// by anchor cell (stable, so the markers' order within a cell) and its cell offsets.
// Entries are staged IMP_CHUNK at a time in LDS -- stencil_box_lower, phi, dphi / dx, the
// tau row and wgt / dV --, one lane computing one (entry, dimension); every lane then
// adds the contributions of its own point, for the entries a wave-wide box test kept.
#include <hip/hip_runtime.h>

#include <climits>

#include "le_imp.h"
#include "le_stencil.h"

namespace ibtk_le {

namespace {

constexpr int IMP_IBLOCK = 128;  // interp: lanes per workgroup
constexpr int IMP_PBLOCK = 256;  // pointwise kernels

// IMPMethod.cpp:119-171, kernel(): returns stencil_box_lower; phi[6], dphi[6].
__device__ __forceinline__ int imp_kernel(double X, double patch_x_lower, double dx, int patch_box_lower, double K,
                                          double* phi, double* dphi) {
    const int kernel_width = 3;
    const double X_o_dx = (X - patch_x_lower) / dx;
    const int stencil_box_lower = d_nint(X_o_dx) + patch_box_lower - kernel_width;
    const double r = 1.0 - X_o_dx + ((stencil_box_lower + kernel_width - 1 - patch_box_lower) + 0.5);

    const double r2 = r * r;
    const double r3 = r * r2;
    const double r4 = r * r3;
    const double r5 = r * r4;
    const double r6 = r * r5;

    const double K2 = K * K;
    const double alpha = 28.0;

    const double beta = (9.0 / 4.0) - (3.0 / 2.0) * (K + r2) + ((22.0 / 3.0) - 7.0 * K) * r - (7.0 / 3.0) * r3;
    const double dbeta = ((22.0 / 3.0) - 7.0 * K) - 3.0 * r - 7.0 * r2;

    const double gamma = (1.0 / 4.0) * (((161.0 / 36.0) - (59.0 / 6.0) * K + 5.0 * K2) * (1.0 / 2.0) * r2 +
                                        (-(109.0 / 24.0) + 5.0 * K) * (1.0 / 3.0) * r4 + (5.0 / 18.0) * r6);
    const double dgamma = (1.0 / 4.0) * (((161.0 / 36.0) - (59.0 / 6.0) * K + 5.0 * K2) * r +
                                         (-(109.0 / 24.0) + 5.0 * K) * (4.0 / 3.0) * r3 + (5.0 / 3.0) * r5);

    const double discr = beta * beta - 4.0 * alpha * gamma;

    phi[0] = (-beta + copysign(1.0, (3.0 / 2.0) - K) * sqrt(discr)) / (2.0 * alpha);
    phi[1] =
        -3.0 * phi[0] - (1.0 / 16.0) + (1.0 / 8.0) * (K + r2) + (1.0 / 12.0) * (3.0 * K - 1.0) * r + (1.0 / 12.0) * r3;
    phi[2] = 2.0 * phi[0] + (1.0 / 4.0) + (1.0 / 6.0) * (4.0 - 3.0 * K) * r - (1.0 / 6.0) * r3;
    phi[3] = 2.0 * phi[0] + (5.0 / 8.0) - (1.0 / 4.0) * (K + r2);
    phi[4] = -3.0 * phi[0] + (1.0 / 4.0) - (1.0 / 6.0) * (4.0 - 3.0 * K) * r + (1.0 / 6.0) * r3;
    phi[5] = phi[0] - (1.0 / 16.0) + (1.0 / 8.0) * (K + r2) - (1.0 / 12.0) * (3.0 * K - 1.0) * r - (1.0 / 12.0) * r3;

    dphi[0] = -(dbeta * phi[0] + dgamma) / (2.0 * alpha * phi[0] + beta);
    dphi[1] = -3.0 * dphi[0] + (1.0 / 12.0) * (3.0 * K - 1.0) + (1.0 / 4.0) * r + (1.0 / 4.0) * r2;
    dphi[2] = 2.0 * dphi[0] + (1.0 / 6.0) * (4.0 - 3.0 * K) - (1.0 / 2.0) * r2;
    dphi[3] = 2.0 * dphi[0] - (1.0 / 2.0) * r;
    dphi[4] = -3.0 * dphi[0] - (1.0 / 6.0) * (4.0 - 3.0 * K) + (1.0 / 2.0) * r2;
    dphi[5] = dphi[0] - (1.0 / 12.0) * (3.0 * K - 1.0) + (1.0 / 4.0) * r - (1.0 / 4.0) * r2;
    return stencil_box_lower;
}

// a member of a three-element kernel-argument array by a run-time index, without
// indexing the argument block through memory
template <class T> __device__ __forceinline__ T pick(const T (&a)[3], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : a[2]); }

__device__ __forceinline__ double pick6(const double (&a)[6], int i) {
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
    return i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : (i == 3 ? a3 : (i == 4 ? a4 : a5))));
}

__device__ __forceinline__ const double* sorted_positions(const ImpParams& P) {
    return P.sorted_X_ref ? *P.sorted_X_ref : P.sorted_X;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// interp
// ---------------------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(IMP_IBLOCK) void k_imp_interp(ImpParams P) {
    const int e = (int)blockIdx.x * IMP_IBLOCK + (int)threadIdx.x;
    if (e >= P.n) return;
    const int s = P.qdst ? P.qdst[e] : P.sorted_s[e];
    if (s < 0) return;
    const double* const sx = sorted_positions(P);
    double X[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) X[d] = sx[(int64_t)ND * e + d];
#pragma unroll 1
    for (int c = 0; c < ND; ++c) {
        const double* const u = c == 0 ? P.comp[0].u : (c == 1 ? P.comp[1].u : P.comp[2].u);
        const int64_t s1 = c == 0 ? P.comp[0].s1 : (c == 1 ? P.comp[1].s1 : P.comp[2].s1);
        const int64_t s2 = c == 0 ? P.comp[0].s2 : (c == 1 ? P.comp[1].s2 : P.comp[2].s2);
        double phi[ND][6], a[ND][6];  // a = dphi / dx
        int lower[ND], glo[ND], ghi[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const double xlo = c == 0 ? P.comp[0].xlo[d] : (c == 1 ? P.comp[1].xlo[d] : P.comp[2].xlo[d]);
            glo[d] = c == 0 ? P.comp[0].lo[d] : (c == 1 ? P.comp[1].lo[d] : P.comp[2].lo[d]);
            ghi[d] = c == 0 ? P.comp[0].hi[d] : (c == 1 ? P.comp[1].hi[d] : P.comp[2].hi[d]);
            double dphi[6];
            lower[d] = imp_kernel(X[d], xlo, P.dx[d], P.ilower[d], P.K, phi[d], dphi);
#pragma unroll
            for (int j = 0; j < 6; ++j) a[d][j] = dphi[j] / P.dx[d];
        }
        double U = 0.0, G[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) G[k] = 0.0;
        if constexpr (ND == 3) {
            // a grid line at a time: unrolled over the planes too, the compiler hoists the
            // 108 x-y products out of the z loop and spills.  The line's y and z weights
            // are selected from their registers, not indexed through memory
#pragma unroll 1
            for (int iz = 0; iz < 6; ++iz) {
                const int z = lower[2] + iz;
                const bool okz = z >= glo[2] && z <= ghi[2];
                const double p2 = pick6(phi[2], iz), a2 = pick6(a[2], iz);
#pragma unroll 1
                for (int iy = 0; iy < 6; ++iy) {
                    const int y = lower[1] + iy;
                    const bool okzy = okz && y >= glo[1] && y <= ghi[1];
                    const double p1 = pick6(phi[1], iy), a1 = pick6(a[1], iy);
                    const double* const row = u + (int64_t)(z - glo[2]) * s2 + (int64_t)(y - glo[1]) * s1 - glo[0];
#pragma unroll
                    for (int ix = 0; ix < 6; ++ix) {
                        const int x = lower[0] + ix;
                        const bool ok = okzy && x >= glo[0] && x <= ghi[0];
                        const double v = ok ? row[x] : 0.0;
                        const double w = (phi[0][ix] * p1) * p2;
                        U += v * w;
                        const double dw0 = (a[0][ix] * p1) * p2;
                        G[0] -= v * dw0;
                        const double dw1 = (phi[0][ix] * a1) * p2;
                        G[1] -= v * dw1;
                        const double dw2 = (phi[0][ix] * p1) * a2;
                        G[2] -= v * dw2;
                    }
                }
            }
        } else {
#pragma unroll
            for (int iy = 0; iy < 6; ++iy) {
                const int y = lower[1] + iy;
                const bool oky = y >= glo[1] && y <= ghi[1];
                const double* const row = u + (int64_t)(y - glo[1]) * s1 - glo[0];
#pragma unroll
                for (int ix = 0; ix < 6; ++ix) {
                    const int x = lower[0] + ix;
                    const bool ok = oky && x >= glo[0] && x <= ghi[0];
                    const double v = ok ? row[x] : 0.0;
                    const double w = phi[0][ix] * phi[1][iy];
                    U += v * w;
                    const double dw0 = a[0][ix] * phi[1][iy];
                    G[0] -= v * dw0;
                    const double dw1 = phi[0][ix] * a[1][iy];
                    G[1] -= v * dw1;
                }
            }
        }
        P.U[(int64_t)ND * s + c] = U;
#pragma unroll
        for (int k = 0; k < ND; ++k) P.GradU[(int64_t)(ND * ND) * s + ND * c + k] = G[k];
    }
}

hipError_t launch_imp_interp(const ImpParams& P, hipStream_t s) {
    if (P.n <= 0) return hipSuccess;
    const unsigned nb = (unsigned)((P.n + IMP_IBLOCK - 1) / IMP_IBLOCK);
    if (P.ndim == 3) hipLaunchKernelGGL(k_imp_interp<3>, dim3(nb), dim3(IMP_IBLOCK), 0, s, P);
    else hipLaunchKernelGGL(k_imp_interp<2>, dim3(nb), dim3(IMP_IBLOCK), 0, s, P);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// spread
// ---------------------------------------------------------------------------------------
// keys[e] = the anchor cell of sorted position e in the anchor grid, x fastest (ncells:
// outside it, such an entry reaches no array point); vals[e] = e
template <int ND>
__global__ __launch_bounds__(IMP_PBLOCK) void k_imp_keys(ImpParams P) {
    const int e = (int)blockIdx.x * IMP_PBLOCK + (int)threadIdx.x;
    if (e >= P.n) return;
    const double* const sx = sorted_positions(P);
    bool in = true;
    int g[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const double X_o_dx = (sx[(int64_t)ND * e + d] - P.xlo[d]) / P.dx[d];
        g[d] = 0;
        if (X_o_dx > -1.0e9 && X_o_dx < 1.0e9) {  // (a NaN fails both)
            g[d] = d_nint(X_o_dx) + P.ilower[d] - P.alo[d];
            if (g[d] < 0 || g[d] >= P.aext[d]) in = false;
        } else {
            in = false;
        }
    }
    unsigned key = (unsigned)P.ncells;
    if (in) {
        key = (unsigned)g[ND - 1];
#pragma unroll
        for (int d = ND - 2; d >= 0; --d) key = key * (unsigned)P.aext[d] + (unsigned)g[d];
    }
    P.keys[e] = key;
    P.vals[e] = e;
}

hipError_t launch_imp_keys(const ImpParams& P, hipStream_t s) {
    if (P.n <= 0) return hipSuccess;
    const unsigned nb = (unsigned)((P.n + IMP_PBLOCK - 1) / IMP_PBLOCK);
    if (P.ndim == 3) hipLaunchKernelGGL(k_imp_keys<3>, dim3(nb), dim3(IMP_PBLOCK), 0, s, P);
    else hipLaunchKernelGGL(k_imp_keys<2>, dim3(nb), dim3(IMP_PBLOCK), 0, s, P);
    return hipGetLastError();
}

template <int ND>
__global__ __launch_bounds__(ND == 3 ? 512 : 256) void k_imp_spread(ImpParams P) {
    constexpr int B = ND == 3 ? IMP_TILE3 : IMP_TILE2;
    constexpr int RW = B + 2 * IMP_REACH;            // anchor cells per dim that reach the tile
    constexpr int NROW = ND == 3 ? RW * RW : RW;     // x-rows of them
    constexpr int NSCAN = 256;
    static_assert(NROW <= NSCAN, "one scan slot per row");
    constexpr int KT0 = IMP_CHUNK * ND;              // the lanes past the kernel evaluations stage tau
    __shared__ int s_inc[NSCAN];    // entries in rows 0 .. r (inclusive scan)
    __shared__ int s_first[NSCAN];  // first position (in svals) of row r
    __shared__ int s_e[IMP_CHUNK];
    __shared__ int s_lo[IMP_CHUNK][4];
    __shared__ double s_phi[IMP_CHUNK][ND][6];
    __shared__ double s_a[IMP_CHUNK][ND][6];
    __shared__ double s_tau[IMP_CHUNK][ND];
    __shared__ double s_scale[IMP_CHUNK];

    const int t = (int)threadIdx.x;
    const int c = (int)blockIdx.y;
    int clo[ND], chi[ND], glo[ND], t0[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        clo[d] = c == 0 ? P.comp[0].clo[d] : (c == 1 ? P.comp[1].clo[d] : P.comp[2].clo[d]);
        chi[d] = c == 0 ? P.comp[0].chi[d] : (c == 1 ? P.comp[1].chi[d] : P.comp[2].chi[d]);
        glo[d] = c == 0 ? P.comp[0].lo[d] : (c == 1 ? P.comp[1].lo[d] : P.comp[2].lo[d]);
    }
    {
        int tt = (int)blockIdx.x;
        t0[0] = clo[0] + (tt % P.nt[0]) * B;
        tt /= P.nt[0];
        if constexpr (ND == 3) {
            t0[1] = clo[1] + (tt % P.nt[1]) * B;
            t0[2] = clo[2] + (tt / P.nt[1]) * B;
        } else {
            t0[1] = clo[1] + tt * B;
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (t0[d] > chi[d]) return;  // the whole workgroup: a tile past this component's clip box

    // the rows of anchor cells that reach the tile and their entry ranges
    int cnt = 0, first = 0;
    if (t < NROW) {
        const int gx0 = max(t0[0] - IMP_REACH - P.alo[0], 0);
        const int gx1 = min(t0[0] + B - 1 + IMP_REACH - P.alo[0], P.aext[0] - 1);
        const int gy = t0[1] - IMP_REACH + (t % RW) - P.alo[1];
        int gz = 0;
        bool ok = gx0 <= gx1 && gy >= 0 && gy < P.aext[1];
        if constexpr (ND == 3) {
            gz = t0[2] - IMP_REACH + (t / RW) - P.alo[2];
            ok = ok && gz >= 0 && gz < P.aext[2];
        }
        if (ok) {
            const int cell0 = (gz * P.aext[1] + gy) * P.aext[0] + gx0;
            first = P.start[cell0];
            cnt = P.start[cell0 + (gx1 - gx0 + 1)] - first;
        }
    }
    if (t < NSCAN) {
        s_inc[t] = cnt;
        s_first[t] = first;
    }
    __syncthreads();
    for (int off = 1; off < NSCAN; off <<= 1) {
        int v = 0;
        if (t < NSCAN && t >= off) v = s_inc[t - off];
        __syncthreads();
        if (t < NSCAN) s_inc[t] += v;
        __syncthreads();
    }
    const int total = s_inc[NSCAN - 1];
    if (total == 0) return;

    // this lane's point
    int i[ND];
    if constexpr (ND == 3) {
        // a wave owns a 4^3 sub-cube: fewer staged entries meet it than meet a whole z plane
        i[0] = t0[0] + (t & 3) + 4 * ((t >> 6) & 1);
        i[1] = t0[1] + ((t >> 2) & 3) + 4 * ((t >> 7) & 1);
        i[2] = t0[2] + ((t >> 4) & 3) + 4 * (t >> 8);
    } else {
        i[0] = t0[0] + (t & 15);
        i[1] = t0[1] + (t >> 4);
    }
    bool mine = true;
#pragma unroll
    for (int d = 0; d < ND; ++d) mine = mine && i[d] <= chi[d];
    double* const u = c == 0 ? P.comp[0].u : (c == 1 ? P.comp[1].u : P.comp[2].u);
    const int64_t s1 = c == 0 ? P.comp[0].s1 : (c == 1 ? P.comp[1].s1 : P.comp[2].s1);
    const int64_t s2 = c == 0 ? P.comp[0].s2 : (c == 1 ? P.comp[1].s2 : P.comp[2].s2);
    int64_t off = (i[0] - glo[0]) + (int64_t)(i[1] - glo[1]) * s1;
    if constexpr (ND == 3) off += (int64_t)(i[2] - glo[2]) * s2;
    double* const ptr = u + (mine ? off : 0);
    double acc = mine ? *ptr : 0.0;
    bool any = false;
    // the box of this wave's points: a 4^3 sub-cube of the tile in 3-D, four rows of 16 in 2-D
    const int wave = t >> 6;
    const int wx0 = ND == 3 ? t0[0] + 4 * (wave & 1) : t0[0], wx1 = ND == 3 ? wx0 + 3 : t0[0] + B - 1;
    const int wy0 = ND == 3 ? t0[1] + 4 * ((wave >> 1) & 1) : t0[1] + 4 * wave, wy1 = wy0 + 3;
    const int wz0 = ND == 3 ? t0[2] + 4 * (wave >> 2) : 0;

    const double* const sx = sorted_positions(P);
    for (int base = 0; base < total; base += IMP_CHUNK) {
        const int m = min(IMP_CHUNK, total - base);
        if (t < m) {  // the chunk's entries: row by row, list order within a row
            const int v = base + t;
            int lo = 0, hi = NSCAN - 1;  // the first row whose inclusive count exceeds v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_inc[mid] > v) hi = mid;
                else lo = mid + 1;
            }
            const int before = lo ? s_inc[lo - 1] : 0;
            s_e[t] = P.svals[s_first[lo] + (v - before)];
        }
        __syncthreads();
        if (t < m * ND) {  // one kernel evaluation: (entry, dimension)
            const int q = t / ND, d = t - q * ND;
            const int e = s_e[q];
            const double xlo = c == 0 ? pick(P.comp[0].xlo, d) : (c == 1 ? pick(P.comp[1].xlo, d) : pick(P.comp[2].xlo, d));
            const double dx = pick(P.dx, d);
            double phi[6], dphi[6];
            s_lo[q][d] = imp_kernel(sx[(int64_t)ND * e + d], xlo, dx, pick(P.ilower, d), P.K, phi, dphi);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                s_phi[q][d][j] = phi[j];
                s_a[q][d][j] = dphi[j] / dx;
            }
        } else if (t >= KT0 && t < KT0 + m) {  // the entry's tau row and wgt / dV
            const int q = t - KT0;
            const int row = P.sorted_s[s_e[q]];
#pragma unroll
            for (int k = 0; k < ND; ++k) s_tau[q][k] = P.tau[(int64_t)(ND * ND) * row + ND * c + k];
            s_scale[q] = P.wgt[row] / P.dV;
        }
        __syncthreads();
        // one test per wave for the whole chunk: lane L looks at entry L's stencil box and the
        // wave keeps the entries whose box meets its points, in their order
        const int lane = t & 63;
        int e0 = 0, e1 = 0, e2 = 0;
        bool hit = false;
        if (lane < m) {
            e0 = s_lo[lane][0];
            e1 = s_lo[lane][1];
            hit = !(e0 + 5 < wx0 || e0 > wx1 || e1 + 5 < wy0 || e1 > wy1);
            if constexpr (ND == 3) {
                e2 = s_lo[lane][2];
                hit = hit && !(e2 + 5 < wz0 || e2 > wz0 + 3);
            }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {
            const int q = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            const int l0 = __builtin_amdgcn_readlane(e0, q), l1 = __builtin_amdgcn_readlane(e1, q);
            const int l2 = ND == 3 ? __builtin_amdgcn_readlane(e2, q) : 0;
            const int ix = i[0] - l0, iy = i[1] - l1;
            const int iz = ND == 3 ? i[ND - 1] - l2 : 0;
            if (!mine || (unsigned)ix >= 6u || (unsigned)iy >= 6u || (unsigned)iz >= 6u) continue;
            // f = sum_k tau(c,k) dw_dx_k in the reference's order and association; the
            // contribution is f (wgt / dV) where the reference has (f wgt) / dV
            double f;
            if constexpr (ND == 3) {
                const double p0 = s_phi[q][0][ix], p1 = s_phi[q][1][iy], p2 = s_phi[q][2][iz];
                const double a0 = s_a[q][0][ix], a1 = s_a[q][1][iy], a2 = s_a[q][2][iz];
                f = s_tau[q][0] * ((a0 * p1) * p2);
                f += s_tau[q][1] * ((p0 * a1) * p2);
                f += s_tau[q][2] * ((p0 * p1) * a2);
            } else {
                const double p0 = s_phi[q][0][ix], p1 = s_phi[q][1][iy];
                const double a0 = s_a[q][0][ix], a1 = s_a[q][1][iy];
                f = s_tau[q][0] * (a0 * p1);
                f += s_tau[q][1] * (p0 * a1);
            }
            acc += f * s_scale[q];
            any = true;
        }
        __syncthreads();
    }
    if (mine && any) *ptr = acc;
}

hipError_t launch_imp_spread(const ImpParams& P, hipStream_t s) {
    if (P.n <= 0) return hipSuccess;
    const long long tiles = (long long)P.nt[0] * P.nt[1] * (P.ndim == 3 ? P.nt[2] : 1);
    if (tiles <= 0 || tiles > INT_MAX) return hipErrorInvalidValue;
    if (P.ndim == 3) hipLaunchKernelGGL(k_imp_spread<3>, dim3((unsigned)tiles, 3), dim3(512), 0, s, P);
    else hipLaunchKernelGGL(k_imp_spread<2>, dim3((unsigned)tiles, 2), dim3(256), 0, s, P);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// pointwise: the deformation gradient update and the stress
// ---------------------------------------------------------------------------------------
namespace {

struct M3 {
    double a[3][3];
};

// rows of NDIM^2 doubles; in 2-D the tensor is padded as the reference's is: (2,2) = z22
template <int ND> __device__ __forceinline__ M3 load(const double* p, double z22) {
    M3 A;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A.a[i][j] = (i < ND && j < ND) ? p[ND * i + j] : (i == 2 && j == 2 ? z22 : 0.0);
    return A;
}
template <int ND> __device__ __forceinline__ void store(double* p, const M3& A) {
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) p[ND * i + j] = A.a[i][j];
}
// libMesh TypeTensor::det
__device__ __forceinline__ double det3(const M3& A) {
    return A.a[0][0] * (A.a[1][1] * A.a[2][2] - A.a[1][2] * A.a[2][1]) -
           A.a[0][1] * (A.a[1][0] * A.a[2][2] - A.a[1][2] * A.a[2][0]) +
           A.a[0][2] * (A.a[1][0] * A.a[2][1] - A.a[1][1] * A.a[2][0]);
}
// tensor_inverse, ibtk/libmesh_utilities.h:310-339
template <int ND> __device__ __forceinline__ M3 inverse(const M3& M) {
    const double(&A)[3][3] = M.a;
    M3 R;
    const double det_A = det3(M);
    if constexpr (ND == 2) {
        R.a[0][0] = +A[1][1] / det_A;
        R.a[0][1] = -A[0][1] / det_A;
        R.a[0][2] = 0.0;
        R.a[1][0] = -A[1][0] / det_A;
        R.a[1][1] = +A[0][0] / det_A;
        R.a[1][2] = 0.0;
        R.a[2][0] = 0.0;
        R.a[2][1] = 0.0;
        R.a[2][2] = 1.0;
    } else {
        R.a[0][0] = +(A[2][2] * A[1][1] - A[2][1] * A[1][2]) / det_A;
        R.a[0][1] = -(A[2][2] * A[0][1] - A[2][1] * A[0][2]) / det_A;
        R.a[0][2] = +(A[1][2] * A[0][1] - A[1][1] * A[0][2]) / det_A;
        R.a[1][0] = -(A[2][2] * A[1][0] - A[2][0] * A[1][2]) / det_A;
        R.a[1][1] = +(A[2][2] * A[0][0] - A[2][0] * A[0][2]) / det_A;
        R.a[1][2] = -(A[1][2] * A[0][0] - A[1][0] * A[0][2]) / det_A;
        R.a[2][0] = +(A[2][1] * A[1][0] - A[2][0] * A[1][1]) / det_A;
        R.a[2][1] = -(A[2][1] * A[0][0] - A[2][0] * A[0][1]) / det_A;
        R.a[2][2] = +(A[1][1] * A[0][0] - A[1][0] * A[0][1]) / det_A;
    }
    return R;
}
__device__ __forceinline__ M3 transpose(const M3& A) {
    M3 R;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R.a[i][j] = A.a[j][i];
    return R;
}
// (A B)(i,j) = sum_k A(i,k) B(k,j), k ascending from 0
__device__ __forceinline__ M3 mul(const M3& A, const M3& B) {
    M3 R;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) v += A.a[i][k] * B.a[k][j];
            R.a[i][j] = v;
        }
    return R;
}
// I + sgn (a dt) G
__device__ __forceinline__ M3 eye_plus(double adt, const M3& G, bool minus) {
    M3 R;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double I = i == j ? 1.0 : 0.0, x = adt * G.a[i][j];
            R.a[i][j] = minus ? I - x : I + x;
        }
    return R;
}

}  // namespace

template <int ND>
__global__ __launch_bounds__(IMP_PBLOCK) void k_imp_update(long long n, double dt, const double* F_cur, const double* Ga,
                                                           const double* Gb, double* F_new, double* F_half) {
    const long long i = (long long)blockIdx.x * IMP_PBLOCK + threadIdx.x;
    if (i >= n) return;
    constexpr int R = ND * ND;
    const M3 F = load<ND>(F_cur + R * i, 1.0);
    const M3 A = load<ND>(Ga + R * i, 0.0), Bm = load<ND>(Gb + R * i, 0.0);
    {
        const double adt = 0.5 * dt;
        store<ND>(F_new + R * i, mul(mul(inverse<ND>(eye_plus(adt, Bm, true)), eye_plus(adt, A, false)), F));
    }
    if (F_half) {
        const double adt = 0.25 * dt;
        store<ND>(F_half + R * i, mul(mul(inverse<ND>(eye_plus(adt, Bm, true)), eye_plus(adt, A, false)), F));
    }
}

hipError_t launch_imp_update(int ndim, long long n, double dt, const double* F_cur, const double* Ga, const double* Gb,
                             double* F_new, double* F_half, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const long long nb = (n + IMP_PBLOCK - 1) / IMP_PBLOCK;
    if (nb > INT_MAX) return hipErrorInvalidValue;
    if (ndim == 3)
        hipLaunchKernelGGL(k_imp_update<3>, dim3((unsigned)nb), dim3(IMP_PBLOCK), 0, s, n, dt, F_cur, Ga, Gb, F_new, F_half);
    else
        hipLaunchKernelGGL(k_imp_update<2>, dim3((unsigned)nb), dim3(IMP_PBLOCK), 0, s, n, dt, F_cur, Ga, Gb, F_new, F_half);
    return hipGetLastError();
}

template <int ND>
__global__ __launch_bounds__(IMP_PBLOCK) void k_imp_stress(long long n, const double* Fp, double* tau, double c1, double p0,
                                                           double beta, const double* table, int nsub,
                                                           const int* subdomain) {
    const long long i = (long long)blockIdx.x * IMP_PBLOCK + threadIdx.x;
    if (i >= n) return;
    constexpr int R = ND * ND;
    if (subdomain) {
        const int sd = subdomain[i];
        if (sd < 0 || sd >= nsub) {  // no such row: the point's stress is not a number
            M3 bad;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) bad.a[a][b] = __builtin_nan("");
            store<ND>(tau + R * i, bad);
            return;
        }
        c1 = table[3 * sd];
        p0 = table[3 * sd + 1];
        beta = table[3 * sd + 2];
    }
    const M3 FF = load<ND>(Fp + R * i, 1.0);
    const M3 FFt = transpose(FF);
    M3 PP;
    const double two_c1 = 2.0 * c1;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) PP.a[a][b] = two_c1 * FF.a[a][b];
    if (p0 != 0.0 || beta != 0.0) {
        const M3 FF_inv_trans = transpose(inverse<ND>(FF));  // tensor_inverse_transpose: the same cofactors
        if (p0 != 0.0) {
            const double s = 2.0 * p0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) PP.a[a][b] -= s * FF_inv_trans.a[a][b];
        }
        if (beta != 0.0) {
            const M3 CC = mul(FFt, FF);
            const double s = beta * log(det3(CC));
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) PP.a[a][b] += s * FF_inv_trans.a[a][b];
        }
    }
    store<ND>(tau + R * i, mul(PP, FFt));
}

hipError_t launch_imp_stress(int ndim, long long n, const double* F, double* tau, double c1, double p0, double beta,
                             const double* table, int nsub, const int* subdomain, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const long long nb = (n + IMP_PBLOCK - 1) / IMP_PBLOCK;
    if (nb > INT_MAX) return hipErrorInvalidValue;
    if (ndim == 3)
        hipLaunchKernelGGL(k_imp_stress<3>, dim3((unsigned)nb), dim3(IMP_PBLOCK), 0, s, n, F, tau, c1, p0, beta, table, nsub,
                           subdomain);
    else
        hipLaunchKernelGGL(k_imp_stress<2>, dim3((unsigned)nb), dim3(IMP_PBLOCK), 0, s, n, F, tau, c1, p0, beta, table, nsub,
                           subdomain);
    return hipGetLastError();
}

}  // namespace ibtk_le
