// le_curl.hip -- the side-centred curl of a side-centred field on one patch,
// w = alpha curl u (+ w): PatchMathOps::curl(side, side), the arithmetic of stoscurl3d
// (ibtk/src/math/fortran/curl3d.f.m4:457-559) followed by the scale and axpy passes of
// GeneralizedIBMethod::interpolateVelocity / spreadForce (GeneralizedIBMethod.cpp:292-319,
// 537-577).  Every component is the difference of two centred first differences, each
// averaged over the four sides around the target side: fac * (an eight-term sum, added
// and subtracted left to right in the reference's operand order), one rounding per
// operation, no contraction.
//
// Work layout: one launch for the three components.  A workgroup of CURL_TX x CURL_TY
// threads owns an x-y tile and marches a z segment.  The planes a step needs -- u0 and u1
// at k-1, k, k+1, u2 at k, k+1 -- sit in LDS with a one-point halo in x and y, in a ring
// of four slots for u0 and u1 and of three for u2; plane k+2 is fetched into registers
// before step k computes and written to the ring after it, so one barrier a step suffices
// (the slot written held plane k-2 of u0 / u1, k-1 of u2, which no wave reads once it has
// passed the previous barrier).  Eleven haloed planes are 53,856 bytes: three workgroups a
// CU, six waves a SIMD.  Every thread
// stores w0, w1 and w2 of its own (i, j) at plane k: each u value is fetched once per tile
// (halo: (TX+2)(TY+2)/(TX TY)) and segment (two more planes), each w value written once.
// Tiles start at the w arrays' first element in x plus a multiple of CURL_TX, so that a
// row of a tile is whole 128-byte lines for pitched, aligned arrays.
//
// A read outside u's array -- the halo of a tile at the box edge where the ghost layer is
// one point wide -- is skipped and feeds only points that are not stored.  In a periodic
// dimension every read is taken at its image in the cell range (the value
// ibtk_le_fill_periodic_ghosts would put there), so u needs no ghost layer in it.
#include <hip/hip_runtime.h>

#include <climits>

#include "le_curl.h"

namespace ibtk_le {

namespace {

constexpr int LX = CURL_TX + 2, LY = CURL_TY + 2, LP = LX * LY;
constexpr int CURL_THREADS = CURL_TX * CURL_TY;
constexpr int SLOTS = 2;  // tile points (halo included) a thread stages per array: LP <= 2 threads
static_assert(LP <= SLOTS * CURL_THREADS, "two staged points a thread cover the haloed tile");

__device__ __forceinline__ int wrap(int i, int lo, int n) {
    int r = (i - lo) % n;
    if (r < 0) r += n;
    return lo + r;
}

// fac * (a - b + c - d + e - f + g - h), left to right
__device__ __forceinline__ double diff8(double fac, double a, double b, double c, double d, double e, double f,
                                        double g, double h) {
    return fac * (((((((a - b) + c) - d) + e) - f) + g) - h);
}

}  // namespace

__global__ __launch_bounds__(CURL_THREADS) void k_curl_side(CurlSide P) {
    // rings: four slots for u0 and u1 (planes k-1 .. k+2), three for u2 (k .. k+2); 53,856
    // bytes, three workgroups a CU
    __shared__ double sm01[2][4][LP];
    __shared__ double sm2[3][LP];
    const int t = threadIdx.x;
    const int tx0 = P.wlo[0] + (int)blockIdx.x * CURL_TX, ty0 = P.ilo[1] + (int)blockIdx.y * CURL_TY;
    const int z0 = P.ilo[2] + (int)blockIdx.z * P.seg;
    const int z1 = min(z0 + P.seg, P.ihi[2] + 1);  // cell planes [z0, z1)
    const int kend = z1 + (z1 == P.ihi[2] + 1 ? 1 : 0);  // the last segment adds w2's face ihi + 1
    const int zb = z0 - 1;  // plane p of u0 / u1 sits in slot (p - zb) & 3, of u2 in slot (p - z0) % 3

    // the staged points of this thread: x-y offsets into each u array, -1 = outside it
    int soff[3][SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int e = t + s * CURL_THREADS;
        const int gx = tx0 - 1 + e % LX, gy = ty0 - 1 + e / LX;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int sx = P.per[0] ? wrap(gx, P.ilo[0], P.ihi[0] - P.ilo[0] + 1) : gx;
            const int sy = P.per[1] ? wrap(gy, P.ilo[1], P.ihi[1] - P.ilo[1] + 1) : gy;
            const bool ok = e < LP && sx >= P.ulo[0] && sx <= P.uhi[a][0] && sy >= P.ulo[1] && sy <= P.uhi[a][1];
            soff[a][s] = ok ? (int)((sx - P.ulo[0]) + (int64_t)(sy - P.ulo[1]) * P.us1[a]) : -1;
        }
    }
    auto fetch = [&](int p, double (&r)[3][SLOTS]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int zp = P.per[2] ? wrap(p, P.ilo[2], P.ihi[2] - P.ilo[2] + 1) : p;
            // u2 is read at planes k and k + 1 only
            const bool zok = zp >= P.ulo[2] && zp <= P.uhi[a][2] && !(a == 2 && p < z0);
            const double* const base = P.u[a] + (int64_t)(zp - P.ulo[2]) * P.us2[a];
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) r[a][s] = zok && soff[a][s] >= 0 ? base[soff[a][s]] : 0.0;
        }
    };
    auto stage = [&](int p, const double (&r)[3][SLOTS]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a == 2 && p < z0) continue;
            double* const dst = a < 2 ? sm01[a][(p - zb) & 3] : sm2[(p - z0) % 3];
            dst[t] = r[a][0];
            if (t + CURL_THREADS < LP) dst[t + CURL_THREADS] = r[a][1];
        }
    };

    const int ti = t % CURL_TX, tj = t / CURL_TX;
    const int i = tx0 + ti, j = ty0 + tj, c = (tj + 1) * LX + ti + 1;
    const bool xc = i >= P.ilo[0] && i <= P.ihi[0], xf = i >= P.ilo[0] && i <= P.ihi[0] + 1;
    const bool yc = j >= P.ilo[1] && j <= P.ihi[1], yf = j >= P.ilo[1] && j <= P.ihi[1] + 1;
    const bool on0 = xf && yc, on1 = xc && yf, on2 = xc && yc;
    int64_t wxy[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) wxy[a] = (i - P.wlo[0]) + (int64_t)(j - P.wlo[1]) * P.ws1[a];
    const double f0 = P.fac[0], f1 = P.fac[1], f2 = P.fac[2], alpha = P.alpha;
    const bool acc = P.accumulate != 0;

    {  // planes z0 - 1, z0, z0 + 1 (z0 + 1 <= z1: a segment holds a plane), all loads in flight at once
        double ra[3][SLOTS], rb[3][SLOTS], rc[3][SLOTS];
        fetch(zb, ra);
        fetch(z0, rb);
        fetch(z0 + 1, rc);
        stage(zb, ra);
        stage(z0, rb);
        stage(z0 + 1, rc);
    }
    __syncthreads();
    double r[3][SLOTS];

    for (int k = z0; k < kend; ++k) {
        const bool pre = k + 2 <= z1;
        if (pre) fetch(k + 2, r);
        const bool cell = k < z1;
        double* const p0 = P.w[0] + wxy[0] + (int64_t)(k - P.wlo[2]) * P.ws2[0];
        double* const p1 = P.w[1] + wxy[1] + (int64_t)(k - P.wlo[2]) * P.ws2[1];
        double* const p2 = P.w[2] + wxy[2] + (int64_t)(k - P.wlo[2]) * P.ws2[2];
        double old0 = 0.0, old1 = 0.0, old2 = 0.0;
        if (acc) {
            if (on0 && cell) old0 = *p0;
            if (on1 && cell) old1 = *p1;
            if (on2) old2 = *p2;
        }
        const double* const am = sm01[0][(k - 1 - zb) & 3] + c;  // u0 at k - 1, k, k + 1
        const double* const a0 = sm01[0][(k - zb) & 3] + c;
        const double* const ap = sm01[0][(k + 1 - zb) & 3] + c;
        const double* const bm = sm01[1][(k - 1 - zb) & 3] + c;  // u1
        const double* const b0 = sm01[1][(k - zb) & 3] + c;
        const double* const bp = sm01[1][(k + 1 - zb) & 3] + c;
        const double* const c0 = sm2[(k - z0) % 3] + c;          // u2 at k, k + 1
        const double* const cp = sm2[(k + 1 - z0) % 3] + c;
        if (cell) {  // uniform over the workgroup
            if (on0) {
                const double du2_dx1 = diff8(f1, c0[LX - 1], c0[-LX - 1], c0[LX], c0[-LX], cp[LX - 1], cp[-LX - 1],
                                             cp[LX], cp[-LX]);
                const double du1_dx2 = diff8(f2, bp[-1], bm[-1], bp[0], bm[0], bp[LX - 1], bm[LX - 1], bp[LX], bm[LX]);
                const double v = alpha * (du2_dx1 - du1_dx2);
                *p0 = acc ? v + old0 : v;
            }
            if (on1) {
                const double du0_dx2 = diff8(f2, ap[-LX], am[-LX], ap[-LX + 1], am[-LX + 1], ap[0], am[0], ap[1], am[1]);
                const double du2_dx0 = diff8(f0, c0[-LX + 1], c0[-LX - 1], c0[1], c0[-1], cp[-LX + 1], cp[-LX - 1],
                                             cp[1], cp[-1]);
                const double v = alpha * (du0_dx2 - du2_dx0);
                *p1 = acc ? v + old1 : v;
            }
        }
        if (on2) {
            const double du1_dx0 = diff8(f0, bm[1], bm[-1], bm[LX + 1], bm[LX - 1], b0[1], b0[-1], b0[LX + 1], b0[LX - 1]);
            const double du0_dx1 = diff8(f1, am[LX], am[-LX], am[LX + 1], am[-LX + 1], a0[LX], a0[-LX], a0[LX + 1],
                                         a0[-LX + 1]);
            const double v = alpha * (du1_dx0 - du0_dx1);
            *p2 = acc ? v + old2 : v;
        }
        if (pre) stage(k + 2, r);
        __syncthreads();
    }
}

hipError_t launch_curl_side(CurlSide P, hipStream_t s) {
    const long long nx = (long long)P.ihi[0] - P.ilo[0] + 1, ny = (long long)P.ihi[1] - P.ilo[1] + 1;
    const int nz = P.ihi[2] - P.ilo[2] + 1;
    // faces ilo .. ihi + 1 in x and y; in x from the w arrays' first element
    const long long tx = (nx + 1 + (P.ilo[0] - P.wlo[0]) + CURL_TX - 1) / CURL_TX, ty = (ny + 1 + CURL_TY - 1) / CURL_TY;
    P.seg = curl_segment(tx * ty, nz);
    const long long tz = ((long long)nz + P.seg - 1) / P.seg;
    if (tx > INT_MAX || ty > 65535 || tz > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_curl_side, dim3((unsigned)tx, (unsigned)ty, (unsigned)tz), dim3(CURL_THREADS), 0, s, P);
    return hipGetLastError();
}

}  // namespace ibtk_le
