// le_meter.hip -- flow meters and pressure gauges on the device: IBInstrumentPanel for one 3-D
// patch of side-centred u and cell-centred p on one rank (src/IB/IBInstrumentPanel.cpp):
//
//   k_meter_update  X_perimeter, X_centroid, r_max, num_web_nodes, the web   initializeHierarchyDependentData :698-923
//                   patches' centroids, area vectors and cells                       init_meter_elements :133-194
//   k_meter_read    flow, mean and point pressure, the flow correction             readInstrumentData :925-1182
//                                                   linear_interp :315-501, compute_flow_correction :199-234
//
// Every output can be the reference's one-rank value bit for bit: the arithmetic is + - * /,
// sqrt, ceil and floor, written operation for operation under -ffp-contract=off, with the
// associations of the reference's Eigen 3.2.1 expressions -- a fixed-size reduction is unrolled
// as halves (Eigen/src/Core/Redux.h:77-106), so a.dot(b) = a0 b0 + (a1 b1 + a2 b2) and norm =
// sqrt(x^2 + (y^2 + z^2)); v / s divides, v /= s multiplies by 1 / s (SelfCwiseBinaryOp.h:181-193).
//
// One workgroup a meter.  The order of a meter's sums is the reference's: it walks the cells
// of the patch box with x fastest and, within a cell, the meter's web patches in insertion
// order (m ascending, then n; multimap::equal_range keeps it).  The read kernel sorts the
// counted patches' keys (linear cell index, m nw + n) in LDS (a bitonic network; the keys are
// distinct, so the result is the unique order), lets every lane evaluate the terms of the
// patches at its sorted positions, and three lanes add the three streams -- staged through LDS
// a chunk at a time -- serially from +0.0.
// No floating-point atomics; the result is the same from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ibtk_le.h"
#include "le_meter.h"

namespace ibtk_le {

namespace {

template <class T> __device__ __forceinline__ T pick(const T (&a)[3], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : a[2]); }

// Eigen's unrolled 3-vector reductions (Redux.h:77-106)
__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
__device__ __forceinline__ double norm3(const double a[3]) { return sqrt(a[0] * a[0] + (a[1] * a[1] + a[2] * a[2])); }
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// IndexUtilities::getCellIndex (IndexUtilities-inl.h:66-89) in the domain frame, one
// dimension.  false: the position is not finite or further than 10^9 cells away.
__device__ __forceinline__ bool cell_index(const MtrDomain& D, const double dx, double X, int d, int& idx) {
    const double dl = X - pick(D.xlo, d), du = X - pick(D.xup, d);
    double c;
    if (fabs(dl) <= fabs(du)) c = (double)pick(D.lo, d) + floor(dl / dx);
    else c = (double)pick(D.hi, d) + floor(du / dx) + 1.0;
    idx = 0;
    if (!(c >= -1.0e9 && c <= 1.0e9)) return false;  // (a NaN fails both)
    idx = (int)c;
    return true;
}

// the cell of X; counted: it lies in the patch box (:889, :911)
__device__ __forceinline__ bool locate(const MtrGrid& g, const MtrDomain& D, const double X[3], int i[3]) {
    bool in = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const bool ok = cell_index(D, g.dx[d], X[d], d, i[d]);
        in = in && ok && i[d] >= g.ilower[d] && i[d] <= g.iupper[d];
    }
    return in;
}

__device__ __forceinline__ bool in_box(const MtrGrid& g, const int i[3]) {
    bool in = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) in = in && i[d] >= g.ilower[d] && i[d] <= g.iupper[d];
    return in;
}

// :990-996
__device__ __forceinline__ void cell_centre(const MtrGrid& g, const int i[3], double Xc[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) Xc[d] = g.xlo[d] + g.dx[d] * ((double)(i[d] - g.ilower[d]) + 0.5);
}

// the 1-D weight of linear_interp (:347, :478)
__device__ __forceinline__ double hat(double X, double Xc, double dx) { return (X < Xc ? X - (Xc - dx) : (Xc + dx) - X) / dx; }

// linear_interp of cell-centred data (:315-369)
__device__ __forceinline__ double interp_cell(const MtrGrid& g, const double* p, const double X[3], const int i[3],
                                              const double X_cell[3]) {
    int s0[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) s0[d] = X[d] < X_cell[d] ? -1 : 0;
    double U = 0.0;
    for (int k2 = s0[2]; k2 <= s0[2] + 1; ++k2)
        for (int k1 = s0[1]; k1 <= s0[1] + 1; ++k1)
            for (int k0 = s0[0]; k0 <= s0[0] + 1; ++k0) {
                const double c0 = X_cell[0] + (double)k0 * g.dx[0];
                const double c1 = X_cell[1] + (double)k1 * g.dx[1];
                const double c2 = X_cell[2] + (double)k2 * g.dx[2];
                const double wgt = (hat(X[0], c0, g.dx[0]) * hat(X[1], c1, g.dx[1])) * hat(X[2], c2, g.dx[2]);
                const int64_t off = (i[0] + k0 - g.glo[0]) + (int64_t)(i[1] + k1 - g.glo[1]) * g.ps1 +
                                    (int64_t)(i[2] + k2 - g.glo[2]) * g.ps2;
                U += p[off] * wgt;
            }
    return U;
}

// linear_interp of side-centred data, one axis (:434-501)
template <int AXIS>
__device__ __forceinline__ double interp_side(const MtrGrid& g, const double* u, const double X[3], const int i[3],
                                              const double X_cell[3]) {
    int s0[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) s0[d] = (d != AXIS && X[d] < X_cell[d]) ? -1 : 0;
    const int64_t s1 = g.us1[AXIS], s2 = g.us2[AXIS];
    double U = 0.0;
    for (int k2 = s0[2]; k2 <= s0[2] + 1; ++k2)
        for (int k1 = s0[1]; k1 <= s0[1] + 1; ++k1)
            for (int k0 = s0[0]; k0 <= s0[0] + 1; ++k0) {
                const double c0 = X_cell[0] + ((double)k0 + (AXIS == 0 ? -0.5 : 0.0)) * g.dx[0];
                const double c1 = X_cell[1] + ((double)k1 + (AXIS == 1 ? -0.5 : 0.0)) * g.dx[1];
                const double c2 = X_cell[2] + ((double)k2 + (AXIS == 2 ? -0.5 : 0.0)) * g.dx[2];
                const double wgt = (hat(X[0], c0, g.dx[0]) * hat(X[1], c1, g.dx[1])) * hat(X[2], c2, g.dx[2]);
                // the lower side of cell i + shift
                const int64_t off = (i[0] + k0 - g.glo[0]) + (int64_t)(i[1] + k1 - g.glo[1]) * s1 +
                                    (int64_t)(i[2] + k2 - g.glo[2]) * s2;
                U += u[off] * wgt;
            }
    return U;
}

// the largest of the lanes' values, in every lane
__device__ __forceinline__ double block_max(double v, double* s) {
    const int t = (int)threadIdx.x;
    __syncthreads();
    s[t] = v;
    for (int off = MTR_BLOCK / 2; off > 0; off >>= 1) {
        __syncthreads();
        if (t < off) s[t] = fmax(s[t], s[t + off]);
    }
    __syncthreads();
    return s[0];
}

// acc + b[0] + b[1] + ... in that order; eight elements are read before they are added, so the
// lane waits for LDS once in eight
__device__ __forceinline__ double serial_add(double acc, const double* b, int len) {
    int i = 0;
    for (; i + 8 <= len; i += 8) {
        const double x0 = b[i], x1 = b[i + 1], x2 = b[i + 2], x3 = b[i + 3], x4 = b[i + 4], x5 = b[i + 5], x6 = b[i + 6],
                     x7 = b[i + 7];
        acc += x0;
        acc += x1;
        acc += x2;
        acc += x3;
        acc += x4;
        acc += x5;
        acc += x6;
        acc += x7;
    }
    for (; i < len; ++i) acc += b[i];
    return acc;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// update: one workgroup per meter
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(MTR_BLOCK) void k_meter_update(MtrPlan M, MtrGrid g, MtrDomain D, const double* X) {
    __shared__ double s_red[MTR_BLOCK];
    __shared__ double s_Xc[3];
    const int l = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const int p0 = M.poff[l], P = M.poff[l + 1] - p0;
    double* const Xp = M.X_per + 3 * (int64_t)p0;

    // X_perimeter[l][n] = X[node] (:752)
    for (int e = t; e < 3 * P; e += MTR_BLOCK) {
        const int n = e / 3, d = e - 3 * n;
        Xp[e] = X[3 * (int64_t)M.node[p0 + n] + d];
    }
    __syncthreads();
    // the centroid: a serial sum from 0, then /= double(P) (:784-792) -- Eigen's v /= s multiplies
    // by Scalar(1) / s (SelfCwiseBinaryOp.h:181-193); a lane a component
    if (t < 3) {
        double v = 0.0;
        for (int n = 0; n < P; ++n) v += Xp[3 * n + t];
        v *= 1.0 / (double)P;
        s_Xc[t] = v;
        M.X_cen[3 * l + t] = v;
    }
    __syncthreads();
    const double Xc[3] = {s_Xc[0], s_Xc[1], s_Xc[2]};
    // r_max (:795-803); std::max keeps its first argument beside a NaN, as fmax does
    double r = 0.0;
    for (int n = t; n < P; n += MTR_BLOCK) {
        const double v[3] = {Xp[3 * n] - Xc[0], Xp[3 * n + 1] - Xc[1], Xp[3 * n + 2] - Xc[2]};
        r = fmax(r, norm3(v));
    }
    r = block_max(r, s_red);
    // num_web_nodes (:828)
    const double q = ceil(r / D.h_finest);
    const bool representable = q >= 0.0 && q <= 1.0e8;
    const int nw = representable ? 2 * (int)q : MTR_NW_BAD;
    if (t == 0) {
        M.nw[l] = nw;
        int ic[3];
        const bool in = locate(g, D, Xc, ic);  // :902-917
        int* const cc = M.cen_cell + 4 * l;
        cc[0] = ic[0];
        cc[1] = ic[1];
        cc[2] = ic[2];
        cc[3] = in ? 1 : 0;
        if (!representable || nw > M.cap) atomicOr(M.flags, MTR_FLAG);
    }
    if (!representable || nw > M.cap) return;  // the whole workgroup: the web does not fit

    // init_meter_elements (:133-194): patch (m, n) is the (m nw + n)-th of the meter
    const int64_t w0 = (int64_t)M.cap * p0;
    const double dnw = (double)nw;
    for (int e = t; e < P * nw; e += MTR_BLOCK) {
        const int m = e / nw, n = e - m * nw;
        const int m1 = (m + 1) % P;
        double Xa[3], Xb[3], X0[3], X1[3], X2[3], X3[3], l0[3], l1[3], d0[3], d1[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            Xa[d] = Xp[3 * m + d];
            Xb[d] = Xp[3 * m1 + d];
            const double dX0 = (Xc[d] - Xa[d]) / dnw;
            const double dX1 = (Xc[d] - Xb[d]) / dnw;
            X0[d] = Xa[d] + (double)n * dX0;
            X1[d] = Xb[d] + (double)n * dX1;
            X2[d] = Xb[d] + (double)(n + 1) * dX1;
            X3[d] = Xa[d] + (double)(n + 1) * dX0;
            const double X01 = 0.5 * (X0[d] + X1[d]);
            const double X12 = 0.5 * (X1[d] + X2[d]);
            const double X23 = 0.5 * (X2[d] + X3[d]);
            const double X30 = 0.5 * (X3[d] + X0[d]);
            l0[d] = X01;
            d0[d] = X23 - X01;
            l1[d] = X12;
            d1[d] = X30 - X12;
        }
        const double d0d0 = dot3(d0, d0);
        const double d0d1 = dot3(d0, d1);
        const double d1d1 = dot3(d1, d1);
        const double d0l0 = dot3(d0, l0);
        const double d0l1 = dot3(d0, l1);
        const double d1l0 = dot3(d1, l0);
        const double d1l1 = dot3(d1, l1);
        const double tt = (-d0l0 * d1d1 + d0l1 * d1d1 + d0d1 * d1l0 - d0d1 * d1l1) / (-d0d1 * d0d1 + d1d1 * d0d0);
        const double ss = (d1l0 * d0d0 - d0d1 * d0l0 + d0d1 * d0l1 - d1l1 * d0d0) / (-d0d1 * d0d1 + d1d1 * d0d0);
        double Xw[3], a[3], b[3], c[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            Xw[d] = 0.5 * (l0[d] + tt * d0[d] + l1[d] + ss * d1[d]);
            a[d] = X2[d] - X0[d];
            b[d] = X3[d] - X1[d];
        }
        cross3(a, b, c);
        int ic[3];
        const bool in = locate(g, D, Xw, ic);  // :880-897
        const int64_t k = w0 + e;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            M.X_web[3 * k + d] = Xw[d];
            M.dA_web[3 * k + d] = 0.5 * c[d];
            M.cell[3 * k + d] = ic[d];
        }
        M.counted[k] = in ? 1 : 0;
    }
}

hipError_t launch_meter_update(const MtrPlan& M, const MtrGrid& g, const MtrDomain& D, const double* X, hipStream_t s) {
    if (M.n_meters <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_meter_update, dim3((unsigned)M.n_meters), dim3(MTR_BLOCK), 0, s, M, g, D, X);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// read: one workgroup per meter
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(MTR_READ_BLOCK) void k_meter_read(MtrPlan M, MtrGrid g, const double* u0, const double* u1,
                                                          const double* u2, const double* p, const double* U,
                                                          double* values) {
    // the sort's keys; afterwards three staging buffers of MTR_CHUNK doubles, then the
    // correction's terms, one double a perimeter node (2 P <= P cap <= MTR_MAX_WEB)
    __shared__ unsigned long long s_key[MTR_MAX_WEB];
    __shared__ double s_sum[3], s_Uc[3];
    __shared__ int s_count;
    const int l = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const int p0 = M.poff[l], P = M.poff[l + 1] - p0;
    const int nw = M.nw[l];
    double* const out = values + 3 * (int64_t)l;
    if (nw == MTR_NW_BAD || nw > M.cap) {  // the web did not fit: flag 64 was latched by the update
        if (t < 3) out[t] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const int N = P * nw;
    const int64_t w0 = (int64_t)M.cap * p0;
    int npad = 1;
    while (npad < N) npad <<= 1;
    const int n0 = g.iupper[0] - g.ilower[0] + 1, n1 = g.iupper[1] - g.ilower[1] + 1;

    // keys: (linear index of the cell, x fastest; insertion index); an uncounted patch sorts last
    if (t == 0) s_count = 0;
    __syncthreads();
    for (int e = t; e < npad; e += MTR_READ_BLOCK) {
        unsigned long long key = ~0ULL;
        if (e < N && M.counted[w0 + e]) {
            const int ic[3] = {M.cell[3 * (w0 + e)], M.cell[3 * (w0 + e) + 1], M.cell[3 * (w0 + e) + 2]};
            if (in_box(g, ic)) {  // (always: read takes the update's box)
                const unsigned long long lin =
                    ((unsigned long long)(ic[2] - g.ilower[2]) * n1 + (ic[1] - g.ilower[1])) * n0 + (ic[0] - g.ilower[0]);
                key = (lin << MTR_WEB_BITS) | (unsigned)e;
                atomicAdd(&s_count, 1);
            }
        }
        s_key[e] = key;
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = t; e < npad; e += MTR_READ_BLOCK) {
                const int x = e ^ j;
                if (x > e) {
                    const unsigned long long a = s_key[e], b = s_key[x];
                    if ((a > b) == ((e & k) == 0)) {
                        s_key[e] = b;
                        s_key[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    const int count = s_count;

    // the terms of the patch at each sorted position (:997-1033)
    double* const tf = M.term + w0;
    double* const tp = M.term + M.total + w0;
    double* const ta = M.term + 2 * M.total + w0;
    for (int pos = t; pos < count; pos += MTR_READ_BLOCK) {
        const int64_t k = w0 + (int64_t)(s_key[pos] & (MTR_MAX_WEB - 1));
        const double X[3] = {M.X_web[3 * k], M.X_web[3 * k + 1], M.X_web[3 * k + 2]};
        const double dA[3] = {M.dA_web[3 * k], M.dA_web[3 * k + 1], M.dA_web[3 * k + 2]};
        const int ic[3] = {M.cell[3 * k], M.cell[3 * k + 1], M.cell[3 * k + 2]};
        double X_cell[3];
        cell_centre(g, ic, X_cell);
        if (u0) {
            const double Uw[3] = {interp_side<0>(g, u0, X, ic, X_cell), interp_side<1>(g, u1, X, ic, X_cell),
                                  interp_side<2>(g, u2, X, ic, X_cell)};
            tf[pos] = dot3(Uw, dA);
        }
        if (p) {
            const double a = norm3(dA);
            tp[pos] = interp_cell(g, p, X, ic, X_cell) * a;
            ta[pos] = a;
        }
    }
    __syncthreads();  // the terms are in memory, the keys are spent

    // The serial sums.  A lane that added straight from memory would wait for every element in
    // turn, so the first three waves stage MTR_CHUNK elements of a stream each in LDS with all
    // their lanes, and their first lanes add them serially from +0.0: wave 0 the flow's terms,
    // wave 1 those of P |dA|, wave 2 those of |dA|; before that, in the same way, the three
    // components of the perimeter's velocities for the centroid's (:1142-1150).
    double* const s_term = reinterpret_cast<double*>(s_key);
    const int wv = t >> 6, ln = t & 63;
    double* const s_buf = s_term + MTR_CHUNK * (wv < 3 ? wv : 0);
    double acc = 0.0;
    for (int base = 0; base < P; base += MTR_CHUNK) {
        const int len = min(MTR_CHUNK, P - base);
        if (wv < 3)
            for (int i = ln; i < len; i += 64) s_buf[i] = U[3 * (int64_t)M.node[p0 + base + i] + wv];
        __syncthreads();
        if (wv < 3 && ln == 0) acc = serial_add(acc, s_buf, len);
        __syncthreads();
    }
    if (wv < 3 && ln == 0) s_Uc[wv] = acc * (1.0 / (double)P);  // v /= s, as for the centroid
    const bool stream = wv < 3 && (wv == 0 ? u0 != nullptr : p != nullptr);
    const double* const src = wv == 0 ? tf : (wv == 1 ? tp : ta);
    acc = 0.0;
    for (int base = 0; base < count; base += MTR_CHUNK) {
        const int len = min(MTR_CHUNK, count - base);
        if (stream)
            for (int i = ln; i < len; i += 64) s_buf[i] = src[base + i];
        __syncthreads();
        if (stream && ln == 0) acc = serial_add(acc, s_buf, len);
        __syncthreads();
    }
    if (wv < 3 && ln == 0) s_sum[wv] = acc;
    __syncthreads();
    // the correction's terms (:214-231), a lane a perimeter node
    {
        const double* const Xp = M.X_per + 3 * (int64_t)p0;
        const double Xc[3] = {M.X_cen[3 * l], M.X_cen[3 * l + 1], M.X_cen[3 * l + 2]};
        for (int m = t; m < P; m += MTR_READ_BLOCK) {
            const int m1 = (m + 1) % P;
            const double* const Ua = U + 3 * (int64_t)M.node[p0 + m];
            const double* const Ub = U + 3 * (int64_t)M.node[p0 + m1];
            double Um[3], a[3], b[3], c[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                Um[d] = (Ua[d] + Ub[d] + s_Uc[d]) / 3.0;
                a[d] = Xc[d] - Xp[3 * m + d];
                b[d] = Xc[d] - Xp[3 * m1 + d];
            }
            cross3(a, b, c);
#pragma unroll
            for (int d = 0; d < 3; ++d) c[d] = 0.5 * c[d];
            s_term[m] = dot3(Um, c);
        }
    }
    __syncthreads();
    if (t == 0) {
        double corr = 0.0;
        for (int m = 0; m < P; ++m) corr += s_term[m];
        out[0] = s_sum[0] - corr;       // :1155
        out[1] = s_sum[1] / s_sum[2];   // :1073
        double point = 0.0;
        const int* const cc = M.cen_cell + 4 * l;
        const int ic[3] = {cc[0], cc[1], cc[2]};
        if (p && cc[3] && in_box(g, ic)) {  // :1047-1057
            const double Xc[3] = {M.X_cen[3 * l], M.X_cen[3 * l + 1], M.X_cen[3 * l + 2]};
            double X_cell[3];
            cell_centre(g, ic, X_cell);
            point = interp_cell(g, p, Xc, ic, X_cell);
        }
        out[2] = point;
    }
}

hipError_t launch_meter_read(const MtrPlan& M, const MtrGrid& g, const double* const u[3], const double* p, const double* U,
                             double* values, hipStream_t s) {
    if (M.n_meters <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_meter_read, dim3((unsigned)M.n_meters), dim3(MTR_READ_BLOCK), 0, s, M, g, u ? u[0] : nullptr,
                       u ? u[1] : nullptr, u ? u[2] : nullptr, p, U, values);
    return hipGetLastError();
}

}  // namespace ibtk_le

// ---------------------------------------------------------------------------
// The C ABI.  create validates the host arrays, lays the perimeter nodes out by meter and
// perimeter position, and allocates everything the device calls use; update and read are
// one launch each on the context stream: no allocation, no host synchronisation.
// ---------------------------------------------------------------------------
using namespace ibtk_le;

#define MTR_HIP_TRY(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return abi_fail(IBTK_LE_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct ibtk_le_meters_s {
    ibtk_le_ctx ctx = nullptr;
    int n_nodes = 0, n_meters = 0, n_per = 0, cap = 0;
    long long total = 0;
    bool updated = false;
    int ilower[3] = {0, 0, 0}, iupper[3] = {0, 0, 0};  // the box of the last update
    int* poff = nullptr;
    int* node = nullptr;
    double* X_per = nullptr;
    double* X_cen = nullptr;
    int* nw = nullptr;
    int* cen_cell = nullptr;
    double* X_web = nullptr;
    double* dA_web = nullptr;
    int* cell = nullptr;
    int* counted = nullptr;
    double* term = nullptr;
};

namespace {

void mtr_free(ibtk_le_meters mt) {
    for (void* p : {(void*)mt->poff, (void*)mt->node, (void*)mt->X_per, (void*)mt->X_cen, (void*)mt->nw, (void*)mt->cen_cell,
                    (void*)mt->X_web, (void*)mt->dA_web, (void*)mt->cell, (void*)mt->counted, (void*)mt->term})
        if (p) (void)hipFree(p);
}

int mtr_common(const char* what, ibtk_le_ctx ctx, ibtk_le_meters mt) {
    if (!ctx) return abi_fail(IBTK_LE_ERR_ARG, "%s: null context", what);
    if (!mt) return abi_fail(IBTK_LE_ERR_ARG, "%s: null meter plan", what);
    if (ctx != mt->ctx) return abi_fail(IBTK_LE_ERR_ARG, "%s: the plan was created on another context", what);
    return IBTK_LE_OK;
}

// empty: the patch box holds no cell, nothing to do (IBTK_LE_OK)
int mtr_geom(const char* what, const ibtk_le_patch_geom* geom, bool& empty) {
    empty = false;
    if (!geom) return abi_fail(IBTK_LE_ERR_ARG, "%s: null geometry", what);
    // the reference aborts in 2-D: "no support for 2D flow meters at this time!" (:121-127)
    if (geom->ndim != 3) return abi_fail(IBTK_LE_ERR_ARG, "%s: flow meters need a 3-D patch (got ndim %d)", what, geom->ndim);
    long long cells = 1;
    for (int d = 0; d < 3; ++d) {
        if (!std::isfinite(geom->dx[d]) || !(geom->dx[d] > 0.0))
            return abi_fail(IBTK_LE_ERR_ARG, "%s: dx[%d] must be finite and positive", what, d);
        if (!std::isfinite(geom->x_lower[d]) || !std::isfinite(geom->x_upper[d]))
            return abi_fail(IBTK_LE_ERR_ARG, "%s: x_lower / x_upper[%d] is not finite", what, d);
        if (geom->gcw[d] < 0) return abi_fail(IBTK_LE_ERR_ARG, "%s: negative ghost width", what);
        if (geom->iupper[d] < geom->ilower[d]) empty = true;
    }
    if (empty) return IBTK_LE_OK;
    for (int d = 0; d < 3; ++d) {
        const long long n = (long long)geom->iupper[d] - geom->ilower[d] + 1;
        if (n > (1LL << 50) / cells) return abi_fail(IBTK_LE_ERR_RANGE, "%s: the patch box exceeds 2^50 cells", what);
        cells *= n;
    }
    if (geom->pitch[0] || geom->pitch[1]) {
        // the pitch covers the widest array of the patch (the ghosted box + 1 face), as everywhere
        const long long n0 = (long long)geom->iupper[0] - geom->ilower[0] + 2 + 2LL * geom->gcw[0];
        const long long n1 = (long long)geom->iupper[1] - geom->ilower[1] + 2 + 2LL * geom->gcw[1];
        if (geom->pitch[0] < n0 || (geom->pitch[1] != 0 && geom->pitch[1] < n1))
            return abi_fail(IBTK_LE_ERR_ARG, "%s: array pitch {%d, %d} below the ghosted extent {%lld, %lld} (+1 face)", what,
                            geom->pitch[0], geom->pitch[1], n0, n1);
    }
    return IBTK_LE_OK;
}

void mtr_grid(const ibtk_le_patch_geom* geom, MtrGrid& g) {
    g = MtrGrid{};
    const bool packed = geom->pitch[0] == 0 && geom->pitch[1] == 0;
    for (int d = 0; d < 3; ++d) {
        g.ilower[d] = geom->ilower[d];
        g.iupper[d] = geom->iupper[d];
        g.glo[d] = geom->ilower[d] - geom->gcw[d];
        g.dx[d] = geom->dx[d];
        g.xlo[d] = geom->x_lower[d];
    }
    // a < 3: the side array of axis a (+ 1 along a); 3: the cell array
    for (int a = 0; a < 4; ++a) {
        int64_t n[3];
        for (int d = 0; d < 3; ++d) n[d] = (int64_t)geom->iupper[d] - geom->ilower[d] + 1 + 2 * (int64_t)geom->gcw[d] + (d == a ? 1 : 0);
        const int64_t s1 = packed ? n[0] : geom->pitch[0];
        const int64_t s2 = s1 * (packed || geom->pitch[1] == 0 ? n[1] : geom->pitch[1]);
        if (a < 3) {
            g.us1[a] = s1;
            g.us2[a] = s2;
        } else {
            g.ps1 = s1;
            g.ps2 = s2;
        }
    }
}

void mtr_plan(ibtk_le_meters mt, MtrPlan& M) {
    M = MtrPlan{};
    M.n_meters = mt->n_meters;
    M.cap = mt->cap;
    M.total = mt->total;
    M.poff = mt->poff;
    M.node = mt->node;
    M.X_per = mt->X_per;
    M.X_cen = mt->X_cen;
    M.nw = mt->nw;
    M.cen_cell = mt->cen_cell;
    M.X_web = mt->X_web;
    M.dA_web = mt->dA_web;
    M.cell = mt->cell;
    M.counted = mt->counted;
    M.term = mt->term;
    M.flags = abi_ctx_flags(mt->ctx);
}

}  // namespace

extern "C" int ibtk_le_meters_create(ibtk_le_ctx ctx, int n_nodes, int n_meters, int n_pts, const int* node, const int* meter,
                                     const int* meter_node, int max_web_nodes, ibtk_le_meters* out) {
    if (!ctx) return abi_fail(IBTK_LE_ERR_ARG, "meters_create: null context");
    if (!out) return abi_fail(IBTK_LE_ERR_ARG, "meters_create: null out");
    if (n_nodes < 0 || n_meters < 0 || n_pts < 0)
        return abi_fail(IBTK_LE_ERR_ARG, "meters_create: negative count (%d nodes, %d meters, %d instrumented points)", n_nodes,
                        n_meters, n_pts);
    if (n_pts > 0 && (!node || !meter || !meter_node)) return abi_fail(IBTK_LE_ERR_ARG, "meters_create: null array");
    if (max_web_nodes < 2 || max_web_nodes % 2 != 0)
        return abi_fail(IBTK_LE_ERR_ARG, "meters_create: max_web_nodes must be even and at least 2 (got %d)", max_web_nodes);
    // P_l = 1 + the largest node index of meter l (:589-625)
    std::vector<int> P((size_t)n_meters, 0);
    std::vector<char> seen((size_t)n_nodes, 0);
    for (int k = 0; k < n_pts; ++k) {
        if (node[k] < 0 || node[k] >= n_nodes)
            return abi_fail(IBTK_LE_ERR_ARG, "instrumented point %d: node index %d is out of range [0, %d)", k, node[k], n_nodes);
        if (meter[k] < 0 || meter[k] >= n_meters)
            return abi_fail(IBTK_LE_ERR_ARG, "instrumented point %d: meter index %d is out of range [0, %d)", k, meter[k], n_meters);
        if (meter_node[k] < 0 || meter_node[k] >= MTR_MAX_WEB)
            return abi_fail(IBTK_LE_ERR_ARG, "instrumented point %d: meter node index %d is out of range [0, %d)", k, meter_node[k],
                            MTR_MAX_WEB);
        if (seen[node[k]]) return abi_fail(IBTK_LE_ERR_ARG, "instrumented point %d: node %d is named twice", k, node[k]);
        seen[node[k]] = 1;
        P[meter[k]] = std::max(P[meter[k]], meter_node[k] + 1);
    }
    std::vector<int> poff((size_t)n_meters + 1, 0);
    for (int l = 0; l < n_meters; ++l) {
        if (P[l] == 0) return abi_fail(IBTK_LE_ERR_ARG, "meters_create: meter %d has no perimeter node", l);
        if ((long long)P[l] * max_web_nodes > MTR_MAX_WEB)
            return abi_fail(IBTK_LE_ERR_ARG, "meters_create: meter %d: %d perimeter nodes times max_web_nodes %d exceeds %d web patches",
                            l, P[l], max_web_nodes, MTR_MAX_WEB);
        poff[l + 1] = poff[l] + P[l];
    }
    const int n_per = poff[n_meters];
    if ((long long)n_per * max_web_nodes > INT_MAX / 4) return abi_fail(IBTK_LE_ERR_RANGE, "meters_create: %d perimeter nodes", n_per);
    std::vector<int> nodes((size_t)n_per, -1);
    for (int k = 0; k < n_pts; ++k) {
        int& slot = nodes[(size_t)poff[meter[k]] + meter_node[k]];
        if (slot >= 0)
            return abi_fail(IBTK_LE_ERR_ARG, "instrumented point %d: node index %d of meter %d is named twice", k, meter_node[k],
                            meter[k]);
        slot = node[k];
    }
    for (int l = 0; l < n_meters; ++l)
        for (int n = 0; n < P[l]; ++n)
            if (nodes[(size_t)poff[l] + n] < 0)
                return abi_fail(IBTK_LE_ERR_ARG, "meters_create: node index %d of meter %d is missing", n, l);

    auto* mt = new ibtk_le_meters_s();
    mt->ctx = ctx;
    mt->n_nodes = n_nodes;
    mt->n_meters = n_meters;
    mt->n_per = n_per;
    mt->cap = max_web_nodes;
    mt->total = (long long)n_per * max_web_nodes;
    int device;
    hipStream_t stream;
    abi_ctx_device_stream(ctx, &device, &stream);
    const size_t nl = (size_t)std::max(n_meters, 1), np = (size_t)std::max(n_per, 1), nt = (size_t)std::max(mt->total, 1LL);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)&mt->poff, (nl + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->node, np * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->X_per, 3 * np * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->X_cen, 3 * nl * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->nw, nl * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->cen_cell, 4 * nl * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->X_web, 3 * nt * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->dA_web, 3 * nt * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->cell, 3 * nt * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->counted, nt * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&mt->term, 3 * nt * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(mt->poff, poff.data(), poff.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_per > 0) e = hipMemcpy(mt->node, nodes.data(), (size_t)n_per * sizeof(int), hipMemcpyHostToDevice);
    // until the first update: webs of no patch, so a read gives the values of nw = 0
    if (e == hipSuccess) e = hipMemset(mt->nw, 0, nl * sizeof(int));
    if (e == hipSuccess) e = hipMemset(mt->cen_cell, 0, 4 * nl * sizeof(int));
    if (e == hipSuccess) e = hipMemset(mt->X_per, 0, 3 * np * sizeof(double));
    if (e == hipSuccess) e = hipMemset(mt->X_cen, 0, 3 * nl * sizeof(double));
    if (e != hipSuccess) {
        mtr_free(mt);
        delete mt;
        return abi_fail(e == hipErrorOutOfMemory ? IBTK_LE_ERR_NOMEM : IBTK_LE_ERR_DEVICE, "meters_create: %s", hipGetErrorString(e));
    }
    *out = mt;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_meters_destroy(ibtk_le_meters mt) {
    if (!mt) return IBTK_LE_OK;
    int device;
    hipStream_t stream;
    abi_ctx_device_stream(mt->ctx, &device, &stream);
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);  // a call in flight may still read the plan
    mtr_free(mt);
    delete mt;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_meters_update(ibtk_le_ctx ctx, ibtk_le_meters mt, const ibtk_le_patch_geom* geom, const int* dom_lo,
                                     const int* dom_hi, const double* dom_xlo, const double* dom_xup, double h_finest,
                                     const double* X_dev) {
    bool empty;
    if (int rc = mtr_common("meters_update", ctx, mt)) return rc;
    if (int rc = mtr_geom("meters_update", geom, empty)) return rc;
    if (!dom_lo || !dom_hi || !dom_xlo || !dom_xup) return abi_fail(IBTK_LE_ERR_ARG, "meters_update: null domain");
    for (int d = 0; d < 3; ++d) {
        if (dom_hi[d] < dom_lo[d]) return abi_fail(IBTK_LE_ERR_ARG, "meters_update: empty domain box in dim %d", d);
        if (!std::isfinite(dom_xlo[d]) || !std::isfinite(dom_xup[d]))
            return abi_fail(IBTK_LE_ERR_ARG, "meters_update: the domain's x_lower / x_upper[%d] is not finite", d);
    }
    if (!std::isfinite(h_finest) || !(h_finest > 0.0)) return abi_fail(IBTK_LE_ERR_ARG, "meters_update: h_finest must be finite and positive");
    if (mt->n_meters == 0 || empty) return IBTK_LE_OK;
    if (!X_dev) return abi_fail(IBTK_LE_ERR_ARG, "meters_update: null array");
    MtrPlan M;
    mtr_plan(mt, M);
    MtrGrid g;
    mtr_grid(geom, g);
    MtrDomain D{};
    for (int d = 0; d < 3; ++d) {
        D.lo[d] = dom_lo[d];
        D.hi[d] = dom_hi[d];
        D.xlo[d] = dom_xlo[d];
        D.xup[d] = dom_xup[d];
    }
    D.h_finest = h_finest;
    int device;
    hipStream_t stream;
    abi_ctx_device_stream(ctx, &device, &stream);
    MTR_HIP_TRY(hipSetDevice(device));
    MTR_HIP_TRY(launch_meter_update(M, g, D, X_dev, stream));
    mt->updated = true;
    for (int d = 0; d < 3; ++d) {
        mt->ilower[d] = geom->ilower[d];
        mt->iupper[d] = geom->iupper[d];
    }
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_meters_read(ibtk_le_ctx ctx, ibtk_le_meters mt, const ibtk_le_patch_geom* geom, const double* const* u_dev,
                                   const double* p_dev, const double* U_dev, double* values_dev) {
    bool empty;
    if (int rc = mtr_common("meters_read", ctx, mt)) return rc;
    if (int rc = mtr_geom("meters_read", geom, empty)) return rc;
    if (u_dev && (!u_dev[0] || !u_dev[1] || !u_dev[2])) return abi_fail(IBTK_LE_ERR_ARG, "meters_read: null side array");
    if (mt->n_meters == 0 || empty) return IBTK_LE_OK;
    if (!U_dev || !values_dev) return abi_fail(IBTK_LE_ERR_ARG, "meters_read: null array");
    if (!mt->updated) return abi_fail(IBTK_LE_ERR_ARG, "meters_read: no ibtk_le_meters_update before it");
    for (int d = 0; d < 3; ++d) {
        if (geom->ilower[d] != mt->ilower[d] || geom->iupper[d] != mt->iupper[d])
            return abi_fail(IBTK_LE_ERR_ARG, "meters_read: the patch box differs from the last update's in dim %d", d);
        // the interpolation rules read one layer around a cell of the patch box
        if ((u_dev || p_dev) && geom->gcw[d] < 1)
            return abi_fail(IBTK_LE_ERR_GHOST_WIDTH, "meters_read: insufficient ghost cells: a ghost width of 1 is needed in dim %d", d);
    }
    MtrPlan M;
    mtr_plan(mt, M);
    MtrGrid g;
    mtr_grid(geom, g);
    int device;
    hipStream_t stream;
    abi_ctx_device_stream(ctx, &device, &stream);
    MTR_HIP_TRY(hipSetDevice(device));
    MTR_HIP_TRY(launch_meter_read(M, g, u_dev, p_dev, U_dev, values_dev, stream));
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_meters_workspace(ibtk_le_ctx ctx, ibtk_le_meters mt, int which, void* dst_dev, long long count) {
    if (int rc = mtr_common("meters_workspace", ctx, mt)) return rc;
    const long long L = mt->n_meters, W = mt->total, S = mt->n_per;
    const void* src = nullptr;
    long long n = 0;
    size_t size = sizeof(double);
    switch (which) {
        case IBTK_LE_METERS_X_CENTROID: src = mt->X_cen, n = 3 * L; break;
        case IBTK_LE_METERS_NUM_WEB_NODES: src = mt->nw, n = L, size = sizeof(int); break;
        case IBTK_LE_METERS_X_WEB: src = mt->X_web, n = 3 * W; break;
        case IBTK_LE_METERS_DA_WEB: src = mt->dA_web, n = 3 * W; break;
        case IBTK_LE_METERS_CELL: src = mt->cell, n = 3 * W, size = sizeof(int); break;
        case IBTK_LE_METERS_COUNTED: src = mt->counted, n = W, size = sizeof(int); break;
        case IBTK_LE_METERS_CENTROID_CELL: src = mt->cen_cell, n = 4 * L, size = sizeof(int); break;
        case IBTK_LE_METERS_X_PERIMETER: src = mt->X_per, n = 3 * S; break;
        default: return abi_fail(IBTK_LE_ERR_ARG, "meters_workspace: unknown array %d", which);
    }
    if (count != n) return abi_fail(IBTK_LE_ERR_ARG, "meters_workspace: array %d holds %lld elements, not %lld", which, n, count);
    if (n == 0) return IBTK_LE_OK;
    if (!dst_dev) return abi_fail(IBTK_LE_ERR_ARG, "meters_workspace: null array");
    int device;
    hipStream_t stream;
    abi_ctx_device_stream(ctx, &device, &stream);
    MTR_HIP_TRY(hipSetDevice(device));
    MTR_HIP_TRY(hipMemcpyAsync(dst_dev, src, (size_t)n * size, hipMemcpyDeviceToDevice, stream));
    return IBTK_LE_OK;
}
