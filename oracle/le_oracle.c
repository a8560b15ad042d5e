/*
 * le_oracle.c -- CPU restatement of IBAMR's Lagrangian-Eulerian interaction
 * kernels (TEST INFRASTRUCTURE ONLY).
 *
 * This file is the parity oracle for the MI355X path.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it, and
 * only as the checker / the timed CPU baseline; the product library
 * (ibamr_amd/lib/libibtk_le.so) never links, calls or falls back to it.
 *
 * PARITY STATUS: pinned to the reference's own Fortran.  The reference routines
 * live in
 *   ibtk/src/lagrangian/fortran/lagrangian_interaction{2,3}d.f.m4
 *   ibtk/src/lagrangian/fortran/lagrangian_delta.f.m4
 * oracle/build_ref.py expands their few m4 macros and compiles them with flang
 * into oracle/_ref/ (never committed); tests/test_ref_pin.py holds this file
 * bitwise equal to that library at -O0 (IB_6 at -O2 only within 1e-13 / 1e-12:
 * the order of its integer powers is the compiler's).  Two deliberate
 * deviations are kept apart from the pin: DISCONTINUOUS_LINEAR 3-D spread and
 * PIECEWISE_CONSTANT markers outside the ghost box (both noted below).  The
 * reference ships no tests, fixtures or recorded outputs for this path
 * (SURVEY.md F4); the kernels' published analytic identities and hand-derived
 * known-answer vectors (tests/golden/, tests/test_oracle_*.py) hold it too.
 *
 * Every routine follows the Fortran text operation by operation (loop order,
 * left-to-right association, NINT = round-half-away-from-zero, division by dx,
 * ghost-box clipping) and cites the file:line it restates.  Compile with
 * -ffp-contract=off so no multiply-add is fused.
 *
 * Array conventions (Fortran, column-major):
 *   u(ilower0-nugc0:iupper0+nugc0, ilower1-nugc1:..., [ilower2-...,] 0:depth-1)
 *   X(0:NDIM-1, 0:*), Xshift(0:NDIM-1, 0:nindices-1), V(0:depth-1, 0:*)
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "le_oracle.h"

/* ---------------------------------------------------------------------- */
/* scalar helpers                                                          */
/* ---------------------------------------------------------------------- */

/* Fortran NINT: nearest integer, halves rounded away from zero. */
static inline int ora_nint(double x) { return (int)round(x); }

/* lagrangian_floor, lagrangian_delta.f.m4:45-58: int(x) - (x < 0).  Note this
 * is NOT floor() at negative integers (it returns -3 for -2.0). */
int ora_lagrangian_floor(double x)
{
    int f = (int)x; /* Fortran int() truncates toward zero */
    if (x < 0.0) f = f - 1;
    return f;
}

/* lagrangian_piecewise_cubic_delta, lagrangian_delta.f.m4:109-130 */
double ora_piecewise_cubic_delta(double r)
{
    if (r < 0.0) r = -r;
    if (r < 1.0) return 1.0 - 0.5 * r - r * r + 0.5 * r * r * r;
    if (r < 2.0) return 1.0 - (11.0 / 6.0) * r + r * r - (1.0 / 6.0) * r * r * r;
    return 0.0;
}

/* lagrangian_ib_3_delta, lagrangian_delta.f.m4:158-180 (its truncated
 * constants sixth/third are kept verbatim). */
double ora_ib_3_delta(double r)
{
    const double sixth = 0.16666666666667;
    const double third = 0.333333333333333;
    if (r < 0.0) r = -r;
    if (r < 0.5) return third * (1.0 + sqrt(1.0 - 3.0 * r * r));
    if (r < 1.5) return sixth * (5.0 - 3.0 * r - sqrt(1.0 - 3.0 * (1.0 - r) * (1.0 - r)));
    return 0.0;
}

/* x**n for the small constant integer powers in the IB_6 formulas, evaluated
 * by binary powering (x^3 = x*x^2, x^4 = (x^2)^2, x^6 = x^2*x^4).  The GPU
 * kernels use the identical helper. */
static inline double ora_powi(double x, int n)
{
    double res = 1.0, cur = x;
    int first = 1;
    while (n) {
        if (n & 1) {
            res = first ? cur : res * cur;
            first = 0;
        }
        n >>= 1;
        if (n) cur = cur * cur;
    }
    return res;
}

/* IB_6 parameter K, lagrangian_interaction3d.f.m4:1893 */
static double ora_ib6_K(void) { return (59.0 / 60.0) * (1.0 - sqrt(1.0 - (3220.0 / 3481.0))); }

/* ---------------------------------------------------------------------- */
/* 1-D weights of the NINT-anchored closed-form kernels                    */
/* ---------------------------------------------------------------------- */

/* Returns ic_lower (absolute index) and fills w[0..W-1].
 * IB_4:     lagrangian_interaction3d.f.m4:1316-1324
 * IB_4_W8:  lagrangian_interaction3d.f.m4:1594-1610
 * IB_6:     lagrangian_interaction3d.f.m4:1914-1945
 * BSPLINE_4 (not in the reference): cubic B-spline on the
 *           IB_4 stencil, phi(r) = 2/3 - r^2 + |r|^3/2 (|r|<1),
 *           (2-|r|)^3/6 (1<=|r|<2). */
int ora_closed_form_weights(int kernel, double X_o_dx, int ilower, double* w)
{
    const int n = ora_nint(X_o_dx);
    int ic_lower;
    double r, q;
    switch (kernel) {
    case LE_IB_4:
        ic_lower = n + ilower - 2;
        r = X_o_dx - ((double)(ic_lower + 1 - ilower) + 0.5);
        q = sqrt(1.0 + 4.0 * r * (1.0 - r));
        w[0] = 0.125 * (3.0 - 2.0 * r - q);
        w[1] = 0.125 * (3.0 - 2.0 * r + q);
        w[2] = 0.125 * (1.0 + 2.0 * r + q);
        w[3] = 0.125 * (1.0 + 2.0 * r - q);
        return ic_lower;
    case LE_BSPLINE_4: {
        ic_lower = n + ilower - 2;
        r = X_o_dx - ((double)(ic_lower + 1 - ilower) + 0.5);
        const double s = 1.0 - r;
        w[0] = (s * s * s) / 6.0;
        w[1] = (2.0 / 3.0) - r * r + 0.5 * (r * r * r);
        w[2] = (2.0 / 3.0) - s * s + 0.5 * (s * s * s);
        w[3] = (r * r * r) / 6.0;
        return ic_lower;
    }
    case LE_IB_4_W8:
        ic_lower = n + ilower - 4;
        r = 0.5 * (X_o_dx - ((double)(ic_lower + 3 - ilower) + 0.5));
        q = sqrt(1.0 + 4.0 * r * (1.0 - r));
        w[1] = 0.0625 * (3.0 - 2.0 * r - q);
        w[3] = 0.0625 * (3.0 - 2.0 * r + q);
        w[5] = 0.0625 * (1.0 + 2.0 * r + q);
        w[7] = 0.0625 * (1.0 + 2.0 * r - q);
        r = r + 0.5;
        q = sqrt(1.0 + 4.0 * r * (1.0 - r));
        w[0] = 0.0625 * (3.0 - 2.0 * r - q);
        w[2] = 0.0625 * (3.0 - 2.0 * r + q);
        w[4] = 0.0625 * (1.0 + 2.0 * r + q);
        w[6] = 0.0625 * (1.0 + 2.0 * r - q);
        return ic_lower;
    case LE_IB_6: {
        const double K = ora_ib6_K();
        ic_lower = n + ilower - 3;
        r = 1.0 - X_o_dx + ((double)(ic_lower + 2 - ilower) + 0.5);
        const double r2 = ora_powi(r, 2), r3 = ora_powi(r, 3);
        const double r4 = ora_powi(r, 4), r6 = ora_powi(r, 6);
        const double alpha = 28.0;
        const double beta = (9.0 / 4.0) - (3.0 / 2.0) * (K + r2) + ((22.0 / 3.0) - 7.0 * K) * r - (7.0 / 3.0) * r3;
        const double gamma = (1.0 / 4.0) * (((161.0 / 36.0) - (59.0 / 6.0) * K + 5.0 * ora_powi(K, 2)) * (1.0 / 2.0) * r2 +
                                             (-(109.0 / 24.0) + 5.0 * K) * (1.0 / 3.0) * r4 + (5.0 / 18.0) * r6);
        const double discr = beta * beta - 4.0 * alpha * gamma;
        const double sgn = ((3.0 / 2.0) - K) >= 0.0 ? 1.0 : -1.0; /* Fortran sign(1,x) */
        const double pm3 = (-beta + sgn * sqrt(discr)) / (2.0 * alpha);
        const double pm2 = -3.0 * pm3 - (1.0 / 16.0) + (1.0 / 8.0) * (K + r2) + (1.0 / 12.0) * (3.0 * K - 1.0) * r +
                           (1.0 / 12.0) * r3;
        const double pm1 = 2.0 * pm3 + (1.0 / 4.0) + (1.0 / 6.0) * (4.0 - 3.0 * K) * r - (1.0 / 6.0) * r3;
        const double p = 2.0 * pm3 + (5.0 / 8.0) - (1.0 / 4.0) * (K + r2);
        const double pp1 = -3.0 * pm3 + (1.0 / 4.0) - (1.0 / 6.0) * (4.0 - 3.0 * K) * r + (1.0 / 6.0) * r3;
        const double pp2 = pm3 - (1.0 / 16.0) + (1.0 / 8.0) * (K + r2) - (1.0 / 12.0) * (3.0 * K - 1.0) * r -
                           (1.0 / 12.0) * r3;
        w[0] = pm3;
        w[1] = pm2;
        w[2] = pm1;
        w[3] = p;
        w[4] = pp1;
        w[5] = pp2;
        return ic_lower;
    }
    default:
        return 0;
    }
}

int ora_stencil_size(int kernel)
{
    /* LEInteractor::getStencilSize, LEInteractor.cpp:668-682 (+ BSPLINE_4) */
    switch (kernel) {
    case LE_PIECEWISE_CONSTANT: return 1;
    case LE_DISCONTINUOUS_LINEAR: return 2;
    case LE_PIECEWISE_LINEAR: return 2;
    case LE_PIECEWISE_CUBIC: return 4;
    case LE_IB_3: return 4;
    case LE_IB_4: return 4;
    case LE_IB_4_W8: return 8;
    case LE_IB_6: return 6;
    case LE_BSPLINE_4: return 4;
    default: return -1;
    }
}

static inline int ora_is_closed_form(int k)
{
    return k == LE_IB_4 || k == LE_IB_4_W8 || k == LE_IB_6 || k == LE_BSPLINE_4;
}

static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int imin(int a, int b) { return a < b ? a : b; }

/* ---------------------------------------------------------------------- */
/* geometry of one patch array                                             */
/* ---------------------------------------------------------------------- */
typedef struct {
    int ndim;
    int lo[3], hi[3]; /* ghost box bounds (inclusive) */
    int64_t n[3];     /* ghost box extents */
} ora_box;

static void ora_box_init(ora_box* b, int ndim, const int* ilower, const int* iupper, const int* nugc)
{
    b->ndim = ndim;
    for (int d = 0; d < 3; ++d) {
        if (d < ndim) {
            b->lo[d] = ilower[d] - nugc[d];
            b->hi[d] = iupper[d] + nugc[d];
        } else {
            b->lo[d] = 0;
            b->hi[d] = 0;
        }
        b->n[d] = (int64_t)(b->hi[d] - b->lo[d] + 1);
    }
}

static inline int64_t ora_idx(const ora_box* b, int i0, int i1, int i2, int d)
{
    return (((int64_t)d * b->n[2] + (i2 - b->lo[2])) * b->n[1] + (i1 - b->lo[1])) * b->n[0] + (i0 - b->lo[0]);
}

/* ---------------------------------------------------------------------- */
/* closed-form kernels (IB_4, IB_4_W8, IB_6, BSPLINE_4)                    */
/* interp: lagrangian_interaction3d.f.m4:1310-1382 (IB_4), 1588-1688,       */
/*         1907-2048; 2D: lagrangian_interaction2d.f.m4:1214-1270 etc.      */
/* spread: lagrangian_interaction3d.f.m4:1447-1519, 1762-1850, 2073-2255    */
/* ---------------------------------------------------------------------- */
static void ora_closed_form(int kernel, int spread, const ora_box* b, const double* dx, const double* x_lower,
                            int depth, const int* ilower, double* u, const int* indices, const double* Xshift,
                            int nindices, const double* X, double* V)
{
    const int ndim = b->ndim;
    const int W = ora_stencil_size(kernel);
    double w[3][8];
    int icl[3], ist[3], isp[3];
    const double h3 = ndim == 3 ? (dx[0] * dx[1] * dx[2]) : (dx[0] * dx[1]);
    for (int l = 0; l < nindices; ++l) {
        const int s = indices[l];
        for (int d = 0; d < ndim; ++d) {
            const double X_o_dx = (X[(int64_t)ndim * s + d] + Xshift[(int64_t)ndim * l + d] - x_lower[d]) / dx[d];
            icl[d] = ora_closed_form_weights(kernel, X_o_dx, ilower[d], w[d]);
            const int icu = icl[d] + (W - 1);
            ist[d] = imax(b->lo[d] - icl[d], 0);
            isp[d] = (W - 1) - imax(icu - b->hi[d], 0);
        }
        if (ndim == 3) {
            double wt[8][8][8];
            for (int i2 = 0; i2 < W; ++i2) {
                const double wz = spread ? w[2][i2] / h3 : w[2][i2];
                for (int i1 = 0; i1 < W; ++i1) {
                    const double wyz = w[1][i1] * wz;
                    for (int i0 = 0; i0 < W; ++i0) wt[i2][i1][i0] = w[0][i0] * wyz;
                }
            }
            for (int d = 0; d < depth; ++d) {
                if (!spread) {
                    double acc = 0.0;
                    for (int i2 = ist[2]; i2 <= isp[2]; ++i2)
                        for (int i1 = ist[1]; i1 <= isp[1]; ++i1)
                            for (int i0 = ist[0]; i0 <= isp[0]; ++i0)
                                acc = acc + wt[i2][i1][i0] * u[ora_idx(b, icl[0] + i0, icl[1] + i1, icl[2] + i2, d)];
                    V[(int64_t)depth * s + d] = acc;
                } else {
                    const double Vd = V[(int64_t)depth * s + d];
                    for (int i2 = ist[2]; i2 <= isp[2]; ++i2)
                        for (int i1 = ist[1]; i1 <= isp[1]; ++i1)
                            for (int i0 = ist[0]; i0 <= isp[0]; ++i0) {
                                const int64_t k = ora_idx(b, icl[0] + i0, icl[1] + i1, icl[2] + i2, d);
                                u[k] = u[k] + wt[i2][i1][i0] * Vd;
                            }
                }
            }
        } else {
            double wt[8][8];
            for (int i1 = 0; i1 < W; ++i1) {
                const double wy = spread ? w[1][i1] / h3 : w[1][i1];
                for (int i0 = 0; i0 < W; ++i0) wt[i1][i0] = w[0][i0] * wy;
            }
            for (int d = 0; d < depth; ++d) {
                if (!spread) {
                    double acc = 0.0;
                    for (int i1 = ist[1]; i1 <= isp[1]; ++i1)
                        for (int i0 = ist[0]; i0 <= isp[0]; ++i0)
                            acc = acc + wt[i1][i0] * u[ora_idx(b, icl[0] + i0, icl[1] + i1, 0, d)];
                    V[(int64_t)depth * s + d] = acc;
                } else {
                    const double Vd = V[(int64_t)depth * s + d];
                    for (int i1 = ist[1]; i1 <= isp[1]; ++i1)
                        for (int i0 = ist[0]; i0 <= isp[0]; ++i0) {
                            const int64_t k = ora_idx(b, icl[0] + i0, icl[1] + i1, 0, d);
                            u[k] = u[k] + wt[i1][i0] * Vd;
                        }
                }
            }
        }
    }
}

/* ---------------------------------------------------------------------- */
/* piecewise constant: lagrangian_interaction3d.f.m4:49-179 (no clipping)  */
/* ---------------------------------------------------------------------- */
static void ora_piecewise_constant(int spread, const ora_box* b, const double* dx, const double* x_lower, int depth,
                                   const int* ilower, double* u, const int* indices, const double* Xshift,
                                   int nindices, const double* X, double* V)
{
    const int ndim = b->ndim;
    const double h3 = ndim == 3 ? (dx[0] * dx[1] * dx[2]) : (dx[0] * dx[1]);
    for (int l = 0; l < nindices; ++l) {
        const int s = indices[l];
        int ic[3] = {0, 0, 0};
        for (int d = 0; d < ndim; ++d)
            ic[d] = ora_nint((X[(int64_t)ndim * s + d] + Xshift[(int64_t)ndim * l + d] - x_lower[d]) / dx[d] - 0.5) +
                    ilower[d];
        /* The reference reads/writes u(ic) unchecked; a cell outside the ghost
         * box is undefined there.  Here (and on the GPU) it is an empty
         * stencil: interp gives 0, spread adds nothing. */
        int inside = 1;
        for (int d = 0; d < ndim; ++d) inside &= (ic[d] >= b->lo[d] && ic[d] <= b->hi[d]);
        for (int d = 0; d < depth; ++d) {
            if (!inside) {
                if (!spread) V[(int64_t)depth * s + d] = 0.0;
                continue;
            }
            const int64_t k = ora_idx(b, ic[0], ic[1], ic[2], d);
            if (!spread)
                V[(int64_t)depth * s + d] = u[k];
            else
                u[k] = u[k] + V[(int64_t)depth * s + d] / h3;
        }
    }
}

/* ---------------------------------------------------------------------- */
/* piecewise linear / discontinuous linear                                 */
/* pw-linear 3D: lagrangian_interaction3d.f.m4:446-683                     */
/* disc-linear 3D: lagrangian_interaction3d.f.m4:188-437.  The reference's */
/* 3D spread leaves ic_center(d) unset for d != axis (:388-410); we follow */
/* the interp / 2D semantics (ic_center for every d), SURVEY.md a4.        */
/* ---------------------------------------------------------------------- */
static void ora_linear(int kernel, int spread, const ora_box* b, const double* dx, const double* x_lower, int depth,
                       int axis, const int* ilower, double* u, const int* indices, const double* Xshift, int nindices,
                       const double* X, double* V)
{
    const int ndim = b->ndim;
    const double h3 = ndim == 3 ? (dx[0] * dx[1] * dx[2]) : (dx[0] * dx[1]);
    for (int l = 0; l < nindices; ++l) {
        const int s = indices[l];
        double w[3][2] = {{1.0, 0.0}, {1.0, 0.0}, {1.0, 0.0}};
        int icl[3] = {0, 0, 0}, tl[3] = {0, 0, 0}, tu[3] = {0, 0, 0};
        for (int d = 0; d < ndim; ++d) {
            const double Xs = X[(int64_t)ndim * s + d] + Xshift[(int64_t)ndim * l + d];
            const int icc = ilower[d] + ora_nint((Xs - x_lower[d]) / dx[d] - 0.5);
            const double Xc = x_lower[d] + ((double)(icc - ilower[d]) + 0.5) * dx[d];
            int lo, up;
            if (kernel == LE_PIECEWISE_LINEAR || d == axis) {
                if (Xs < Xc) {
                    lo = icc - 1;
                    up = icc;
                    w[d][0] = (Xc - Xs) / dx[d];
                    w[d][1] = 1.0 - w[d][0];
                } else {
                    lo = icc;
                    up = icc + 1;
                    w[d][0] = 1.0 + (Xc - Xs) / dx[d];
                    w[d][1] = 1.0 - w[d][0];
                }
            } else {
                w[d][0] = 1.0;
                lo = icc;
                up = icc;
            }
            icl[d] = lo;
            tl[d] = imax(lo, b->lo[d]);
            tu[d] = imin(up, b->hi[d]);
        }
        for (int d = 0; d < depth; ++d) {
            if (ndim == 3) {
                if (!spread) {
                    double acc = 0.0;
                    for (int i2 = tl[2]; i2 <= tu[2]; ++i2)
                        for (int i1 = tl[1]; i1 <= tu[1]; ++i1)
                            for (int i0 = tl[0]; i0 <= tu[0]; ++i0)
                                acc = acc + w[0][i0 - icl[0]] * w[1][i1 - icl[1]] * w[2][i2 - icl[2]] *
                                                u[ora_idx(b, i0, i1, i2, d)];
                    V[(int64_t)depth * s + d] = acc;
                } else {
                    const double Vd = V[(int64_t)depth * s + d];
                    for (int i2 = tl[2]; i2 <= tu[2]; ++i2)
                        for (int i1 = tl[1]; i1 <= tu[1]; ++i1)
                            for (int i0 = tl[0]; i0 <= tu[0]; ++i0) {
                                const int64_t k = ora_idx(b, i0, i1, i2, d);
                                u[k] = u[k] + (w[0][i0 - icl[0]] * w[1][i1 - icl[1]] * w[2][i2 - icl[2]] * Vd / h3);
                            }
                }
            } else {
                if (!spread) {
                    double acc = 0.0;
                    for (int i1 = tl[1]; i1 <= tu[1]; ++i1)
                        for (int i0 = tl[0]; i0 <= tu[0]; ++i0)
                            acc = acc + w[0][i0 - icl[0]] * w[1][i1 - icl[1]] * u[ora_idx(b, i0, i1, 0, d)];
                    V[(int64_t)depth * s + d] = acc;
                } else {
                    const double Vd = V[(int64_t)depth * s + d];
                    for (int i1 = tl[1]; i1 <= tu[1]; ++i1)
                        for (int i0 = tl[0]; i0 <= tu[0]; ++i0) {
                            const int64_t k = ora_idx(b, i0, i1, 0, d);
                            u[k] = u[k] + (w[0][i0 - icl[0]] * w[1][i1 - icl[1]] * Vd / h3);
                        }
                }
            }
        }
    }
}

/* ---------------------------------------------------------------------- */
/* piecewise cubic / IB_3 (per-point delta evaluation, clip-then-weigh)    */
/* pw-cubic 3D: lagrangian_interaction3d.f.m4:692-971 -- note the stencil  */
/* side is decided with the UNSHIFTED X(d,s) (:764, :909).                 */
/* IB_3 3D: lagrangian_interaction3d.f.m4:980-1250.                        */
/* ---------------------------------------------------------------------- */
static void ora_cubic_ib3(int kernel, int spread, const ora_box* b, const double* dx, const double* x_lower, int depth,
                          const int* ilower, double* u, const int* indices, const double* Xshift, int nindices,
                          const double* X, double* V)
{
    const int ndim = b->ndim;
    const double h3 = ndim == 3 ? (dx[0] * dx[1] * dx[2]) : (dx[0] * dx[1]);
    for (int l = 0; l < nindices; ++l) {
        const int s = indices[l];
        int lo[3] = {0, 0, 0}, up[3] = {0, 0, 0};
        double w[3][4] = {{1.0, 0, 0, 0}, {1.0, 0, 0, 0}, {1.0, 0, 0, 0}};
        for (int d = 0; d < ndim; ++d) {
            const double Xs = X[(int64_t)ndim * s + d] + Xshift[(int64_t)ndim * l + d];
            const int icc = ora_lagrangian_floor((Xs - x_lower[d]) / dx[d]) + ilower[d];
            const double Xc = x_lower[d] + ((double)(icc - ilower[d]) + 0.5) * dx[d];
            if (kernel == LE_PIECEWISE_CUBIC) {
                if (X[(int64_t)ndim * s + d] < Xc) {
                    lo[d] = icc - 2;
                    up[d] = icc + 1;
                } else {
                    lo[d] = icc - 1;
                    up[d] = icc + 2;
                }
            } else {
                lo[d] = icc - 1;
                up[d] = icc + 1;
            }
            lo[d] = imax(lo[d], b->lo[d]);
            up[d] = imin(up[d], b->hi[d]);
            for (int ic = lo[d]; ic <= up[d]; ++ic) {
                const double Xci = x_lower[d] + ((double)(ic - ilower[d]) + 0.5) * dx[d];
                const double r = (Xs - Xci) / dx[d];
                w[d][ic - lo[d]] = kernel == LE_PIECEWISE_CUBIC ? ora_piecewise_cubic_delta(r) : ora_ib_3_delta(r);
            }
        }
        for (int d = 0; d < depth; ++d) {
            if (ndim == 3) {
                if (!spread) {
                    double acc = 0.0;
                    for (int i2 = lo[2]; i2 <= up[2]; ++i2)
                        for (int i1 = lo[1]; i1 <= up[1]; ++i1)
                            for (int i0 = lo[0]; i0 <= up[0]; ++i0)
                                acc = acc + w[0][i0 - lo[0]] * w[1][i1 - lo[1]] * w[2][i2 - lo[2]] *
                                                u[ora_idx(b, i0, i1, i2, d)];
                    V[(int64_t)depth * s + d] = acc;
                } else {
                    const double Vd = V[(int64_t)depth * s + d];
                    for (int i2 = lo[2]; i2 <= up[2]; ++i2)
                        for (int i1 = lo[1]; i1 <= up[1]; ++i1)
                            for (int i0 = lo[0]; i0 <= up[0]; ++i0) {
                                const int64_t k = ora_idx(b, i0, i1, i2, d);
                                u[k] = u[k] + (w[0][i0 - lo[0]] * w[1][i1 - lo[1]] * w[2][i2 - lo[2]] * Vd / h3);
                            }
                }
            } else {
                if (!spread) {
                    double acc = 0.0;
                    for (int i1 = lo[1]; i1 <= up[1]; ++i1)
                        for (int i0 = lo[0]; i0 <= up[0]; ++i0)
                            acc = acc + w[0][i0 - lo[0]] * w[1][i1 - lo[1]] * u[ora_idx(b, i0, i1, 0, d)];
                    V[(int64_t)depth * s + d] = acc;
                } else {
                    const double Vd = V[(int64_t)depth * s + d];
                    for (int i1 = lo[1]; i1 <= up[1]; ++i1)
                        for (int i0 = lo[0]; i0 <= up[0]; ++i0) {
                            const int64_t k = ora_idx(b, i0, i1, 0, d);
                            u[k] = u[k] + (w[0][i0 - lo[0]] * w[1][i1 - lo[1]] * Vd / h3);
                        }
                }
            }
        }
    }
}

/* ---------------------------------------------------------------------- */
/* dispatch (the string if-chain of LEInteractor.cpp:2431-2708 / 2750-3027) */
/* ---------------------------------------------------------------------- */
static int ora_dispatch(int kernel, int spread, int ndim, const double* dx, const double* x_lower, int depth, int axis,
                        const int* ilower, const int* iupper, const int* nugc, double* u, const int* indices,
                        const double* Xshift, int nindices, const double* X, double* V)
{
    ora_box b;
    if (ndim != 2 && ndim != 3) return -1;
    ora_box_init(&b, ndim, ilower, iupper, nugc);
    if (nindices <= 0) return 0;
    if (ora_is_closed_form(kernel))
        ora_closed_form(kernel, spread, &b, dx, x_lower, depth, ilower, u, indices, Xshift, nindices, X, V);
    else if (kernel == LE_PIECEWISE_CONSTANT)
        ora_piecewise_constant(spread, &b, dx, x_lower, depth, ilower, u, indices, Xshift, nindices, X, V);
    else if (kernel == LE_PIECEWISE_LINEAR || kernel == LE_DISCONTINUOUS_LINEAR)
        ora_linear(kernel, spread, &b, dx, x_lower, depth, axis, ilower, u, indices, Xshift, nindices, X, V);
    else if (kernel == LE_PIECEWISE_CUBIC || kernel == LE_IB_3)
        ora_cubic_ib3(kernel, spread, &b, dx, x_lower, depth, ilower, u, indices, Xshift, nindices, X, V);
    else
        return -2;
    return 0;
}

int ora_interp(int kernel, int ndim, const double* dx, const double* x_lower, int depth, int axis, const int* ilower,
               const int* iupper, const int* nugc, const double* u, const int* indices, const double* Xshift,
               int nindices, const double* X, double* V)
{
    return ora_dispatch(kernel, 0, ndim, dx, x_lower, depth, axis, ilower, iupper, nugc, (double*)u, indices, Xshift,
                        nindices, X, V);
}

int ora_spread(int kernel, int ndim, const double* dx, const double* x_lower, int depth, int axis, const int* ilower,
               const int* iupper, const int* nugc, double* u, const int* indices, const double* Xshift, int nindices,
               const double* X, const double* V)
{
    return ora_dispatch(kernel, 1, ndim, dx, x_lower, depth, axis, ilower, iupper, nugc, u, indices, Xshift, nindices,
                        X, (double*)V);
}

/* ---------------------------------------------------------------------- */
/* USER_DEFINED: LEInteractor::userDefinedInterpolate / userDefinedSpread   */
/* (LEInteractor.cpp:3141-3266, 3268-3393), a host kernel function phi(r)  */
/* ---------------------------------------------------------------------- */
static void ora_user(double (*phi)(double), int S, int spread, const ora_box* b, const double* dx,
                     const double* x_lower, int depth, const int* ilower, const int* iupper, const int* nugc,
                     double* u, const int* indices, const double* Xshift, int n, const double* X, double* V)
{
    const int nd = b->ndim;
    double w[3][64];
    for (int l = 0; l < n; ++l) {
        const int s = indices[l];
        int center[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        double xcell[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < nd; ++d) { /* :3174-3180 */
            center[d] = (int)floor((X[d + s * nd] + Xshift[d + l * nd] - x_lower[d]) / dx[d]) + ilower[d];
            xcell[d] = x_lower[d] + ((double)(center[d] - ilower[d]) + 0.5) * dx[d];
        }
        for (int d = 0; d < nd; ++d) { /* :3184-3207 (the unshifted X against the cell centre) */
            if (S % 2 == 0) {
                if (X[d + s * nd] < xcell[d]) {
                    lo[d] = center[d] - S / 2;
                    hi[d] = center[d] + S / 2 - 1;
                } else {
                    lo[d] = center[d] - S / 2 + 1;
                    hi[d] = center[d] + S / 2;
                }
            } else {
                lo[d] = center[d] - S / 2;
                hi[d] = center[d] + S / 2;
            }
        }
        for (int d = 0; d < nd; ++d) { /* :3209-3213 */
            lo[d] = imin(imax(lo[d], ilower[d] - nugc[d]), iupper[d] + nugc[d]);
            hi[d] = imin(imax(hi[d], ilower[d] - nugc[d]), iupper[d] + nugc[d]);
        }
        for (int d = 0; d < nd; ++d) /* :3216-3238 */
            for (int ic = lo[d]; ic <= hi[d]; ++ic)
                w[d][ic - lo[d]] =
                    phi((X[d + s * nd] + Xshift[d + l * nd] - (xcell[d] + (double)(ic - center[d]) * dx[d])) / dx[d]);
        const int lo2 = nd == 3 ? lo[2] : 0, hi2 = nd == 3 ? hi[2] : 0;
        for (int dd = 0; dd < depth; ++dd) {
            if (!spread) V[dd + s * depth] = 0.0; /* :3243 */
            for (int ic2 = lo2; ic2 <= hi2; ++ic2)
                for (int ic1 = lo[1]; ic1 <= hi[1]; ++ic1)
                    for (int ic0 = lo[0]; ic0 <= hi[0]; ++ic0) {
                        const int64_t k = ora_idx(b, ic0, ic1, ic2, dd);
                        if (nd == 3) {
                            const double ww = w[0][ic0 - lo[0]] * w[1][ic1 - lo[1]] * w[2][ic2 - lo2];
                            if (spread) /* :3381-3382 */
                                u[k] += ww * V[dd + s * depth] / (dx[0] * dx[1] * dx[2]);
                            else /* :3256 */
                                V[dd + s * depth] += ww * u[k];
                        } else {
                            const double ww = w[0][ic0 - lo[0]] * w[1][ic1 - lo[1]];
                            if (spread) /* :3378 */
                                u[k] += ww * V[dd + s * depth] / (dx[0] * dx[1]);
                            else /* :3253 */
                                V[dd + s * depth] += ww * u[k];
                        }
                    }
        }
    }
}

int ora_user_call(double (*phi)(double), int S, int spread, int ndim, const double* dx, const double* x_lower,
                  int depth, const int* ilower, const int* iupper, const int* nugc, double* u, const int* indices,
                  const double* Xshift, int nindices, const double* X, double* V)
{
    ora_box b;
    if (ndim != 2 && ndim != 3) return -1;
    if (S < 1 || S > 64) return -3;
    ora_box_init(&b, ndim, ilower, iupper, nugc);
    if (nindices <= 0) return 0;
    ora_user(phi, S, spread, &b, dx, x_lower, depth, ilower, iupper, nugc, u, indices, Xshift, nindices, X, V);
    return 0;
}
