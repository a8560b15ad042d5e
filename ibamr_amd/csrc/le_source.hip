// le_source.hip -- internal fluid sources and sinks on the device: the two IBStrategy
// operations of IBMethod that are not LEInteractor calls, for one patch of cell-centred
// data of depth 1 in 2-D and 3-D (src/IB/IBMethod.cpp, src/IB/IBStandardSourceGen.cpp):
//
//   k_src_locations  X_src = mean of a source's nodes   IBStandardSourceGen::getSourceLocations :195-250
//   k_src_setup      r, the stencil box, the 1-D weights             IBMethod.cpp :832-845, :854-855
//   k_src_spread     q(i) += Q_n wgt                       IBMethod::spreadFluidSource :828-859
//   k_src_field      integrals, the boundary-cell offset                         :863-941, :960-1003
//   k_src_pressure   P_src[n] = sum p(i) wgt - p_norm    IBMethod::interpolatePressure :1005-1063
//
// The kernel function is IBMethod's own, cos_kernel(x, r) = 0.5 (1 + cos(pi x / r)) / r for
// |x| <= r and 0 beyond (:124-134), with a radius per source and dimension rounded to a whole
// number of cells, at least two (:835).  A 1-D weight depends on the source, the dimension
// and the cell index alone, so the setup kernel evaluates each once into a table of the
// plan's workspace and both the spread and the pressure interpolation read it there: every
// cell sees the value the reference computes at that cell, and the two operators use the
// identical weights.
//
// Spread: owner gathers.  A workgroup takes a tile of one source's clipped box; a cell is
// owned by the lowest-numbered source whose box covers it, and the owner's lane walks all
// sources in ascending n -- their boxes and strengths staged SRC_CHUNK at a time in LDS --
// adding every covering contribution to the value it read, and stores once.  No atomics:
// the order is the reference's (its source loop is the outermost) and the result is the same
// from run to run.  Nothing outside the union of the clipped boxes is written.
//
// The integrals are two-stage reductions in a fixed order (SRC_NPART workgroups, each over
// its own rows of the patch box and a fixed tree, then one workgroup over the partial sums).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ibtk_le.h"
#include "le_source.h"

namespace ibtk_le {

namespace {

constexpr int SRC_BLOCK = 256;   // lanes of the reductions, the pressure kernel and the pointwise kernels
constexpr int SRC_SETUP = 128;   // lanes of the setup kernel: (dimension, table entry)
constexpr int SRC_TPAD = 40;     // table entries per dimension in the setup kernel's lane numbering
static_assert(3 * SRC_TPAD <= SRC_SETUP && SRC_TAB <= SRC_TPAD, "one lane per table entry");
static_assert(SRC_NPART % SRC_BLOCK == 0, "the final stage gives every lane the same share");

struct SrcDom {
    int lo[3], hi[3];
};

template <class T> __device__ __forceinline__ T pick(const T (&a)[3], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : a[2]); }

// IBMethod.cpp:124-134
__device__ __forceinline__ double cos_kernel(double x, double eps) {
    if (fabs(x) > eps) return 0.0;
    return 0.5 * (1.0 + cos(3.14159265358979323846 * x / eps)) / eps;
}

// The radius (IBMethod.cpp:835), the centre cell (IndexUtilities::getCellIndex,
// IndexUtilities-inl.h:66-89) and the half width (:844) of a source in dimension d.
// Returns false when the source has no stencil here: a position that is not finite or
// further than 10^9 cells away, or a radius beyond the tables.
__device__ __forceinline__ bool src_stencil(const SrcGrid& g, double r_src, double X, int d, double& r, int& centre,
                                            int& half) {
    const double dx = pick(g.dx, d);
    const double R = fmax(floor(r_src / dx + 0.5), 2.0);
    r = R * dx;
    centre = 0;
    half = 0;
    if (!(R <= (double)SRC_RMAX)) return false;
    half = (int)(r / dx) + 1;
    const double dl = X - pick(g.xlo, d), du = X - pick(g.xup, d);
    double c;
    if (fabs(dl) <= fabs(du)) c = (double)pick(g.ilower, d) + floor(dl / dx);
    else c = (double)pick(g.iupper, d) + floor(du / dx) + 1.0;
    if (!(c >= -1.0e9 && c <= 1.0e9)) return false;  // (a NaN fails both)
    centre = (int)c;
    return true;
}

__device__ __forceinline__ int64_t cell_offset(const SrcGrid& g, int i0, int i1, int i2) {
    int64_t off = (i0 - g.glo[0]) + (int64_t)(i1 - g.glo[1]) * g.s1;
    if (g.ndim == 3) off += (int64_t)(i2 - g.glo[2]) * g.s2;
    return off;
}

// the sum (MAX: the maximum) of the lanes' values in a fixed tree; the result in every lane
template <bool MAX> __device__ __forceinline__ double block_reduce(double v, double* s) {
    const int t = (int)threadIdx.x;
    __syncthreads();
    s[t] = v;
    for (int off = SRC_BLOCK / 2; off > 0; off >>= 1) {
        __syncthreads();
        if (t < off) s[t] = MAX ? fmax(s[t], s[t + off]) : s[t] + s[t + off];
    }
    __syncthreads();
    return s[0];
}

}  // namespace

// ---------------------------------------------------------------------------------------
// locations
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SRC_BLOCK) void k_src_locations(int ndim, int n_src, const int* off, const int* nodes,
                                                              const double* X, double* X_src) {
    const int e = (int)blockIdx.x * SRC_BLOCK + (int)threadIdx.x;
    if (e >= n_src * ndim) return;
    const int k = e / ndim, d = e - k * ndim;
    const int a = off[k], b = off[k + 1];
    const double count = (double)(b - a);
    double v = 0.0;  // Point::Zero()
    for (int i = a; i < b; ++i) v += X[(int64_t)ndim * nodes[i] + d] / count;
    X_src[e] = v;
}

hipError_t launch_src_locations(int ndim, int n_src, const int* off, const int* nodes, const double* X, double* X_src,
                                hipStream_t s) {
    if (n_src <= 0) return hipSuccess;
    const unsigned nb = (unsigned)(((long long)n_src * ndim + SRC_BLOCK - 1) / SRC_BLOCK);
    hipLaunchKernelGGL(k_src_locations, dim3(nb), dim3(SRC_BLOCK), 0, s, ndim, n_src, off, nodes, X, X_src);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// setup: one workgroup per source, one lane per (dimension, table entry)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SRC_SETUP) void k_src_setup(SrcParams P, const double* X_src) {
    const int n = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const int d = t / SRC_TPAD, j = t - d * SRC_TPAD;
    if (d >= 3) return;
    SrcBox* const box = P.box + n;
    if (d >= P.g.ndim) {  // the dimension a 2-D patch lacks: one cell, index 0
        if (j == 0) {
            box->lo[d] = 0;
            box->hi[d] = 0;
            box->base[d] = 0;
            if (d == 2) box->pad = 0;
        }
        return;
    }
    const double X = X_src[(int64_t)P.g.ndim * n + d];
    double r;
    int centre, half;
    const bool ok = src_stencil(P.g, P.r_src[n], X, d, r, centre, half);
    const int base = centre - half;
    if (j == 0) {
        // cut to the patch box, never to the ghost box (:848)
        box->base[d] = base;
        box->lo[d] = ok ? max(base, pick(P.g.ilower, d)) : 0;
        box->hi[d] = ok ? min(centre + half, pick(P.g.iupper, d)) : -1;
        if (d == 2) box->pad = 0;
    }
    if (ok && j <= 2 * half && j < SRC_TAB) {
        const int i = base + j;
        // :854-855
        const double X_center = pick(P.g.xlo, d) + pick(P.g.dx, d) * ((double)(i - pick(P.g.ilower, d)) + 0.5);
        P.w[((int64_t)n * 3 + d) * SRC_TAB + j] = cos_kernel(X_center - X, r);
    }
}

hipError_t launch_src_setup(const SrcParams& P, const double* X_src, hipStream_t s) {
    if (P.n_src <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_src_setup, dim3((unsigned)P.n_src), dim3(SRC_SETUP), 0, s, P, X_src);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// spread
// ---------------------------------------------------------------------------------------
struct SrcTiles {
    int nt[3];
    int per_source;
};

template <int ND>
__global__ __launch_bounds__(ND == 3 ? 512 : 64) void k_src_spread(SrcParams P, SrcTiles T, double* q, const double* Q) {
    constexpr int B = ND == 3 ? SRC_TILE3 : SRC_TILE2;
    static_assert((ND == 3 ? B * B * B : B * B) >= SRC_CHUNK, "a lane stages a source");
    __shared__ int s_lo[SRC_CHUNK][3], s_hi[SRC_CHUNK][3], s_base[SRC_CHUNK][3];
    __shared__ double s_Q[SRC_CHUNK];
    __shared__ int s_hit[SRC_CHUNK];

    const int t = (int)threadIdx.x;
    const int n = (int)blockIdx.x / T.per_source;
    int t0[ND], t1[ND];
    {
        const SrcBox own = P.box[n];
        int tt = (int)blockIdx.x - n * T.per_source;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int ntd = pick(T.nt, d);
            t0[d] = own.lo[d] + (tt % ntd) * B;
            tt /= ntd;
            t1[d] = min(t0[d] + B - 1, own.hi[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (t0[d] > t1[d]) return;  // the whole workgroup: a tile past this source's clipped box

    // this lane's cell
    int i[3] = {0, 0, 0};
    if constexpr (ND == 3) {
        i[0] = t0[0] + (t & 7);
        i[1] = t0[1] + ((t >> 3) & 7);
        i[2] = t0[2] + (t >> 6);
    } else {
        i[0] = t0[0] + (t & 7);
        i[1] = t0[1] + (t >> 3);
    }
    bool mine = true;
#pragma unroll
    for (int d = 0; d < ND; ++d) mine = mine && i[d] <= t1[d];
    double* const ptr = q + (mine ? cell_offset(P.g, i[0], i[1], i[2]) : 0);
    double acc = mine ? *ptr : 0.0;
    bool owner = mine;  // until a lower-numbered source covers the cell

    for (int base = 0; base < P.n_src; base += SRC_CHUNK) {
        const int m_end = min(SRC_CHUNK, P.n_src - base);
        if (t < SRC_CHUNK) {
            int hit = 0;
            if (t < m_end) {
                const SrcBox b = P.box[base + t];
                hit = 1;
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    s_lo[t][d] = b.lo[d];
                    s_hi[t][d] = b.hi[d];
                    s_base[t][d] = b.base[d];
                    if (b.lo[d] > b.hi[d] || b.hi[d] < t0[d] || b.lo[d] > t1[d]) hit = 0;  // misses the tile
                }
                s_Q[t] = Q[base + t];
            }
            s_hit[t] = hit;
        }
        __syncthreads();
        for (int j = 0; j < m_end; ++j) {
            if (!s_hit[j]) continue;  // the same for every lane
            bool in = owner;
#pragma unroll
            for (int d = 0; d < ND; ++d) in = in && i[d] >= s_lo[j][d] && i[d] <= s_hi[j][d];
            if (!in) continue;
            const int m = base + j;
            if (m < n) {
                owner = false;  // source m's workgroups own this cell
                continue;
            }
            const double* const w = P.w + (int64_t)m * 3 * SRC_TAB;
            const double w0 = w[i[0] - s_base[j][0]];
            const double w1 = w[SRC_TAB + (i[1] - s_base[j][1])];
            double wgt = w0 * w1;
            if constexpr (ND == 3) wgt = wgt * w[2 * SRC_TAB + (i[2] - s_base[j][2])];
            acc += s_Q[j] * wgt;  // :857
        }
        // (also the barrier before the next chunk overwrites the staged boxes)
        if (!__syncthreads_or(owner ? 1 : 0)) return;
    }
    if (owner) *ptr = acc;
}

hipError_t launch_src_spread(const SrcParams& P, const int nt[3], double* q, const double* Q, hipStream_t s) {
    if (P.n_src <= 0) return hipSuccess;
    SrcTiles T;
    long long per = 1;
    for (int d = 0; d < 3; ++d) {
        T.nt[d] = d < P.g.ndim ? nt[d] : 1;
        per *= T.nt[d];
    }
    if (per <= 0) return hipSuccess;  // no source has a stencil
    const long long grid = per * P.n_src;
    if (grid > INT_MAX) return hipErrorInvalidValue;
    T.per_source = (int)per;
    if (P.g.ndim == 3) hipLaunchKernelGGL(k_src_spread<3>, dim3((unsigned)grid), dim3(512), 0, s, P, T, q, Q);
    else hipLaunchKernelGGL(k_src_spread<2>, dim3((unsigned)grid), dim3(64), 0, s, P, T, q, Q);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// integrals over the patch box, the boundary-cell offset
// ---------------------------------------------------------------------------------------
namespace {

// domain \ interior, the interior being the domain box shrunk by one cell in every dimension
// but the last (IBMethod.cpp:899-907)
__device__ __forceinline__ bool bdry_cell(int ndim, const SrcDom& D, int i0, int i1, int i2) {
    bool in = i0 >= D.lo[0] && i0 <= D.hi[0] && i1 >= D.lo[1] && i1 <= D.hi[1];
    if (ndim == 3) in = in && i2 >= D.lo[2] && i2 <= D.hi[2];
    bool edge = i0 == D.lo[0] || i0 == D.hi[0];
    if (ndim == 3) edge = edge || i1 == D.lo[1] || i1 == D.hi[1];
    return in && edge;
}

enum { F_INTEGRAL = 0, F_OFFSET = 1, F_BDRY = 2 };

}  // namespace

// Workgroup b takes the rows b, b + SRC_NPART, ... of the patch box, a lane every
// SRC_BLOCK-th cell of a row.  F_INTEGRAL: part[b] = sum q dV.  F_OFFSET: the boundary cells
// get += totals[2] first (:919-931), then part[b] = sum q dV and part[SRC_NPART + b] = max |q|.
// F_BDRY: part[b] = sum p dV over the boundary cells (:983-997).
template <int MODE>
__global__ __launch_bounds__(SRC_BLOCK) void k_src_field(SrcParams P, double* q, SrcDom D, double dV, const double* totals) {
    __shared__ double s_red[SRC_BLOCK];
    const int t = (int)threadIdx.x;
    const SrcGrid& g = P.g;
    const int n0 = g.iupper[0] - g.ilower[0] + 1, n1 = g.iupper[1] - g.ilower[1] + 1;
    const int n2 = g.ndim == 3 ? g.iupper[2] - g.ilower[2] + 1 : 1;
    const long long rows = (long long)n1 * n2;
    const double q_norm = MODE == F_OFFSET ? totals[2] : 0.0;
    double sum = 0.0, mx = 0.0;
    for (long long r = blockIdx.x; r < rows; r += SRC_NPART) {
        const int i2 = (int)(r / n1) + (g.ndim == 3 ? g.ilower[2] : 0);
        const int i1 = (int)(r % n1) + g.ilower[1];
        double* const row = q + cell_offset(g, g.ilower[0], i1, i2);
        for (int x = t; x < n0; x += SRC_BLOCK) {
            const bool bd = MODE != F_INTEGRAL && bdry_cell(g.ndim, D, g.ilower[0] + x, i1, i2);
            if (MODE == F_BDRY && !bd) continue;
            double v = row[x];
            if (MODE == F_OFFSET) {
                if (bd) {
                    v += q_norm;
                    row[x] = v;
                }
                mx = fmax(mx, fabs(v));
            }
            sum += v * dV;
        }
    }
    sum = block_reduce<false>(sum, s_red);
    if (MODE == F_OFFSET) mx = block_reduce<true>(mx, s_red);
    if (t == 0) {
        P.part[blockIdx.x] = sum;
        if (MODE == F_OFFSET) P.part[SRC_NPART + blockIdx.x] = mx;
    }
}

// One workgroup over the partial sums.  STAGE 0: q_total, Q_sum, Q_max, the test at :877,
// q_norm.  STAGE 1: integral_after and the test at :934.  STAGE 2: the normalisation
// pressure (:1002).
template <int STAGE>
__global__ __launch_bounds__(SRC_BLOCK) void k_src_finish(SrcParams P, const double* Q, double vol, int normalize,
                                                           double* totals) {
    __shared__ double s_red[SRC_BLOCK];
    const int t = (int)threadIdx.x;
    constexpr int SHARE = SRC_NPART / SRC_BLOCK;
    double sum = 0.0, mx = 0.0;
    for (int k = 0; k < SHARE; ++k) {
        sum += P.part[t * SHARE + k];
        if (STAGE == 1) mx = fmax(mx, P.part[SRC_NPART + t * SHARE + k]);
    }
    sum = block_reduce<false>(sum, s_red);
    if (STAGE == 1) mx = block_reduce<true>(mx, s_red);
    if (t != 0) return;
    if (STAGE == 0) {
        const double q_total = sum;
        double Q_sum = 0.0, Q_max = 0.0;
        for (int n = 0; n < P.n_src; ++n) {  // std::accumulate, :870-874
            Q_sum += Q[n];
            Q_max = fmax(Q_max, fabs(Q[n]));
        }
        if (fabs(q_total - Q_sum) > 1.0e-12 && fabs(q_total - Q_sum) / fmax(Q_max, 1.0) > 1.0e-12) atomicOr(P.flags, SRC_FLAG);
        totals[0] = q_total;
        totals[1] = Q_sum;
        totals[2] = normalize ? -q_total / vol : 0.0;  // :913
        if (!normalize) totals[3] = q_total;           // no second integral: the field is as it was
    } else if (STAGE == 1) {
        totals[3] = sum;
        if (fabs(sum) > 1.0e-10 * fmax(1.0, mx)) atomicOr(P.flags, SRC_FLAG);
    } else {
        P.scal[0] = sum / vol;
    }
}

hipError_t launch_src_normalize(const SrcParams& P, double* q, const double* Q, const int dom_lo[3], const int dom_hi[3],
                                double vol, int normalize, double* totals, hipStream_t s) {
    SrcDom D{};
    for (int d = 0; d < 3; ++d) {
        D.lo[d] = normalize ? dom_lo[d] : 0;
        D.hi[d] = normalize ? dom_hi[d] : -1;
    }
    const double dV = P.g.ndim == 3 ? (P.g.dx[0] * P.g.dx[1]) * P.g.dx[2] : P.g.dx[0] * P.g.dx[1];
    hipLaunchKernelGGL(k_src_field<F_INTEGRAL>, dim3(SRC_NPART), dim3(SRC_BLOCK), 0, s, P, q, D, dV, totals);
    hipLaunchKernelGGL(k_src_finish<0>, dim3(1), dim3(SRC_BLOCK), 0, s, P, Q, vol, normalize, totals);
    if (normalize) {
        hipLaunchKernelGGL(k_src_field<F_OFFSET>, dim3(SRC_NPART), dim3(SRC_BLOCK), 0, s, P, q, D, dV, totals);
        hipLaunchKernelGGL(k_src_finish<1>, dim3(1), dim3(SRC_BLOCK), 0, s, P, Q, vol, normalize, totals);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// pressure: one workgroup per source
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SRC_BLOCK) void k_src_pressure(SrcParams P, const double* p, double* P_src, int use_norm) {
    __shared__ double s_w[3][SRC_TAB];  // cos_kernel dx, :1055
    __shared__ double s_red[SRC_BLOCK];
    const int n = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const SrcGrid& g = P.g;
    const SrcBox b = P.box[n];
    int ext[3] = {1, 1, 1};
    long long cells = 1;
    for (int d = 0; d < g.ndim; ++d) {
        ext[d] = max(b.hi[d] - b.lo[d] + 1, 0);
        cells *= ext[d];
    }
    double sum = 0.0;
    if (cells > 0) {  // the same for every lane
        if (t < 3 * SRC_TPAD) {
            const int d = t / SRC_TPAD, j = t - d * SRC_TPAD;
            // the entries of the clipped box only: the others may never have been written
            if (d < g.ndim && j >= b.lo[d] - b.base[d] && j <= b.hi[d] - b.base[d])
                s_w[d][j] = P.w[((int64_t)n * 3 + d) * SRC_TAB + j] * pick(g.dx, d);
        }
        __syncthreads();
        // lane t takes the cells t, t + SRC_BLOCK, ... of the box, x fastest
        for (long long c = t; c < cells; c += SRC_BLOCK) {
            const int x = (int)(c % ext[0]);
            const long long yz = c / ext[0];
            const int y = (int)(yz % ext[1]), z = (int)(yz / ext[1]);
            const int i0 = b.lo[0] + x, i1 = b.lo[1] + y, i2 = g.ndim == 3 ? b.lo[2] + z : 0;
            double wgt = s_w[0][i0 - b.base[0]] * s_w[1][i1 - b.base[1]];
            if (g.ndim == 3) wgt = wgt * s_w[2][i2 - b.base[2]];
            sum += p[cell_offset(g, i0, i1, i2)] * wgt;  // :1057
        }
    }
    sum = block_reduce<false>(sum, s_red);
    if (t == 0) P_src[n] = use_norm ? sum - P.scal[0] : sum;  // :1062-1063
}

hipError_t launch_src_pressure(const SrcParams& P, const double* p, double* P_src, int use_norm, const int dom_lo[3],
                               const int dom_hi[3], double vol, hipStream_t s) {
    if (P.n_src <= 0) return hipSuccess;
    if (use_norm) {
        SrcDom D{};
        for (int d = 0; d < 3; ++d) {
            D.lo[d] = dom_lo[d];
            D.hi[d] = dom_hi[d];
        }
        const double dV = P.g.ndim == 3 ? (P.g.dx[0] * P.g.dx[1]) * P.g.dx[2] : P.g.dx[0] * P.g.dx[1];
        hipLaunchKernelGGL(k_src_field<F_BDRY>, dim3(SRC_NPART), dim3(SRC_BLOCK), 0, s, P, const_cast<double*>(p), D, dV,
                           (const double*)nullptr);
        hipLaunchKernelGGL(k_src_finish<2>, dim3(1), dim3(SRC_BLOCK), 0, s, P, (const double*)nullptr, vol, 0,
                           (double*)nullptr);
    }
    hipLaunchKernelGGL(k_src_pressure, dim3((unsigned)P.n_src), dim3(SRC_BLOCK), 0, s, P, p, P_src, use_norm);
    return hipGetLastError();
}

}  // namespace ibtk_le

// ---------------------------------------------------------------------------
// The C ABI.  create validates the host arrays, groups the nodes by source (each group in
// ascending local index) and allocates everything the device calls use; the device calls
// are launches on the context stream: no allocation, no host synchronisation.
// ---------------------------------------------------------------------------
using namespace ibtk_le;

#define SRC_HIP_TRY(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return abi_fail(IBTK_LE_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct ibtk_le_sources_s {
    ibtk_le_ctx ctx = nullptr;
    int ndim = 0, n_nodes = 0, n_src = 0, n_pts = 0;
    std::vector<double> r_host;  // the radii: the host checks R against the tables from them
    double* r_src = nullptr;     // device copies
    int* off = nullptr;          // n_src + 1
    int* nodes = nullptr;        // n_pts
    SrcBox* box = nullptr;       // workspace (SrcParams)
    double* w = nullptr;
    double* part = nullptr;
    double* scal = nullptr;
};

namespace {

void src_where(ibtk_le_ctx ctx, int& device, hipStream_t& stream) { abi_ctx_device_stream(ctx, &device, &stream); }

void src_free(ibtk_le_sources s) {
    for (void* p : {(void*)s->r_src, (void*)s->off, (void*)s->nodes, (void*)s->box, (void*)s->w, (void*)s->part,
                    (void*)s->scal})
        if (p) (void)hipFree(p);
}

// the checks every device call shares
int src_common(const char* what, ibtk_le_ctx ctx, ibtk_le_sources s) {
    if (!ctx) return abi_fail(IBTK_LE_ERR_ARG, "%s: null context", what);
    if (!s) return abi_fail(IBTK_LE_ERR_ARG, "%s: null source plan", what);
    if (ctx != s->ctx) return abi_fail(IBTK_LE_ERR_ARG, "%s: the plan was created on another context", what);
    return IBTK_LE_OK;
}

// empty: the patch box holds no cell, nothing to do (IBTK_LE_OK)
int src_geom(const char* what, ibtk_le_sources s, const ibtk_le_patch_geom* geom, bool& empty) {
    empty = false;
    if (!geom) return abi_fail(IBTK_LE_ERR_ARG, "%s: null geometry", what);
    if (geom->ndim != 2 && geom->ndim != 3) return abi_fail(IBTK_LE_ERR_ARG, "%s: ndim must be 2 or 3 (got %d)", what, geom->ndim);
    if (geom->ndim != s->ndim)
        return abi_fail(IBTK_LE_ERR_ARG, "%s: a %d-D geometry for a %d-D source plan", what, geom->ndim, s->ndim);
    for (int d = 0; d < geom->ndim; ++d) {
        if (!std::isfinite(geom->dx[d]) || !(geom->dx[d] > 0.0))
            return abi_fail(IBTK_LE_ERR_ARG, "%s: dx[%d] must be finite and positive", what, d);
        if (!std::isfinite(geom->x_lower[d]) || !std::isfinite(geom->x_upper[d]))
            return abi_fail(IBTK_LE_ERR_ARG, "%s: x_lower / x_upper[%d] is not finite", what, d);
        if (geom->gcw[d] < 0) return abi_fail(IBTK_LE_ERR_ARG, "%s: negative ghost width", what);
        if (geom->iupper[d] < geom->ilower[d]) empty = true;
    }
    if (geom->pitch[0] || geom->pitch[1]) {
        if (geom->ndim != 3) return abi_fail(IBTK_LE_ERR_ARG, "%s: an array pitch needs a 3-D patch", what);
        if (!empty) {
            // the pitch covers the widest array of the patch (the ghosted box + 1 face), as everywhere
            const long long n0 = (long long)geom->iupper[0] - geom->ilower[0] + 2 + 2LL * geom->gcw[0];
            const long long n1 = (long long)geom->iupper[1] - geom->ilower[1] + 2 + 2LL * geom->gcw[1];
            if (geom->pitch[0] < n0 || (geom->pitch[1] != 0 && geom->pitch[1] < n1))
                return abi_fail(IBTK_LE_ERR_ARG, "%s: array pitch {%d, %d} below the ghosted extent {%lld, %lld} (+1 face)",
                                what, geom->pitch[0], geom->pitch[1], n0, n1);
        }
    }
    return IBTK_LE_OK;
}

int src_domain(const char* what, int ndim, const int* dom_lo, const int* dom_hi) {
    if (!dom_lo != !dom_hi) return abi_fail(IBTK_LE_ERR_ARG, "%s: dom_lo and dom_hi go together", what);
    if (dom_lo)
        for (int d = 0; d < ndim; ++d)
            if (dom_hi[d] < dom_lo[d]) return abi_fail(IBTK_LE_ERR_ARG, "%s: empty domain box in dim %d", what, d);
    return IBTK_LE_OK;
}

// every radius within the tables at this spacing; nt: the tiles a clipped box can take
int src_radii(const char* what, ibtk_le_sources s, const ibtk_le_patch_geom* geom, int nt[3]) {
    const int B = s->ndim == 3 ? SRC_TILE3 : SRC_TILE2;
    for (int d = 0; d < 3; ++d) nt[d] = d < s->ndim ? 0 : 1;
    for (int n = 0; n < s->n_src; ++n)
        for (int d = 0; d < s->ndim; ++d) {
            const double dx = geom->dx[d];
            const double R = std::max(std::floor(s->r_host[n] / dx + 0.5), 2.0);
            if (!(R <= (double)SRC_RMAX))
                return abi_fail(IBTK_LE_ERR_ARG, "%s: source %d has a radius of %g cells in dim %d; the tables hold %d", what, n,
                                R, d, SRC_RMAX);
            const int half = (int)((R * dx) / dx) + 1;
            const long long cells = std::min<long long>(2LL * half + 1, (long long)geom->iupper[d] - geom->ilower[d] + 1);
            nt[d] = std::max(nt[d], (int)((cells + B - 1) / B));
        }
    return IBTK_LE_OK;
}

void src_params(ibtk_le_sources s, const ibtk_le_patch_geom* geom, SrcParams& P) {
    P = SrcParams{};
    SrcGrid& g = P.g;
    g.ndim = geom->ndim;
    int64_t n[3] = {1, 1, 1};
    for (int d = 0; d < 3; ++d) {
        const bool in = d < geom->ndim;
        g.ilower[d] = in ? geom->ilower[d] : 0;
        g.iupper[d] = in ? geom->iupper[d] : 0;
        g.glo[d] = in ? geom->ilower[d] - geom->gcw[d] : 0;
        g.dx[d] = in ? geom->dx[d] : 1.0;
        g.xlo[d] = in ? geom->x_lower[d] : 0.0;
        g.xup[d] = in ? geom->x_upper[d] : 1.0;
        if (in) n[d] = (int64_t)geom->iupper[d] - geom->ilower[d] + 1 + 2 * (int64_t)geom->gcw[d];
    }
    if (geom->pitch[0] == 0 && geom->pitch[1] == 0) {
        g.s1 = n[0];
        g.s2 = n[0] * n[1];
    } else {
        g.s1 = geom->pitch[0];
        g.s2 = g.s1 * (geom->pitch[1] ? geom->pitch[1] : n[1]);
    }
    P.n_src = s->n_src;
    P.r_src = s->r_src;
    P.box = s->box;
    P.w = s->w;
    P.part = s->part;
    P.scal = s->scal;
    P.flags = abi_ctx_flags(s->ctx);
}

// cells of domain \ interior (IBMethod.cpp:899-908) inside [lo, hi]
long long src_bdry_cells(int ndim, const int* dom_lo, const int* dom_hi, const int* lo, const int* hi) {
    long long all = 1, inner = 1;
    for (int d = 0; d < ndim; ++d) {
        const int shrink = d < ndim - 1 ? 1 : 0;
        const long long a = (long long)std::min(hi[d], dom_hi[d]) - std::max(lo[d], dom_lo[d]) + 1;
        const long long b = (long long)std::min(hi[d], dom_hi[d] - shrink) - std::max(lo[d], dom_lo[d] + shrink) + 1;
        all *= std::max(a, 0LL);
        inner *= std::max(b, 0LL);
    }
    return all - inner;
}

}  // namespace

extern "C" int ibtk_le_sources_create(ibtk_le_ctx ctx, int ndim, int n_nodes, int n_src, const double* r_src, int n_pts,
                                      const int* node, const int* source, ibtk_le_sources* out) {
    if (!ctx) return abi_fail(IBTK_LE_ERR_ARG, "sources_create: null context");
    if (!out) return abi_fail(IBTK_LE_ERR_ARG, "sources_create: null out");
    if (ndim != 2 && ndim != 3) return abi_fail(IBTK_LE_ERR_ARG, "sources_create: ndim must be 2 or 3 (got %d)", ndim);
    if (n_nodes < 0 || n_src < 0 || n_pts < 0)
        return abi_fail(IBTK_LE_ERR_ARG, "sources_create: negative count (%d nodes, %d sources, %d source points)", n_nodes,
                        n_src, n_pts);
    if ((n_src > 0 && !r_src) || (n_pts > 0 && (!node || !source))) return abi_fail(IBTK_LE_ERR_ARG, "sources_create: null array");
    if ((long long)n_src * 3 * SRC_TAB > INT_MAX) return abi_fail(IBTK_LE_ERR_RANGE, "sources_create: %d sources", n_src);
    for (int n = 0; n < n_src; ++n)
        if (!std::isfinite(r_src[n]) || !(r_src[n] > 0.0))
            return abi_fail(IBTK_LE_ERR_ARG, "sources_create: the radius of source %d must be finite and positive", n);
    std::vector<int> off((size_t)n_src + 1, 0);
    std::vector<char> seen((size_t)n_nodes, 0);
    for (int k = 0; k < n_pts; ++k) {
        if (node[k] < 0 || node[k] >= n_nodes)
            return abi_fail(IBTK_LE_ERR_ARG, "source point %d: node index %d is out of range [0, %d)", k, node[k], n_nodes);
        if (source[k] < 0 || source[k] >= n_src)
            return abi_fail(IBTK_LE_ERR_ARG, "source point %d: source index %d is out of range [0, %d)", k, source[k], n_src);
        if (seen[node[k]]) return abi_fail(IBTK_LE_ERR_ARG, "source point %d: node %d is named twice", k, node[k]);
        seen[node[k]] = 1;
        ++off[(size_t)source[k] + 1];
    }
    for (int n = 0; n < n_src; ++n) off[n + 1] += off[n];
    std::vector<int> nodes((size_t)n_pts), at(off.begin(), off.end() - 1);
    for (int k = 0; k < n_pts; ++k) nodes[(size_t)at[source[k]]++] = node[k];
    for (int n = 0; n < n_src; ++n) std::sort(nodes.begin() + off[n], nodes.begin() + off[n + 1]);  // ascending local index

    auto* s = new ibtk_le_sources_s();
    s->ctx = ctx;
    s->ndim = ndim;
    s->n_nodes = n_nodes;
    s->n_src = n_src;
    s->n_pts = n_pts;
    s->r_host.assign(r_src, r_src + n_src);
    int device;
    hipStream_t stream;
    src_where(ctx, device, stream);
    const size_t ns = (size_t)std::max(n_src, 1), np = (size_t)std::max(n_pts, 1);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)&s->r_src, ns * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&s->off, (ns + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&s->nodes, np * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&s->box, ns * sizeof(SrcBox));
    if (e == hipSuccess) e = hipMalloc((void**)&s->w, ns * 3 * SRC_TAB * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&s->part, 2 * SRC_NPART * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&s->scal, 4 * sizeof(double));
    if (e == hipSuccess && n_src > 0) e = hipMemcpy(s->r_src, r_src, (size_t)n_src * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_pts > 0) e = hipMemcpy(s->nodes, nodes.data(), (size_t)n_pts * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->scal, 0, 4 * sizeof(double));
    if (e != hipSuccess) {
        src_free(s);
        delete s;
        return abi_fail(e == hipErrorOutOfMemory ? IBTK_LE_ERR_NOMEM : IBTK_LE_ERR_DEVICE, "sources_create: %s",
                        hipGetErrorString(e));
    }
    *out = s;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_sources_destroy(ibtk_le_sources s) {
    if (!s) return IBTK_LE_OK;
    int device;
    hipStream_t stream;
    src_where(s->ctx, device, stream);
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);  // a call in flight may still read the plan
    src_free(s);
    delete s;
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_source_locations(ibtk_le_ctx ctx, ibtk_le_sources s, const double* X_dev, double* X_src_dev) {
    if (int rc = src_common("source_locations", ctx, s)) return rc;
    if (s->n_src == 0) return IBTK_LE_OK;
    if (!X_src_dev || (s->n_pts > 0 && !X_dev)) return abi_fail(IBTK_LE_ERR_ARG, "source_locations: null array");
    int device;
    hipStream_t stream;
    src_where(ctx, device, stream);
    SRC_HIP_TRY(hipSetDevice(device));
    SRC_HIP_TRY(launch_src_locations(s->ndim, s->n_src, s->off, s->nodes, X_dev, X_src_dev, stream));
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_source_spread(ibtk_le_ctx ctx, ibtk_le_sources s, const ibtk_le_patch_geom* geom, double* q_dev,
                                     const double* X_src_dev, const double* Q_src_dev) {
    bool empty;
    if (int rc = src_common("source_spread", ctx, s)) return rc;
    if (int rc = src_geom("source_spread", s, geom, empty)) return rc;
    if (s->n_src == 0 || empty) return IBTK_LE_OK;
    if (!q_dev || !X_src_dev || !Q_src_dev) return abi_fail(IBTK_LE_ERR_ARG, "source_spread: null array");
    int nt[3];
    if (int rc = src_radii("source_spread", s, geom, nt)) return rc;
    SrcParams P;
    src_params(s, geom, P);
    int device;
    hipStream_t stream;
    src_where(ctx, device, stream);
    SRC_HIP_TRY(hipSetDevice(device));
    SRC_HIP_TRY(launch_src_setup(P, X_src_dev, stream));
    SRC_HIP_TRY(launch_src_spread(P, nt, q_dev, Q_src_dev, stream));
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_source_normalize(ibtk_le_ctx ctx, ibtk_le_sources s, const ibtk_le_patch_geom* geom, double* q_dev,
                                        const int* dom_lo, const int* dom_hi, const double* Q_src_dev, int normalize,
                                        double* totals_dev) {
    bool empty;
    if (int rc = src_common("source_normalize", ctx, s)) return rc;
    if (int rc = src_geom("source_normalize", s, geom, empty)) return rc;
    if (int rc = src_domain("source_normalize", geom->ndim, dom_lo, dom_hi)) return rc;
    if (normalize && !dom_lo) return abi_fail(IBTK_LE_ERR_ARG, "source_normalize: the normalisation needs the domain box");
    if (s->n_src == 0 || empty) return IBTK_LE_OK;
    if (!q_dev || !Q_src_dev || !totals_dev) return abi_fail(IBTK_LE_ERR_ARG, "source_normalize: null array");
    SrcParams P;
    src_params(s, geom, P);
    double vol = 1.0;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (normalize) {
        // :908-912: the cells of domain \ interior, times dx0, dx1, dx2 in turn
        vol = (double)src_bdry_cells(geom->ndim, dom_lo, dom_hi, dom_lo, dom_hi);
        for (int d = 0; d < geom->ndim; ++d) {
            vol *= geom->dx[d];
            lo[d] = dom_lo[d];
            hi[d] = dom_hi[d];
        }
    }
    int device;
    hipStream_t stream;
    src_where(ctx, device, stream);
    SRC_HIP_TRY(hipSetDevice(device));
    SRC_HIP_TRY(launch_src_normalize(P, q_dev, Q_src_dev, lo, hi, vol, normalize ? 1 : 0, totals_dev, stream));
    return IBTK_LE_OK;
}

extern "C" int ibtk_le_source_pressure(ibtk_le_ctx ctx, ibtk_le_sources s, const ibtk_le_patch_geom* geom,
                                       const double* p_dev, const double* X_src_dev, double* P_src_dev, const int* dom_lo,
                                       const int* dom_hi) {
    bool empty;
    if (int rc = src_common("source_pressure", ctx, s)) return rc;
    if (int rc = src_geom("source_pressure", s, geom, empty)) return rc;
    if (int rc = src_domain("source_pressure", geom->ndim, dom_lo, dom_hi)) return rc;
    if (s->n_src == 0 || empty) return IBTK_LE_OK;
    if (!p_dev || !X_src_dev || !P_src_dev) return abi_fail(IBTK_LE_ERR_ARG, "source_pressure: null array");
    int nt[3];
    if (int rc = src_radii("source_pressure", s, geom, nt)) return rc;
    SrcParams P;
    src_params(s, geom, P);
    double vol = 0.0;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (dom_lo) {
        // :995: every boundary cell of the patch adds its weight dV
        const double dV = geom->ndim == 3 ? (geom->dx[0] * geom->dx[1]) * geom->dx[2] : geom->dx[0] * geom->dx[1];
        vol = (double)src_bdry_cells(geom->ndim, dom_lo, dom_hi, geom->ilower, geom->iupper) * dV;
        for (int d = 0; d < geom->ndim; ++d) {
            lo[d] = dom_lo[d];
            hi[d] = dom_hi[d];
        }
    }
    int device;
    hipStream_t stream;
    src_where(ctx, device, stream);
    SRC_HIP_TRY(hipSetDevice(device));
    SRC_HIP_TRY(launch_src_setup(P, X_src_dev, stream));
    SRC_HIP_TRY(launch_src_pressure(P, p_dev, P_src_dev, dom_lo ? 1 : 0, lo, hi, vol, stream));
    return IBTK_LE_OK;
}
