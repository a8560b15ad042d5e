// le_hot.hip -- the 2-D hot path on CDNA4 (gfx950): brick binning,
// interpolation and spreading.  Replaces the l-loops of
// ibtk/src/lagrangian/fortran/lagrangian_interaction2d.f.m4.  Everything here
// is 2-D; the 3-D path is le_sweep.hip's column sweeps.
//
// Work decomposition:
//  * bin: key = brick id (tiled, le_bricks.h) << 8 | cell-in-brick of the
//    marker's cell-frame stencil anchor (16^2-cell bricks); stable device radix
//    sort; brick CSR; then one coalescing pass writes the sorted marker index
//    and the sorted shifted position X(s)+Xshift(l), so the interp/spread
//    kernels read their markers contiguously.
//  * interp: one workgroup item = 2x2 bricks (one brick for the kernels wider
//    than 4 points), component after component.  The union stencil region
//    of the item's markers is loaded from HBM with every load of a thread in
//    flight at once and staged in LDS; one thread per marker then sums its W^2
//    stencil from LDS in the Fortran loop order, so the result is bitwise the
//    oracle's.
//  * spread: one workgroup item = a super-brick of 2x2 bricks, component after
//    component.  The candidate lists (k_cand, once per binning) hold, per
//    super-brick and class of two anchor rows, the sorted entries whose stencil
//    can reach it, in canonical (sorted) order.  The workgroup loads u_old of
//    its points into LDS; its waves take the classes of a phase concurrently,
//    64 candidates at a time with lane = candidate, and add stencil point after
//    stencil point (ds_add_f64 into LDS).  A grid point receives its
//    contributions in a fixed order (phase, class list order, stencil point,
//    lane): no global atomics, deterministic and bit-stable run to run.  That
//    order is the Fortran's sequential l-loop reassociated, so the result is
//    not bitwise the oracle's on the same list: tests/test_gpu_2d_dense.py saw
//    1 of its 43 spreads agree bit for bit (PIECEWISE_CONSTANT, cell data), the
//    others within 2e-15 of the largest value, against a tolerance of 1e-12.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>

#include "le_bricks.h"
#include "le_internal.h"
#include "le_stencil.h"

namespace ibtk_le {

constexpr int SBLOCK = 256;  // spread workgroup (4 waves); the interp runs BLOCK = 256 threads (le_internal.h)

static int num_cus() {
    static int ncu = 0;
    if (!ncu) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0)
            ncu = 256;
    }
    return ncu;
}

static int grid_for(long items, int per_cu) {
    long g = (long)num_cus() * per_cu;
    if (g > items) g = items;
    if (g >= 8) g &= ~7L;
    return (int)(g > 0 ? g : 1);
}

// ---------------------------------------------------------------------------
// binning
// ---------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(BLOCK) void k_bin(Params p, int n, unsigned* keys, int* vals) {
    constexpr int B = BrickT::B;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = p.indices ? p.indices[i] : i;
    bool out = false;
    int rel[2] = {0, 0};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double Xs = p.X[(int64_t)2 * s + d] + (p.Xshift ? p.Xshift[(int64_t)2 * i + d] : 0.0);
        const double xo = (Xs - p.bg.xlo[d]) / p.bg.dx[d];
        if (!(fabs(xo) < 1.0e9)) {  // also catches NaN
            out = true;
            continue;
        }
        rel[d] = key_anchor<K>(xo) + p.bg.ilower[d] - p.bg.kmin[d];
        if (rel[d] < 0 || rel[d] >= p.bg.nb[d] * B) out = true;
    }
    unsigned key;
    if (out) {
        key = (unsigned)p.bg.nbricks << BrickT::SHIFT;
    } else {
        int bc[2] = {0, 0};
        unsigned local = 0;
        for (int d = 1; d >= 0; --d) {
            bc[d] = rel[d] / B;
            local = local * (unsigned)B + (unsigned)(rel[d] - bc[d] * B);
        }
        key = ((unsigned)brick_id(p.bg, bc) << BrickT::SHIFT) | local;
    }
    keys[i] = key;
    vals[i] = i;
}

// bs[b] = first sorted position whose bucket (key >> shift) >= b, for b in [0, nbuckets]
// (buckets = cell planes of bricks: plane_start).
__global__ __launch_bounds__(BLOCK) void k_brick_start(const unsigned* keys, int n, int nbricks, int shift, int* bs) {  // nbricks = nbuckets
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    const int bi = (i < n) ? (int)min(keys[i] >> shift, (unsigned)nbricks) : nbricks + 1;
    const int bp = (i == 0) ? -1 : (int)min(keys[i - 1] >> shift, (unsigned)nbricks);
    for (int b = bp + 1; b <= bi && b <= nbricks; ++b) bs[b] = i;
}

// sorted marker index and sorted X(s) + Xshift(l) (the Fortran's X(d,s)+Xshift(d,l))
__global__ __launch_bounds__(BLOCK) void k_gather_sorted(Params p, int n, int* sorted_s, double* sorted_X) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n) return;
    const int l = p.sorted_l[e];
    const int s = p.indices ? p.indices[l] : l;
    sorted_s[e] = s;
#pragma unroll
    for (int d = 0; d < 2; ++d)
        sorted_X[(int64_t)2 * e + d] = p.X[(int64_t)2 * s + d] + (p.Xshift ? p.Xshift[(int64_t)2 * l + d] : 0.0);
}

template <int K>
hipError_t launch_bin_t(const Params& p, int n, unsigned* keys, int* vals, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((k_bin<K>), dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, p, n, keys, vals);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// interpolation
// ---------------------------------------------------------------------------
// Interpolation work item: a group of GB consecutive bricks (2x2 bricks, or
// one brick for the wide kernels) and all its markers; per component the union
// stencil region of the group, R0 x R1 points, is staged in LDS.
template <int K> struct IShape {
    using T = KT<K>;
    static constexpr int B = BrickT::B;
    static constexpr int GB = T::W <= 4 ? 4 : 1;   // bricks per item (ids b..b+GB-1: 2x2 in Morton order)
    static constexpr int E0 = GB == 4 ? 2 * B : B;  // anchor extent of the item in dims 0 and 1
    static constexpr int R0 = E0 + T::HI - T::LO, R1 = R0;
    static constexpr int RV = R0 * R1;
    static constexpr int NL = (RV + BLOCK - 1) / BLOCK;  // staged values per thread
};

template <int K>
__device__ __forceinline__ void marker_stencils_x(const Params& p, const CompDesc& cd, const double* Xs, int s,
                                                  St<KT<K>::W>* st) {
    constexpr int FAM = KT<K>::FAM;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double Xraw = (FAM == 2) ? p.X[(int64_t)2 * s + d] : Xs[d];
        stencil1d<K>(Xs[d], Xraw, cd.xlo[d], p.bg.dx[d], cd.ilower[d], cd.lo[d], cd.hi[d], d == cd.axis, p.K6,
                     st[d]);
    }
}

// region value loads of component cd for the item whose region starts at r0
template <int K>
__device__ __forceinline__ void stage_load(const CompDesc& cd, const int* r0, double* v) {
    using S = IShape<K>;
    constexpr int R0 = S::R0, R1 = S::R1, RV = S::RV;
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int R = d == 0 ? R0 : R1;
        inside = inside && r0[d] >= cd.lo[d] && r0[d] + R - 1 <= cd.hi[d];
    }
    const int64_t o0 = (int64_t)(r0[0] - cd.lo[0]) + (int64_t)(r0[1] - cd.lo[1]) * cd.s1;
    // (recomputed per item on purpose: hoisted out of the item loop, the 3*NL
    // index registers would stay live through the stencil sums)
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
#pragma unroll
    for (int k = 0; k < S::NL; ++k) {
        const int q = t + k * BLOCK;
        v[k] = 0.0;
        if (q < RV) {
            const int i0 = q % R0, i1 = (q / R0) % R1;
            if (inside) {
                v[k] = cd.u[o0 + i0 + (int64_t)i1 * cd.s1];
            } else {
                const int g0 = r0[0] + i0, g1 = r0[1] + i1;
                const bool in = g0 >= cd.lo[0] && g0 <= cd.hi[0] && g1 >= cd.lo[1] && g1 <= cd.hi[1];
                if (in)
                    v[k] = cd.u[(int64_t)(g0 - cd.lo[0]) + (int64_t)(g1 - cd.lo[1]) * cd.s1];
            }
        }
    }
}

// One workgroup item = GB bricks, every component: the component's region is
// staged in LDS (the next component's loads are in flight while this one is
// summed), then one thread per marker sums its W^2 stencil from LDS in the
// Fortran loop order -- bitwise the oracle's value.
template <int K>
__global__ __launch_bounds__(BLOCK) void k_interp(Params p) {
    using T = KT<K>;
    using S = IShape<K>;
    constexpr int W = T::W, FAM = T::FAM, B = S::B, R0 = S::R0, R1 = S::R1, NL = S::NL;
    __shared__ double reg[S::RV];
    const int nc = p.ncomp;
    const int nitems = p.bg.nbricks / S::GB;
    const int G = gridDim.x;
    const int tid = threadIdx.x;
    for (int round = 0; round < nitems; round += G) {
        const int it = xcd_item(round, G, blockIdx.x);
        if (it >= nitems) continue;
        const int b0 = it * S::GB;
        const int beg = p.plane_start[b0 * B], end = p.plane_start[(b0 + S::GB) * B];
        if (beg == end) continue;
        int bc[2];
        brick_coords(p.bg, b0, bc);
        int r0[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) r0[d] = p.bg.kmin[d] + bc[d] * B + T::LO;
        // this thread's first marker, kept across the components
        const int e0 = beg + tid;
        int s0 = 0;
        double x0[2];
        if (e0 < end) {
            s0 = p.sorted_s[e0];
#pragma unroll
            for (int d = 0; d < 2; ++d) x0[d] = p.sorted_X[(int64_t)2 * e0 + d];
        }
        for (int c = 0; c < nc; ++c) {
            const CompDesc& cd = p.comp[c];
            {
                double v[NL];
                stage_load<K>(cd, r0, v);
                __syncthreads();  // the previous readers of reg are done
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    const int q = tid + k * BLOCK;
                    if (q < S::RV) reg[q] = v[k];
                }
                __syncthreads();
            }

            for (int e = e0; e < end; e += BLOCK) {
                int s = s0;
                double xs[2];
#pragma unroll
                for (int d = 0; d < 2; ++d) xs[d] = x0[d];
                if (e != e0) {
                    s = p.sorted_s[e];
#pragma unroll
                    for (int d = 0; d < 2; ++d) xs[d] = p.sorted_X[(int64_t)2 * e + d];
                }
                St<W> st[2];
                marker_stencils_x<K>(p, cd, xs, s, st);
                bool ok = true;
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int R = d == 0 ? R0 : R1;
                    if (st[d].ist <= st[d].isp)
                        ok = ok && (st[d].icl + st[d].ist >= r0[d]) && (st[d].icl + st[d].isp < r0[d] + R);
                }
                if (!ok) {
                    atomicOr(p.err, 1);
                    continue;
                }
                double acc = 0.0;
                if constexpr (FAM == 3) {
                    if (st[0].ist <= st[0].isp && st[1].ist <= st[1].isp)
                        acc = reg[st[0].icl - r0[0] + R0 * (st[1].icl - r0[1])];
                } else {
                    // Clipped stencil entries (outside [ist, isp]) get weight 0 and a
                    // clamped (in-region) LDS index: acc + 0 == acc, so the sum equals
                    // the Fortran's clipped sum bit for bit, without per-term branches.
                    double w[2][W];
                    int o[2][W];
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        const int R = d == 0 ? R0 : R1;
                        const int stride = d == 0 ? 1 : R0;
#pragma unroll
                        for (int i = 0; i < W; ++i) {
                            const bool in = i >= st[d].ist && i <= st[d].isp;
                            w[d][i] = in ? st[d].w[i] : 0.0;
                            o[d][i] = min(max(st[d].icl + i - r0[d], 0), R - 1) * stride;
                        }
                    }
#pragma unroll
                    for (int i1 = 0; i1 < W; ++i1) {
                        const double* row = reg + o[1][i1];
#pragma unroll
                        for (int i0 = 0; i0 < W; ++i0) {
                            if constexpr (FAM == 0) {
                                const double wt = w[0][i0] * w[1][i1];
                                acc = acc + wt * row[o[0][i0]];
                            } else {
                                acc = acc + w[0][i0] * w[1][i1] * row[o[0][i0]];
                            }
                        }
                    }
                }
                const int sq = p.qdst ? p.qdst[e] : s;
                if (sq >= 0) p.Qout[(int64_t)p.Q_depth * sq + cd.qcomp] = acc;
            }
        }
    }
}

// Entries binned "outside" (no stencil point can reach any array): V = 0.
__global__ __launch_bounds__(BLOCK) void k_interp_outside(Params p, int n) {
    const int first = p.plane_start[p.bg.nbricks * BRICK2];
    for (int e = first + blockIdx.x * BLOCK + threadIdx.x; e < n; e += gridDim.x * BLOCK) {
        const int s = p.qdst ? p.qdst[e] : p.sorted_s[e];
        if (s < 0) continue;
        for (int c = 0; c < p.ncomp; ++c) p.Qout[(int64_t)p.Q_depth * s + p.comp[c].qcomp] = 0.0;
    }
}

template <int K>
hipError_t launch_interp_t(const Params& p, int n, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    using S = IShape<K>;
    if (ev0) (void)hipEventRecord(ev0, s);
    const long items = (long)(p.bg.nbricks / S::GB);
    hipLaunchKernelGGL((k_interp<K>), dim3(grid_for(items, 64)), dim3(BLOCK), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (n > 0) hipLaunchKernelGGL(k_interp_outside, dim3(64), dim3(BLOCK), 0, s, p, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// spreading
// ---------------------------------------------------------------------------
// Work item: one super-brick (2x2 bricks: 32^2 cells).
// Its candidates -- the markers whose stencil can reach it -- are grouped into
// "classes" of CW anchor rows (y).  A class's stencils lie in
// CW + HI - LO consecutive rows, so classes NPH apart never touch the same
// grid point: in phase ph the waves of the workgroup take the classes
// ph, ph + NPH, ... concurrently, phases separated by a barrier.
template <int K> struct SShape {
    using BT = BrickT;
    static constexpr int B = BT::B, SB = BT::SB, SBV = BT::SBV, GROUP = BT::GROUP;
    static constexpr int W = KT<K>::W, LO = KT<K>::LO, HI = KT<K>::HI;
    static constexpr int NQ = SBLOCK / 64;                                // waves
    static constexpr int NBR = 16;                                        // neighbourhood bricks (4 per dim)
    static constexpr int KMAX = 4;                                        // entries per thread per list sub-pass
    static constexpr int CW = 2;                                          // anchor rows per class
    static constexpr int NCLS = (SB - 1 + HI - LO) / CW + 1;              // classes of a super-brick
    static constexpr int NPH = 1 + (HI - LO + CW - 1) / CW;               // phases
    static constexpr int NACC = SBV / SBLOCK;                             // u values per thread
    static constexpr int LB = 4;                                          // log2(B)
    static constexpr int MAXOFF = (W - 1) * (1 + SB);
    static constexpr int TRASH = 64 + MAXOFF + 1;                         // per-lane sink of masked points
    static_assert(HI <= B && -LO <= B, "a stencil must not reach beyond the neighbouring brick");
    static_assert(NPH * CW >= CW + HI - LO, "classes of one phase must be disjoint");
};

// The sorted entries that can reach super-brick `sb`: for each of the 4x4
// bricks around it, the run of its cell rows (entries of a brick are sorted by
// cell, y slowest) whose anchors can reach the
// super-brick, the runs ranked by brick id (= canonical order).  Returns the
// number of entries; npre[] are the runs' prefix offsets, sst[] their starts,
// soff[] the packed 2-bit (offset + 1) of their bricks.
template <int K>
__device__ int neighbourhood(const Params& p, int sb, int* nid, int* nst, int* nln, int* sst, int* soff, int* npre) {
    using S = SShape<K>;
    constexpr int B = S::B, NBR = S::NBR, HI = S::HI, LO = S::LO;
    const int tid = threadIdx.x;
    int bc0[2];
    brick_coords(p.bg, sb * S::GROUP, bc0);
    __syncthreads();  // the tables are free
    if (tid < NBR) {
        const int o[2] = {tid & 3, (tid >> 2) & 3};
        const int q[2] = {bc0[0] + o[0] - 1, bc0[1] + o[1] - 1};
        bool valid = true;
        for (int d = 0; d < 2; ++d) valid = valid && q[d] >= 0 && q[d] < p.bg.nb[d];
        const int ol = o[1];
        const int plo = ol == 0 ? B - HI : 0;       // rows whose anchors reach the super-brick
        const int phi = ol == 3 ? -LO - 1 : B - 1;  // (inclusive)
        int id = INT_MAX, st = 0, ln = 0;
        if (valid) {
            id = brick_id(p.bg, q);
            st = p.plane_start[id * B + plo];
            ln = p.plane_start[id * B + phi + 1] - st;
        }
        nid[tid] = id;
        nst[tid] = st;
        nln[tid] = ln;
    }
    __syncthreads();
    if (tid < NBR) {
        const int my = nid[tid];
        int rank = 0;
        for (int k = 0; k < NBR; ++k) {
            const int o = nid[k];
            rank += (o < my) || (o == my && k < tid);
        }
        sst[rank] = nst[tid];
        soff[rank] = tid;
        npre[rank + 1] = nln[tid];
    }
    __syncthreads();
    if (tid == 0) {
        npre[0] = 0;
        for (int k = 0; k < NBR; ++k) npre[k + 1] += npre[k];
    }
    __syncthreads();
    return npre[NBR];
}

// entry e of the neighbourhood -> sorted index (and the packed brick offset)
template <int NBR> __device__ __forceinline__ int entry_of(int e, const int* npre, const int* sst, const int* soff, int& ro) {
    int lo = 0, hi = NBR - 1;  // largest j with npre[j] <= e
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (npre[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    ro = soff[lo];
    return sst[lo] + (e - npre[lo]);
}

// class of the entry with this key (in the brick at packed offset ro) for the
// super-brick, or -1 if its stencil cannot reach the super-brick
template <int K> __device__ __forceinline__ int cand_class(unsigned key, int ro) {
    using S = SShape<K>;
    bool cand = true;
    int rl = 0;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int rel = (((ro >> (2 * d)) & 3) - 1) * S::B + (int)((key >> (S::LB * d)) & (S::B - 1));
        cand = cand && rel >= -S::HI && rel <= S::SB - 1 - S::LO;
        rl = rel;
    }
    return cand ? (rl + S::HI) / S::CW : -1;
}

// Candidate lists, built once per binning: for super-brick sb and class k, the
// entries of that class whose stencil can reach sb, in canonical order, at
// [off[sb*NCLS + k], off[sb*NCLS + k + 1]).  Pass 1 counts, an exclusive scan
// gives the offsets, pass 2 writes (ordered block compaction per class).
template <int K, bool WRITE>
__global__ __launch_bounds__(SBLOCK) void k_cand(Params p, int* counts_or_offs, int* out) {
    using S = SShape<K>;
    constexpr int NBR = S::NBR, KMAX = S::KMAX, NQ = S::NQ, NCLS = S::NCLS;
    __shared__ int nid[NBR], nst[NBR], nln[NBR], sst[NBR], soff[NBR], npre[NBR + 1];
    __shared__ int cnt[KMAX * NQ * NCLS];
    __shared__ int cbase[NCLS];
    const int nitems = p.bg.nbricks / S::GROUP;
    const int sb = xcd_item(0, gridDim.x, blockIdx.x);
    if (sb >= nitems) return;
    const int total = neighbourhood<K>(p, sb, nid, nst, nln, sst, soff, npre);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!WRITE) {
        if (tid < NCLS) cbase[tid] = 0;
        __syncthreads();
        for (int e = tid; e < total; e += SBLOCK) {
            int ro;
            const int idx = entry_of<NBR>(e, npre, sst, soff, ro);
            const int k = cand_class<K>(p.sorted_key[idx], ro);
            if (k >= 0) atomicAdd(&cbase[k], 1);
        }
        __syncthreads();
        if (tid < NCLS) counts_or_offs[sb * NCLS + tid] = cbase[tid];
        return;
    }
    if (tid < NCLS) cbase[tid] = counts_or_offs[sb * NCLS + tid];
    for (int e0 = 0; e0 < total; e0 += KMAX * SBLOCK) {
        int eidx[KMAX], cls[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int e = e0 + k * SBLOCK + tid;
            eidx[k] = -1;
            cls[k] = -1;
            int ro = 0;
            if (e < total) eidx[k] = entry_of<NBR>(e, npre, sst, soff, ro);
            if (eidx[k] >= 0) cls[k] = cand_class<K>(p.sorted_key[eidx[k]], ro);
        }
        // per (sub-pass slot, wave, class) counts; entry order is (k, wave, lane)
        unsigned long long mine[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            mine[k] = 0ull;
            for (int c = 0; c < NCLS; ++c) {
                const unsigned long long b = __ballot(cls[k] == c);
                if (cls[k] == c) mine[k] = b;
                if (lane == 0) cnt[(k * NQ + wave) * NCLS + c] = __popcll(b);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int c = cls[k];
            if (c >= 0) {
                int pos = cbase[c];
                for (int j = 0; j < k * NQ + wave; ++j) pos += cnt[j * NCLS + c];
                pos += __popcll(mine[k] & ((1ull << lane) - 1ull));
                out[pos] = eidx[k];
            }
        }
        __syncthreads();
        if (tid < NCLS) {
            int t = 0;
            for (int j = 0; j < KMAX * NQ; ++j) t += cnt[j * NCLS + tid];
            cbase[tid] += t;
        }
        __syncthreads();
    }
}

// sorted_F[c * n + e] = Q(qcomp_c, s(e)): the spread values in sorted order, so
// the spread kernel's loads of them are contiguous and not behind the s load.
__global__ __launch_bounds__(BLOCK) void k_gather_F(Params p, int n, double* out) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n) return;
    const int s = p.sorted_s[e];
    // density-weighted spread: F ds rounded once, as LDataManager.cpp:446-451 forms it
    const double w = p.ds ? p.ds[s] : 1.0;
    for (int c = 0; c < p.ncomp; ++c) {
        const double v = p.Qin[(int64_t)p.Q_depth * s + p.comp[c].qcomp];
        out[(int64_t)c * n + e] = p.ds ? v * w : v;
    }
}

// Spread of one super-brick, component after component: u_old goes to LDS; in
// each phase every wave takes its classes' candidates 64 at a time, one per
// lane: the lane computes the candidate's 1-D weights in registers and adds its
// W^2 stencil points to LDS (ds_add_f64, one instruction per stencil point
// for the 64 candidates; points outside the super-brick or clipped by the
// ghost box go to a per-lane sink).  A grid point receives its contributions
// in a fixed order -- phase, class list order, stencil point, lane -- so the
// result is deterministic run to run (and equal to the sequential Fortran sum
// up to reassociation).
template <int K>
__global__ __launch_bounds__(SBLOCK) void k_spread(Params p) {
    using T = KT<K>;
    using S = SShape<K>;
    constexpr int W = T::W, FAM = T::FAM, LO = T::LO, HI = T::HI;
    constexpr int B = S::B, SB = S::SB, SBV = S::SBV, NQ = S::NQ, NCLS = S::NCLS, NPH = S::NPH, CW = S::CW;
    __shared__ double acc[SBV + S::TRASH];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nc = p.ncomp;
    const int n = p.nsorted;
    const int nitems = p.bg.nbricks / S::GROUP;
    const int G = gridDim.x;
    const int sink = SBV + lane;  // this lane's sink slot
    for (int round = 0; round < nitems; round += G) {
        const int sb = xcd_item(round, G, blockIdx.x);
        if (sb >= nitems) continue;
        const int* off = p.cand_off + (int64_t)sb * NCLS;
        if (off[NCLS] == off[0]) continue;  // no candidates: u unchanged
        int bc0[2];
        brick_coords(p.bg, sb * S::GROUP, bc0);
        int kb0[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) kb0[d] = p.bg.kmin[d] + bc0[d] * B;

        // the first 64 candidates of this wave's first class in each phase:
        // indices and positions loaded once, kept across the components
        int idx0[NPH];
        double X0[NPH][2];
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph) {
            const int k = ph + NPH * wave;
            idx0[ph] = -1;
            if (k < NCLS) {
                const int e = off[k] + lane;
                if (e < off[k + 1]) idx0[ph] = p.cand_idx[e];
            }
        }
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
            for (int d = 0; d < 2; ++d) X0[ph][d] = idx0[ph] >= 0 ? p.sorted_X[(int64_t)2 * idx0[ph] + d] : 0.0;

        for (int c = 0; c < nc; ++c) {
            const CompDesc& cd = p.comp[c];
            bool inside = true;
#pragma unroll
            for (int d = 0; d < 2; ++d) inside = inside && kb0[d] >= cd.lo[d] && kb0[d] + SB - 1 <= cd.hi[d];
            const int64_t o0 = (int64_t)(kb0[0] - cd.lo[0]) + (int64_t)(kb0[1] - cd.lo[1]) * cd.s1;
            double v[S::NACC];
#pragma unroll
            for (int k = 0; k < S::NACC; ++k) {
                const int q = tid + k * SBLOCK;
                const int i0 = q % SB, i1 = q / SB;
                v[k] = 0.0;
                if (inside) {
                    v[k] = cd.u[o0 + i0 + (int64_t)i1 * cd.s1];
                } else {
                    const int g0 = kb0[0] + i0, g1 = kb0[1] + i1;
                    if (g0 >= cd.lo[0] && g0 <= cd.hi[0] && g1 >= cd.lo[1] && g1 <= cd.hi[1])
                        v[k] = cd.u[(int64_t)(g0 - cd.lo[0]) + (int64_t)(g1 - cd.lo[1]) * cd.s1];
                }
            }
            double F0[NPH];
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) F0[ph] = idx0[ph] >= 0 ? p.sorted_F[(int64_t)c * n + idx0[ph]] : 0.0;
            __syncthreads();  // the previous component's write-back has read acc
#pragma unroll
            for (int k = 0; k < S::NACC; ++k) acc[tid + k * SBLOCK] = v[k];
            __syncthreads();

#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) {
                for (int k = ph + NPH * wave; k < NCLS; k += NPH * NQ) {
                    const int first = k == ph + NPH * wave;
                    for (int e0 = off[k]; e0 < off[k + 1]; e0 += 64) {
                        // ---- this lane's candidate
                        int idx;
                        double Xs[2], F;
                        if (first && e0 == off[k]) {
                            idx = idx0[ph];
#pragma unroll
                            for (int d = 0; d < 2; ++d) Xs[d] = X0[ph][d];
                            F = F0[ph];
                        } else {
                            const int e = e0 + lane;
                            idx = e < off[k + 1] ? p.cand_idx[e] : -1;
#pragma unroll
                            for (int d = 0; d < 2; ++d) Xs[d] = idx >= 0 ? p.sorted_X[(int64_t)2 * idx + d] : 0.0;
                            F = idx >= 0 ? p.sorted_F[(int64_t)c * n + idx] : 0.0;
                        }
                        const int s = (FAM == 2 && idx >= 0) ? p.sorted_s[idx] : 0;
                        St<W> st[2];
                        marker_stencils_x<K>(p, cd, Xs, s, st);
                        // valid stencil indices per dim: inside the clip range and the super-brick
                        unsigned vm[2] = {0u, 0u};
                        double w[2][W];
                        int base = 0, mul = 1;
#pragma unroll
                        for (int d = 0; d < 2; ++d) {
#pragma unroll
                            for (int i = 0; i < W; ++i) {
                                const int lc = st[d].icl + i - kb0[d];
                                if (idx >= 0 && i >= st[d].ist && i <= st[d].isp && lc >= 0 && lc < SB) vm[d] |= 1u << i;
                                // closed form: wy = w1/(dx0*dx1)
                                w[d][i] = (FAM == 0 && d == 1) ? st[d].w[i] / p.h3 : st[d].w[i];
                            }
                            base += (st[d].icl - kb0[d]) * mul;
                            mul *= SB;
                        }
                        // class invariant: the stencil's rows lie in the class footprint
                        if (idx >= 0 && st[1].ist <= st[1].isp) {
                            const int y0 = st[1].icl + st[1].ist - kb0[1], y1 = st[1].icl + st[1].isp - kb0[1];
                            if (y0 < k * CW - HI + LO || y1 > k * CW + CW - 1) atomicOr(p.err, 2);
                        }
                        // ---- add the W^2 points (lane = candidate)
#pragma unroll
                        for (int i1 = 0; i1 < W; ++i1) {
                            const bool v1 = ((vm[1] >> i1) & 1u) != 0u;
#pragma unroll
                            for (int i0 = 0; i0 < W; ++i0) {
                                const bool on = v1 && ((vm[0] >> i0) & 1u);
                                double cv;
                                if constexpr (FAM == 3) cv = F / p.h3;
                                else if constexpr (FAM == 0) cv = (w[0][i0] * w[1][i1]) * F;
                                else cv = w[0][i0] * w[1][i1] * F / p.h3;  // f.m4:668-672
                                const int a = on ? base : sink;
                                __hip_atomic_fetch_add(&acc[a + i0 + SB * i1], cv, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                    }
                }
                __syncthreads();  // phase boundary
            }
            // write back the super-brick's points
#pragma unroll
            for (int k = 0; k < S::NACC; ++k) {
                const int q = tid + k * SBLOCK;
                const int i0 = q % SB, i1 = q / SB;
                if (inside) {
                    cd.u[o0 + i0 + (int64_t)i1 * cd.s1] = acc[q];
                } else {
                    const int g0 = kb0[0] + i0, g1 = kb0[1] + i1;
                    if (g0 >= cd.lo[0] && g0 <= cd.hi[0] && g1 >= cd.lo[1] && g1 <= cd.hi[1])
                        cd.u[(int64_t)(g0 - cd.lo[0]) + (int64_t)(g1 - cd.lo[1]) * cd.s1] = acc[q];
                }
            }
        }
    }
}

template <int K>
hipError_t launch_cand_t(const Params& p, bool write, int* counts_or_offs, int* out, hipStream_t s) {
    using S = SShape<K>;
    const int items = p.bg.nbricks / S::GROUP;
    if (write)
        hipLaunchKernelGGL((k_cand<K, true>), dim3(items), dim3(SBLOCK), 0, s, p, counts_or_offs, out);
    else
        hipLaunchKernelGGL((k_cand<K, false>), dim3(items), dim3(SBLOCK), 0, s, p, counts_or_offs, out);
    return hipGetLastError();
}

template <int K> int cand_classes_t() { return SShape<K>::NCLS; }

template <int K>
hipError_t launch_spread_t(const Params& p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    using S = SShape<K>;
    if (ev0) (void)hipEventRecord(ev0, s);
    if (p.nsorted > 0)
        hipLaunchKernelGGL(k_gather_F, dim3((p.nsorted + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, p, p.nsorted,
                           const_cast<double*>(p.sorted_F));
    const long items = (long)(p.bg.nbricks / S::GROUP);
    hipLaunchKernelGGL((k_spread<K>), dim3(grid_for(items, 64)), dim3(SBLOCK), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
#define IBTK_LE_DISPATCH(KV, CALL)                                     \
    switch (KV) {                                                      \
    case K_PIECEWISE_CONSTANT: return CALL<K_PIECEWISE_CONSTANT>;      \
    case K_DISCONTINUOUS_LINEAR: return CALL<K_DISCONTINUOUS_LINEAR>;  \
    case K_PIECEWISE_LINEAR: return CALL<K_PIECEWISE_LINEAR>;          \
    case K_PIECEWISE_CUBIC: return CALL<K_PIECEWISE_CUBIC>;            \
    case K_IB_3: return CALL<K_IB_3>;                                  \
    case K_IB_4: return CALL<K_IB_4>;                                  \
    case K_IB_4_W8: return CALL<K_IB_4_W8>;                            \
    case K_IB_6: return CALL<K_IB_6>;                                  \
    case K_BSPLINE_4: return CALL<K_BSPLINE_4>;                        \
    default: return nullptr;                                           \
    }

using BinFn = hipError_t (*)(const Params&, int, unsigned*, int*, hipStream_t);
using InterpFn = hipError_t (*)(const Params&, int, hipStream_t, hipEvent_t, hipEvent_t);
using SpreadFn = hipError_t (*)(const Params&, hipStream_t, hipEvent_t, hipEvent_t);
using CandFn = hipError_t (*)(const Params&, bool, int*, int*, hipStream_t);
using ClsFn = int (*)();

static BinFn pick_bin(int k) { IBTK_LE_DISPATCH(k, launch_bin_t) }
static InterpFn pick_interp(int k) { IBTK_LE_DISPATCH(k, launch_interp_t) }
static SpreadFn pick_spread(int k) { IBTK_LE_DISPATCH(k, launch_spread_t) }
static CandFn pick_cand(int k) { IBTK_LE_DISPATCH(k, launch_cand_t) }
static ClsFn pick_cls(int k) { IBTK_LE_DISPATCH(k, cand_classes_t) }

hipError_t launch_bin(int kernel, const Params& p, int n, unsigned* keys, int* vals, hipStream_t s) {
    BinFn f = pick_bin(kernel);
    return f ? f(p, n, keys, vals, s) : hipErrorInvalidValue;
}
hipError_t launch_brick_start(const unsigned* keys, int n, int nbricks, int shift, int* bs, hipStream_t s) {
    hipLaunchKernelGGL(k_brick_start, dim3((n + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, keys, n, nbricks, shift,
                       bs);
    return hipGetLastError();
}
hipError_t launch_gather_sorted(const Params& p, int n, int* sorted_s, double* sorted_X, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_sorted, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, p, n, sorted_s, sorted_X);
    return hipGetLastError();
}
hipError_t launch_interp(int kernel, const Params& p, int n, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    InterpFn f = pick_interp(kernel);
    return f ? f(p, n, s, ev0, ev1) : hipErrorInvalidValue;
}
hipError_t launch_cand(int kernel, const Params& p, bool write, int* counts_or_offs, int* out, hipStream_t s) {
    CandFn f = pick_cand(kernel);
    return f ? f(p, write, counts_or_offs, out, s) : hipErrorInvalidValue;
}
int cand_classes(int kernel) {
    ClsFn f = pick_cls(kernel);
    return f ? f() : 0;
}
hipError_t launch_spread(int kernel, const Params& p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    SpreadFn f = pick_spread(kernel);
    return f ? f(p, s, ev0, ev1) : hipErrorInvalidValue;
}

}  // namespace ibtk_le
