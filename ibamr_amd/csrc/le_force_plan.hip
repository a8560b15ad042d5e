// le_force_plan.hip -- the force plan of le_force.hip rebuilt on the device for a new
// numbering of the nodes (ibtk_le_forcegen_renumber, le_abi.cpp).
//
// The spec store (ibtk_le_forcespecs) keeps every spring, beam and target point in deck
// order with Lagrangian vertex indices.  order[i] is the Lagrangian index of node i; its
// inverse perm[lag] = node, or -1 for a vertex the numbering does not hold.  The
// reference numbers the specs "master by master in local node order, deck order within a
// master" (IBStandardInitializer.cpp:2815-2952), so per class:
//   1. keys: key[j] = perm[master of spec j] (the sentinel n_nodes for a dropped spec);
//   2. a stable sort of (key, j): position k of the result is the reference's spec k;
//   3. entries: spec k yields R entries (2 per spring, 3 per beam, 1 per target point),
//      entry R k + role keyed by the node of that role;
//   4. a stable sort of the entries by node: a node's entries ascend in k, roles in
//      statement order within one k -- the rows of the host plan (le_abi.cpp);
//   5. row offsets: off[i] = the first sorted entry keyed >= i;
//   6. gather: the record of every sorted entry, node indices through perm.
// The records come out byte for byte as the host counting sort of ibtk_le_forcegen_set_*
// writes them for perm.
//
// Indices.  The store's indices were checked on the host ([0, num_vertex)).  order comes
// from the caller's device memory: k_fp_scatter range-checks every entry before it is
// used as an index and detects a vertex listed twice; the key kernels find a kept spec
// with an absent endpoint.  Each writes the first offender into the status record and
// every later kernel skips what was flagged, so a bad order ends in a status, never in a
// stray access.
#include <hip/hip_runtime.h>

#include <climits>

#include "le_internal.h"

namespace ibtk_le {

namespace {

constexpr int FP_BLOCK = 256;

inline unsigned fp_grid(long n) { return (unsigned)((n + FP_BLOCK - 1) / FP_BLOCK); }

__global__ __launch_bounds__(FP_BLOCK) void k_fp_init(int* __restrict__ perm, int nv, FpStatus* __restrict__ st) {
    const long i = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i < nv) perm[i] = -1;
    if (i == 0) {
        st->bad_order = INT_MAX;
        st->dup_lag = INT_MAX;
        st->bad_spec[0] = st->bad_spec[1] = st->bad_spec[2] = INT_MAX;
        st->kept[0] = st->kept[1] = st->kept[2] = 0;
        st->need_U = 0;
    }
}

// perm[order[i]] = i.  An entry outside [0, nv) is flagged and not used; a vertex named
// twice is flagged (which of its nodes perm keeps is then arbitrary, and irrelevant).
__global__ __launch_bounds__(FP_BLOCK) void k_fp_scatter(const int* __restrict__ order, int n_order, int nv,
                                                         int* __restrict__ perm, FpStatus* __restrict__ st) {
    const long i = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n_order) return;
    const int v = order[i];
    if (v < 0 || v >= nv) {
        atomicMin(&st->bad_order, (int)i);
        return;
    }
    if (atomicCAS(&perm[v], -1, (int)i) != -1) atomicMin(&st->dup_lag, v);
}

// the vertices of a spec by role: the master first
__device__ __forceinline__ void fp_nodes(const FgSpring& r, int (&v)[2]) {
    v[0] = r.m;
    v[1] = r.s;
}
template <int ND>
__device__ __forceinline__ void fp_nodes(const FgBeam<ND>& r, int (&v)[3]) {
    v[0] = r.m;
    v[1] = r.nx;
    v[2] = r.pv;
}

// Springs and beams, spec j of the deck: key = its master's node, or the sentinel when
// the master is absent (dropped) or another endpoint is (an error, flagged).
template <class Rec, int R>
__global__ __launch_bounds__(FP_BLOCK) void k_fp_deck_keys(const Rec* __restrict__ rec, int n,
                                                           const int* __restrict__ perm, unsigned sentinel,
                                                           unsigned* __restrict__ keys, int* __restrict__ vals,
                                                           int* __restrict__ bad) {
    const long j = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= n) return;
    int v[R];
    fp_nodes(rec[j], v);
    const int pm = perm[v[0]];
    bool ok = pm >= 0;
    if (ok) {
#pragma unroll
        for (int q = 1; q < R; ++q) ok = ok && perm[v[q]] >= 0;
        if (!ok) atomicMin(bad, (int)j);
    }
    keys[j] = ok ? (unsigned)pm : sentinel;
    vals[j] = (int)j;
}

template <int ND>
__global__ __launch_bounds__(FP_BLOCK) void k_fp_target_keys(const int* __restrict__ node,
                                                             const FgTarget<ND>* __restrict__ rec, int n,
                                                             const int* __restrict__ perm, unsigned sentinel,
                                                             unsigned* __restrict__ keys, int* __restrict__ vals,
                                                             int* __restrict__ need_U) {
    const long j = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= n) return;
    const int pn = perm[node[j]];
    keys[j] = pn >= 0 ? (unsigned)pn : sentinel;
    vals[j] = (int)j;
    if (pn >= 0 && rec[j].eta != 0.0) *need_U = 1;  // every writer stores the same word
}

// spec k of the new numbering is deck spec dv[k]; its R entries, keyed by their nodes
template <class Rec, int R>
__global__ __launch_bounds__(FP_BLOCK) void k_fp_entries(const Rec* __restrict__ rec, int n,
                                                         const int* __restrict__ dv, const int* __restrict__ perm,
                                                         unsigned sentinel, unsigned* __restrict__ ekeys,
                                                         int* __restrict__ evals) {
    const long k = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (k >= n) return;
    int v[R], pn[R];
    fp_nodes(rec[dv[k]], v);
    bool ok = true;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        pn[q] = perm[v[q]];
        ok = ok && pn[q] >= 0;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        ekeys[R * k + q] = ok ? (unsigned)pn[q] : sentinel;
        evals[R * k + q] = (int)(R * k + q);
    }
}

// off[i] = the first sorted entry keyed >= i, i = 0 .. n_nodes; off[n_nodes] counts the
// kept entries (the dropped ones carry the sentinel n_nodes)
__global__ __launch_bounds__(FP_BLOCK) void k_fp_offsets(const unsigned* __restrict__ skeys, int E, int n_nodes,
                                                         int R, long long* __restrict__ off, int* __restrict__ kept) {
    const long i = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i > n_nodes) return;
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (skeys[mid] < (unsigned)i) lo = mid + 1;
        else hi = mid;
    }
    off[i] = lo;
    if (i == n_nodes) *kept = lo / R;
}

__global__ __launch_bounds__(FP_BLOCK) void k_fp_gather_springs(const unsigned* __restrict__ skeys,
                                                                const int* __restrict__ svals, int E,
                                                                unsigned sentinel, const int* __restrict__ dv,
                                                                const FgSpring* __restrict__ rec,
                                                                const int* __restrict__ perm,
                                                                FgSpring* __restrict__ out) {
    const long p = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (p >= E || skeys[p] >= sentinel) return;
    FgSpring r = rec[dv[svals[p] / 2]];
    r.m = perm[r.m];
    r.s = perm[r.s];
    out[p] = r;
}

template <int ND>
__global__ __launch_bounds__(FP_BLOCK) void k_fp_gather_beams(const unsigned* __restrict__ skeys,
                                                              const int* __restrict__ svals, int E, unsigned sentinel,
                                                              const int* __restrict__ dv,
                                                              const FgBeam<ND>* __restrict__ rec,
                                                              const int* __restrict__ perm,
                                                              FgBeam<ND>* __restrict__ out) {
    const long p = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (p >= E || skeys[p] >= sentinel) return;
    const int e = svals[p];
    FgBeam<ND> r = rec[dv[e / 3]];
    r.m = perm[r.m];
    r.nx = perm[r.nx];
    r.pv = perm[r.pv];
    r.role = e % 3;
    out[p] = r;
}

template <int ND>
__global__ __launch_bounds__(FP_BLOCK) void k_fp_gather_targets(const unsigned* __restrict__ skeys,
                                                                const int* __restrict__ svals, int E,
                                                                unsigned sentinel,
                                                                const FgTarget<ND>* __restrict__ rec,
                                                                FgTarget<ND>* __restrict__ out) {
    const long p = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (p >= E || skeys[p] >= sentinel) return;
    out[p] = rec[svals[p]];
}

}  // namespace

hipError_t launch_fp_perm(const int* order, int n_order, int nv, int* perm, FpStatus* st, hipStream_t s) {
    hipLaunchKernelGGL(k_fp_init, dim3(fp_grid(nv > 0 ? nv : 1)), dim3(FP_BLOCK), 0, s, perm, nv, st);
    if (n_order > 0)
        hipLaunchKernelGGL(k_fp_scatter, dim3(fp_grid(n_order)), dim3(FP_BLOCK), 0, s, order, n_order, nv, perm, st);
    return hipGetLastError();
}

hipError_t launch_fp_deck_keys(int cls, int ndim, const void* rec, int n, const int* perm, unsigned sentinel,
                               unsigned* keys, int* vals, FpStatus* st, hipStream_t s) {
    const dim3 g(fp_grid(n)), b(FP_BLOCK);
    if (cls == 0)
        hipLaunchKernelGGL((k_fp_deck_keys<FgSpring, 2>), g, b, 0, s, static_cast<const FgSpring*>(rec), n, perm,
                           sentinel, keys, vals, &st->bad_spec[0]);
    else if (ndim == 2)
        hipLaunchKernelGGL((k_fp_deck_keys<FgBeam<2>, 3>), g, b, 0, s, static_cast<const FgBeam<2>*>(rec), n, perm,
                           sentinel, keys, vals, &st->bad_spec[1]);
    else
        hipLaunchKernelGGL((k_fp_deck_keys<FgBeam<3>, 3>), g, b, 0, s, static_cast<const FgBeam<3>*>(rec), n, perm,
                           sentinel, keys, vals, &st->bad_spec[1]);
    return hipGetLastError();
}

hipError_t launch_fp_target_keys(int ndim, const int* node, const void* rec, int n, const int* perm,
                                 unsigned sentinel, unsigned* keys, int* vals, FpStatus* st, hipStream_t s) {
    const dim3 g(fp_grid(n)), b(FP_BLOCK);
    if (ndim == 2)
        hipLaunchKernelGGL((k_fp_target_keys<2>), g, b, 0, s, node, static_cast<const FgTarget<2>*>(rec), n, perm,
                           sentinel, keys, vals, &st->need_U);
    else
        hipLaunchKernelGGL((k_fp_target_keys<3>), g, b, 0, s, node, static_cast<const FgTarget<3>*>(rec), n, perm,
                           sentinel, keys, vals, &st->need_U);
    return hipGetLastError();
}

hipError_t launch_fp_entries(int cls, int ndim, const void* rec, int n, const int* dv, const int* perm,
                             unsigned sentinel, unsigned* ekeys, int* evals, hipStream_t s) {
    const dim3 g(fp_grid(n)), b(FP_BLOCK);
    if (cls == 0)
        hipLaunchKernelGGL((k_fp_entries<FgSpring, 2>), g, b, 0, s, static_cast<const FgSpring*>(rec), n, dv, perm,
                           sentinel, ekeys, evals);
    else if (ndim == 2)
        hipLaunchKernelGGL((k_fp_entries<FgBeam<2>, 3>), g, b, 0, s, static_cast<const FgBeam<2>*>(rec), n, dv, perm,
                           sentinel, ekeys, evals);
    else
        hipLaunchKernelGGL((k_fp_entries<FgBeam<3>, 3>), g, b, 0, s, static_cast<const FgBeam<3>*>(rec), n, dv, perm,
                           sentinel, ekeys, evals);
    return hipGetLastError();
}

hipError_t launch_fp_offsets(int cls, const unsigned* skeys, int E, int n_nodes, long long* off, FpStatus* st,
                             hipStream_t s) {
    const int R = cls == 0 ? 2 : cls == 1 ? 3 : 1;
    hipLaunchKernelGGL(k_fp_offsets, dim3(fp_grid((long)n_nodes + 1)), dim3(FP_BLOCK), 0, s, skeys, E, n_nodes, R, off,
                       &st->kept[cls]);
    return hipGetLastError();
}

hipError_t launch_fp_gather(int cls, int ndim, const unsigned* skeys, const int* svals, int E, unsigned sentinel,
                            const int* dv, const void* rec, const int* perm, void* out, hipStream_t s) {
    const dim3 g(fp_grid(E)), b(FP_BLOCK);
    if (cls == 0)
        hipLaunchKernelGGL(k_fp_gather_springs, g, b, 0, s, skeys, svals, E, sentinel, dv,
                           static_cast<const FgSpring*>(rec), perm, static_cast<FgSpring*>(out));
    else if (cls == 1 && ndim == 2)
        hipLaunchKernelGGL((k_fp_gather_beams<2>), g, b, 0, s, skeys, svals, E, sentinel, dv,
                           static_cast<const FgBeam<2>*>(rec), perm, static_cast<FgBeam<2>*>(out));
    else if (cls == 1)
        hipLaunchKernelGGL((k_fp_gather_beams<3>), g, b, 0, s, skeys, svals, E, sentinel, dv,
                           static_cast<const FgBeam<3>*>(rec), perm, static_cast<FgBeam<3>*>(out));
    else if (ndim == 2)
        hipLaunchKernelGGL((k_fp_gather_targets<2>), g, b, 0, s, skeys, svals, E, sentinel,
                           static_cast<const FgTarget<2>*>(rec), static_cast<FgTarget<2>*>(out));
    else
        hipLaunchKernelGGL((k_fp_gather_targets<3>), g, b, 0, s, skeys, svals, E, sentinel,
                           static_cast<const FgTarget<3>*>(rec), static_cast<FgTarget<3>*>(out));
    return hipGetLastError();
}

}  // namespace ibtk_le
