// le_imp.h -- internal descriptors of the immersed material point stages (le_imp.hip).
// Not part of the C-ABI (include/ibtk_le.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ibtk_le {

// The spread's tile of side points a workgroup owns (ibamr_amd.imp.IMP_TILE): IMP_TILE3^3
// in 3-D, IMP_TILE2^2 in 2-D; entries are staged in LDS IMP_CHUNK at a time.
constexpr int IMP_TILE3 = 8, IMP_TILE2 = 16, IMP_CHUNK = 64;
constexpr int IMP_REACH = 3;      // a stencil index lies within IMP_REACH of the cell-frame NINT anchor
constexpr int IMP_MIN_GHOST = 4;  // LEInteractor::getMinimumGhostWidth("IB_6")

// One side component in the reference's frame: x_lower[d] - 0.5 dx[d] for d == component,
// ghost box [lo, hi] (hi + 1 along its own axis), clip box [clo, chi] of the spread.
struct ImpComp {
    double* u;
    int lo[3], hi[3];
    int clo[3], chi[3];
    double xlo[3];
    int64_t s1, s2;
};

struct ImpParams {
    int ndim;
    int n;                              // list entries, in the markers' sorted order
    const double* sorted_X;             // X(s) + Xshift(l) per sorted position [NDIM]
    const double* const* sorted_X_ref;  // or the device cell naming the current buffer (a re-binned 3-D list)
    const int* sorted_s;                // sorted position -> marker row
    const int* qdst;                    // interp: the row a sorted entry writes, -1: a later duplicate does
    ImpComp comp[3];
    double dx[3];
    double xlo[3];  // cell-frame x_lower
    int ilower[3];
    double K;       // IB_6's K, from the host
    // interp
    double* U;
    double* GradU;
    // spread
    const double* tau;
    const double* wgt;
    double dV;          // (dx0 dx1) dx2
    int alo[3], aext[3];  // the anchor-cell grid: the ghost box widened by IMP_REACH + 1
    int ncells;           // its size; key ncells = outside
    int nt[3];            // tiles per dim
    unsigned* keys;       // anchor cell per sorted position ...
    int* vals;            // ... and the position
    const int* svals;     // positions sorted by anchor cell (stable: the markers' order within a cell)
    const int* start;     // ncells + 1 offsets into svals
};

hipError_t launch_imp_interp(const ImpParams& P, hipStream_t s);
hipError_t launch_imp_keys(const ImpParams& P, hipStream_t s);
hipError_t launch_imp_spread(const ImpParams& P, hipStream_t s);

// F_new = inv(I - a dt Gb) (I + a dt Ga) F_cur, a = 0.5; F_half (or null) the same with a = 0.25
hipError_t launch_imp_update(int ndim, long long n, double dt, const double* F_cur, const double* Ga, const double* Gb,
                             double* F_new, double* F_half, hipStream_t s);
// tau = PP FF^T; par = {c1, p0, beta}, or row subdomain[i] of table[nsub][3]
hipError_t launch_imp_stress(int ndim, long long n, const double* F, double* tau, double c1, double p0, double beta,
                             const double* table, int nsub, const int* subdomain, hipStream_t s);

}  // namespace ibtk_le
