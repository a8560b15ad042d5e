// le_source.h -- internal descriptors of the fluid source / sink path (le_source.hip).
// Not part of the C-ABI (include/ibtk_le.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ibtk_le_ctx_s;

namespace ibtk_le {

// What le_source.hip needs of le_abi.cpp (see le_rod.h), and the context's flag word.
int abi_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void abi_ctx_device_stream(ibtk_le_ctx_s* ctx, int* device, hipStream_t* stream);
int* abi_ctx_flags(ibtk_le_ctx_s* ctx);

constexpr int SRC_RMAX = 16;               // largest source radius in cells the tables hold
constexpr int SRC_TAB = 2 * SRC_RMAX + 3;  // 1-D weights per (source, dimension): 2 (R + 1) + 1
constexpr int SRC_CHUNK = 64;              // sources staged in LDS at a time
constexpr int SRC_TILE3 = 8;               // edge of a spread tile, 3-D (512 lanes)
constexpr int SRC_TILE2 = 8;               // ... 2-D (64 lanes: the boxes are at most 35 cells wide)
constexpr int SRC_NPART = 1024;            // workgroups, and partial sums, of a field reduction
constexpr int SRC_FLAG = 32;               // the context flag an inconsistent source integral latches

// One source's stencil on the patch: the clipped box [lo, hi] (hi < lo in a dimension:
// empty) and the lower corner of the unclipped box, the origin of its weight tables.
struct SrcBox {
    int lo[3], hi[3], base[3];
    int pad;
};

// The cell-centred array of depth 1 and its patch.
struct SrcGrid {
    int ndim;
    int ilower[3], iupper[3];  // patch box
    int glo[3];                // ghost box lower
    int64_t s1, s2;            // strides of dims 1 and 2 (elements)
    double dx[3], xlo[3], xup[3];
};

struct SrcParams {
    SrcGrid g;
    int n_src;
    const double* r_src;  // device: radii
    SrcBox* box;          // workspace: n_src boxes
    double* w;            // workspace: [n_src][3][SRC_TAB] cos_kernel values
    double* part;         // workspace: 2 SRC_NPART partial sums / maxima
    double* scal;         // workspace: [0] the normalisation pressure
    int* flags;           // the context's flag word
};

// X_src[k][d] = sum_i X[node_i][d] / double(count_k), serially in list order
hipError_t launch_src_locations(int ndim, int n_src, const int* off, const int* nodes, const double* X, double* X_src,
                                hipStream_t s);
// the boxes and weight tables of every source at X_src
hipError_t launch_src_setup(const SrcParams& P, const double* X_src, hipStream_t s);
// nt: tiles per dimension a source's box can take; q(i) += Q_n wgt
hipError_t launch_src_spread(const SrcParams& P, const int nt[3], double* q, const double* Q, hipStream_t s);
// totals = {q_total, Q_sum, q_norm, integral_after}; vol = the boundary cells' volume
hipError_t launch_src_normalize(const SrcParams& P, double* q, const double* Q, const int dom_lo[3], const int dom_hi[3],
                                double vol, int normalize, double* totals, hipStream_t s);
// P_src[n] = sum p wgt - p_norm; use_norm: p_norm = (sum p dV over the boundary cells) / vol, else 0
hipError_t launch_src_pressure(const SrcParams& P, const double* p, double* P_src, int use_norm, const int dom_lo[3],
                               const int dom_hi[3], double vol, hipStream_t s);

}  // namespace ibtk_le
