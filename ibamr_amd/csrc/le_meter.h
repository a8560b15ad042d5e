// le_meter.h -- internal descriptors of the flow meters and pressure gauges (le_meter.hip).
// Not part of the C-ABI (include/ibtk_le.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ibtk_le_ctx_s;

namespace ibtk_le {

// What le_meter.hip needs of le_abi.cpp (see le_source.h).
int abi_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void abi_ctx_device_stream(ibtk_le_ctx_s* ctx, int* device, hipStream_t* stream);
int* abi_ctx_flags(ibtk_le_ctx_s* ctx);

constexpr int MTR_BLOCK = 256;      // lanes of the update's workgroup: one workgroup per meter
constexpr int MTR_READ_BLOCK = 1024; // ... of the read's: the sort's stages and the terms go four times as wide
constexpr int MTR_MAX_WEB = 4096;   // most web patches of one meter, P_l * max_web_nodes: the sort's keys fill 32 KiB of LDS
constexpr int MTR_WEB_BITS = 12;    // a web patch's insertion index m nw + n fits in this many bits
constexpr int MTR_CHUNK = 1024;     // elements of a serial sum staged in LDS at a time (three streams of them)
constexpr int MTR_FLAG = 64;        // the context flag a web wider than max_web_nodes latches
constexpr int MTR_NW_BAD = -1;      // num_web_nodes of a meter whose r_max / h_finest no int holds
static_assert(MTR_MAX_WEB == 1 << MTR_WEB_BITS, "the sort key's low bits hold the insertion index");
static_assert(3 * MTR_CHUNK <= MTR_MAX_WEB && MTR_READ_BLOCK >= 3 * 64, "three waves stage their streams where the keys were");

// The patch: its box, the frames of the side arrays u[3] and of the cell array p.
struct MtrGrid {
    int ilower[3], iupper[3];
    int glo[3];                // ghost box lower
    int64_t us1[3], us2[3];    // strides of dims 1 and 2 of u[a] (elements)
    int64_t ps1, ps2;          // ... of p
    double dx[3], xlo[3];
};

// The domain frame IndexUtilities::getCellIndex works in, and the finest spacing.
struct MtrDomain {
    int lo[3], hi[3];
    double xlo[3], xup[3];
    double h_finest;
};

// The plan (device pointers).  Meter l has P_l = poff[l + 1] - poff[l] perimeter nodes, the
// local node of perimeter position n at node[poff[l] + n], and room for cap P_l web patches
// from web patch cap poff[l] on; patch (m, n) of a web of nw nodes a spoke is the
// (m nw + n)-th of them.
struct MtrPlan {
    int n_meters, cap;
    int64_t total;     // cap sum P: the web patches the workspace holds
    const int* poff;
    const int* node;
    double* X_per;     // [sum P][3]  X_perimeter, as of the last update
    double* X_cen;     // [n_meters][3]
    int* nw;           // [n_meters]  num_web_nodes (MTR_NW_BAD: not representable)
    int* cen_cell;     // [n_meters][4]  the centroid's cell, and whether it is counted
    double* X_web;     // [cap sum P][3]
    double* dA_web;    // [cap sum P][3]
    int* cell;         // [cap sum P][3]
    int* counted;      // [cap sum P]
    double* term;      // [3][cap sum P]  a meter's terms in the order of its sums
    int* flags;        // the context's flag word
};

hipError_t launch_meter_update(const MtrPlan& M, const MtrGrid& g, const MtrDomain& D, const double* X, hipStream_t s);
hipError_t launch_meter_read(const MtrPlan& M, const MtrGrid& g, const double* const u[3], const double* p, const double* U,
                             double* values, hipStream_t s);

}  // namespace ibtk_le
