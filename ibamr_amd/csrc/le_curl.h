// le_curl.h -- internal descriptor of the side-centred curl (le_curl.hip).
// Not part of the C-ABI (include/ibtk_le.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ibtk_le {

// The workgroup's x-y tile and the longest z segment it marches (ibamr_amd.gib.CURL_TILE).
// A grid with few tiles is cut into shorter segments, down to CURL_MIN_SEG planes, so that
// a small box still spreads over the machine (curl_segment below).
constexpr int CURL_TX = 32, CURL_TY = 16, CURL_TZ = 32;
constexpr int CURL_MIN_SEG = 4;
constexpr int CURL_FILL_WGS = 2048;  // workgroups a launch aims for before segments grow to CURL_TZ

// w = alpha curl u (+ w) on one patch of side data.  Array a of u covers
// [ulo[d], uhi[a][d]] (the ghost box, + 1 along its own axis), element (x, y, z) at
// (x - ulo[0]) + (y - ulo[1]) us1[a] + (z - ulo[2]) us2[a]; w likewise from wlo.
struct CurlSide {
    const double* u[3];
    double* w[3];
    int ilo[3], ihi[3];  // the cell box
    int ulo[3], uhi[3][3];
    int wlo[3];
    int64_t us1[3], us2[3], ws1[3], ws2[3];
    double fac[3];  // 0.125 / dx[d]
    double alpha;
    int accumulate;
    int per[3];  // read dim d at the periodic image of the cell range
    int seg;     // planes per z segment
};

// planes per z segment for a box of nz planes and tiles x-y tiles
inline int curl_segment(long long tiles, int nz) {
    const long long want = (CURL_FILL_WGS + tiles - 1) / tiles;  // segments wanted
    long long seg = (nz + want - 1) / want;
    if (seg < CURL_MIN_SEG) seg = CURL_MIN_SEG;
    if (seg > CURL_TZ) seg = CURL_TZ;
    return (int)seg;
}

hipError_t launch_curl_side(CurlSide P, hipStream_t s);

}  // namespace ibtk_le
