// le_rod.h -- internal descriptors of the Kirchhoff rod path (le_rod.hip).
// Not part of the C-ABI (include/ibtk_le.h is).
#pragma once
#include <hip/hip_runtime.h>

struct ibtk_le_ctx_s;

namespace ibtk_le {

// What le_rod.hip needs of le_abi.cpp, whose context type and error string are private to
// it: the calling thread's last error (returns `code`), and a context's device and stream.
int abi_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void abi_ctx_device_stream(ibtk_le_ctx_s* ctx, int* device, hipStream_t* stream);

// One entry of the rod plan: the whole rod, node indices in [0, n).  The row's node is
// the rod's curr end when curr == node, else its next end.  88 bytes, no padding.
struct RodRec {
    int curr, next;
    double p[10];  // ds a1 a2 a3 b1 b2 b3 kappa1 kappa2 tau
};
static_assert(sizeof(RodRec) == 88, "the rod record has no padding");

struct RodGenParams {
    long n;                // nodes
    const long long* off;  // n + 1 row offsets
    const RodRec* rec;
    const double *X, *D;   // [n][3], [n][9]
    double *F, *N;         // [n][3] each
    int accumulate_F, accumulate_N;
};
hipError_t launch_rodgen(const RodGenParams& p, hipStream_t s);
// D_new[l] = R(e, |e| dt) D_cur[l] row by row, e = W0[l] (W1 NULL) or 0.5 (W0[l] + W1[l])
hipError_t launch_director_update(long n, double dt, const double* D_cur, const double* W0, const double* W1,
                                  double* D_new, hipStream_t s);

}  // namespace ibtk_le
