// Host-side plumbing shared by the twelve translation units of libdsp_frontend.so: the error string, HIP_TRY, the grid size,
// and (host_checks.h) the vocabulary of the argument checks.
#pragma once

#include <hip/hip_runtime.h>

#include "dsp_common.h"
#include "workspace.h"

// Sets the calling thread's error string (dsp_last_error) and returns `code`.  Defined in dsp_frontend.hip.
__attribute__((visibility("hidden"))) int dsp_fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return dsp_fail(DSP_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

#include "host_checks.h"

static inline int grid_for(int64_t work_items, int per_block) {
    int64_t blocks = (work_items + per_block - 1) / per_block;
    if (blocks < 1) blocks = 1;
    const int64_t cap = (int64_t)dsp_cu_count() * 8;  // CUs x 8 resident blocks; the kernels grid-stride beyond
    return (int)(blocks < cap ? blocks : cap);
}
