// hip_check.h -- how the host files of the library (device_api.hip, multi_gpu.hip) turn a failed HIP call into DSRT_ERR_HIP and a message.
// Host code only: no kernel file includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dsrt.h"
#include "../host/host_internal.hpp"

namespace dsrt {

static inline bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

}  // namespace dsrt

#define HIP_TRY(expr) do { if (!dsrt::hip_ok((expr), #expr)) return DSRT_ERR_HIP; } while (0)
