// XPS_HIP_CHECK: a failed HIP call is a failed XPS_CHECK naming the call.
// Pulls in the HIP runtime, so only HIP translation units include it
// (hip_util.h stays loadable without HIP).
#pragma once

#include <hip/hip_runtime.h>

#include "base.h"

#define XPS_HIP_CHECK(cmd)                                                            \
  do {                                                                                \
    hipError_t e_ = (cmd);                                                            \
    XPS_CHECK(e_ == hipSuccess) << "HIP error: " << hipGetErrorString(e_) << " in " #cmd; \
  } while (0)
