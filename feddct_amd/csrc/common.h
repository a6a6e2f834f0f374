// common.h — internal helpers shared by the libfedagg.so translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fedagg.h"
#include "err.h"

#define FA_HIP_TRY(expr)                                                        \
  do {                                                                          \
    hipError_t e_ = (expr);                                                     \
    if (e_ != hipSuccess)                                                       \
      return fa::set_err(FA_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));    \
  } while (0)
