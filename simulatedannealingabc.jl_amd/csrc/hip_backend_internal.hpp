// hip_backend_internal.hpp -- what the translation units of HipBackend (hip_backend*.hip) share.
#pragma once
#include "hip_backend.hpp"

#include <hip/hip_runtime.h>

#define HB_CHECK(expr, what)                       \
  do {                                             \
    const int rc_ = check((expr), (what));         \
    if (rc_) return rc_;                           \
  } while (0)

// launchers report hipGetLastError(), which is sticky: clear whatever an earlier, unrelated HIP call left
#define HB_LAUNCH(expr, what)                      \
  do {                                             \
    (void)hipGetLastError();                       \
    const int e_ = (expr);                         \
    launches_ += 1;                                \
    if (e_) return check((hipError_t)e_, (what));  \
  } while (0)
