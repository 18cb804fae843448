// gsr_host.h -- the one error path of libgsr_hip.so, included by every translation unit that defines a C entry point.
// A refusal is `return fail(code, "text", ...)`: the text goes into the calling thread's message buffer, which gsr_last_error()
// hands out, and the code comes back.  Buffer and fail() are defined once, in gsr_api.hip; nothing else writes to the buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/gsr.h"

namespace gsr {

constexpr size_t GSR_ERR_TEXT_BYTES = 512;   // the message buffer, per thread; longer texts are cut (no message comes near it)

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

}  // namespace gsr

#define HIP_TRY(expr, what)                                                                                   \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return gsr::fail(GSR_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(_e), (int)_e); \
    } while (0)
