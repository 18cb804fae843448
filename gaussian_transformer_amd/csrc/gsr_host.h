// gsr_host.h -- the one error path of libgsr_hip.so, included by every translation unit that defines a C entry point.
// A refusal is `return fail(code, "text", ...)`: the text goes into the calling thread's message buffer, which gsr_last_error()
// hands out, and the code comes back.  Buffer and fail() are defined once, in gsr_api.hip; nothing else writes to the buffer.
// Also the host's one way from a runtime SH degree / flag to a kernel's template arguments (with_sh_degree, with_flag), for the
// launchers of preprocess.hip, pergauss_bwd.hip and pose_grad.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

#include "../../include/gsr.h"

namespace gsr {

constexpr size_t GSR_ERR_TEXT_BYTES = 512;   // the message buffer, per thread; longer texts are cut (no message comes near it)

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Runtime value -> template argument of a kernel: f is a generic lambda and gets std::integral_constant<int, d> (an SH degree; d
// outside 0..2 takes 3, the largest a kernel is instantiated for) or std::bool_constant<b>; `decltype(D)::value` is the constant.
template <class F>
inline void with_sh_degree(int d, F &&f) {
    switch (d) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 3>{}); break;
    }
}
template <class F>
inline void with_flag(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace gsr

#define HIP_TRY(expr, what)                                                                                   \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return gsr::fail(GSR_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(_e), (int)_e); \
    } while (0)
// a nested check that has left its text already: the caller returns the bare code
#define GSR_TRY(expr) do { const int32_t _rc = (expr); if (_rc != GSR_OK) return _rc; } while (0)
