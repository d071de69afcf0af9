// Host helpers of the translation units that drive the device (train.cpp, encode.hip, decode.hip, pack.hip).
#ifndef MBPE_HIP_HOST_H
#define MBPE_HIP_HOST_H

#include "mbpe.h"
#include "../host/mbpe_host.h"

#include <hip/hip_runtime.h>

#include <string>

namespace mbpe {

inline std::string hip_err(const char *what, hipError_t e) { return std::string(what) + ": " + hipGetErrorString(e); }

// A failed HIP call ends the enclosing function: its text becomes the last error, out of memory MBPE_ERR_OOM, anything
// else MBPE_ERR_HIP.  clear_last: also reset the runtime's own last error, so that a later hipGetLastError() of this
// thread does not report the failure once more (the encoder does; the trainer and the decoder never did).
#define MBPE_HIP_CHECK(expr, clear_last)                                      \
    do {                                                                      \
        hipError_t e__ = (expr);                                              \
        if (e__ != hipSuccess) {                                              \
            mbpe_host::set_last_error(mbpe::hip_err(#expr, e__));             \
            if (clear_last) (void)hipGetLastError();                          \
            return e__ == hipErrorOutOfMemory ? MBPE_ERR_OOM : MBPE_ERR_HIP;  \
        }                                                                     \
    } while (0)

// a device buffer of at least want_bytes: kept when it is large enough, replaced (contents lost) otherwise.  Both
// policies are spelled at every call: clear_last as in MBPE_HIP_CHECK; n_allocs counts the hipMalloc calls, or NULL
template <typename T>
int grow(T **p, uint64_t *cap, uint64_t want_bytes, bool clear_last, uint64_t *n_allocs) {
    if (*p && *cap >= want_bytes) return MBPE_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    MBPE_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(p), want_bytes), clear_last);
    if (n_allocs) ++*n_allocs;
    *cap = want_bytes;
    return MBPE_OK;
}

// std::stoi on the remainder of a NUL-led chunk (reference Tokenizer.h:86-93): the value when it parses, i.e. when
// the chunk collapses to a single token
inline bool stoi_value(const uint8_t *s, uint64_t n, long long *out) {
    uint64_t i = 0;
    while (i < n && (s[i] == ' ' || (s[i] >= 9 && s[i] <= 13))) i++;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    if (i >= n || s[i] < '0' || s[i] > '9') return false;
    long long v = 0;
    while (i < n && s[i] >= '0' && s[i] <= '9') {
        v = v * 10 + (s[i] - '0');
        if (v > 4294967296LL) return false;
        i++;
    }
    if (neg) v = -v;
    if (v > 2147483647LL || v < -2147483648LL) return false;
    *out = v;
    return true;
}

}  // namespace mbpe

#endif
