// Host helpers of the translation units that drive the device (train.cpp, wide_run.cpp, encode.hip, decode.hip,
// pack.hip, split.hip).
#ifndef MBPE_HIP_HOST_H
#define MBPE_HIP_HOST_H

#include "mbpe.h"
#include "../host/mbpe_host.h"

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

namespace mbpe {

inline std::string hip_err(const char *what, hipError_t e) { return std::string(what) + ": " + hipGetErrorString(e); }

// the way an entry point gives up: the text becomes the last error, the code its result
inline int fail(int code, const std::string &msg) {
    mbpe_host::set_last_error(msg);
    return code;
}

inline int find_device(int device_id) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device_id < 0 || device_id >= n_dev)
        return fail(MBPE_ERR_NO_DEVICE, "no usable HIP device (the MI355X path has no CPU fallback)");
    return MBPE_OK;
}

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

// A kernel that leaves one scalar: a zeroed T on the device, enqueue(T *) puts the work on `stream`, the value comes
// back in *out once the stream has run.  The scalar is freed on every path.
template <typename T, typename Enqueue>
hipError_t read_scalar(hipStream_t stream, T *out, Enqueue enqueue) {
    T *d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(T));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d, 0, sizeof(T), stream);
    if (e == hipSuccess) { enqueue(d); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(T), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d);
    return e;
}

// What a handle decides once for all its device memory: clear_last as in MBPE_HIP_CHECK; n_allocs counts the
// hipMalloc calls that succeeded (mbpe_*_alloc_count)
struct DevAlloc {
    bool clear_last;
    uint64_t n_allocs = 0;
};

inline void dev_free(void *p) { (void)hipFree(p); }

// An owned device buffer.  cap is the byte count that was asked for, never rounded: callers divide it.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { dev_free(p_); }
    // at least want_bytes: kept when it is large enough, else freed first and then replaced (contents lost; null and
    // empty when that fails)
    int reserve(uint64_t want_bytes, DevAlloc &a) {
        T **p = &p_;                              // (the text of the check below is the text of its error)
        if (*p && cap_ >= want_bytes) return MBPE_OK;
        if (*p) dev_free(*p);
        *p = nullptr;
        cap_ = 0;
        MBPE_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(p), want_bytes), a.clear_last);
        ++a.n_allocs;
        cap_ = want_bytes;
        return MBPE_OK;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    uint64_t bytes() const { return cap_; }
    T *release() { T *p = p_; p_ = nullptr; cap_ = 0; return p; }
    void swap(DevBuf &o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    // reserve that keeps the first used_bytes: at least want_bytes, grown geometrically into a new buffer with a
    // device-to-device copy on `stream`, which is waited for before the old buffer goes
    int grow(uint64_t used_bytes, uint64_t want_bytes, DevAlloc &a, hipStream_t stream) {
        if (p_ && cap_ >= want_bytes) return MBPE_OK;
        DevBuf bigger;
        const int rc = bigger.reserve(want_bytes > 2 * cap_ ? want_bytes : 2 * cap_, a);
        if (rc != MBPE_OK) return rc;
        if (p_ && used_bytes) {
            MBPE_HIP_CHECK(hipMemcpyAsync(bigger.p_, p_, used_bytes, hipMemcpyDeviceToDevice, stream), a.clear_last);
            MBPE_HIP_CHECK(hipStreamSynchronize(stream), a.clear_last);
        }
        swap(bigger);
        return MBPE_OK;
    }

private:
    T *p_ = nullptr;
    uint64_t cap_ = 0;
};

// The device side every handle starts from: a non-blocking stream, two timing events, the allocation policy.  A
// handle derives from it, so its buffers go first, then the events, then the stream (hipSetDevice comes before).
struct DevQueue {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevAlloc mem;
    explicit DevQueue(bool clear_last) : mem{clear_last} {}
    ~DevQueue() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int open(int device_id) {
        device = device_id;
        MBPE_HIP_CHECK(hipSetDevice(device_id), mem.clear_last);
        MBPE_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), mem.clear_last);
        MBPE_HIP_CHECK(hipEventCreate(&ev0), mem.clear_last);
        MBPE_HIP_CHECK(hipEventCreate(&ev1), mem.clear_last);
        return MBPE_OK;
    }
    // what was enqueued between the events has run; its device time
    int wait(float *ms) {
        MBPE_HIP_CHECK(hipStreamSynchronize(stream), mem.clear_last);
        MBPE_HIP_CHECK(hipGetLastError(), mem.clear_last);
        MBPE_HIP_CHECK(hipEventElapsedTime(ms, ev0, ev1), mem.clear_last);
        return MBPE_OK;
    }
    int finish(float *ms) {                       // ev1 goes here, with nothing after it
        MBPE_HIP_CHECK(hipEventRecord(ev1, stream), mem.clear_last);
        return wait(ms);
    }
};

// The device side of a one-shot call: a stream, two events and the buffers it had to allocate, all released at its end
struct OneShot : DevQueue {
    OneShot() : DevQueue(true) {}
    std::vector<DevBuf<uint8_t>> bufs;
    // device memory for n bytes (at least one), filled from `host` when that is given
    int alloc(void **out, uint64_t n, const void *host) {
        *out = nullptr;
        bufs.emplace_back();
        const int rc = bufs.back().reserve(n ? n : 1, mem);
        if (rc != MBPE_OK) return rc;
        *out = bufs.back();
        if (host && n) MBPE_HIP_CHECK(hipMemcpyAsync(*out, host, n, hipMemcpyHostToDevice, stream), true);
        return MBPE_OK;
    }
};

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
