// Device buffers of a training run are kept when the run ends and handed out again to the next one that asks for the
// same sizes (mbpe_train_begin twice on one corpus: no 25 GB of hipFree / hipMalloc in between).
#ifndef MBPE_DEV_POOL_H
#define MBPE_DEV_POOL_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <map>
#include <unordered_map>

namespace mbpe {

class DevPool {
public:
    // an idle buffer of exactly `bytes` (0 counts as 4), or a new one; out of memory: the idle ones go and it tries again
    template <typename T>
    hipError_t alloc(T **p, size_t bytes) {
        if (bytes == 0) bytes = 4;
        void *q = nullptr;
        auto it = idle_.find(bytes);
        if (it != idle_.end()) {
            q = it->second;
            idle_.erase(it);
        } else {
            hipError_t e = hipMalloc(&q, bytes);
            if (e == hipErrorOutOfMemory && !idle_.empty()) {
                trim();
                e = hipMalloc(&q, bytes);
            }
            if (e != hipSuccess) return e;
        }
        live_[q] = bytes;
        *p = static_cast<T *>(q);
        return hipSuccess;
    }
    // back to the idle list (a pointer the pool does not know is freed)
    template <typename T>
    void free(T *&p) {
        auto it = live_.find((void *)p);
        if (it != live_.end()) {
            idle_.emplace(it->second, it->first);
            live_.erase(it);
        } else if (p) {
            (void)hipFree((void *)p);
        }
        p = nullptr;
    }
    // a buffer that leaves the pool for good (freed right away)
    template <typename T>
    void release(T *p) {
        live_.erase((void *)p);
        if (p) (void)hipFree((void *)p);
    }
    // the idle buffers go back to the driver
    void trim() {
        for (auto &kv : idle_) (void)hipFree(kv.second);
        idle_.clear();
    }

private:
    std::unordered_map<void *, size_t> live_;
    std::multimap<size_t, void *> idle_;
};

}  // namespace mbpe

#endif
