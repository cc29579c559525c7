// A device array grown on demand (never shrunk; the old block is freed before the new one is
// allocated, its contents are not kept).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace orbhip {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
};

}  // namespace orbhip
