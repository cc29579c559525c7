// The staging block's buffers and its shader upload (stage.h).
#include "stage.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace orbhip {

StageBlock::~StageBlock() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
}

hipError_t StageBlock::ensure(size_t dev_bytes, size_t host_bytes) {
    if (!d || dcap < dev_bytes) {
        if (d) (void)hipFree(d);
        d = nullptr;
        dcap = 0;
        if (hipError_t e = hipMalloc((void**)&d, std::max<size_t>(dev_bytes, 1))) return e;
        dcap = dev_bytes;
    }
    if (!h || hcap < host_bytes) {
        if (h) (void)hipHostFree(h);
        h = hd = nullptr;
        hcap = 0;
        const size_t cap = slack ? host_bytes + host_bytes / 4 : host_bytes;
        if (hipError_t e = hipHostMalloc((void**)&h, std::max<size_t>(cap, 1), hipHostMallocDefault)) return e;
        hcap = cap;
        if (hipError_t e = hipHostGetDevicePointer((void**)&hd, h, 0)) return e;
    }
    return hipSuccess;
}

namespace {
// The staged inputs to device memory by the shader: every lane reads two 16-byte pieces of the
// pinned staging block over the bus (~140 KB per search: a few us) instead of a DMA-engine copy,
// whose start-up and ~15 GB/s rate cost ~12 us per call (rocprofv3 memory-copy trace, r03).
// ORBHIP_PROJ_DMA=1 restores hipMemcpyAsync (A/B, read per call).
__global__ __launch_bounds__(256) void k_upload(const uint4* __restrict__ src, uint4* __restrict__ dst, int n16) {
    const int i = blockIdx.x * 512 + threadIdx.x;
    uint4 a{}, b{};
    if (i < n16) a = src[i];
    if (i + 256 < n16) b = src[i + 256];
    if (i < n16) dst[i] = a;
    if (i + 256 < n16) dst[i + 256] = b;
}
}  // namespace

hipError_t upload_inputs(const void* hd, void* d, const void* h, size_t bytes, hipStream_t st) {
    const char* e = std::getenv("ORBHIP_PROJ_DMA");
    if (e && e[0] == '1') return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st);
    const int n16 = (int)((bytes + 15) / 16);   // reads whole 16-byte pieces: the block's segments are 256-byte aligned
    if (n16 == 0) return hipSuccess;
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((n16 + 511) / 512)), dim3(256), 0, st, (const uint4*)hd, (uint4*)d,
                       n16);
    return hipGetLastError();
}

namespace {
// MapPoint::PredictScale on the host (clamped before the conversion: the same for every finite value)
int host_predict_scale(float ratio, float log_sf, int n_levels) {
    const float fl = std::ceil(std::log(ratio) / log_sf);
    return !(fl > 0.0f) ? 0 : (fl >= (float)n_levels ? n_levels - 1 : (int)fl);
}
float float_of_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
}  // namespace

const float* level_thresholds(float log_sf, int n_levels) {
    static std::mutex mu;
    static std::map<std::pair<uint32_t, int>, std::vector<float>> cache;
    uint32_t key;
    std::memcpy(&key, &log_sf, 4);
    const std::lock_guard<std::mutex> lock(mu);
    std::vector<float>& thr = cache[{key, n_levels}];
    if (thr.empty()) {
        thr.assign((size_t)std::max(n_levels, 1), 0.0f);
        const uint32_t inf = 0x7F800000u;   // the positive floats in bit order: 1 (the least subnormal) .. +inf
        for (int k = 1; k < n_levels; k++) {
            if (host_predict_scale(float_of_bits(inf), log_sf, n_levels) < k) {
                thr[k] = std::numeric_limits<float>::infinity();
                continue;
            }
            uint32_t lo = 1u, hi = inf;   // the least bit pattern whose level is >= k lies in [lo, hi]
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (host_predict_scale(float_of_bits(mid), log_sf, n_levels) >= k) hi = mid;
                else lo = mid + 1;
            }
            thr[k] = float_of_bits(lo);
        }
    }
    return thr.data();
}

LevelSteps level_steps(float log_sf, int n_levels) {
    const float* thr = level_thresholds(log_sf, n_levels);
    LevelSteps s;
    for (int k = 0; k < kStepArgs; k++) s.thr[k] = k < n_levels ? thr[k] : std::numeric_limits<float>::quiet_NaN();
    return s;
}

}  // namespace orbhip
