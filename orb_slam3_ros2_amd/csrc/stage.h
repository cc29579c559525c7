// The staging block of a host call: one block of bytes laid out once, filled in a pinned host
// image, uploaded, read by the kernels at fixed offsets, and its tail read back (DESIGN.md
// "Staging block"). StageLayout is plain C++ (host-only code can include this file); the rest
// needs the HIP runtime.
#pragma once
#include <stddef.h>

namespace orbhip {

// Offsets of consecutive segments, each starting on a multiple of `align` (a power of two).
// take(0) takes no space and returns where the next segment would start.
struct StageLayout {
    size_t align, off = 0;
    explicit StageLayout(size_t alignment) : align(alignment) {}
    size_t take(size_t bytes) {
        off = (off + align - 1) & ~(align - 1);
        const size_t o = off;
        off += bytes;
        return o;
    }
    size_t total() { return take(0); }   // the aligned end
};

}  // namespace orbhip

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>

#include "../../include/orbhip.h"
#include "geom.h"

// `return ORBHIP_ERR_DEVICE` from the calling function, with a line on stderr, when a HIP call fails
#define ORBHIP_HIPOK(unit, x)                                                                      \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            std::fprintf(stderr, "orbhip%s: %s failed: %s (%s:%d)\n", unit, #x,                    \
                         hipGetErrorString(e_), __FILE__, __LINE__);                               \
            return ORBHIP_ERR_DEVICE;                                                              \
        }                                                                                          \
    } while (0)

namespace orbhip {

// Device block + pinned host image, grown on demand (never shrunk; freed before reallocating).
struct StageBlock {
    uint8_t* d = nullptr;    // device block
    uint8_t* h = nullptr;    // pinned image
    uint8_t* hd = nullptr;   // h as the device addresses it (kernels may write results there: no download)
    size_t dcap = 0, hcap = 0;
    const bool slack;        // grow the pinned side by a quarter more than asked
    explicit StageBlock(bool pinned_slack) : slack(pinned_slack) {}
    StageBlock(const StageBlock&) = delete;
    StageBlock& operator=(const StageBlock&) = delete;
    ~StageBlock();
    hipError_t ensure(size_t dev_bytes, size_t host_bytes);

    // copy-in to the pinned image
    void put(size_t o, const void* src, size_t bytes) {
        if (bytes) std::memcpy(h + o, src, bytes);
    }
    void put_or_zero(size_t o, const void* src, size_t bytes) {   // optional arrays
        if (src) put(o, src, bytes);
        else std::memset(h + o, 0, bytes);
    }
};

// Staged host inputs (pinned block h, its device alias hd) to device memory d by a shader copy
// (small blocks: no DMA-engine start-up); ORBHIP_PROJ_DMA=1 uses hipMemcpyAsync.
hipError_t upload_inputs(const void* hd, void* d, const void* h, size_t bytes, hipStream_t st);

// PredictScale's steps for a scale pyramid (geom.h predict_scale): n_levels floats, thr[k] = the
// smallest float ratio whose level ceil(log(ratio) / log_sf), clamped to [0, n_levels - 1], is >= k
// with the host's own log (a bisection over the float bit patterns: the level is monotone in the
// ratio), +inf where no ratio reaches k; thr[0] = 0, unused. Computed once per (log_sf, n_levels)
// and kept for the process; the pointer stays valid.
const float* level_thresholds(float log_sf, int n_levels);
// their first kStepArgs as a kernel argument (NaN from n_levels on)
LevelSteps level_steps(float log_sf, int n_levels);

// An orbhip_local_points in a block. The segments are taken in the order points, normals,
// min_dist, max_dist, desc, skip; put() copies the arrays in and returns them as the kernels see them.
struct DevPoints {
    int n;
    const float *pts, *nrm, *mind, *maxd;
    const uint8_t *desc, *skip;
};
struct PointsLayout {
    size_t pts, nrm, mind, maxd, desc, skip;
    PointsLayout(StageLayout& lay, size_t n)
        : pts(lay.take(n * 12)), nrm(lay.take(n * 12)), mind(lay.take(n * 4)), maxd(lay.take(n * 4)),
          desc(lay.take(n * 32)), skip(lay.take(n)) {}
    // M.skip == nullptr: a null device pointer, or (zero_skip) a segment of zeros
    DevPoints put(StageBlock& s, const orbhip_local_points& M, bool zero_skip) const {
        const size_t n = (size_t)M.n;
        s.put(pts, M.points, n * 12);
        s.put(nrm, M.normals, n * 12);
        s.put(mind, M.min_dist, n * 4);
        s.put(maxd, M.max_dist, n * 4);
        s.put(desc, M.desc, n * 32);
        const bool has_skip = M.skip || zero_skip;
        if (has_skip) s.put_or_zero(skip, M.skip, n);
        return {M.n, (const float*)(s.d + pts), (const float*)(s.d + nrm), (const float*)(s.d + mind),
                (const float*)(s.d + maxd), s.d + desc, has_skip ? s.d + skip : nullptr};
    }
};

// A keyframe's n keypoints and descriptors from element `base` of the segments at o_kps / o_desc
// (its claimed bytes go in by put / put_or_zero: their place and null rule differ per call)
inline void put_keyframe(StageBlock& s, size_t o_kps, size_t o_desc, size_t base, const orbhip_kp* kps,
                         const uint8_t* desc, size_t n) {
    s.put(o_kps + base * sizeof(orbhip_kp), kps, n * sizeof(orbhip_kp));
    s.put(o_desc + base * 32, desc, n * 32);
}

}  // namespace orbhip
#endif  // __HIPCC__
