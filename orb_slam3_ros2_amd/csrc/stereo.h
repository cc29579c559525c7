// Frame::ComputeStereoMatches on the device (stereo_kernels.hip, stereo.cpp): rectified stereo
// pairs whose frames the extractor has just processed. The kernels read the pyramids where the
// extraction left them (level 0: the caller's frames; levels >= 1: the workspace's pyramid block).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbhip.h"
#include "orbhip_plan.h"

namespace orbhip {

constexpr int kStereoMaxKp = 65535;   // right keypoints per frame: the search packs (distance << 16 | iR)

// P pairs: frame 2p is the left one, 2p + 1 the right one. Keypoints, descriptors and counts are
// laid out as orbhip_extract_batch_device writes 2P frames (frame f at f * cap); the outputs and
// the scratch have cap entries per pair (pair p at p * cap).
struct StereoArgs {
    const ExtractPlan* d_plan;   // level geometry and scale factors (device copy of the frame size's plan)
    const uint8_t* img;          // level 0
    int stride;
    int64_t fstride;
    const uint8_t* pyr;          // levels >= 1, frame f at pyr + f * pyr_bytes
    const orbhip_kp* kps;
    const uint8_t* desc;
    const int32_t* n;
    int cap, P;
    float bf, b;
    int center_patch;
    float *u_right, *depth;
    int32_t* status_out;         // nullable
    int32_t* n_stereo;
    int32_t *status, *sad;       // scratch
    int32_t* best_r;             // nullable (test hook)
};
void launch_stereo(const StereoArgs& a, hipStream_t st);
// k_stereo_median alone (test hook): reads n, status and sad, writes status, u_right, depth, n_stereo
void launch_stereo_median(const StereoArgs& a, hipStream_t st);

struct ExtractWorkspace;
int stereo_device(ExtractWorkspace* ws, const uint8_t* d_imgs, int P, int w, int h, int stride, int64_t fstride,
                  const orbhip_stereo_params& prm, orbhip_kp* d_kps, uint8_t* d_desc, int cap, int32_t* d_n,
                  int32_t* d_mono, float* d_u_right, float* d_depth, int32_t* d_status, int32_t* d_n_stereo,
                  hipStream_t st);
int stereo_host(ExtractWorkspace* ws, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                const orbhip_stereo_params& prm, orbhip_kp* kps_l, uint8_t* desc_l, int* n_l, orbhip_kp* kps_r,
                uint8_t* desc_r, int* n_r, int cap, float* u_right, float* depth, int32_t* status, int* n_stereo);
// test hook: caller-supplied keypoints on both sides, the pyramids by the extractor's pyramid stage
int stereo_test_match(ExtractWorkspace* ws, const uint8_t* left, const uint8_t* right, int w, int h,
                      const orbhip_stereo_params& prm, const orbhip_kp* kps_l, const uint8_t* desc_l, int n_l,
                      const orbhip_kp* kps_r, const uint8_t* desc_r, int n_r, float* u_right, float* depth,
                      int32_t* status, int32_t* best_r, int32_t* sad, int* n_stereo);
// test hook: k_stereo_median alone on one pair's n caller-supplied entries (status, u_right and depth
// in place; device arrays of its own, the null stream)
int stereo_test_median(int32_t* status, const int32_t* sad, float* u_right, float* depth, int n, int* n_stereo);

}  // namespace orbhip
