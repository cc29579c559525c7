// ORB extraction on the device (extract.cpp, beside extract_kernels.hip): the plans of a context,
// their device images and every scratch buffer of the extractor.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbhip.h"
#include "extract_plan.h"

namespace orbhip {
struct StageTimer;
class GraphCache;
struct ExtractWorkspace;
// prm, tab, timer and graphs are the owning context's and outlive the workspace; `st` is the
// context's stream (the host-image calls run on it)
ExtractWorkspace* extract_ws_create(int device, const orbhip_orb_params* prm, const OrbTables* tab, StageTimer* timer,
                                    GraphCache* graphs, hipStream_t st);
void extract_ws_destroy(ExtractWorkspace* ws);
// cone_tile: k_pyr_cone tile edge in last-level pixels (0: 10, the one-frame latency optimum);
// fast_nt: k_fast_cells threads per cell (0: by batch size; 128/256/512/1024)
void extract_set_hints(ExtractWorkspace* ws, int cone_tile, int fast_nt);
int extract_max_keypoints(ExtractWorkspace* ws, int w, int h);
int extract_batch(ExtractWorkspace* ws, const uint8_t* d_imgs, int B, int w, int h, int stride, int64_t fstride,
                  int lap0, int lap1, orbhip_kp* d_kps, uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono,
                  hipStream_t st);
int extract_host(ExtractWorkspace* ws, const uint8_t* img, int w, int h, int stride, int lap0, int lap1,
                 orbhip_kp* kps, uint8_t* desc32, int cap, int* n_out, int* mono_index);
// ---- for the stereo stage (stereo.cpp), which runs behind an extraction of the same call ----
// The plan of a frame size and the workspace's buffers as they are at the call (so: after the
// extraction). Frame f's pyramid levels >= 1 lie at d_pyr + f * plan->pyr_bytes + lv[l].pyr_off.
struct ExtractView {
    const ExtractPlan *plan, *d_plan;   // host / device copy
    int kp_cap;                         // orbhip_max_keypoints
    hipStream_t stream;                 // the context's
    const uint8_t* d_pyr;
    // the host-image path's frames (w x h, packed) and outputs (frame f at f * kp_cap)
    const uint8_t* d_in;
    orbhip_kp* d_kps;
    uint8_t* d_desc;
    int32_t *d_n, *d_err;
};
int extract_view(ExtractWorkspace* ws, int w, int h, ExtractView* v);
// stereo scratch of `entries` keypoints through the workspace's grow(); outputs: also the
// device-side outputs of a host call (best, u_right, depth, `pairs` n_stereo)
struct StereoScratch {
    int32_t *status, *sad, *best, *n_stereo;
    float *u_right, *depth;
};
int extract_stereo_scratch(ExtractWorkspace* ws, size_t entries, int pairs, bool outputs, StereoScratch* s);
// two host images as frames 0 and 1 of the host-image path with vLappingArea {0, 0} (the context's
// stream, no synchronisation); pyramid_only: upload and pyramid stage alone
int extract_host_pair(ExtractWorkspace* ws, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                      bool pyramid_only);
// test hooks (orbhip_test_extract_debug, _candidates, _cells)
int extract_test_debug(ExtractWorkspace* ws, const uint8_t* img, int w, int h, int lap0, int lap1, uint8_t* pyr,
                       uint32_t* cand, int32_t* cand_cnt, void* lvl, int32_t* lvl_cnt, int32_t* lvl_nlap,
                       int32_t* sizes);
int extract_test_candidates(ExtractWorkspace* ws, int w, int h, int frame, int64_t* n);
int extract_test_cells(ExtractWorkspace* ws, int w, int h, int32_t* out6, int cap);
}  // namespace orbhip
