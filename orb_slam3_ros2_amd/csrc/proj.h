// Projection-guided matching on the device (proj_kernels.hip) and SearchForInitialization (init_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbhip.h"

namespace orbhip {
struct ProjWorkspace;
// The rectified-stereo part of a search (a null pointer: the monocular search): mvuRight of the
// frame's keypoints, mbf, the direction of SearchByProjection(CurrentFrame, LastFrame, th, false)
// (1 forward, -1 backward, 0 neither) and SearchLocalPoints' mTrackProjXR output (or null).
struct ProjStereo {
    const float* u_right;
    float bf;
    int dir;
    float* proj_xr;
};
// dir of the pair (current Tcw, last Tlw) against the baseline b, in float as the reference
int proj_direction(const float cur_q[4], const float cur_t[3], const float last_q[4], const float last_t[3], float b);
ProjWorkspace* proj_ws_create();
void proj_ws_destroy(ProjWorkspace* w);
int proj_search_last(ProjWorkspace* ws, const orbhip_frame* F, const orbhip_proj_last* L, float th,
                     int check_orientation, int32_t* match, int* rounds_out, hipStream_t st,
                     const ProjStereo* sx = nullptr);
int proj_search_local(ProjWorkspace* ws, const orbhip_frame* F, const orbhip_local_points* M, float view_cos_limit,
                      float th, float nnratio, int far_points, float th_far, uint8_t* in_view, int32_t* level,
                      int32_t* match, int* rounds_out, hipStream_t st, const ProjStereo* sx = nullptr);
// test hooks (orbhip_test_proj_route, _proj_stats, _predict_scale_sweep)
int proj_test_route(int n, int nq, int max_octave, int32_t* out4);
int proj_test_stats(const ProjWorkspace* ws, int32_t* out4);
// (thr: level_thresholds(log_sf, n_levels) in device memory)
void launch_predict_scale_sweep(uint32_t lo_bits, uint32_t hi_bits, float log_sf, const float* thr, int n_levels,
                                const int8_t* ref, unsigned long long* mismatches, hipStream_t st);
// SearchForInitialization (init_kernels.hip), on the same workspace (proj_ws.h)
int init_search(ProjWorkspace* ws, const orbhip_init_frame* F1, const orbhip_init_frame* F2, float* prev_matched,
                int window_size, float nnratio, int check_orientation, int32_t* matches12, hipStream_t st);
// test hooks (orbhip_test_init_route: a call's envelope from its sizes, host only;
// orbhip_test_init_stats: the route of the last init_search on the workspace)
int init_test_route(int n1, int n2, int nq0, int nr0, int32_t* out4);
int init_test_stats(ProjWorkspace* ws, int32_t* out8, hipStream_t st);
}  // namespace orbhip
