// liborbhip.so host side: the context and the C-ABI of include/orbhip.h. Every entry point checks
// its arguments, sets the context's device and forwards to the unit that owns the work (the
// extractor: extract.h; matcher, BoW, camera, triangulation, Fuse: orbhip_kernels.h; the camera
// front-end on top of this ABI: frontend.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/orbhip.h"
#include "extract.h"
#include "orbhip_ctx.h"
#include "orbhip_ba.h"
#include "pose_opt.h"
#include "sim3_opt.h"
#include "essential_graph.h"
#include "proj.h"
#include "kfdb.h"
#include "ba_chol_blocked.h"
#include "ba_chol_dag.h"
#include "ba_nd.h"
#include "orbhip_kernels.h"
#include "graph_cache.h"
#include "stage.h"
#include "stereo.h"

using namespace orbhip;

#define HIPOK(x) ORBHIP_HIPOK("", x)

struct orbhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    orbhip_orb_params prm{};
    OrbTables tab;   // ORBextractor ctor tables
    ExtractWorkspace* ext = nullptr;
    MatchWorkspace* match = nullptr;
    BowWorkspace* bow = nullptr;
    CameraWorkspace* cam = nullptr;
    BaWorkspace* ba = nullptr;
    PoseWorkspace* pose = nullptr;
    ProjWorkspace* proj = nullptr;
    StageBlock tri_stage{false};    // SearchForTriangulation's block (stage.h)
    StageBlock fuse_stage{false};   // Fuse's, Fuse with a Sim3's and the Sim3 projection search's
    StageBlock sim3_stage{false};   // Sim3Solver's
    StageBlock sim3_opt_stage{false};   // OptimizeSim3's
    StageBlock two_view_stage{false};   // TwoViewReconstruction's
    StageBlock eg_stage{false};     // OptimizeEssentialGraph's
    EgWorkspace* eg = nullptr;      // its dense system and solver buffers (created with the first call)
    StageTimer timer;
    GraphCache graphs;   // replays of repeated per-frame launch sequences (graph_cache.h)
};

hipStream_t ctx_stream(const orbhip_ctx* c) { return c->stream; }
void ctx_set_extract_hints(orbhip_ctx* c, int cone_tile, int fast_nt) { extract_set_hints(c->ext, cone_tile, fast_nt); }

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

int orbhip_abi_version(void) { return ORBHIP_ABI_VERSION; }

int orbhip_bgr_to_gray_device(orbhip_ctx* c, const uint8_t* d_bgr, int B, int w, int h, int src_stride,
                              int64_t src_fstride, uint8_t* d_gray, int dst_stride, int64_t dst_fstride, void* stream) {
    if (!c || !d_bgr || !d_gray || B < 0 || w <= 0 || h <= 0 || src_stride < 3 * w || dst_stride < w ||
        (B > 1 && (src_fstride < (int64_t)src_stride * h || dst_fstride < (int64_t)dst_stride * h)))
        return ORBHIP_ERR_ARG;
    if (B == 0) return ORBHIP_OK;
    HIPOK(hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t st = (hipStream_t)stream;   // NULL = the HIP null stream (HIP convention)
    launch_bgr2gray(d_bgr, B, w, h, src_stride, src_fstride, d_gray, dst_stride, dst_fstride, st);
    HIPOK(hipGetLastError());
    return ORBHIP_OK;
}

static bool valid_cam(const orbhip_pinhole* c) {
    return c && c->fx != 0.0f && c->fy != 0.0f && std::isfinite(c->fx) && std::isfinite(c->fy);
}

int orbhip_undistort_keypoints(orbhip_ctx* c, const orbhip_pinhole* cam, const orbhip_kp* kps, int n, orbhip_kp* out) {
    if (!c || !valid_cam(cam) || n < 0 || (n > 0 && (!kps || !out))) return ORBHIP_ERR_ARG;
    if (n == 0) return ORBHIP_OK;
    if (cam->k1 == 0.0f) {   // mvKeysUn = mvKeys
        if (out != kps) std::memmove(out, kps, sizeof(orbhip_kp) * (size_t)n);
        return ORBHIP_OK;
    }
    HIPOK(hipSetDevice(c->device));
    return undistort_kps_host(c->cam, *cam, kps, n, out, c->stream);
}

int orbhip_undistort_keypoints_device(orbhip_ctx* c, const orbhip_pinhole* cam, const orbhip_kp* d_kps,
                                      const int32_t* d_n, int B, int cap, orbhip_kp* d_out, void* stream) {
    if (!c || !valid_cam(cam) || B < 0 || cap < 0 || (B > 0 && (!d_kps || !d_n || !d_out))) return ORBHIP_ERR_ARG;
    if (B == 0 || cap == 0) return ORBHIP_OK;
    HIPOK(hipSetDevice(c->device));
    (void)hipGetLastError();
    launch_undistort_kps(d_kps, d_n, 0, B, cap, *cam, d_out, (hipStream_t)stream);   // k1 == 0: a copy
    HIPOK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_image_bounds(orbhip_ctx* c, const orbhip_pinhole* cam, int cols, int rows, float bounds[4]) {
    if (!c || !valid_cam(cam) || cols <= 0 || rows <= 0 || !bounds) return ORBHIP_ERR_ARG;
    if (cam->k1 == 0.0f) {
        bounds[0] = 0.0f; bounds[1] = (float)cols; bounds[2] = 0.0f; bounds[3] = (float)rows;
        return ORBHIP_OK;
    }
    HIPOK(hipSetDevice(c->device));
    return image_bounds_host(c->cam, *cam, cols, rows, bounds, c->stream);
}

int orbhip_create(orbhip_ctx** out, int device, const orbhip_orb_params* params) {
    if (!out) return ORBHIP_ERR_ARG;
    *out = nullptr;
    orbhip_orb_params p = {1000, 1.2f, 8, 20, 7};
    if (params) p = *params;
    if (p.n_features < 0 || p.n_levels < 1 || p.n_levels > kMaxLevels || !(p.scale_factor >= 1.0f))
        return ORBHIP_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ORBHIP_ERR_DEVICE;
    // device < 0: the calling thread's current HIP device (the rank's GPU after torch.cuda.set_device
    // / hipSetDevice in a one-process-per-GPU job)
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return ORBHIP_ERR_DEVICE;
    if (device < 0 || device >= ndev) return ORBHIP_ERR_DEVICE;
    std::unique_ptr<orbhip_ctx> c(new orbhip_ctx());
    c->device = device;
    c->prm = p;
    HIPOK(hipSetDevice(device));
    HIPOK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (!octree_set_lds_limit(160 * 1024)) return ORBHIP_ERR_DEVICE;
    c->tab = build_orb_tables(p);
    c->ext = extract_ws_create(device, &c->prm, &c->tab, &c->timer, &c->graphs, c->stream);
    c->match = match_ws_create();
    c->bow = bow_ws_create();
    c->cam = camera_ws_create();
    *out = c.release();
    return ORBHIP_OK;
}

int orbhip_destroy(orbhip_ctx* c) {
    if (!c) return ORBHIP_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->graphs.graphs()) (void)hipDeviceSynchronize();   // replays may run on caller streams
    c->graphs.clear();
    if (c->timer.created) {
        for (int i = 0; i < 2 * StageTimer::kCap; i++) (void)hipEventDestroy(c->timer.ev[i]);
        if (c->timer.dstamp) (void)hipFree(c->timer.dstamp);
    }
    ba_destroy(c->ba);
    if (c->stream) dag_stream_retired(c->stream);   // before the stream goes: no solve may wait on it
    pose_ws_destroy(c->pose);
    proj_ws_destroy(c->proj);
    eg_ws_destroy(c->eg);
    extract_ws_destroy(c->ext);
    match_ws_destroy(c->match);
    bow_ws_destroy(c->bow);
    camera_ws_destroy(c->cam);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return ORBHIP_OK;
}

int orbhip_level_info(orbhip_ctx* c, int w, int h, int32_t* lw, int32_t* lh, int32_t* nf, float* sc) {
    if (!c || w <= 0 || h <= 0) return ORBHIP_ERR_ARG;
    for (int l = 0; l < c->prm.n_levels; l++) {
        if (lw) lw[l] = round_even_f((float)w * c->tab.inv_scale[l]);
        if (lh) lh[l] = round_even_f((float)h * c->tab.inv_scale[l]);
        if (nf) nf[l] = c->tab.feat[l];
        if (sc) sc[l] = c->tab.scale[l];
    }
    return ORBHIP_OK;
}

int orbhip_max_keypoints(orbhip_ctx* c, int w, int h) {
    if (!c || w <= 0 || h <= 0) return ORBHIP_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return ORBHIP_ERR_DEVICE;
    return extract_max_keypoints(c->ext, w, h);
}

int orbhip_extract_batch_device(orbhip_ctx* c, const uint8_t* d_imgs, int B, int w, int h, int stride,
                                int64_t frame_stride, int lap0, int lap1, orbhip_kp* d_kps, uint8_t* d_desc, int cap,
                                int32_t* d_n, int32_t* d_mono, void* stream) {
    if (!c || !d_imgs || B <= 0 || w <= 0 || h <= 0 || stride < w || !d_kps || !d_desc || !d_n || !d_mono || cap <= 0)
        return ORBHIP_ERR_ARG;
    if (B > 1 && frame_stride < (int64_t)stride * h) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    // stream NULL = the HIP null stream (HIP convention), here and in the other *_device calls
    return extract_batch(c->ext, d_imgs, B, w, h, stride, frame_stride, lap0, lap1, d_kps, d_desc, cap, d_n, d_mono,
                         (hipStream_t)stream);
}

int orbhip_extract(orbhip_ctx* c, const uint8_t* img, int w, int h, int stride, int lap0, int lap1, orbhip_kp* kps,
                   uint8_t* desc32, int cap, int* n_out, int* mono_index) {
    if (!c || !n_out) return ORBHIP_ERR_ARG;
    *n_out = 0;
    if (mono_index) *mono_index = -1;
    if (!img || w <= 0 || h <= 0) return ORBHIP_ERR_EMPTY;   // operator(): _image.empty() -> -1
    if (stride < w || (cap > 0 && (!kps || !desc32))) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return extract_host(c->ext, img, w, h, stride, lap0, lap1, kps, desc32, cap, n_out, mono_index);
}

// ---- rectified stereo frames: both extractions and Frame::ComputeStereoMatches (stereo.cpp) ----
int orbhip_extract_stereo(orbhip_ctx* c, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                          const orbhip_stereo_params* params, orbhip_kp* kps_l, uint8_t* desc_l, int* n_l,
                          orbhip_kp* kps_r, uint8_t* desc_r, int* n_r, int cap, float* u_right, float* depth,
                          int32_t* status, int* n_stereo) {
    if (!c || !n_l || !n_r || !n_stereo || !params) return ORBHIP_ERR_ARG;
    *n_l = *n_r = *n_stereo = 0;
    if (!left || !right || w <= 0 || h <= 0) return ORBHIP_ERR_EMPTY;
    if (stride < w || !kps_l || !desc_l || !kps_r || !desc_r || !u_right || !depth) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return stereo_host(c->ext, left, right, w, h, stride, *params, kps_l, desc_l, n_l, kps_r, desc_r, n_r, cap,
                       u_right, depth, status, n_stereo);
}

int orbhip_extract_stereo_device(orbhip_ctx* c, const uint8_t* d_imgs, int P, int w, int h, int stride,
                                 int64_t frame_stride, const orbhip_stereo_params* params, orbhip_kp* d_kps,
                                 uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono, float* d_u_right,
                                 float* d_depth, int32_t* d_status, int32_t* d_n_stereo, void* stream) {
    if (!c || !params || P < 1 || !d_kps || !d_desc || !d_n || !d_mono || !d_u_right || !d_depth || !d_n_stereo)
        return ORBHIP_ERR_ARG;
    if (!d_imgs || w <= 0 || h <= 0) return ORBHIP_ERR_EMPTY;
    if (stride < w || frame_stride < (int64_t)stride * h) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return stereo_device(c->ext, d_imgs, P, w, h, stride, frame_stride, *params, d_kps, d_desc, cap, d_n, d_mono,
                         d_u_right, d_depth, d_status, d_n_stereo, (hipStream_t)stream);
}

int orbhip_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    if (!a || !b) return ORBHIP_ERR_ARG;
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

int orbhip_match_bf(orbhip_ctx* c, const uint8_t* q, const float* qa, int nq, const uint8_t* t, const float* ta,
                    int nt, int th_low, float ratio, int check_orientation, int32_t* match, int32_t* best_d,
                    int32_t* second_d) {
    if (!c || nq < 0 || nt < 0 || (nq > 0 && (!q || !qa || !match || !best_d || !second_d)) || (nt > 0 && (!t || !ta)))
        return ORBHIP_ERR_ARG;
    if (nq == 0) return 0;
    HIPOK(hipSetDevice(c->device));
    return match_bf_host(c->match, q, qa, nq, t, ta, nt, th_low, ratio, check_orientation, match, best_d, second_d,
                         c->stream);
}

int orbhip_match_pairs_device(orbhip_ctx* c, const orbhip_kp* d_kps, const uint8_t* d_desc, const int32_t* d_n, int B,
                              int cap, int th_low, float ratio, int check_orientation, int32_t* d_match,
                              int32_t* d_best, int32_t* d_second, int32_t* d_nmatch, void* stream) {
    if (!c || !d_kps || !d_desc || !d_n || B < 2 || cap <= 0 || !d_match || !d_best || !d_second || !d_nmatch)
        return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return match_pairs_device(c->match, c->graphs, c->timer, d_kps, d_desc, d_n, B, cap, th_low, ratio,
                              check_orientation, d_match, d_best, d_second, d_nmatch, (hipStream_t)stream);
}

int orbhip_match_frames_device(orbhip_ctx* c, const orbhip_kp* d_q_kps, const uint8_t* d_q_desc, const int32_t* d_nq,
                               const orbhip_kp* d_t_kps, const uint8_t* d_t_desc, const int32_t* d_nt, int cap,
                               int th_low, float ratio, int check_orientation, int32_t* d_match, int32_t* d_best,
                               int32_t* d_second, int32_t* d_nmatch, void* stream) {
    if (!c || !d_q_kps || !d_q_desc || !d_nq || !d_t_kps || !d_t_desc || !d_nt || cap <= 0 || !d_match || !d_best ||
        !d_second || !d_nmatch)
        return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return match_frames_device(c->match, c->graphs, c->timer, d_q_kps, d_q_desc, d_nq, d_t_kps, d_t_desc, d_nt, cap,
                               th_low, ratio, check_orientation, d_match, d_best, d_second, d_nmatch,
                               (hipStream_t)stream);
}

int orbhip_launch_graphs(orbhip_ctx* c) {
    if (!c) return ORBHIP_ERR_ARG;
    return c->graphs.graphs();
}

int orbhip_profile_stage(orbhip_ctx* c, int stage) {
    if (!c || stage < 0 || stage > 16 || stage == 12 || stage == 14) return ORBHIP_ERR_ARG;   // 12 and 14 are no stages: callers rely on their refusal
    HIPOK(hipSetDevice(c->device));
    StageTimer& t = c->timer;
    if (!t.created) {
        for (int i = 0; i < 2 * StageTimer::kCap; i++) HIPOK(hipEventCreate(&t.ev[i]));
        HIPOK(hipMalloc((void**)&t.dstamp, 2 * StageTimer::kCap * sizeof(unsigned long long)));
        t.created = true;
    }
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemset(t.dstamp, 0xFF, StageTimer::kCap * sizeof(unsigned long long)));   // minima: ~0
    HIPOK(hipMemset(t.dstamp + StageTimer::kCap, 0, StageTimer::kCap * sizeof(unsigned long long)));
    t.stage = stage;
    t.n = 0;
    return ORBHIP_OK;
}

int orbhip_profile_collect(orbhip_ctx* c, double* total_ms, int32_t* count) {
    if (!c || !total_ms || !count) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    StageTimer& t = c->timer;
    double s = 0;
    for (int i = 0; i < t.n; i++) {
        HIPOK(hipEventSynchronize(t.ev[2 * i + 1]));
        float ms = 0;
        HIPOK(hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]));
        s += ms;
    }
    // the pyramid's k_pyr_cone and k_octree also stamp their execution span from the device (first
    // workgroup start -> last workgroup end, as rocprofv3's kernel trace counts it): used when every
    // timed launch stamped (the k_resize cascade of batches does not)
    if ((t.stage == 1 || t.stage == 3) && t.n > 0 && t.dstamp) {
        std::vector<unsigned long long> h(2 * (size_t)t.n);
        HIPOK(hipMemcpy(h.data(), t.dstamp, t.n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(h.data() + t.n, t.dstamp + StageTimer::kCap, t.n * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
        int rate_khz = 0;
        HIPOK(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c->device));
        bool all = rate_khz > 0;
        double d = 0;
        for (int i = 0; i < t.n && all; i++) {
            all = h[t.n + i] != 0 && h[i] != ~0ull && h[t.n + i] >= h[i];
            d += (double)(h[t.n + i] - h[i]);
        }
        if (all) s = d / rate_khz;   // ticks / kHz = ms
        HIPOK(hipMemset(t.dstamp, 0xFF, t.n * sizeof(unsigned long long)));
        HIPOK(hipMemset(t.dstamp + StageTimer::kCap, 0, t.n * sizeof(unsigned long long)));
    }
    *total_ms = s;
    *count = t.n;
    t.n = 0;
    return ORBHIP_OK;
}

int orbhip_ba_solve(orbhip_ctx* c, const orbhip_ba_problem* prob, orbhip_ba_result* res, const volatile int* stop) {
    if (!c || !prob || !res) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->ba) c->ba = ba_create();
    if (!c->ba) return ORBHIP_ERR_DEVICE;
    return ba_solve(c->ba, prob, res, stop, c->stream);
}

int orbhip_ba_stats(orbhip_ctx* c, int64_t out[4]) {
    if (!c || !out) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    long long l = 0, h = 0, t = 0, r = 0;
    dag_device_stats(&l, &h);
    ba_stats(c->ba, &t, &r);
    out[0] = l; out[1] = h; out[2] = t; out[3] = r;
    return ORBHIP_OK;
}

int orbhip_ba_solve_batch(orbhip_ctx* c, const orbhip_ba_problem* probs, int B, orbhip_ba_result* res,
                          const volatile int* stop) {
    if (!c || !probs || !res || B <= 0) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->ba) c->ba = ba_create();
    if (!c->ba) return ORBHIP_ERR_DEVICE;
    std::vector<const orbhip_ba_problem*> pp(B);
    std::vector<orbhip_ba_result*> rr(B);
    for (int b = 0; b < B; b++) { pp[b] = probs + b; rr[b] = res + b; }
    return ba_solve_batch(c->ba, pp.data(), B, rr.data(), stop, c->stream, kShardNone);
}

int orbhip_ba_solve_stereo_batch(orbhip_ctx* c, const orbhip_ba_stereo_problem* probs, int B, orbhip_ba_result* res,
                                 const volatile int* stop) {
    if (!c || !probs || !res || B <= 0) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->ba) c->ba = ba_create();
    if (!c->ba) return ORBHIP_ERR_DEVICE;
    std::vector<const orbhip_ba_problem*> pp(B);
    std::vector<orbhip_ba_result*> rr(B);
    std::vector<BaStereoExt> sx(B);
    for (int b = 0; b < B; b++) {
        pp[b] = &probs[b].mono;
        rr[b] = res + b;
        sx[b] = BaStereoExt{probs[b].edge_ur, probs[b].bf, probs[b].huber_delta_stereo};
    }
    return ba_solve_batch(c->ba, pp.data(), B, rr.data(), stop, c->stream, kShardNone, false, false, sx.data());
}

int orbhip_ba_solve_stereo(orbhip_ctx* c, const orbhip_ba_stereo_problem* prob, orbhip_ba_result* res,
                           const volatile int* stop) {
    return orbhip_ba_solve_stereo_batch(c, prob, 1, res, stop);
}

int orbhip_pose_optimization_batch(orbhip_ctx* c, const orbhip_pose_problem* probs, int B,
                                   orbhip_pose_result* res) {
    if (!c || !probs || !res || B <= 0) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->pose) c->pose = pose_ws_create();
    if (!c->pose) return ORBHIP_ERR_DEVICE;
    return pose_opt_batch(c->pose, probs, B, res, c->stream);
}

int orbhip_pose_optimization(orbhip_ctx* c, const orbhip_pose_problem* prob, orbhip_pose_result* res) {
    const int rc = orbhip_pose_optimization_batch(c, prob, 1, res);
    return rc < 0 ? rc : res->n_inliers;
}

int orbhip_search_by_projection_last(orbhip_ctx* c, const orbhip_frame* cur, const orbhip_proj_last* last,
                                     float th, int check_orientation, int32_t* match) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->proj) c->proj = proj_ws_create();
    return proj_search_last(c->proj, cur, last, th, check_orientation, match, nullptr, c->stream);
}

int orbhip_search_local_points(orbhip_ctx* c, const orbhip_frame* frame, const orbhip_local_points* mps,
                               float view_cos_limit, float th, float nnratio, int far_points, float th_far,
                               uint8_t* in_view, int32_t* level, int32_t* match) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->proj) c->proj = proj_ws_create();
    return proj_search_local(c->proj, frame, mps, view_cos_limit, th, nnratio, far_points, th_far, in_view, level,
                             match, nullptr, c->stream);
}

int orbhip_pose_optimization_stereo_batch(orbhip_ctx* c, const orbhip_pose_stereo_problem* probs, int B,
                                          orbhip_pose_result* res) {
    if (!c || !probs || !res || B <= 0) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->pose) c->pose = pose_ws_create();
    if (!c->pose) return ORBHIP_ERR_DEVICE;
    return pose_opt_stereo_batch(c->pose, probs, B, res, c->stream);
}

int orbhip_pose_optimization_stereo(orbhip_ctx* c, const orbhip_pose_stereo_problem* prob, orbhip_pose_result* res) {
    const int rc = orbhip_pose_optimization_stereo_batch(c, prob, 1, res);
    return rc < 0 ? rc : res->n_inliers;
}

int orbhip_search_by_projection_last_stereo(orbhip_ctx* c, const orbhip_stereo_view* cur, const orbhip_proj_last* last,
                                            const float last_pose_q[4], const float last_pose_t[3], float th,
                                            int check_orientation, int32_t* match, int32_t* direction) {
    if (!c || !cur || !last_pose_q || !last_pose_t || (cur->frame.n > 0 && !cur->u_right) || !(cur->bf > 0.0f) ||
        !(cur->b > 0.0f))
        return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->proj) c->proj = proj_ws_create();
    const ProjStereo sx{cur->u_right, cur->bf,
                        proj_direction(cur->frame.pose_q, cur->frame.pose_t, last_pose_q, last_pose_t, cur->b), nullptr};
    const int rc = proj_search_last(c->proj, &cur->frame, last, th, check_orientation, match, nullptr, c->stream, &sx);
    if (rc >= 0 && direction) *direction = sx.dir;
    return rc;
}

int orbhip_search_local_points_stereo(orbhip_ctx* c, const orbhip_stereo_view* frame, const orbhip_local_points* mps,
                                      float view_cos_limit, float th, float nnratio, int far_points, float th_far,
                                      uint8_t* in_view, int32_t* level, float* proj_xr, int32_t* match) {
    if (!c || !frame || (frame->frame.n > 0 && !frame->u_right) || !(frame->bf > 0.0f) || !(frame->b > 0.0f))
        return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->proj) c->proj = proj_ws_create();
    const ProjStereo sx{frame->u_right, frame->bf, 0, proj_xr};
    return proj_search_local(c->proj, &frame->frame, mps, view_cos_limit, th, nnratio, far_points, th_far, in_view,
                             level, match, nullptr, c->stream, &sx);
}

int orbhip_search_for_initialization(orbhip_ctx* c, const orbhip_init_frame* f1, const orbhip_init_frame* f2,
                                     float* prev_matched, int window_size, float nnratio, int check_orientation,
                                     int32_t* matches12) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->proj) c->proj = proj_ws_create();
    return init_search(c->proj, f1, f2, prev_matched, window_size, nnratio, check_orientation, matches12, c->stream);
}

struct orbhip_kfdb {
    orbhip::KfDb* d = nullptr;
    int device = 0;
};

int orbhip_kfdb_create(orbhip_ctx* c, int max_kf, orbhip_kfdb** out) {
    if (!c || !out) return ORBHIP_ERR_ARG;
    *out = nullptr;
    HIPOK(hipSetDevice(c->device));
    int rc = ORBHIP_OK;
    KfDb* d = kfdb_create(max_kf, c->stream, &rc);
    if (!d) return rc;
    *out = new orbhip_kfdb{d, c->device};
    return ORBHIP_OK;
}

int orbhip_kfdb_destroy(orbhip_kfdb* db) {
    if (!db) return ORBHIP_ERR_ARG;
    (void)hipSetDevice(db->device);
    kfdb_destroy(db->d);
    delete db;
    return ORBHIP_OK;
}

int orbhip_kfdb_add(orbhip_kfdb* db, int kf, const int32_t* words, const double* values, int n) {
    if (!db) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(db->device));
    return kfdb_add(db->d, kf, words, values, n);
}

int orbhip_kfdb_erase(orbhip_kfdb* db, int kf) {
    if (!db) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(db->device));
    return kfdb_erase(db->d, kf);
}

int orbhip_kfdb_detect_relocalization(orbhip_kfdb* db, const orbhip_kfdb_query* q, int32_t* out, int cap) {
    if (!db) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(db->device));
    return kfdb_detect_relocalization(db->d, q, out, cap);
}

int orbhip_kfdb_detect_nbest(orbhip_kfdb* db, const orbhip_kfdb_query* q, const uint8_t* connected, int n,
                             int32_t* loop_out, int32_t* n_loop, int32_t* merge_out, int32_t* n_merge) {
    if (!db) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(db->device));
    return kfdb_detect_nbest(db->d, q, connected, n, loop_out, n_loop, merge_out, n_merge);
}

int orbhip_comm_unique_id(uint8_t* id) {
    if (!id) return ORBHIP_ERR_ARG;
    return ba_comm_unique_id(id);
}

int orbhip_comm_init(orbhip_ctx* c, int nranks, int rank, const uint8_t* id) {
    if (!c || !id) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->ba) c->ba = ba_create();
    if (!c->ba) return ORBHIP_ERR_DEVICE;
    return ba_comm_init(c->ba, nranks, rank, id);
}

int orbhip_ba_solve_sharded(orbhip_ctx* c, const orbhip_ba_problem* shard, orbhip_ba_result* res,
                            const volatile int* stop) {
    if (!c || !shard || !res || !c->ba) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    const orbhip_ba_problem* pp[1] = {shard};
    orbhip_ba_result* rr[1] = {res};
    return ba_solve_batch(c->ba, pp, 1, rr, stop, c->stream, kShardRccl);
}

int orbhip_ba_solve_sharded_segments(orbhip_ctx* c, const orbhip_ba_problem* shards, int nlocal, orbhip_ba_result* res,
                                     const volatile int* stop) {
    if (!c || !shards || !res || nlocal <= 0 || !c->ba) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    std::vector<const orbhip_ba_problem*> pp(nlocal);
    std::vector<orbhip_ba_result*> rr(nlocal);
    for (int b = 0; b < nlocal; b++) { pp[b] = shards + b; rr[b] = res + b; }
    return ba_solve_batch(c->ba, pp.data(), nlocal, rr.data(), stop, c->stream, kShardRccl);
}

int orbhip_ba_solve_shards_local(orbhip_ctx* c, const orbhip_ba_problem* shards, int nshards, orbhip_ba_result* res,
                                 const volatile int* stop) {
    if (!c || !shards || !res || nshards <= 0) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->ba) c->ba = ba_create();
    if (!c->ba) return ORBHIP_ERR_DEVICE;
    std::vector<const orbhip_ba_problem*> pp(nshards);
    std::vector<orbhip_ba_result*> rr(nshards);
    for (int b = 0; b < nshards; b++) { pp[b] = shards + b; rr[b] = res + b; }
    return ba_solve_batch(c->ba, pp.data(), nshards, rr.data(), stop, c->stream, kShardLocal);
}

// ---- bag of words (a13/a14) ----
int orbhip_vocab_create(orbhip_ctx* c, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                        const uint8_t* is_leaf, const uint8_t* desc32, const double* weight, orbhip_vocab** out) {
    if (!c) return ORBHIP_ERR_ARG;
    return vocab_build(c->device, k, L, scoring, weighting, n_nodes, parent, is_leaf, desc32, weight, out);
}

int orbhip_vocab_load_text(orbhip_ctx* c, const char* path, orbhip_vocab** out) {
    if (!c || !path || !out) return ORBHIP_ERR_ARG;
    return vocab_load_text(c->device, path, out);
}

int orbhip_vocab_destroy(orbhip_vocab* v) { return vocab_destroy(v); }

int orbhip_vocab_info(const orbhip_vocab* v, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words) {
    return vocab_info(v, k, L, n_nodes, n_words);
}

int orbhip_bow_transform(orbhip_ctx* c, const orbhip_vocab* v, const uint8_t* desc, int n, int levelsup,
                         int32_t* word, int32_t* node, double* weight) {
    if (!c || !v || n < 0 || (n && (!desc || !word || !node || !weight))) return ORBHIP_ERR_ARG;
    if (n == 0) return ORBHIP_OK;
    HIPOK(hipSetDevice(c->device));
    return bow_transform_host(c->bow, v, desc, n, levelsup, word, node, weight, c->stream);
}

int orbhip_bow_transform_device(orbhip_ctx* c, const orbhip_vocab* v, const uint8_t* d_desc, const int32_t* d_n,
                                int B, int cap, int levelsup, int32_t* d_word, int32_t* d_node, double* d_weight,
                                void* stream) {
    if (!c || !v || !d_desc || !d_n || B <= 0 || cap <= 0 || !d_word || !d_node || !d_weight) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return bow_transform_device(v, d_desc, d_n, B, cap, levelsup, d_word, d_node, d_weight, (hipStream_t)stream);
}

int orbhip_search_bow(orbhip_ctx* c, const uint8_t* kf_desc, const float* kf_angle, const int32_t* kf_node,
                      const double* kf_weight, const uint8_t* kf_valid, int nkf, const uint8_t* f_desc,
                      const float* f_angle, const int32_t* f_node, const double* f_weight, int nf, float ratio,
                      int check_orientation, int th_low, int32_t* match) {
    if (!c || nkf < 0 || nf < 0 || (nf && !match)) return ORBHIP_ERR_ARG;
    if (nkf > kBowMax || nf > kBowMax) return ORBHIP_ERR_UNSUPPORTED;
    if (nf == 0) return 0;
    for (int i = 0; i < nf; i++) match[i] = -1;
    if (nkf == 0) return 0;
    if (!kf_desc || !kf_angle || !kf_node || !kf_weight || !kf_valid || !f_desc || !f_angle || !f_node || !f_weight)
        return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return search_bow_host(c->bow, kf_desc, kf_angle, kf_node, kf_weight, kf_valid, nkf, f_desc, f_angle, f_node,
                           f_weight, nf, ratio, check_orientation, th_low, match, c->stream);
}

// ---- SearchForTriangulation: KF1 against B neighbours ----
int orbhip_triangulation_geometry(const orbhip_tri_keyframe* kf1, const orbhip_tri_keyframe* kf2, float F12[9],
                                  float ep[2]) {
    if (!kf1 || !kf2 || !F12 || !ep) return ORBHIP_ERR_ARG;
    tri_geometry(*kf1, *kf2, F12, ep);
    return ORBHIP_OK;
}

int orbhip_search_for_triangulation(orbhip_ctx* c, const orbhip_tri_keyframe* kf1, const orbhip_tri_keyframe* nbrs,
                                    int B, const float* scale_factors, const float* level_sigma2, int n_levels,
                                    int check_orientation, int32_t* match12, int32_t* nmatches) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return tri_search(c->tri_stage, c->timer, c->stream, kf1, nbrs, B, scale_factors, level_sigma2, n_levels,
                      check_orientation, match12, nmatches);
}

// ---- CreateNewMapPoints: the search and the triangulation of its matches, or the latter alone ----
int orbhip_create_new_map_points(orbhip_ctx* c, const orbhip_tri_keyframe* kf1, const orbhip_tri_keyframe* nbrs, int B,
                                 const float* median_depth, const float* scale_factors, const float* level_sigma2,
                                 int n_levels, int check_orientation, const orbhip_tri_params* params,
                                 orbhip_new_points* out) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return tri_new_points(c->tri_stage, c->timer, c->stream, kf1, nbrs, B, nullptr, median_depth, scale_factors,
                          level_sigma2, n_levels, check_orientation, params, out);
}

int orbhip_triangulate_matches(orbhip_ctx* c, const orbhip_tri_keyframe* kf1, const orbhip_tri_keyframe* nbrs, int B,
                               const int32_t* match12_in, const float* scale_factors, const float* level_sigma2,
                               int n_levels, const orbhip_tri_params* params, orbhip_new_points* out) {
    if (!c || !match12_in) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return tri_new_points(c->tri_stage, c->timer, c->stream, kf1, nbrs, B, match12_in, nullptr, scale_factors,
                          level_sigma2, n_levels, 0, params, out);
}

// ---- the same three calls on rectified-stereo keyframes ----
// The stereo keyframes of a call taken apart (entry 0: KF1): the argument checks of the stereo part,
// before anything is uploaded. B outside [0, kTriMaxPairs] or null pointers are the inner call's to
// refuse (count = 0 then).
struct TriStereoCall {
    orbhip_tri_keyframe kf[1 + kTriMaxPairs];
    const float* ur[1 + kTriMaxPairs];
    const float* depth[1 + kTriMaxPairs];
    float bf[1 + kTriMaxPairs], b[1 + kTriMaxPairs];
    TriStereo sx{ur, depth, bf, b};
    int count = 0;
    int take(const orbhip_tri_stereo_keyframe* kf1, const orbhip_tri_stereo_keyframe* nbrs, int B) {
        if (!kf1) return ORBHIP_OK;
        const int nb = (B > 0 && B <= kTriMaxPairs && nbrs) ? B : 0;
        for (int s = 0; s <= nb; s++) {
            const orbhip_tri_stereo_keyframe& k = s ? nbrs[s - 1] : *kf1;
            if ((k.kf.n > 0 && (!k.u_right || !k.depth)) || !(k.bf > 0.0f) || !(k.b > 0.0f)) return ORBHIP_ERR_ARG;
            kf[s] = k.kf; ur[s] = k.u_right; depth[s] = k.depth; bf[s] = k.bf; b[s] = k.b;
        }
        count = 1 + nb;
        return ORBHIP_OK;
    }
    const orbhip_tri_keyframe* kf1() const { return count ? &kf[0] : nullptr; }
    const orbhip_tri_keyframe* nbrs() const { return count > 1 ? &kf[1] : nullptr; }
    const TriStereo* stereo() const { return count ? &sx : nullptr; }
};

int orbhip_search_for_triangulation_stereo(orbhip_ctx* c, const orbhip_tri_stereo_keyframe* kf1,
                                           const orbhip_tri_stereo_keyframe* nbrs, int B, const float* scale_factors,
                                           const float* level_sigma2, int n_levels, int check_orientation,
                                           int32_t* match12, int32_t* nmatches) {
    if (!c) return ORBHIP_ERR_ARG;
    TriStereoCall t;
    if (const int rc = t.take(kf1, nbrs, B)) return rc;
    HIPOK(hipSetDevice(c->device));
    return tri_search(c->tri_stage, c->timer, c->stream, t.kf1(), t.nbrs(), B, scale_factors, level_sigma2, n_levels,
                      check_orientation, match12, nmatches, t.stereo());
}

int orbhip_create_new_map_points_stereo(orbhip_ctx* c, const orbhip_tri_stereo_keyframe* kf1,
                                        const orbhip_tri_stereo_keyframe* nbrs, int B, const float* scale_factors,
                                        const float* level_sigma2, int n_levels, int check_orientation,
                                        const orbhip_tri_params* params, orbhip_new_points* out, uint8_t* source) {
    if (!c) return ORBHIP_ERR_ARG;
    TriStereoCall t;
    if (const int rc = t.take(kf1, nbrs, B)) return rc;
    HIPOK(hipSetDevice(c->device));
    return tri_new_points(c->tri_stage, c->timer, c->stream, t.kf1(), t.nbrs(), B, nullptr, nullptr, scale_factors,
                          level_sigma2, n_levels, check_orientation, params, out, t.stereo(), source);
}

int orbhip_triangulate_matches_stereo(orbhip_ctx* c, const orbhip_tri_stereo_keyframe* kf1,
                                      const orbhip_tri_stereo_keyframe* nbrs, int B, const int32_t* match12_in,
                                      const float* scale_factors, const float* level_sigma2, int n_levels,
                                      const orbhip_tri_params* params, orbhip_new_points* out, uint8_t* source) {
    if (!c || !match12_in) return ORBHIP_ERR_ARG;
    TriStereoCall t;
    if (const int rc = t.take(kf1, nbrs, B)) return rc;
    HIPOK(hipSetDevice(c->device));
    return tri_new_points(c->tri_stage, c->timer, c->stream, t.kf1(), t.nbrs(), B, match12_in, nullptr, scale_factors,
                          level_sigma2, n_levels, 0, params, out, t.stereo(), source);
}

// ---- Fuse: B keyframes against one list of MapPoints ----
int orbhip_fuse(orbhip_ctx* c, const orbhip_frame* kfs, int B, const orbhip_local_points* mps,
                const uint8_t* pair_skip, const float* inv_level_sigma2, float th, int32_t* best_idx,
                int32_t* best_dist, int32_t* level, int32_t* nfused) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return fuse_search(c->fuse_stage, c->timer, c->stream, kfs, B, mps, pair_skip, true, inv_level_sigma2, th,
                       best_idx, best_dist, level, nfused);
}

// Fuse on rectified-stereo keyframes. The argument checks of the stereo part come first (nothing is
// uploaded before them); B outside (0, kFuseMaxKf] or a null kfs is fuse_search's to refuse.
int orbhip_fuse_stereo(orbhip_ctx* c, const orbhip_stereo_view* kfs, int B, const orbhip_local_points* mps,
                       const uint8_t* pair_skip, const float* inv_level_sigma2, float th, int32_t* best_idx,
                       int32_t* best_dist, int32_t* level, int32_t* nfused) {
    if (!c) return ORBHIP_ERR_ARG;
    const int nb = (kfs && B > 0 && B <= kFuseMaxKf) ? B : 0;
    orbhip_frame frames[kFuseMaxKf];   // the views taken apart, on the stack: no allocation per call
    const float* ur[kFuseMaxKf];
    float bf[kFuseMaxKf];
    for (int b = 0; b < nb; b++) {
        const orbhip_stereo_view& v = kfs[b];
        if ((v.frame.n > 0 && !v.u_right) || !(v.bf > 0.0f) || !(v.b > 0.0f)) return ORBHIP_ERR_ARG;
        frames[b] = v.frame;
        ur[b] = v.u_right;
        bf[b] = v.bf;
    }
    HIPOK(hipSetDevice(c->device));
    const FuseStereo sx{ur, bf};
    return fuse_search(c->fuse_stage, c->timer, c->stream, nb ? frames : nullptr, B, mps, pair_skip, true,
                       inv_level_sigma2, th, best_idx, best_dist, level, nfused, nb ? &sx : nullptr);
}

// ---- LoopClosing: Fuse and SearchByProjection with a Sim3 (the pose arrives as Tcw = (R, t / s)) ----
int orbhip_fuse_sim3(orbhip_ctx* c, const orbhip_frame* kfs, int B, const orbhip_local_points* mps,
                     const uint8_t* pair_skip, float th, int32_t* best_idx, int32_t* best_dist, int32_t* level,
                     int32_t* nfused) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return fuse_search(c->fuse_stage, c->timer, c->stream, kfs, B, mps, pair_skip, false, nullptr, th, best_idx,
                       best_dist, level, nfused);
}

int orbhip_search_by_projection_sim3(orbhip_ctx* c, const orbhip_frame* kf, const orbhip_local_points* mps, float th,
                                     float ratio_hamming, int32_t* match, int32_t* match_dist, int32_t* level) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return sim3_search(c->fuse_stage, c->timer, c->stream, kf, mps, th, ratio_hamming, match, match_dist, level);
}

// ---- LoopClosing: Sim3Solver, every hypothesis of every candidate ----
int orbhip_sim3_solve_batch(orbhip_ctx* c, const orbhip_sim3_problem* probs, int B, orbhip_sim3_result* res) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return sim3_solve_batch(c->sim3_stage, c->timer, c->stream, probs, B, res);
}

int orbhip_sim3_solve(orbhip_ctx* c, const orbhip_sim3_problem* prob, orbhip_sim3_result* res) {
    if (!prob || !res) return ORBHIP_ERR_ARG;
    return orbhip_sim3_solve_batch(c, prob, 1, res);
}

// ---- Tracking: TwoViewReconstruction, every frame pair of a call ----
int orbhip_two_view_reconstruct_batch(orbhip_ctx* c, const orbhip_two_view_problem* probs, int B,
                                      orbhip_two_view_result* res) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return two_view_batch(c->two_view_stage, c->timer, c->stream, probs, B, res);
}

int orbhip_two_view_reconstruct(orbhip_ctx* c, const orbhip_two_view_problem* prob, orbhip_two_view_result* res) {
    if (!prob || !res) return ORBHIP_ERR_ARG;
    return orbhip_two_view_reconstruct_batch(c, prob, 1, res);
}

// ---- LoopClosing: OptimizeSim3, every candidate's refinement in one launch ----
int orbhip_optimize_sim3_batch(orbhip_ctx* c, const orbhip_sim3_opt_problem* probs, int B,
                               orbhip_sim3_opt_result* res) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return sim3_opt_batch(c->sim3_opt_stage, c->timer, c->stream, probs, B, res);
}

// ---- LoopClosing: OptimizeEssentialGraph ----
int orbhip_optimize_essential_graph(orbhip_ctx* c, const orbhip_essential_graph_problem* prob,
                                    orbhip_essential_graph_result* res) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->eg) c->eg = eg_ws_create();
    return eg_optimize(c->eg, c->eg_stage, c->timer, c->stream, prob, res);
}

int orbhip_optimize_sim3(orbhip_ctx* c, const orbhip_sim3_opt_problem* prob, orbhip_sim3_opt_result* res) {
    if (!prob || !res) return ORBHIP_ERR_ARG;
    const int rc = orbhip_optimize_sim3_batch(c, prob, 1, res);
    return rc < 0 ? rc : res->n_in;
}

// the stored list capacity of the Sim3 projection search; the resolve has no round cap other than
// (points with a list) + 1 (tests assert that their chain is deeper than the capacity)
int orbhip_test_sim3_list_cap(void) { return kSim3ListCap; }

// host only: OptimizeEssentialGraph's argument check, and for a problem it accepts the size of its
// system, the solver route (0 dag, 1 blocked) and the number of blocks of H's lower triangle
int orbhip_test_essential_graph_check(const orbhip_essential_graph_problem* prob,
                                      const orbhip_essential_graph_result* res, int32_t* out3) {
    const int rc = eg_check(prob, res);
    if (rc || !out3) return rc;
    EgStructure s;
    eg_structure(prob, s);
    const char* env = std::getenv("ORBHIP_EG_BLOCKED");
    out3[0] = s.n;
    out3[1] = ((env && env[0] == '1') || s.n < kEgDagMinN) ? 1 : 0;
    out3[2] = (int32_t)s.blocks.size();
    return ORBHIP_OK;
}

// ---- test hooks (not part of the reference surface) ----
int orbhip_test_cholesky(const double* A, const double* b, double* x, int n, unsigned long long* phases5,
                         float* ms) {
    if (!A || !b || !x || !phases5 || !ms || n <= 0 || n > 480) return ORBHIP_ERR_ARG;
    return ba_test_cholesky(A, b, x, n, phases5, ms);
}
int orbhip_test_cholesky_reg(const double* A, const double* b, double* x, int n, int reps, float* ms,
                             unsigned long long* phases5) {
    if (!A || !b || !x || !ms) return ORBHIP_ERR_ARG;
    return ba_test_cholesky_reg(A, b, x, n, reps, ms, phases5);
}
int orbhip_test_cholesky_blocked(const double* A, const double* b, double* x, int n, float* ms) {
    if (!A || !b || !x || n <= 0 || !ms) return ORBHIP_ERR_ARG;
    return chol_blocked_test(A, b, x, n, ms);
}
int orbhip_test_cholesky_dag(const double* A, const double* b, double* x, int n, int reps, int max_helpers, float* ms,
                             unsigned long long* dbg) {
    if (!A || !b || !x || n <= 0 || reps < 1) return ORBHIP_ERR_ARG;
    return chol_dag_test(A, b, x, n, reps, max_helpers, ms, dbg);
}
// host only (no device): the BA preparation serial vs on host threads (identical lists -> 0)
int orbhip_test_ba_prepare(const orbhip_ba_problem* prob, int threads, double* out4) {
    if (!prob || threads < 1) return ORBHIP_ERR_ARG;
    return ba_test_prepare(prob, threads, out4);
}
// nested-dissection solve of a pose-structured SPD system (ba_nd.hip): K segments (0 = planned)
int orbhip_test_nd_solve(const double* A, const double* b, double* x, int np, const int* bi, const int* bj, int nblk,
                         int K, int reps, float* ms, int* K_used) {
    if (!A || !b || !x || np <= 0 || !bi || !bj || nblk <= 0 || reps < 1) return ORBHIP_ERR_ARG;
    return nd_test(A, b, x, np, bi, bj, nblk, K, reps, ms, K_used);
}
// the same, with the two halves timed alone (stage_ms[0]: interior factorizations + separator
// assembly, stage_ms[1]: separator solve + interior back-substitution) and the plan's segment
// starts (seg_out: the plan's K + 1 pose indices, then the band's half-width; capacity 65)
int orbhip_test_nd_stages(const double* A, const double* b, double* x, int np, const int* bi, const int* bj, int nblk,
                          int K, int reps, float* ms, int* K_used, float* stage_ms, int* seg_out) {
    if (!A || !b || !x || np <= 0 || !bi || !bj || nblk <= 0 || reps < 1 || !stage_ms || !seg_out) return ORBHIP_ERR_ARG;
    return nd_test(A, b, x, np, bi, bj, nblk, K, reps, ms, K_used, stage_ms, seg_out);
}

// host only (no device): the matcher's dispatch decision (match_route, the function run_match
// follows) for a call shape. out4 = {trains per chunk (0 = k_match_fused), chunks per pair,
// xcd_runs run length, 4-byte partials}
int orbhip_test_match_route(int npairs, int max_q, int max_t, int fused_allowed, int32_t* out4) {
    if (!out4 || npairs <= 0 || max_q < 0 || max_t < 0) return ORBHIP_ERR_ARG;
    const MatchRoute r = match_route(npairs, max_q, max_t, fused_allowed != 0);
    out4[0] = r.tc; out4[1] = r.nch; out4[2] = r.xrun; out4[3] = r.pk;
    return ORBHIP_OK;
}

// host only (no device): the projection searches' decisions for a call's sizes (the functions
// proj_search_last / proj_search_local call, under the current ORBHIP_PROJ_* switches). out4 =
// {1 = the list form applies, ent_cap, list capacity, 1 = one launch}; max_octave stands for the
// largest octave among the frame's keypoints
int orbhip_test_proj_route(int n, int nq, int max_octave, int32_t* out4) {
    return proj_test_route(n, nq, max_octave, out4);
}
// the last projection search on this context: out4 = {form (0 lists + resolve, 1 a list overflowed
// and the rounds produced the result, 2 rounds only, -1 none yet or no queries), rounds, list
// entries the resolve saw (form 0), that call's ent_cap}
int orbhip_test_proj_stats(orbhip_ctx* c, int32_t* out4) {
    if (!c) return ORBHIP_ERR_ARG;
    return proj_test_stats(c->proj, out4);
}
// the last SearchForInitialization on this context: out8 = {form (0 the rounds converged, 1 the
// chain after a claim-slot overflow, 2 the chain after the round cap, 3 the chain by
// ORBHIP_INIT_CHAIN, -1 none yet / no queries / an error), the round that changed nothing (else the
// rounds run), init_ahead after the call, octave-0 keypoints of F1, of F2, queries with need == 1,
// with need == 2 (one device-to-host copy of that call's need[]; -1 when it is gone), 0}
// host only (no device): SearchForInitialization's envelope for a call's sizes (n1 / n2 keypoints,
// nq0 / nr0 of them on octave 0), the function init_search itself follows. out4 = {the return code
// the call would get from its sizes (0, ORBHIP_ERR_ARG, ORBHIP_ERR_UNSUPPORTED), the chain's
// dynamic LDS bytes, entries per query list, parallel rounds before the chain takes over}
int orbhip_test_init_route(int n1, int n2, int nq0, int nr0, int32_t* out4) {
    return init_test_route(n1, n2, nq0, nr0, out4);
}
int orbhip_test_init_stats(orbhip_ctx* c, int32_t* out8) {
    if (!c) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    if (!c->proj) c->proj = proj_ws_create();   // a fresh context reports the workspace's initial state
    return init_test_stats(c->proj, out8, c->stream);
}

// the persistent KeyFrame members of a KeyFrameDatabase (mode 0: mnRelocQuery / mnRelocWords /
// mRelocScore, mode 1: the mnPlaceRecognition* ones), max_kf entries each, after a stream sync
int orbhip_test_kfdb_members(orbhip_kfdb* db, int mode, int64_t* query, int32_t* words, float* score) {
    if (!db) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(db->device));
    return kfdb_members(db->d, mode, (long long*)query, words, score);
}

int orbhip_test_sincosf(const float* x, float* cs, float* sn, int64_t n) {
    if (!x || !cs || !sn || n <= 0) return ORBHIP_ERR_ARG;
    float *dx = nullptr, *dc = nullptr, *ds = nullptr;
    HIPOK(hipMalloc((void**)&dx, n * 4));
    HIPOK(hipMalloc((void**)&dc, n * 4));
    HIPOK(hipMalloc((void**)&ds, n * 4));
    HIPOK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
    launch_sincos_probe(dx, dc, ds, n, nullptr);
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemcpy(cs, dc, n * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(sn, ds, n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dc); (void)hipFree(ds);
    return ORBHIP_OK;
}

// Compare device sinf/cosf with host reference values over float bit range [lo, hi].
int64_t orbhip_test_sincosf_sweep(uint32_t lo, uint32_t hi, const float* ref_c, const float* ref_s) {
    if (hi < lo || !ref_c || !ref_s) return ORBHIP_ERR_ARG;
    const size_t n = (size_t)hi - lo + 1;
    float *dc = nullptr, *ds = nullptr;
    unsigned long long* dm = nullptr;
    unsigned long long hm = 0;
    if (hipMalloc((void**)&dc, n * 4) != hipSuccess) return ORBHIP_ERR_DEVICE;
    if (hipMalloc((void**)&ds, n * 4) != hipSuccess) return ORBHIP_ERR_DEVICE;
    if (hipMalloc((void**)&dm, 8) != hipSuccess) return ORBHIP_ERR_DEVICE;
    (void)hipMemset(dm, 0, 8);
    (void)hipMemcpy(dc, ref_c, n * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(ds, ref_s, n * 4, hipMemcpyHostToDevice);
    launch_sincos_sweep(lo, hi, dc, ds, dm, nullptr);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(&hm, dm, 8, hipMemcpyDeviceToHost);
    (void)hipFree(dc); (void)hipFree(ds); (void)hipFree(dm);
    return (int64_t)hm;
}

// host only (no device): PredictScale's steps as the searches hand them to the device
// (level_thresholds, stage.h): n_levels floats, out[0] unused
int orbhip_test_level_thresholds(float log_sf, int n_levels, float* out) {
    if (!out || n_levels < 1 || n_levels > 127) return ORBHIP_ERR_ARG;
    std::memcpy(out, level_thresholds(log_sf, n_levels), 4 * (size_t)n_levels);
    return ORBHIP_OK;
}

// Compare the device's predict_scale (geom.h) with host levels (int8, one per float) over the
// float bit range [lo, hi]; returns the number of ratios whose level differs.
int64_t orbhip_test_predict_scale_sweep(uint32_t lo, uint32_t hi, float log_sf, int n_levels, const int8_t* ref) {
    if (hi < lo || !ref || n_levels < 1 || n_levels > 127) return ORBHIP_ERR_ARG;
    const size_t n = (size_t)hi - lo + 1;
    int8_t* dr = nullptr;
    float* dt = nullptr;
    unsigned long long* dm = nullptr;
    unsigned long long hm = 0;
    if (hipMalloc((void**)&dr, n) != hipSuccess) return ORBHIP_ERR_DEVICE;
    if (hipMalloc((void**)&dm, 8) != hipSuccess) { (void)hipFree(dr); return ORBHIP_ERR_DEVICE; }
    if (hipMalloc((void**)&dt, 4 * (size_t)n_levels) != hipSuccess) {
        (void)hipFree(dr); (void)hipFree(dm);
        return ORBHIP_ERR_DEVICE;
    }
    const float* thr = level_thresholds(log_sf, n_levels);
    bool ok = hipMemset(dm, 0, 8) == hipSuccess && hipMemcpy(dr, ref, n, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dt, thr, 4 * (size_t)n_levels, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_predict_scale_sweep(lo, hi, log_sf, dt, n_levels, dr, dm, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&hm, dm, 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(dr); (void)hipFree(dm); (void)hipFree(dt);
    return ok ? (int64_t)hm : (int64_t)ORBHIP_ERR_DEVICE;
}

// the extractor's hooks (extract.cpp): one frame's intermediates, its FAST candidate count, a
// plan's cell table
int orbhip_test_extract_debug(orbhip_ctx* c, const uint8_t* img, int w, int h, int lap0, int lap1, uint8_t* pyr,
                              uint32_t* cand, int32_t* cand_cnt, void* lvl, int32_t* lvl_cnt, int32_t* lvl_nlap,
                              int32_t* sizes /* n_slots_total, n_cells_total, kp_slots_total, err */) {
    if (!c || !img) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return extract_test_debug(c->ext, img, w, h, lap0, lap1, pyr, cand, cand_cnt, lvl, lvl_cnt, lvl_nlap, sizes);
}

// The stereo kernels alone on caller-supplied keypoints and descriptors of both sides (n_l outputs
// each; best_r: the search's winner or -1; sad: the best SAD or -1 where none was formed). The
// pyramids come from the extractor's own pyramid stage.
int orbhip_test_stereo_match(orbhip_ctx* c, const uint8_t* left, const uint8_t* right, int w, int h,
                             const orbhip_stereo_params* params, const orbhip_kp* kps_l, const uint8_t* desc_l,
                             int n_l, const orbhip_kp* kps_r, const uint8_t* desc_r, int n_r, float* u_right,
                             float* depth, int32_t* status, int32_t* best_r, int32_t* sad, int* n_stereo) {
    if (!c || !left || !right || w <= 0 || h <= 0 || !params || !n_stereo || (n_l > 0 && (!kps_l || !desc_l)) ||
        (n_r > 0 && (!kps_r || !desc_r)) || (n_l > 0 && (!u_right || !depth || !status || !best_r || !sad)))
        return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return stereo_test_match(c->ext, left, right, w, h, *params, kps_l, desc_l, n_l, kps_r, desc_r, n_r, u_right,
                             depth, status, best_r, sad, n_stereo);
}

// k_stereo_median alone on one pair's n entries: status (1 = accepted) with u_right and depth are
// updated in place by the median cut, n_stereo is the number left at 1.
int orbhip_test_stereo_median(orbhip_ctx* c, int32_t* status, const int32_t* sad, float* u_right, float* depth, int n,
                              int* n_stereo) {
    if (!c || n < 0 || !n_stereo || (n > 0 && (!status || !sad || !u_right || !depth))) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return stereo_test_median(status, sad, u_right, depth, n, n_stereo);
}

int orbhip_test_candidates(orbhip_ctx* c, int w, int h, int frame, int64_t* n) {
    if (!c || !n || frame < 0) return ORBHIP_ERR_ARG;
    HIPOK(hipSetDevice(c->device));
    return extract_test_candidates(c->ext, w, h, frame, n);
}

int orbhip_test_cells(orbhip_ctx* c, int w, int h, int32_t* out6, int cap) {
    if (!c) return ORBHIP_ERR_ARG;
    return extract_test_cells(c->ext, w, h, out6, cap);
}

// Device timing trace (diagnostics; see orbhip_device.h TR_*): on != 0 allocates a zeroed
// buffer of kTraceKernels x kTraceStride u64 and points every kernel unit at it; on == 0 copies
// it to `out` (if non-null, kTraceKernels * kTraceStride entries) and detaches it.
int orbhip_test_trace(int on, unsigned long long* out) {
    static unsigned long long* buf = nullptr;
    const size_t n = (size_t)kTraceKernels * kTraceStride;
    if (on) {
        if (!buf) HIPOK(hipMalloc((void**)&buf, n * sizeof(unsigned long long)));
        HIPOK(hipMemset(buf, 0, n * sizeof(unsigned long long)));
        trace_set_extract(buf);
        trace_set_match(buf);
        trace_set_proj(buf);
        return ORBHIP_OK;
    }
    HIPOK(hipDeviceSynchronize());
    if (buf && out) HIPOK(hipMemcpy(out, buf, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    trace_set_extract(nullptr);
    trace_set_match(nullptr);
    trace_set_proj(nullptr);
    return ORBHIP_OK;
}

}  // extern "C"
