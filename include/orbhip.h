/*
 * orbhip.h — C-ABI of liborbhip.so, the MI355X (gfx950) ORB front-end + BA back-end.
 *
 * Drop-in boundary for the hot path of EricPedley/ORB_SLAM3_ROS2.
 * Each entry point names the reference interface it replaces:
 *   R:src/imu_mono_realsense.cpp:337   System::TrackMonocular -> Frame(mono) -> Frame::ExtractORB
 *   U:src/Frame.cc::Frame::ExtractORB  calls ORBextractor::operator()(im, Mat(), kps, desc, {0,1000})
 *   U:src/ORBextractor.cc::ORBextractor::operator()          -> orbhip_extract / orbhip_extract_batch_device
 *   U:src/ORBextractor.cc::ORBextractor::ORBextractor(...)   -> orbhip_create (orbhip_orb_params)
 *   U:src/ORBmatcher.cc::ORBmatcher::DescriptorDistance      -> orbhip_descriptor_distance
 *   U:src/ORBmatcher.cc  best/second + ratio + TH_LOW + rotation histogram -> orbhip_match_bf*
 *   U:src/Optimizer.cc::Optimizer::LocalBundleAdjustment / BundleAdjustment -> orbhip_ba_solve
 *
 * Conventions:
 *  - Plain pointers and sizes only; no C++ types, no exceptions cross this ABI.
 *  - The caller owns every host buffer. A context owns its device memory, pinned
 *    staging and one HIP stream (used by the host-buffer entry points). The *_device entry
 *    points run on the caller's `stream` argument; NULL is the HIP null stream. One context
 *    per calling thread; a context is not re-entrant; distinct contexts are safe to use
 *    concurrently.
 *  - Status: 0 ok, < 0 error (orbhip_status).
 *  - Parity contract: keypoints/descriptors bit-exact with the CPU restatement in
 *    oracle/ (the reference's own path cannot be built here: SURVEY.md §0, §8c).
 */
#ifndef ORBHIP_H
#define ORBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBHIP_ABI_VERSION 1

typedef enum {
    ORBHIP_OK = 0,
    ORBHIP_ERR_ARG = -1,          /* bad argument (null pointer, bad size, ...) */
    ORBHIP_ERR_CAPACITY = -2,     /* caller buffer too small; *n_out holds the required count */
    ORBHIP_ERR_DEVICE = -3,       /* HIP runtime failure / no device */
    ORBHIP_ERR_NOT_PD = -4,       /* reduced camera system not positive definite */
    ORBHIP_ERR_UNSUPPORTED = -5,  /* configuration outside the supported envelope */
    ORBHIP_ERR_EMPTY = -6,        /* empty image: ORBextractor::operator() returns -1 */
    ORBHIP_ERR_TIMEOUT = -7       /* a persistent-solver hand-off timed out (ORBHIP_DAG_RERUN=0) */
} orbhip_status;

typedef struct orbhip_ctx orbhip_ctx;

/* ORBextractor ctor arguments; YAML keys ORBextractor.{nFeatures, scaleFactor, nLevels,
 * iniThFAST, minThFAST} (R:config/Monocular/MilkV.yaml:42-55). */
typedef struct {
    int32_t n_features;
    float scale_factor;
    int32_t n_levels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} orbhip_orb_params;

/* cv::KeyPoint as produced by ORBextractor (class_id is always -1 there, omitted). */
typedef struct {
    float x, y;       /* level-0 pixel coordinates (pt *= mvScaleFactor[octave]) */
    float size;       /* (int)(31 * mvScaleFactor[octave]) */
    float angle;      /* IC_Angle, degrees [0, 360) */
    float response;   /* FAST score */
    int32_t octave;   /* pyramid level */
} orbhip_kp;

/* ---- context ------------------------------------------------------------------- */
int orbhip_abi_version(void);
/* device: HIP ordinal, or < 0 for the calling thread's current device (hipGetDevice: one process
   per GPU). params may be NULL -> ORB_SLAM3 defaults (1000, 1.2, 8, 20, 7). */
int orbhip_create(orbhip_ctx** out, int device, const orbhip_orb_params* params);
int orbhip_destroy(orbhip_ctx* ctx);
/* Per-level tables of the ORBextractor ctor: mvScaleFactor, mnFeaturesPerLevel. */
int orbhip_level_info(orbhip_ctx* ctx, int w, int h, int32_t* level_w, int32_t* level_h,
                      int32_t* n_feat, float* scale);
/* Max keypoints one frame can yield for this context at size w x h (cap for outputs). */
int orbhip_max_keypoints(orbhip_ctx* ctx, int w, int h);

/* ---- ORB extraction --------------------------------------------------------------
 * orbhip_extract: ORBextractor::operator()(img, Mat(), kps, desc, {lap0, lap1}).
 * Host image (CV_8UC1, row stride in bytes), host outputs (cap entries). *mono_index
 * receives the return value of operator() (kps with lap0 <= x <= lap1 fill the array
 * from the end, the rest from the front). Empty image -> ORBHIP_ERR_EMPTY (reference: -1). */
int orbhip_extract(orbhip_ctx* ctx, const uint8_t* img, int w, int h, int stride, int lap0, int lap1,
                   orbhip_kp* kps, uint8_t* desc32, int cap, int* n_out, int* mono_index);

/* Batched, fully device-resident form (torch-ROCm ingest, benchmarks). d_imgs: B frames,
 * frame f at d_imgs + f*frame_stride, rows `stride` bytes apart. Outputs per frame f:
 * d_kps[f*cap ...], d_desc[(f*cap ...)*32], d_n[f], d_mono[f]. Asynchronous on `stream`
 * (hipStream_t; NULL = the HIP null stream, as in every HIP API — torch's default stream).
 *
 * Input layout contract (also orbhip_extract_stereo_device and orbhip_frontend_push): d_imgs may
 * have any byte alignment; stride >= w, and frame_stride >= stride*h when B > 1 (neither needs to
 * be a multiple of anything), else ORBHIP_ERR_ARG and nothing is launched. Of each row the library
 * reads only the first w bytes, plus padding up to the next 4-byte boundary when that boundary lies
 * within `stride` (rows are read as aligned 4-byte words when the frame's address and `stride` are
 * both multiples of 4, byte by byte otherwise), and it reads nothing past the last row: every read
 * of frame f lies in [d_imgs + f*frame_stride, + (h-1)*stride + w rounded up as above). One
 * exception inside that range: for a keypoint within 23 columns of the right edge the descriptor
 * stage may read up to 5 bytes past w of a row that another row of the frame follows (padding or
 * that next row's first bytes). Padding bytes never influence a result. */
int orbhip_extract_batch_device(orbhip_ctx* ctx, const uint8_t* d_imgs, int B, int w, int h, int stride,
                                int64_t frame_stride, int lap0, int lap1, orbhip_kp* d_kps, uint8_t* d_desc,
                                int cap, int32_t* d_n, int32_t* d_mono, void* stream);

/* ---- rectified stereo frames ---------------------------------------------------------
 * U:src/Frame.cc Frame(imLeft, imRight, ...): ExtractORB(0, left, 0, 0), ExtractORB(1, right, 0, 0),
 * then Frame::ComputeStereoMatches (DESIGN.md section 4 "Stereo"): mvuRight / mvDepth per left
 * keypoint, -1 where there is no match. bf = mbf (baseline x fx), b = mb (baseline in metres);
 * center_patch != 0 subtracts each 11x11 patch's centre pixel before the L1 distance (ORB_SLAM2 and
 * early ORB_SLAM3; 0 = the raw patches of ORB_SLAM3 v1.0). status (may be NULL) per left keypoint:
 * 1 accepted, 2 no candidate in its row or maxU < 0, 3 best descriptor distance >= 75, 4 the
 * iniu / endu test, 5 best SAD at +-L, 6 |deltaR| > 1, 7 disparity outside [0, bf / b), 8 removed by
 * the median cut, 9 a window outside its pyramid level or an octave outside [0, n_levels).
 * u_right, depth and status have cap entries per left frame; entries at or past the left frame's
 * keypoint count are left untouched; *n_stereo counts the status-1 keypoints. NULL pointers (status
 * excepted), bf <= 0, b <= 0, P < 1: ORBHIP_ERR_ARG; an empty image: ORBHIP_ERR_EMPTY; cap below
 * orbhip_max_keypoints(w, h): ORBHIP_ERR_CAPACITY. */
typedef struct {
    float bf, b;
    int32_t center_patch;
} orbhip_stereo_params;

/* Host images (row stride in bytes) and host outputs. */
int orbhip_extract_stereo(orbhip_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                          const orbhip_stereo_params* params, orbhip_kp* kps_l, uint8_t* desc_l, int* n_l,
                          orbhip_kp* kps_r, uint8_t* desc_r, int* n_r, int cap, float* u_right, float* depth,
                          int32_t* status, int* n_stereo);

/* P pairs, device-resident: frames 2p (left) and 2p + 1 (right) of d_imgs, and the keypoint outputs
 * of the 2P frames, laid out as orbhip_extract_batch_device lays them out. Stereo outputs of pair p
 * at p*cap, d_n_stereo[p]. Asynchronous on `stream`, no host synchronisation. */
int orbhip_extract_stereo_device(orbhip_ctx* ctx, const uint8_t* d_imgs, int P, int w, int h, int stride,
                                 int64_t frame_stride, const orbhip_stereo_params* params, orbhip_kp* d_kps,
                                 uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono, float* d_u_right,
                                 float* d_depth, int32_t* d_status, int32_t* d_n_stereo, void* stream);

/* ---- distorted pinhole camera -----------------------------------
 * U:src/CameraModels/Pinhole (fx fy cx cy) + U:src/Frame.cc mDistCoef (k1 k2 p1 p2 [k3]), as the
 * node's camera file gives them (R:config/Monocular/MilkV.yaml:10-25). k1 == 0 means no
 * distortion (the reference's test: mDistCoef.at<float>(0) == 0). */
typedef struct orbhip_pinhole {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
} orbhip_pinhole;

/* U:src/Frame.cc::Frame::UndistortKeyPoints: mvKeysUn from mvKeys through cv::undistortPoints
 * (OpenCV 4.5.4, 5 fixed-point rounds, fp64), bit-exact. Host buffers; out may alias kps.
 * k1 == 0: out = kps. Replaces the cv::undistortPoints call inside Frame(mono) after ExtractORB. */
int orbhip_undistort_keypoints(orbhip_ctx* ctx, const orbhip_pinhole* cam, const orbhip_kp* kps, int n,
                               orbhip_kp* out);
/* The same on the device over an extraction batch: d_kps[b*cap + i] for i < d_n[b] -> d_out
 * (may alias). Asynchronous on `stream` (NULL = the HIP null stream). */
int orbhip_undistort_keypoints_device(orbhip_ctx* ctx, const orbhip_pinhole* cam, const orbhip_kp* d_kps,
                                      const int32_t* d_n, int B, int cap, orbhip_kp* d_out, void* stream);
/* U:src/Frame.cc::Frame::ComputeImageBounds: bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY} from the
 * undistorted image corners ({0, cols, 0, rows} when k1 == 0). These bounds define the 64 x 48
 * frame grid the projection / initialisation searches use (orbhip_frame.min_x ...). */
int orbhip_image_bounds(orbhip_ctx* ctx, const orbhip_pinhole* cam, int cols, int rows, float bounds[4]);

/* ---- ingest (a23) -------------------------------------------------------------------
 * cv_bridge::toCvShare(bgr8 msg, MONO8) -> cvtColor(COLOR_BGR2GRAY) (R:src/imu_mono_realsense.cpp:298)
 * on the device, bit-exact: Y = (B*1868 + G*9617 + R*4899 + 2^13) >> 14. B frames of w x h
 * BGR (3 bytes/px, rows `src_stride` bytes apart, frames `src_fstride` apart) -> u8 gray
 * (rows `dst_stride`, frames `dst_fstride`), ready for orbhip_extract_batch_device.
 * Asynchronous on `stream` (NULL = the HIP null stream). */
int orbhip_bgr_to_gray_device(orbhip_ctx* ctx, const uint8_t* d_bgr, int B, int w, int h, int src_stride,
                              int64_t src_fstride, uint8_t* d_gray, int dst_stride, int64_t dst_fstride,
                              void* stream);

/* ---- Hamming matching ------------------------------------------------------------- */
/* ORBmatcher::DescriptorDistance (host helper, popcount of xor over 32 bytes). */
int orbhip_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Brute-force top-2 over the whole train set (order-free: no greedy vnMatches21 pass),
 * accept best <= th_low && (float)best < ratio*(float)second, then (if check_orientation)
 * the rotation-histogram filter (HISTO_LENGTH 30, ComputeThreeMaxima). best/second start at
 * 256 (SearchByBoW). match[i] = train index or -1. Host buffers. Returns #matches >= 0. */
int orbhip_match_bf(orbhip_ctx* ctx, const uint8_t* q_desc, const float* q_angle, int nq,
                    const uint8_t* t_desc, const float* t_angle, int nt, int th_low, float ratio,
                    int check_orientation, int32_t* match, int32_t* best_d, int32_t* second_d);

/* Device form over extractor outputs: pairs (frame p, frame p+1) for p in [0, B-1), each
 * frame's kps/desc at f*cap as written by orbhip_extract_batch_device. Outputs at p*cap;
 * d_nmatch[p] = #matches. Asynchronous. */
int orbhip_match_pairs_device(orbhip_ctx* ctx, const orbhip_kp* d_kps, const uint8_t* d_desc,
                              const int32_t* d_n, int B, int cap, int th_low, float ratio,
                              int check_orientation, int32_t* d_match, int32_t* d_best,
                              int32_t* d_second, int32_t* d_nmatch, void* stream);

/* Device form over two arbitrary frames (e.g. frame t vs t-1 in a 2-slot ring): query
 * set (d_q_kps/d_q_desc, count *d_nq) vs train set (d_t_kps/d_t_desc, count *d_nt), both laid
 * out like one frame of orbhip_extract_batch_device (cap entries). Outputs (cap entries) and
 * *d_nmatch on the device. Asynchronous; no host synchronisation. */
int orbhip_match_frames_device(orbhip_ctx* ctx, const orbhip_kp* d_q_kps, const uint8_t* d_q_desc,
                               const int32_t* d_nq, const orbhip_kp* d_t_kps, const uint8_t* d_t_desc,
                               const int32_t* d_nt, int cap, int th_low, float ratio, int check_orientation,
                               int32_t* d_match, int32_t* d_best, int32_t* d_second, int32_t* d_nmatch,
                               void* stream);

/* ---- camera front-end stream -------------------------------------------------------
 * One camera's frames, as Tracking receives them (Frame ctor -> ExtractORB, then matching
 * against the last frame), pipelined on the device: frame k is extracted at batch 1 on
 * context k % frames_in_flight (each context = its own HIP stream / hardware queue) into
 * output slot k % slots (slots = 2 * frames_in_flight, 2 for 1), then the previous frame
 * (queries) is matched to it (train) as orbhip_match_frames_device does with (th_low, ratio,
 * check_orientation). Cross-frame hand-offs are device events; push never blocks the host.
 * Same kernels and results as the one-frame calls. Frame 0 has no match (*nmatch = -1).
 *   push: d_img = device u8 frame (w x h, rows `stride` bytes apart), vLappingArea
 *         {lap0, lap1}; returns the slot index (>= 0) or an error (< 0). The caller keeps
 *         d_img unchanged until the frame completes.
 *   view: device pointers of a slot's outputs (valid until the slot is reused, `slots`
 *         pushes later); frame = number of the frame held (-1 none).
 *   wait: the frame in `slot` complete: host-blocking (stream NULL) or stream-ordered. With
 *         one frame in flight the stream is one in-order HIP stream and push records no event:
 *         the first wait that needs one records it then (covering every frame pushed so far).
 *   context: context j (0 <= j < frames_in_flight), e.g. for orbhip_profile_stage. */
typedef struct orbhip_frontend orbhip_frontend;
typedef struct {
    int64_t frame;
    int32_t cap, slots;
    orbhip_kp* kps;          /* cap entries */
    uint8_t* desc;           /* cap x 32 */
    int32_t* n;              /* 1 */
    int32_t* mono;           /* 1: operator()'s return value */
    int32_t* match;          /* cap: previous frame's keypoint i -> this frame's index or -1 */
    int32_t* best;           /* cap */
    int32_t* second;         /* cap */
    int32_t* nmatch;         /* 1 */
} orbhip_frontend_slot;
int orbhip_frontend_create(orbhip_frontend** out, int device, const orbhip_orb_params* params, int w, int h,
                           int frames_in_flight, int th_low, float ratio, int check_orientation);
int orbhip_frontend_destroy(orbhip_frontend* fe);
int orbhip_frontend_push(orbhip_frontend* fe, const uint8_t* d_img, int stride, int lap0, int lap1);
int orbhip_frontend_view(orbhip_frontend* fe, int slot, orbhip_frontend_slot* out);
int orbhip_frontend_wait(orbhip_frontend* fe, int slot, void* stream);
int orbhip_frontend_context(orbhip_frontend* fe, int j, orbhip_ctx** out);

/* ---- diagnostics: live kernel timing ----------------------------------------------
 * orbhip_profile_stage selects ONE stage whose launches are bracketed by hipEvents on the
 * stream they run on (0 off, 1 pyramid resize, 2 FAST cells, 3 octree, 4 orientation +
 * descriptor, 5 Hamming top-2, 6 rotation filter, 7 SearchForTriangulation: the ordering pre-pass
 * and the search of one call form one pair, 8 Fuse and Fuse with a Sim3: the grid build and the
 * search of one call form one pair, 9 SearchByProjection with a Sim3: the grid build, the search and
 * the resolve of one call form one pair, 10 the triangulation of CreateNewMapPoints: k_tri_points
 * and k_tri_claim of one call form one pair, 11 Sim3Solver: k_sim3_ransac and k_sim3_select of one
 * call form one pair, 13 OptimizeSim3: k_sim3_opt, 15 OptimizeEssentialGraph: the first to the last kernel of
 * one call form one pair, 16 TwoViewReconstruction: the four launches of one call form one pair;
 * 12 and 14 are no stages and are refused). orbhip_profile_collect synchronises and
 * returns the summed duration (ms) and the number of bracketed launches, then resets. The one-launch
 * pyramid (k_pyr_cone) and the octree also time themselves on the device (first workgroup start to
 * last workgroup end, s_memrealtime: the span rocprofv3's kernel trace reports); their stages
 * return that span when every launch recorded it, the event pairs otherwise. */
int orbhip_profile_stage(orbhip_ctx* ctx, int stage);
int orbhip_profile_collect(orbhip_ctx* ctx, double* total_ms, int32_t* count);

/* With ORBHIP_GRAPH=1 in the environment, repeated calls of orbhip_extract_batch_device /
 * orbhip_match_*_device with identical arguments on a non-NULL stream are replayed from a
 * captured hipGraph (from the second such call on: one hipGraphLaunch instead of the kernel
 * launches). Same kernels, same results. Off by default (the replay adds device time on this
 * runtime); always direct while a profile stage is selected or on a capturing stream.
 * Returns the number of launch graphs the context holds. */
int orbhip_launch_graphs(orbhip_ctx* ctx);

/* ---- bundle adjustment ------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment / BundleAdjustment problem (SoA, host memory).
 * Poses are Tcw = (q, t): q = unit quaternion (x, y, z, w), t translation, float, as
 * Sophus::SE3f stores them. Edges are EdgeSE3ProjectXYZ mono observations. */
typedef struct {
    int32_t n_poses, n_points, n_edges;
    const float* pose_q;        /* n_poses x 4 (x,y,z,w) */
    const float* pose_t;        /* n_poses x 3 */
    const uint8_t* pose_fixed;  /* n_poses (1 = fixed vertex) */
    const float* points;        /* n_points x 3 (world) */
    const int32_t* edge_pose;   /* n_edges */
    const int32_t* edge_point;  /* n_edges */
    const float* edge_uv;       /* n_edges x 2 (undistorted keypoint) */
    const int32_t* edge_octave; /* n_edges */
    const float* inv_sigma2;    /* per octave: information = I * invSigma2[octave] */
    int32_t n_octaves;
    float fx, fy, cx, cy;       /* Pinhole mvParameters (float) */
    float huber_delta;          /* sqrt(5.991) for LBA; <= 0 disables the robust kernel */
    int32_t iterations;         /* optimize(n): 10 for LBA */
    int32_t early_stop;         /* vendored-g2o chi2 stall stop, 0 = off */
} orbhip_ba_problem;

typedef struct {
    float* pose_q;              /* n_poses x 4 out (fixed poses copied through) */
    float* pose_t;              /* n_poses x 3 out */
    float* points;              /* n_points x 3 out */
    float* edge_chi2;           /* n_edges out: e->chi2() after optimize (for the 5.991 erase) */
    uint8_t* edge_depth_ok;     /* n_edges out: e->isDepthPositive() */
    double initial_chi2;        /* activeRobustChi2 before iteration 0 */
    double final_chi2;          /* activeRobustChi2 of the accepted state */
    int32_t iterations_done;    /* SparseOptimizer::optimize return value */
    int32_t lm_trials;          /* total Levenberg trials */
} orbhip_ba_result;

/* stop_flag: polled between LM iterations/trials (LocalMapping mbAbortBA -> g2o
 * setForceStopFlag). May be NULL. */
int orbhip_ba_solve(orbhip_ctx* ctx, const orbhip_ba_problem* prob, orbhip_ba_result* res,
                    const volatile int* stop_flag);

/* Concurrency: LocalMapping's LBA and LoopClosing's GBA (R:src/imu_mono_realsense.cpp:99-100
 * spawns both threads) may solve at the same time on two contexts. The persistent Cholesky
 * (one launch owning every CU) is serialised per device across contexts and streams, so two
 * solves never hold parts of the chip at once. A hand-off that still times out (its bounded spin,
 * ORBHIP_DAG_SPIN_MAX polls, runs out) never becomes a silently rejected LM trial: the solve is run
 * again on the non-persistent solvers (same g2o schedule), or, with ORBHIP_DAG_RERUN=0 in the
 * environment, returns ORBHIP_ERR_TIMEOUT.
 * orbhip_ba_stats: out[0] persistent solves launched on the context's device (every context),
 * out[1] of them launched after waiting for another stream's solve, out[2] hand-off timeouts this
 * context saw, out[3] solves it re-ran. */
int orbhip_ba_stats(orbhip_ctx* ctx, int64_t out[4]);

/* B independent problems solved together (SURVEY.md §8e replicas: concurrent maps / agents,
 * or a batch of local windows). Each problem follows its own exact LM schedule; all share the
 * kernel launches of a round. probs / res: arrays of B structs. */
int orbhip_ba_solve_batch(orbhip_ctx* ctx, const orbhip_ba_problem* probs, int B, orbhip_ba_result* res,
                          const volatile int* stop_flag);

/* LocalBundleAdjustment / BundleAdjustment of a rectified-stereo system: an observation with
 * edge_ur[e] >= 0 (the keyframe's mvuRight; 0.0f counts) is g2o's EdgeStereoSE3ProjectXYZ:
 * observation (u, v, ur), error obs - (fx x/z + cx, fy y/z + cy, fx x/z + cx - bf/z), information
 * I3 * invSigma2[octave], chi2 over the three terms, and a Huber delta of its own
 * (thHuberStereo = thHuber3D = sqrt(7.815)). Every other observation is the monocular edge of
 * orbhip_ba_problem, unchanged, and so is the LM schedule. orbhip_ba_result is unchanged:
 * edge_chi2 of a stereo edge is the three-term chi2 (the caller erases at 7.815 on stereo edges,
 * 5.991 on monocular ones). ORBHIP_ERR_ARG, before anything runs and with no result written:
 * edge_ur NULL with n_edges > 0, bf <= 0 while some edge_ur[e] >= 0, and whatever
 * orbhip_ba_solve rejects. A call whose problems hold no stereo edge runs orbhip_ba_solve's
 * kernels (the same bits). The sharded entries (orbhip_ba_solve_sharded, _sharded_segments,
 * _shards_local) have no stereo form. */
typedef struct {
    orbhip_ba_problem mono;      /* every field as in orbhip_ba_solve */
    const float* edge_ur;        /* n_edges: mvuRight of the observation (< 0: monocular edge) */
    float bf;                    /* mbf */
    float huber_delta_stereo;    /* sqrt(7.815); <= 0: no robust kernel on stereo edges */
} orbhip_ba_stereo_problem;
int orbhip_ba_solve_stereo(orbhip_ctx* ctx, const orbhip_ba_stereo_problem* prob, orbhip_ba_result* res,
                           const volatile int* stop_flag);
int orbhip_ba_solve_stereo_batch(orbhip_ctx* ctx, const orbhip_ba_stereo_problem* probs, int B,
                                 orbhip_ba_result* res, const volatile int* stop_flag);

/* ---- projection-guided matching ---------------------------
 * The current Frame as U:src/Frame.cc holds it after extraction: keypoints mvKeysUn (= mvKeys,
 * distortion k1 == 0), descriptors, image bounds mnMinX..mnMaxY (ComputeImageBounds), the
 * 64 x 48 grid implied by them (AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea), the
 * scale tables and the pose Tcw. claimed[k] = mvpMapPoints[k] set (with observations) before
 * the call (NULL: none). At most 65535 keypoints. */
typedef struct {
    int32_t n;
    const orbhip_kp* kps;       /* n: mvKeysUn */
    const uint8_t* desc;        /* n x 32: mDescriptors */
    const uint8_t* claimed;     /* n or NULL */
    float min_x, max_x, min_y, max_y;
    const float* scale_factors; /* mvScaleFactors */
    int32_t n_levels;
    float log_scale_factor;     /* mfLogScaleFactor */
    float fx, fy, cx, cy;       /* Pinhole mvParameters */
    float pose_q[4];            /* Tcw rotation (x, y, z, w) */
    float pose_t[3];
} orbhip_frame;

/* U:src/ORBmatcher.cc::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th,
 * bMono = true) (TrackWithMotionModel). Queries: LastFrame entries i with a MapPoint that is
 * not an outlier, in index order: world position, pMP->GetDescriptor(), LastFrame keypoint
 * octave and angle. match[q] = CurrentFrame keypoint assigned to query q (the adapter sets
 * CurrentFrame.mvpMapPoints[match[q]] = pMP) or -1. Returns nmatches. */
typedef struct {
    int32_t n;
    const float* points;        /* n x 3 */
    const uint8_t* desc;        /* n x 32 */
    const int32_t* octave;      /* n */
    const float* angle;         /* n: LastFrame.mvKeysUn[i].angle */
} orbhip_proj_last;
int orbhip_search_by_projection_last(orbhip_ctx* ctx, const orbhip_frame* cur, const orbhip_proj_last* last,
                                     float th, int check_orientation, int32_t* match);

/* U:src/Tracking.cc::SearchLocalPoints: Frame::isInFrustum(pMP, view_cos_limit = 0.5) for every
 * local MapPoint not skipped, then U:src/ORBmatcher.cc::SearchByProjection(F, vpMapPoints, th,
 * bFarPoints, thFarPoints) in vpMapPoints order. Per point: GetWorldPos, GetNormal,
 * mfMinDistance, mfMaxDistance, GetDescriptor; skip[m] = bad / already matched in this frame.
 * Outputs: in_view[m] = mbTrackInView, level[m] = mnTrackScaleLevel, match[m] = F keypoint or -1.
 * Returns nmatches. */
typedef struct {
    int32_t n;
    const float* points;        /* n x 3 */
    const float* normals;       /* n x 3 */
    const float* min_dist;      /* n: mfMinDistance */
    const float* max_dist;      /* n: mfMaxDistance */
    const uint8_t* desc;        /* n x 32 */
    const uint8_t* skip;        /* n or NULL */
} orbhip_local_points;
int orbhip_search_local_points(orbhip_ctx* ctx, const orbhip_frame* frame, const orbhip_local_points* mps,
                               float view_cos_limit, float th, float nnratio, int far_points, float th_far,
                               uint8_t* in_view, int32_t* level, int32_t* match);

/* The two searches on a rectified-stereo Frame (the stereo branches of both SearchByProjection
 * forms): u_right = mvuRight (n entries), bf = mbf, b = mb. A candidate keypoint k with
 * u_right[k] > 0 is skipped when |ur - u_right[k]| > the query's window radius, ur = u - bf * invz
 * the query's projection into the right image.
 * orbhip_search_by_projection_last_stereo is SearchByProjection(CurrentFrame, LastFrame, th,
 * bMono = false): last_pose_q / last_pose_t = LastFrame.GetPose() (Tlw); with tlc = Rlw twc + tlw
 * the camera moved forward (tlc.z > b: levels nLastOctave and up), backward (-tlc.z > b: levels 0
 * .. nLastOctave) or neither (nLastOctave - 1 .. nLastOctave + 1). direction (may be NULL)
 * receives 1 / -1 / 0. orbhip_search_local_points_stereo also returns proj_xr (may be NULL):
 * mTrackProjXR where in_view[m], untouched elsewhere. Both return ORBHIP_ERR_ARG when u_right is
 * NULL with n > 0, or bf <= 0 or b <= 0. */
typedef struct {
    orbhip_frame frame;
    const float* u_right;       /* frame.n: mvuRight */
    float bf, b;                /* mbf, mb */
} orbhip_stereo_view;
int orbhip_search_by_projection_last_stereo(orbhip_ctx* ctx, const orbhip_stereo_view* cur,
                                            const orbhip_proj_last* last, const float last_pose_q[4],
                                            const float last_pose_t[3], float th, int check_orientation,
                                            int32_t* match, int32_t* direction);
int orbhip_search_local_points_stereo(orbhip_ctx* ctx, const orbhip_stereo_view* frame,
                                      const orbhip_local_points* mps, float view_cos_limit, float th, float nnratio,
                                      int far_points, float th_far, uint8_t* in_view, int32_t* level, float* proj_xr,
                                      int32_t* match);

/* ---- monocular initialisation matching -------------------------------------------
 * U:src/ORBmatcher.cc::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>&
 * vbPrevMatched, vector<int>& vnMatches12, int windowSize), called by
 * U:src/Tracking.cc::MonocularInitialization as ORBmatcher(0.9, true) with windowSize 100.
 * Exact greedy semantics: F1 keypoints of octave 0 in index order, F2.GetFeaturesInArea(
 * vbPrevMatched[i1], windowSize, 0, 0) on F2's 64 x 48 grid (bounds min_x..max_y), candidates
 * with vMatchedDistance <= dist skipped, TH_LOW = 50 and the nnratio test, later better matches
 * steal the F2 keypoint, rotation histogram over all pushes (ComputeThreeMaxima).
 * prev_matched (n1 x 2 floats) is updated in place for the surviving matches; matches12[n1]
 * receives vnMatches12. Returns nmatches. Octaves must be >= 0. Envelope: 4 * (F2 octave-0
 * keypoints) + 4 * (F1 octave-0 keypoints) <= 150 KiB (ORBHIP_ERR_UNSUPPORTED beyond). */
typedef struct {
    int32_t n;
    const orbhip_kp* kps;       /* n: mvKeysUn */
    const uint8_t* desc;        /* n x 32 */
    float min_x, max_x, min_y, max_y;   /* mnMinX, mnMaxX, mnMinY, mnMaxY (grid of F2) */
} orbhip_init_frame;
int orbhip_search_for_initialization(orbhip_ctx* ctx, const orbhip_init_frame* f1, const orbhip_init_frame* f2,
                                     float* prev_matched, int window_size, float nnratio, int check_orientation,
                                     int32_t* matches12);

/* ---- KeyFrameDatabase place recognition ---------------------
 * U:src/KeyFrameDatabase.cc. The database lives on the device: add/erase mirror
 * KeyFrameDatabase::add(pKF) / erase(pKF) with the KF's BowVector (ascending word ids, L1
 * values; slot = the adapter's KeyFrame index, < max_kf). The KeyFrame members the queries use
 * (mnRelocQuery/Words, mRelocScore, mnPlaceRecognitionQuery/Words/Score) persist in the
 * database between queries, as on the KeyFrames. Per query the adapter passes the query
 * BowVector (<= 3072 words), a unique query id (Frame / KeyFrame mnId), covis = max_kf x 10
 * slots of KeyFrame::GetBestCovisibilityKeyFrames(10) (-1 padded), and optionally the map id of
 * every slot (GetMap()) with the query's map, and flags (bit 0 isBad(), bit 1 GetMap()->IsBad()). */
typedef struct orbhip_kfdb orbhip_kfdb;
typedef struct {
    int64_t query_id;
    const int32_t* words;
    const double* values;
    int32_t n;
    const int32_t* covis;       /* max_kf x 10, entries < max_kf (else ORBHIP_ERR_ARG); < 0 ends a row */
    const int32_t* kf_map;      /* max_kf or NULL (one map) */
    int32_t query_map;
    const uint8_t* kf_flags;    /* max_kf or NULL */
} orbhip_kfdb_query;
int orbhip_kfdb_create(orbhip_ctx* ctx, int max_kf, orbhip_kfdb** out);
int orbhip_kfdb_destroy(orbhip_kfdb* db);
int orbhip_kfdb_add(orbhip_kfdb* db, int kf, const int32_t* words, const double* values, int n);
int orbhip_kfdb_erase(orbhip_kfdb* db, int kf);
/* DetectRelocalizationCandidates(F, pMap): writes up to cap slots, returns the full count. */
int orbhip_kfdb_detect_relocalization(orbhip_kfdb* db, const orbhip_kfdb_query* q, int32_t* out, int cap);
/* DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, n): connected = max_kf flags of
 * pKF->GetConnectedKeyFrames() (or NULL); n <= 32. Returns n_loop + n_merge. */
int orbhip_kfdb_detect_nbest(orbhip_kfdb* db, const orbhip_kfdb_query* q, const uint8_t* connected, int n,
                             int32_t* loop_out, int32_t* n_loop, int32_t* merge_out, int32_t* n_merge);

/* ---- motion-only bundle adjustment -------------------------
 * U:src/Optimizer.cc::Optimizer::PoseOptimization(Frame* pFrame), monocular observations:
 * one VertexSE3Expmap (Tcw), EdgeSE3ProjectXYZOnlyPose per matched MapPoint (information
 * I * mvInvLevelSigma2[octave], Huber sqrt(5.991)), 4 rounds of Levenberg optimize(10) each
 * from the frame's initial pose, chi2 > 5.991 -> outlier after every round, robust kernel
 * dropped after round 2, early stop after round 0 for < 10 edges. The adapter fills one
 * problem per Frame from its mvpMapPoints (non-NULL entries, mvuRight < 0) and writes back
 * SetPose(result) and mvbOutlier[i] = outlier[k]. Returns nInitialCorrespondences - nBad
 * (0, pose untouched, when < 3 correspondences). */
typedef struct {
    int32_t n;                  /* correspondences */
    const float* pose_q;        /* 4: initial Tcw rotation (x, y, z, w) = pFrame->GetPose() */
    const float* pose_t;        /* 3 */
    const float* points;        /* n x 3: MapPoint::GetWorldPos() */
    const float* uv;            /* n x 2: mvKeysUn[i].pt */
    const int32_t* octave;      /* n: mvKeysUn[i].octave */
    const float* inv_sigma2;    /* per octave: mvInvLevelSigma2 */
    int32_t n_octaves;
    float fx, fy, cx, cy;       /* Pinhole mvParameters */
} orbhip_pose_problem;

typedef struct {
    float pose_q[4];            /* optimised Tcw */
    float pose_t[3];
    uint8_t* outlier;           /* n out (caller-owned, may be NULL): mvbOutlier */
    int32_t n_inliers;          /* PoseOptimization return value */
    int32_t lm_trials;          /* total Levenberg trials over the 4 rounds */
} orbhip_pose_result;

int orbhip_pose_optimization(orbhip_ctx* ctx, const orbhip_pose_problem* prob, orbhip_pose_result* res);
/* B frames (e.g. every camera of a rig, or a batch of agents) in one launch, one wavefront each. */
int orbhip_pose_optimization_batch(orbhip_ctx* ctx, const orbhip_pose_problem* probs, int B,
                                   orbhip_pose_result* res);

/* PoseOptimization of a rectified-stereo Frame, as upstream builds the problem: observation i
 * with u_right[i] >= 0 (mvuRight; 0.0f counts) is an EdgeStereoSE3ProjectXYZOnlyPose (obs (u, v,
 * u_right), projection (fx x/z + cx, fy y/z + cy, fx x/z + cx - bf/z), information
 * I3 * mvInvLevelSigma2[octave], Huber sqrt(7.815), outlier iff chi2 > 7.815), every other
 * observation the monocular edge above, unchanged. Rounds, early stop and return value as
 * orbhip_pose_optimization. ORBHIP_ERR_ARG (before anything runs, no result written) when u_right
 * is NULL with n > 0, an octave is out of range, or bf <= 0 while some u_right[i] >= 0. */
typedef struct {
    int32_t n;                  /* correspondences */
    const float* pose_q;        /* 4 */
    const float* pose_t;        /* 3 */
    const float* points;        /* n x 3 */
    const float* uv;            /* n x 2 */
    const int32_t* octave;      /* n */
    const float* inv_sigma2;    /* per octave */
    int32_t n_octaves;
    float fx, fy, cx, cy;
    const float* u_right;       /* n: mvuRight[i] (< 0: monocular observation) */
    float bf;                   /* mbf = baseline * fx */
} orbhip_pose_stereo_problem;
int orbhip_pose_optimization_stereo(orbhip_ctx* ctx, const orbhip_pose_stereo_problem* prob, orbhip_pose_result* res);
int orbhip_pose_optimization_stereo_batch(orbhip_ctx* ctx, const orbhip_pose_stereo_problem* probs, int B,
                                          orbhip_pose_result* res);

/* ---- bag of words -----------------------------------------
 * DBoW2 vocabulary in the ORBvoc.txt node order (Thirdparty/DBoW2 TemplatedVocabulary):
 * node 0 = root, node i (i >= 1) = line i of the text file with (parent, is_leaf, 32-byte
 * descriptor, weight); children keep file order; word ids follow leaf order.
 *   orbhip_vocab_load_text   TemplatedVocabulary::loadFromTextFile ("k L scoring weighting" header)
 *   orbhip_bow_transform     per-descriptor transform(feature, word, weight, &node, levelsup)
 *                            (U:src/Frame.cc::ComputeBoW: levelsup 4); the caller builds the
 *                            BowVector (weights summed per word, L1-normalised) and FeatureVector
 *                            (node -> ascending feature indices, weight > 0 only)
 *   orbhip_search_bow        U:src/ORBmatcher.cc::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches):
 *                            match[f] = KF feature index matched to frame feature f, or -1 (the
 *                            adapter maps it to the KF's MapPoint*); kf_valid[i] = the KF feature
 *                            has a good map point. Returns nmatches. n <= 2048 per side. */
typedef struct orbhip_vocab orbhip_vocab;
int orbhip_vocab_create(orbhip_ctx* ctx, int k, int L, int scoring, int weighting, int n_nodes,
                        const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc32,
                        const double* weight, orbhip_vocab** out);
int orbhip_vocab_load_text(orbhip_ctx* ctx, const char* path, orbhip_vocab** out);
int orbhip_vocab_destroy(orbhip_vocab* vocab);
int orbhip_vocab_info(const orbhip_vocab* vocab, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words);
int orbhip_bow_transform(orbhip_ctx* ctx, const orbhip_vocab* vocab, const uint8_t* desc32, int n, int levelsup,
                         int32_t* word_id, int32_t* node_id, double* weight);
/* device form over extractor outputs: B frames, descriptors at f*cap, counts d_n[f]; outputs at f*cap */
int orbhip_bow_transform_device(orbhip_ctx* ctx, const orbhip_vocab* vocab, const uint8_t* d_desc,
                                const int32_t* d_n, int B, int cap, int levelsup, int32_t* d_word,
                                int32_t* d_node, double* d_weight, void* stream);
int orbhip_search_bow(orbhip_ctx* ctx, const uint8_t* kf_desc, const float* kf_angle, const int32_t* kf_node,
                      const double* kf_weight, const uint8_t* kf_valid, int nkf, const uint8_t* f_desc,
                      const float* f_angle, const int32_t* f_node, const double* f_weight, int nf,
                      float ratio, int check_orientation, int th_low, int32_t* match);

/* ---- new map points: SearchForTriangulation -------------------------
 * U:src/ORBmatcher.cc::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo = false,
 * bCoarse = false), as U:src/LocalMapping.cc::CreateNewMapPoints calls it (ORBmatcher(0.6, false))
 * once per covisible neighbour: monocular, one pinhole camera per keyframe, mvKeysUn. KF1 is
 * matched against B neighbours in one call. Per shared FeatureVector node, every KF1 feature
 * without a MapPoint takes the KF2 feature without a MapPoint of least descriptor distance
 * (<= TH_LOW = 50; of equal distances the highest index) among those that are not within
 * 10 * sqrt(mvScaleFactors[octave2]) px of the epipole and lie within 3.84 * mvLevelSigma2[octave2]
 * of the epipolar line x1^T F12. No ratio test; several KF1 features may share one KF2 feature
 * (vbMatched2 is never set upstream). With check_orientation the rotation histogram
 * (HISTO_LENGTH 30, ComputeThreeMaxima) drops matches outside the main bins. DESIGN.md fixes the
 * fp32 operation order of the geometry and of every gate. */
typedef struct {
    int32_t n;                 /* <= 2048 */
    const orbhip_kp* kps;      /* mvKeysUn */
    const uint8_t* desc;       /* n x 32 */
    const int32_t* node;       /* orbhip_bow_transform node ids (levelsup 4), -1 = none */
    const double* weight;      /* > 0: in the FeatureVector */
    const uint8_t* has_mp;     /* GetMapPoint(i) != NULL */
    float fx, fy, cx, cy;
    float pose_q[4], pose_t[3];/* Tcw, (x, y, z, w) as orbhip_frame */
} orbhip_tri_keyframe;

/* host only, no context: the per-pair geometry the kernel consumes. F12 row-major
 * (K1^-T [t12]x R12 K2^-1 with closed-form K^-1), ep = KF1's camera centre in image 2. Only the
 * intrinsics and poses of the two keyframes are read. */
int orbhip_triangulation_geometry(const orbhip_tri_keyframe* kf1, const orbhip_tri_keyframe* kf2,
                                  float F12[9], float ep[2]);

/* KF1 against B neighbours in one call. match12: B x kf1->n (idx2 or -1), nmatches: B.
 * Returns the sum of nmatches. n > 2048 on either side or B > 64: ORBHIP_ERR_UNSUPPORTED; a
 * keypoint octave outside [0, n_levels): ORBHIP_ERR_ARG. One upload, one launch pair (KF1's
 * FeatureVector ordered once, then one work-group per neighbour), one read-back. */
int orbhip_search_for_triangulation(orbhip_ctx* ctx, const orbhip_tri_keyframe* kf1,
                                    const orbhip_tri_keyframe* nbrs, int B,
                                    const float* scale_factors, const float* level_sigma2, int n_levels,
                                    int check_orientation, int32_t* match12, int32_t* nmatches);

/* ---- new map points: the triangulation of CreateNewMapPoints ----------
 * U:src/LocalMapping.cc::CreateNewMapPoints after SearchForTriangulation, monocular: per neighbour
 * the baseline / median-depth gate, per matched pair the parallax, GeometricTools::Triangulate,
 * the depth, reprojection (5.991 * mvLevelSigma2), distance and scale-ratio checks, in the order
 * and arithmetic DESIGN.md "CreateNewMapPoints" fixes (fp32 in a fixed order; the null vector of
 * the 4x4 system by an fp64 one-sided Jacobi). status per (neighbour, KF1 feature): 0 no match,
 * 1 accepted, 2 cosParallax <= 0, 3 parallax too low, 4 null vector with w == 0, 5 / 6 not in
 * front of KF1 / KF2, 7 / 8 reprojection error in KF1 / KF2, 9 on a camera centre, 10 beyond
 * far_threshold, 11 scale ratio. Every status is that of the state at call time. A KF1 feature
 * accepted by several neighbours becomes ONE new point, that of the first such neighbour
 * (first[idx1]): with check_orientation = 0 this is upstream's sequential result, where a feature
 * triangulated with one neighbour has a MapPoint when the next neighbour is searched. The new
 * points are listed in upstream's creation order: ascending neighbour, then ascending idx1. */
typedef struct {
    double cos_parallax_max;   /* 0.9998 (0.9996 in the inertial mode) */
    float ratio_factor;        /* 1.5f * mfScaleFactor */
    float far_threshold;       /* mThFarPoints; <= 0: off */
} orbhip_tri_params;

typedef struct {               /* caller-allocated; optional members may be NULL */
    int32_t* match12;          /* B x n1, optional */
    int32_t* nmatches;         /* B */
    uint8_t* gated;            /* B: 1 = baseline / median depth below 0.01, neighbour not searched */
    uint8_t* status;           /* B x n1, optional */
    float* x3d_all;            /* B x n1 x 3, optional: the point of every pair whose status is 1 or >= 5
                                  (zeros elsewhere); diagnostics and tests, not copied back when NULL */
    int32_t* first;            /* n1: the first neighbour that accepts the feature, or -1 */
    int32_t* nnew;             /* B: new points per neighbour */
    int32_t* new_nbr;          /* n1 entries each; the first <return value> are the list, */
    int32_t* new_idx1;         /* the rest -1 (new_x3d: n1 x 3, the rest 0) */
    int32_t* new_idx2;
    float* new_x3d;
} orbhip_new_points;

/* SearchForTriangulation of KF1 against the B neighbours and the triangulation of its matches in
 * one call: one upload, the kernels back to back on the context's stream (match12 never leaves
 * the device in between), one read-back. median_depth: B values (KF2's ComputeSceneMedianDepth(2))
 * or NULL = no neighbour is gated; a gated neighbour is not uploaded. Returns the number of new
 * points. The envelope and the error codes are those of orbhip_search_for_triangulation. */
int orbhip_create_new_map_points(orbhip_ctx* ctx, const orbhip_tri_keyframe* kf1,
                                 const orbhip_tri_keyframe* nbrs, int B, const float* median_depth,
                                 const float* scale_factors, const float* level_sigma2, int n_levels,
                                 int check_orientation, const orbhip_tri_params* params,
                                 orbhip_new_points* out);

/* The same from given matches (match12_in: B x n1, idx2 or -1): no search, no gating (gated = 0).
 * Only n, kps, the intrinsics and the pose of a keyframe are read (desc, node, weight, has_mp may
 * be NULL). An entry of match12_in outside [-1, n2): ORBHIP_ERR_ARG. */
int orbhip_triangulate_matches(orbhip_ctx* ctx, const orbhip_tri_keyframe* kf1,
                               const orbhip_tri_keyframe* nbrs, int B, const int32_t* match12_in,
                               const float* scale_factors, const float* level_sigma2, int n_levels,
                               const orbhip_tri_params* params, orbhip_new_points* out);

/* ---- new map points of a rectified-stereo system ---------------------------------------
 * The stereo branches of SearchForTriangulation (bOnlyStereo = false, bCoarse = false) and of
 * CreateNewMapPoints (DESIGN.md "Stereo LocalMapping"). A keyframe carries u_right = mvuRight and
 * depth = mvDepth per feature and bf = mbf, b = mb; a feature is stereo when u_right >= 0 (0.0f
 * counts). Differences from the monocular calls above, everything else being their rule:
 *  - search: the epipole exclusion applies only when neither feature is stereo;
 *  - neighbour b is gated when baseline < nbrs[b].b (there is no median_depth);
 *  - per pair: with cosS the stereo parallax of the features (feature 1's when it is stereo, else
 *    feature 2's) the point is triangulated when cosP < cosS && cosP > 0 && (a feature is stereo ||
 *    cosP < cos_parallax_max); else unprojected from KF1 (feature 1 stereo and the better stereo
 *    parallax) or from KF2; else status 2 / 3. Unprojecting a feature with depth <= 0 (or NaN):
 *    status 12;
 *  - the reprojection test of a stereo feature is (eX, eY, eR) against 7.8 * mvLevelSigma2
 *    (status 7 / 8), eR = (u - bf / z) - u_right.
 * source (B x n1, optional): 0 no point, 1 triangulated, 2 / 3 unprojected from KF1 / KF2.
 * Envelopes and errors of the monocular calls; also ORBHIP_ERR_ARG, before anything is uploaded or
 * launched, when u_right or depth is NULL with n > 0, or bf <= 0 or b <= 0, in any keyframe. With
 * every u_right < 0 and b below every baseline they compute what the monocular calls compute
 * without median_depth. */
typedef struct {
    orbhip_tri_keyframe kf;
    const float* u_right;      /* kf.n: mvuRight */
    const float* depth;        /* kf.n: mvDepth */
    float bf, b;               /* mbf, mb */
} orbhip_tri_stereo_keyframe;
int orbhip_search_for_triangulation_stereo(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe* kf1,
                                           const orbhip_tri_stereo_keyframe* nbrs, int B,
                                           const float* scale_factors, const float* level_sigma2, int n_levels,
                                           int check_orientation, int32_t* match12, int32_t* nmatches);
int orbhip_create_new_map_points_stereo(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe* kf1,
                                        const orbhip_tri_stereo_keyframe* nbrs, int B,
                                        const float* scale_factors, const float* level_sigma2, int n_levels,
                                        int check_orientation, const orbhip_tri_params* params,
                                        orbhip_new_points* out, uint8_t* source /* B x n1 or NULL */);
int orbhip_triangulate_matches_stereo(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe* kf1,
                                      const orbhip_tri_stereo_keyframe* nbrs, int B, const int32_t* match12_in,
                                      const float* scale_factors, const float* level_sigma2, int n_levels,
                                      const orbhip_tri_params* params, orbhip_new_points* out,
                                      uint8_t* source /* B x n1 or NULL */);

/* ---- map point fusion: Fuse ------------------------------------------
 * U:src/ORBmatcher.cc::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th,
 * bRight = false), as U:src/LocalMapping.cc::SearchInNeighbors calls it: monocular, one pinhole
 * camera, mvKeysUn, no stereo coordinate (orbhip_fuse_stereo below is the stereo branch). B
 * keyframes are searched for the same list of MapPoints in one call. Per (keyframe b, MapPoint m)
 * not skipped: the point is projected with Tcw (quaternion form), must lie in front of the
 * camera, inside the image (IsInImage: the maximum is strict),
 * within [0.8 mfMinDistance, 1.2 mfMaxDistance] of the camera centre and within 60 degrees of its
 * normal; PredictScale gives the level, th * mvScaleFactors[level] the window of
 * KeyFrame::GetFeaturesInArea; a candidate keypoint needs octave in [level - 1, level] and a squared
 * reprojection error e2 with e2 * inv_level_sigma2[octave] <= 5.99; of the candidates the one of
 * least descriptor distance wins (the first in the reference's walk order among equals) and is
 * accepted at distance <= TH_LOW = 50. No pair reads state another pair writes: the call sees every
 * MapPoint as it is at call time, and the adapter applies Replace / AddObservation / AddMapPoint in
 * upstream order. DESIGN.md fixes the fp32 operation order of every gate.
 *
 * kfs[b]: mvKeysUn, descriptors, image bounds, scale tables, intrinsics, Tcw; claimed is ignored
 * (the adapter looks pKF->GetMapPoint(best_idx) up itself). All keyframes of a call share n_levels,
 * scale_factors (by value) and log_scale_factor, else ORBHIP_ERR_ARG. mps->skip[m] = !pMP ||
 * pMP->isBad(); pair_skip[b * n + m] = pMP->IsInKeyFrame(kf b) (NULL: none).
 * Outputs, B x mps->n: best_idx = the keypoint of keyframe b the point fuses into, or -1;
 * best_dist (optional) = the least distance over the gated candidates, 256 without one, reported
 * even above 50; level (optional) = nPredictedLevel, -1 when the point was skipped or rejected before
 * PredictScale. nfused[b] = accepted points of keyframe b; returns their sum. B = 0 or n = 0: 0.
 * B > 64, mps->n > 65536, a keyframe of more than 65535 keypoints or n_levels > 256:
 * ORBHIP_ERR_UNSUPPORTED; a keypoint octave outside [0, n_levels): ORBHIP_ERR_ARG. One upload, two
 * launches (the keyframes' grids, the search), one read-back. */
int orbhip_fuse(orbhip_ctx* ctx, const orbhip_frame* kfs, int B, const orbhip_local_points* mps,
                const uint8_t* pair_skip /* B x mps->n or NULL: IsInKeyFrame(kf b) */,
                const float* inv_level_sigma2 /* n_levels */, float th,
                int32_t* best_idx /* B x n */, int32_t* best_dist /* B x n or NULL */,
                int32_t* level /* B x n or NULL */, int32_t* nfused /* B */);

/* Fuse on rectified-stereo keyframes (the stereo branch of the same upstream function, bRight =
 * false): kfs[b] = the keyframe as orbhip_fuse takes it plus u_right = mvuRight, bf = mbf, b = mb.
 * Everything is the rule of orbhip_fuse except the chi-square gate of a candidate keypoint k with
 * u_right[k] >= 0 (0.0f counts): with invz = 1.0f / Pc.z and er = (u - bf * invz) - u_right[k] the
 * candidate needs ((ex^2 + ey^2) + er^2) * inv_level_sigma2[octave] <= 7.8. A candidate with
 * u_right[k] < 0 (or NaN) takes the two-term test at 5.99; the window has no right-coordinate gate
 * (DESIGN.md "Stereo LocalMapping"). Arguments, outputs, envelope and errors of orbhip_fuse; also
 * ORBHIP_ERR_ARG, before anything is uploaded or launched, when u_right is NULL with n > 0 or bf <= 0
 * or b <= 0 in any keyframe. With every u_right < 0 it computes what orbhip_fuse computes. Fuse with a
 * Sim3 has no chi-square gate and therefore no stereo form. */
int orbhip_fuse_stereo(orbhip_ctx* ctx, const orbhip_stereo_view* kfs, int B, const orbhip_local_points* mps,
                       const uint8_t* pair_skip /* B x mps->n or NULL */,
                       const float* inv_level_sigma2 /* n_levels */, float th,
                       int32_t* best_idx /* B x n */, int32_t* best_dist /* B x n or NULL */,
                       int32_t* level /* B x n or NULL */, int32_t* nfused /* B */);

/* ---- LoopClosing: Fuse and SearchByProjection with a Sim3 ------------------------------
 * U:src/ORBmatcher.cc::Fuse(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
 * float th, vector<MapPoint*>& vpReplacePoint) (LoopClosing::SearchAndFuse, th = 4) and
 * ::SearchByProjection(KeyFrame* pKF, Sophus::Sim3<float>& Scw, const vector<MapPoint*>& vpPoints,
 * vector<MapPoint*>& vpMatched, int th, float ratioHamming) (DetectCommonRegionsFromBoW,
 * DetectAndReffineSim3FromLastKF, FindMatchesByProjection; also the overload with vpPointsKFs /
 * vpMatchedKF, which computes the same). Both decompose Scw first: the adapter passes
 * Tcw = (Scw.rotationMatrix(), Scw.translation() / Scw.scale()) in pose_q / pose_t and the library
 * never sees the scale. Per (keyframe, point) the gates are those of orbhip_fuse up to
 * the window of GetFeaturesInArea and the octave in [level - 1, level]; there is NO chi-square gate.
 *
 * orbhip_fuse_sim3: arguments, outputs, envelope and errors of orbhip_fuse without inv_level_sigma2;
 * it computes what orbhip_fuse computes with an all-zero inv_level_sigma2. mps->skip[m] = isBad(),
 * pair_skip[b * n + m] = pKF_b->GetMapPoints().count(pMP). The adapter fills vpReplacePoint[m] from
 * pKF->GetMapPoint(best_idx) or calls AddObservation / AddMapPoint, in upstream order.
 *
 * orbhip_search_by_projection_sim3: one keyframe. kf->claimed[k] = vpMatched[k] != NULL at call time
 * (NULL: none); mps->skip[m] = isBad() || pMP is in vpMatched at call time (spAlreadyFound). The
 * sequential greedy pass of upstream, exactly: for m ascending, of the gated candidates whose
 * keypoint is claimed neither at call time nor by an earlier point of this call, the one of least
 * descriptor distance (the first in the reference's walk order among equals); if (float)distance <=
 * 50.0f * ratio_hamming the point claims it. match[m] = that keypoint or -1 (the adapter sets
 * vpMatched[match[m]] = pMP, or vpMatchedKF[match[m]] = vpPointsKFs[m]); match_dist (optional) = its
 * distance, 256 when -1; level (optional) as orbhip_fuse. Returns nmatches; n = 0: 0.
 * ratio_hamming not positive and finite: ORBHIP_ERR_ARG. mps->n > 65536, more than 65535 keypoints or
 * n_levels > 256: ORBHIP_ERR_UNSUPPORTED; a keypoint octave outside [0, n_levels): ORBHIP_ERR_ARG. One
 * upload, three launches (the grid, the candidate lists, the greedy pass as a fixed point in one
 * work-group), one read-back. */
int orbhip_fuse_sim3(orbhip_ctx* ctx, const orbhip_frame* kfs, int B, const orbhip_local_points* mps,
                     const uint8_t* pair_skip /* B x mps->n or NULL */, float th,
                     int32_t* best_idx /* B x n */, int32_t* best_dist /* B x n or NULL */,
                     int32_t* level /* B x n or NULL */, int32_t* nfused /* B */);
int orbhip_search_by_projection_sim3(orbhip_ctx* ctx, const orbhip_frame* kf, const orbhip_local_points* mps,
                                     float th, float ratio_hamming, int32_t* match /* n */,
                                     int32_t* match_dist /* n or NULL */, int32_t* level /* n or NULL */);

/* ---- LoopClosing: Sim3Solver (Horn's closed form on RANSAC triples) -------------------
 * U:src/Sim3Solver.cc (LoopClosing::DetectCommonRegionsFromBoW, between SearchByBoW and
 * SearchByProjection(Scw)). Every hypothesis of every candidate keyframe in one call: the
 * hypotheses are independent once their triples are drawn, and upstream's sequential rule ("the
 * first above mRansacMinInliers converges, else the best so far") is applied afterwards in its
 * order-free form, with the same result (DESIGN.md "Sim3Solver" has the operation order).
 *
 * A problem is what upstream's constructor prepares: the n correspondences its filter leaves, X1 /
 * X2 = the map points in the frames of camera 1 / 2 (Rcw Xw + tcw), the two pinhole cameras as
 * (fx, fy, cx, cy), and the error bounds mvnMaxError1 / 2. QUIRK: upstream keeps 9.210 *
 * sigma2[octave] in a vector<size_t>, so its bound is that product TRUNCATED to an integer; the
 * adapter passes max_err = (float)(size_t)(9.210 * (double)sigma2). The library only compares
 * against the bound. min_inliers = mRansacMinInliers, fix_scale = mbFixScale. The library draws no
 * random numbers: triples holds n_hyp triples of indices into [0, n), drawn by the caller as
 * upstream draws them.
 *
 * Per hypothesis h: ComputeSim3 on the triple in fp32 (the rotation from the eigenvector of Horn's
 * 4x4 matrix, computed by a fixed number of fp64 Jacobi sweeps and converted through the
 * quaternion, not through atan2 / the angle-axis vector), then CheckInliers over all n
 * correspondences: an inlier iff both squared reprojection errors are BELOW their bounds; there is
 * no depth test. A degenerate triple gives NaN or inf, which fail every comparison: 0 inliers, no
 * special case. n_inliers[h] = the count, hyp[13 h ..] = (s, R row-major, t) of T12 = [s R | t].
 * Selection, for h ascending as upstream's iterate(): converged = the first h with n_inliers[h] >
 * min_inliers, or -1; best = converged, or without one the LAST h of the largest count (upstream
 * replaces the best on >=, and a count of 0 qualifies). sel and inliers (one byte per
 * correspondence) are those of hypothesis `best`.
 *
 * Returns the number of problems that converged. B = 0: 0. B > 64, n > 8192 or n_hyp > 4096:
 * ORBHIP_ERR_UNSUPPORTED. ORBHIP_ERR_ARG, before anything is uploaded and with no output touched: n <
 * 3, n_hyp < 1, a NULL required pointer, a triple index outside [0, n) or repeated within its triple,
 * a focal length that is not positive and finite, min_inliers < 0. One upload, two launches, one
 * read-back. */
typedef struct {
    float cam1[4], cam2[4];        /* fx, fy, cx, cy */
    int32_t n;                     /* correspondences */
    const float* X1;               /* n x 3 */
    const float* X2;               /* n x 3 */
    const float* max_err1;         /* n: the truncated bounds (above) */
    const float* max_err2;         /* n */
    int32_t fix_scale;
    int32_t min_inliers;
    int32_t n_hyp;
    const int32_t* triples;        /* n_hyp x 3 */
} orbhip_sim3_problem;

typedef struct {                   /* the pointers are the caller's */
    int32_t* n_inliers;            /* n_hyp */
    float* hyp;                    /* n_hyp x 13, or NULL */
    uint8_t* inliers;              /* n, or NULL */
    float sel[13];                 /* (s, R row-major, t) of hypothesis `best` */
    int32_t converged;             /* hypothesis index, or -1 */
    int32_t best;
} orbhip_sim3_result;

int orbhip_sim3_solve_batch(orbhip_ctx* ctx, const orbhip_sim3_problem* probs, int B, orbhip_sim3_result* res);
/* B = 1 */
int orbhip_sim3_solve(orbhip_ctx* ctx, const orbhip_sim3_problem* prob, orbhip_sim3_result* res);

/* ---- Tracking: TwoViewReconstruction (monocular initialisation) --------------------------
 * U:src/TwoViewReconstruction.cc (Tracking::MonocularInitialization, between SearchForInitialization
 * and CreateInitialMapMonocular). Both RANSACs (homography and fundamental matrix), the model
 * choice, the motion hypotheses and their CheckRT for every frame pair of a call (DESIGN.md
 * "TwoViewReconstruction" has the operation order).
 *
 * A problem is what upstream's Reconstruct receives: the undistorted keypoints of the two frames
 * (only x and y are read), matches12 = vMatches12 (n1 entries, -1 = unmatched), K as (fx, fy, cx,
 * cy), sigma = mSigma and n_hyp = mMaxIterations. mvMatches12 is the list of pairs (i, matches12[i])
 * with a match, in index order; N is its length. The library draws no random numbers: sets holds
 * n_hyp sets of 8 indices into [0, N), drawn by the caller as upstream draws them.
 *
 * Per set h and model: Normalize (once per problem, upstream's running fp32 sums), ComputeH21 /
 * ComputeF21 with the null vector from a fixed number of fp64 Jacobi sweeps on the system's 9x9 Gram
 * matrix, CheckHomography / CheckFundamental over all N matches in fp32. The score is the sum of
 * upstream's fp32 terms, added in fp64 (exact, hence order-free) and rounded once. best_h / best_f =
 * the first hypothesis whose score is above every earlier one, from 0 (-1: none; a NaN score never
 * wins); SH / SF its score, H21 / F21 its matrix, inliers_h / inliers_f (optional, N bytes, by match)
 * its vbMatchesInliers. model = 0 (H) when SH / (SH + SF) > 0.50, else 1 (F); -1 when SH + SF == 0,
 * which fails. ReconstructH (the eight Faugeras hypotheses, none at the d1/d2, d2/d3 exit) or
 * ReconstructF (the four of DecomposeE) with minParallax = 1.0 and minTriangulated = 50: per motion
 * hypothesis m CheckRT gives n_good[m], cos_sel[m] (the min(50, n_good - 1)-th smallest cosine, by
 * counting) and parallax[m] in degrees (through the device's acosf); chosen = the accepted
 * hypothesis or -1. On success R21 / t21 are its motion, p3d[3 i ..] the point of keypoint i of
 * frame 1 where CheckRT counted it (0 elsewhere) and triangulated[i] = vbTriangulated[i]; on failure
 * R21, t21, p3d and triangulated are 0.
 *
 * Returns the number of problems that succeeded. B = 0: 0. B > 64, N > 8192 or n_hyp > 4096:
 * ORBHIP_ERR_UNSUPPORTED. ORBHIP_ERR_ARG, before anything is uploaded and with no output touched: N <
 * 8, n_hyp < 1, a NULL required pointer, a matches12 entry outside [-1, n2), a set index outside
 * [0, N) or repeated within its set, a focal length or sigma that is not positive and finite. One
 * upload, four launches, one read-back. */
typedef struct {
    int32_t n1, n2;                /* keypoints of frame 1 / 2 */
    const orbhip_kp* kps1;         /* n1, undistorted */
    const orbhip_kp* kps2;         /* n2 */
    const int32_t* matches12;      /* n1: index into kps2, or -1 */
    float K[4];                    /* fx, fy, cx, cy */
    float sigma;
    int32_t n_hyp;
    const int32_t* sets;           /* n_hyp x 8 */
} orbhip_two_view_problem;

typedef struct {                   /* the pointers are the caller's */
    float* p3d;                    /* n1 x 3 */
    uint8_t* triangulated;         /* n1 */
    uint8_t* inliers_h;            /* N, or NULL */
    uint8_t* inliers_f;            /* N, or NULL */
    int32_t success;
    int32_t model;                 /* 0 = H, 1 = F, -1 = neither */
    int32_t best_h, best_f;        /* hypothesis index, or -1 */
    int32_t chosen;                /* motion hypothesis index, or -1 */
    float SH, SF;
    float H21[9], F21[9];          /* row-major */
    float R21[9], t21[3];
    int32_t n_good[8];
    float parallax[8];
    float cos_sel[8];
} orbhip_two_view_result;

int orbhip_two_view_reconstruct_batch(orbhip_ctx* ctx, const orbhip_two_view_problem* probs, int B,
                                      orbhip_two_view_result* res);
/* B = 1 */
int orbhip_two_view_reconstruct(orbhip_ctx* ctx, const orbhip_two_view_problem* prob, orbhip_two_view_result* res);

/* ---- LoopClosing: Optimizer::OptimizeSim3 (the Sim3 refinement between the two projection searches)
 * U:src/Optimizer.cc::OptimizeSim3 (LoopClosing::DetectCommonRegionsFromBoW step 4 and the end of
 * DetectAndReffineSim3FromLastKF). One VertexSim3Expmap S12 = (r, t, s), map(X) = s r X + t; per kept
 * correspondence an EdgeSim3ProjectXYZ (obs1 - cam1.project(S12.map(X2c)), information
 * inv_sigma2_1) and an EdgeInverseSim3ProjectXYZ (obs2 - cam2.project(S12^-1.map(X1c)),
 * inv_sigma2_2), both Huber (float)sqrt(th2), with g2o's numeric Jacobians (central differences,
 * 1e-9). optimize(5); pairs with either chi2 > th2 are removed (n_bad; the chi2 of the last
 * computeActiveErrors that saw the edge) and the kernels dropped; n - n_bad < 10 returns 0 with
 * S12 untouched; optimize(n_bad > 0 ? 10 : 5); pairs with either recomputed chi2 > th2 are cleared,
 * the others counted in n_in. DESIGN.md "OptimizeSim3" has the operation order.
 *
 * A problem is what upstream's filter loop leaves: X1c / X2c = the map points
 * in the frames of camera 1 / 2 (float products Rcw Xw + tcw), obs1 / obs2 as upstream sets them
 * (obs2 of a match without a keypoint in KF2 is the NORMALISED x / z, y / z: upstream's quirk,
 * kept by the adapter), the information values already looked up per correspondence, the two
 * pinhole cameras as (fx, fy, cx, cy), and g2oS12 in double: the rotation as the quaternion
 * q = (x, y, z, w) of Eigen::Quaterniond(R) (taken as given, not normalised, as g2o::Sim3 holds it),
 * t and s. LoopClosing passes th2 = 10.
 *
 * keep[i] (caller-owned, may be NULL) = 1 where the match survives, 0 where upstream sets
 * vpMatches1[idx] = NULL. lm_trials counts the Levenberg trials of both rounds. mAcumHessian is
 * zero upstream (its accumulation is commented out) and is not returned.
 *
 * orbhip_optimize_sim3_batch returns ORBHIP_OK, orbhip_optimize_sim3 n_in (upstream's return
 * value). n = 0: n_in = 0 and S12 copied through. B = 0: ORBHIP_OK. B > 64 or n > 8192:
 * ORBHIP_ERR_UNSUPPORTED. ORBHIP_ERR_ARG, before anything is uploaded and with no output touched: a NULL
 * required pointer with n > 0, n < 0, a focal length, th2 or s that is not positive and finite, a
 * non-finite q or t. One upload, one launch, one read-back. */
typedef struct {
    int32_t n;                     /* correspondences */
    const float* X1c;              /* n x 3 */
    const float* X2c;              /* n x 3 */
    const float* obs1;             /* n x 2 */
    const float* obs2;             /* n x 2 */
    const float* inv_sigma2_1;     /* n */
    const float* inv_sigma2_2;     /* n */
    float cam1[4], cam2[4];        /* fx, fy, cx, cy */
    double q[4];                   /* S12 rotation, quaternion (x, y, z, w) */
    double t[3];
    double s;
    double th2;
    int32_t fix_scale;
} orbhip_sim3_opt_problem;

typedef struct {
    double q[4], t[3], s;          /* the optimised S12 (the input where n_in = 0 by the < 10 rule) */
    int32_t n_in;                  /* upstream's return value */
    int32_t n_bad;                 /* pairs removed after the first round */
    int32_t lm_trials;
    uint8_t* keep;                 /* n, or NULL; the caller's */
} orbhip_sim3_opt_result;

int orbhip_optimize_sim3_batch(orbhip_ctx* ctx, const orbhip_sim3_opt_problem* probs, int B,
                               orbhip_sim3_opt_result* res);
/* B = 1; returns n_in */
int orbhip_optimize_sim3(orbhip_ctx* ctx, const orbhip_sim3_opt_problem* prob, orbhip_sim3_opt_result* res);

/* ---- LoopClosing: OptimizeEssentialGraph (CorrectLoop, MergeLocal) -------------------
 * U:src/Optimizer.cc::Optimizer::OptimizeEssentialGraph on the device: the 7-dof pose graph over the
 * keyframes of a map. The adapter builds the graph from the Map; the library receives
 * arrays only, so one call serves both upstream overloads: the caller decides which vertices are fixed
 * (CorrectLoop: the map's initial keyframe; MergeLocal: its list of fixed keyframes).
 * OptimizeEssentialGraph4DoF is not covered.
 *
 * Vertices are VertexSim3Expmap: the estimate (q xyzw, t, s) as g2o::Sim3, never renormalised, one
 * fix_scale for the graph (oplus(u): u[6] = 0, estimate = Sim3(u) * estimate). Edges are
 * EdgeSim3(i, j, Sji) with vertex(0) = i, vertex(1) = j, information I7 and no robust kernel:
 * e = (Sji * Si * Sj^-1).log(), chi2 = e.e, g2o's numeric Jacobians (central differences of 1e-9;
 * a fixed vertex gets none). Several edges between one pair sum. BlockSolver_7_3 + Levenberg with
 * setUserLambdaInit(lambda_init): initializeOptimization(); computeActiveErrors();
 * optimize(iterations); each trial is one solve of (H + lambda I) x = b over the free vertices, a
 * failed pivot a rejected trial. Then every map point m: P' = Swc_corrected[ref].map(Scw_before[ref]
 * .map(P)), Scw_before the vertex's input estimate, Swc_corrected the inverse of its optimised one,
 * in double, P float in and out.
 *
 * The library does not reorder: H's blocks follow the caller's vertex order. Keyframe-id order keeps
 * the spanning-tree and covisibility blocks near the diagonal and puts the loop edges' rows last,
 * where their fill is cheap. solver reports the linear solver: 0 the persistent tiled solver, 1 the
 * blocked one (7 x free vertices < 70, or ORBHIP_EG_BLOCKED=1 in the environment), 2 the blocked one
 * after a hand-off timeout of the persistent one (the call ran again).
 *
 * Envelope: 7 x free vertices <= 4096 (585 free vertices), n_edges <= 65536, n_points <= 2^22,
 * n_vertices <= 65535; beyond it ORBHIP_ERR_UNSUPPORTED. ORBHIP_ERR_ARG, before anything is uploaded
 * and with no output touched: a NULL required pointer, a negative count, an edge index out of range
 * or i == j, a point_ref out of range, an estimate or measurement that is not finite or whose s is
 * not positive, lambda_init <= 0, iterations < 0. n_edges = 0, iterations = 0 or no free vertex: the
 * estimates are copied through and the points still corrected (by the identity), ORBHIP_OK.
 * Profile stage 15 brackets the call's launches (14 is no stage and stays refused). */
typedef struct {
    int32_t n_vertices;            /* caller's order, recommended: keyframe id */
    const double* S;               /* n_vertices x 8: q(x,y,z,w), t, s */
    const uint8_t* fixed;          /* n_vertices */
    int32_t n_edges;
    const int32_t* edge_ij;        /* n_edges x 2: vertex(0) = i, vertex(1) = j */
    const double* edge_S;          /* n_edges x 8: the measurement Sji */
    int32_t fix_scale, iterations; /* upstream: 20 */
    double lambda_init;            /* upstream: 1e-16; must be > 0 */
    int32_t n_points;              /* may be 0 */
    const float* points;           /* n_points x 3 */
    const int32_t* point_ref;      /* n_points: vertex index */
} orbhip_essential_graph_problem;

typedef struct {
    double* S;                     /* n_vertices x 8, the caller's: corrected Siw (fixed ones copied through bit for bit) */
    float* points;                 /* n_points x 3, the caller's, or NULL when n_points = 0 */
    double chi2_initial, chi2_final;
    int32_t iterations_run, lm_trials, lm_rejected;
    int32_t solver;                /* 0 dag, 1 blocked, 2 blocked after a timeout */
} orbhip_essential_graph_result;

int orbhip_optimize_essential_graph(orbhip_ctx* ctx, const orbhip_essential_graph_problem* prob,
                                    orbhip_essential_graph_result* res);

/* ---- multi-GPU BundleAdjustment (SURVEY.md §8e, C5 GlobalBundleAdjustment) --------
 * One process per GPU. Landmarks (with their edges) are partitioned across ranks; every rank
 * holds all poses. Per LM trial the ranks sum their Schur contributions (the reduced camera
 * system S, its right-hand side, Hpp, chi2 / scale terms) with RCCL all-reduces over xGMI, solve
 * the identical S redundantly and back-substitute their own landmarks; all ranks follow one LM
 * schedule and return identical poses.
 *   orbhip_comm_unique_id  rank 0 only; send the 128 bytes to every rank (any transport)
 *   orbhip_comm_init       collective over the ranks: creates the context's communicator
 *   orbhip_ba_solve_sharded  collective: this rank's shard (all poses, its landmarks/edges);
 *                            the stop flag is agreed on (max over ranks) at each iteration
 *   orbhip_ba_solve_sharded_segments  collective: this rank holds nlocal consecutive shards
 *                            (segments rank*nlocal .. rank*nlocal+nlocal-1 of nranks*nlocal; the
 *                            same nlocal on every rank, else ORBHIP_ERR_ARG); they are summed on
 *                            the device, then all-reduced over the ranks
 *   orbhip_ba_solve_shards_local  the same decomposition with all shards in one process on one
 *                            device (the sums run on the device): single-GPU model and test. */
int orbhip_comm_unique_id(uint8_t* id128);
int orbhip_comm_init(orbhip_ctx* ctx, int nranks, int rank, const uint8_t* id128);
int orbhip_ba_solve_sharded(orbhip_ctx* ctx, const orbhip_ba_problem* shard, orbhip_ba_result* res,
                            const volatile int* stop_flag);
int orbhip_ba_solve_sharded_segments(orbhip_ctx* ctx, const orbhip_ba_problem* shards, int nlocal,
                                     orbhip_ba_result* res, const volatile int* stop_flag);
int orbhip_ba_solve_shards_local(orbhip_ctx* ctx, const orbhip_ba_problem* shards, int nshards,
                                 orbhip_ba_result* res, const volatile int* stop_flag);

#ifdef __cplusplus
}
#endif
#endif /* ORBHIP_H */
