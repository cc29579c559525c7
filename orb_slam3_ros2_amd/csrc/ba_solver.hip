// gfx950 bundle adjustment: the g2o problem of Optimizer::LocalBundleAdjustment /
// BundleAdjustment (U:src/Optimizer.cc) solved with the Levenberg-Marquardt schedule of
// OptimizationAlgorithmLevenberg and the Schur complement of BlockSolver<6,3>.
//
// Batched: every kernel runs over grid.y = the problems (problem index from act[]), so B
// independent problems (SURVEY.md §8e "replicas": concurrent maps / agents, or a batch of local
// windows) share each launch. Every solve is device-driven: a slot advances every problem by one LM
// trial with no host round trip (the g2o control flow on the device, LmCtl). The sharded solves run
// the same slots with their collectives between the kernels and the controller's sums split from
// its decisions (BaArgs::sync). fp64 throughout:
//   k_ba_errors        EdgeSE3ProjectXYZ::computeError + RobustKernelHuber::robustify; in a trial
//                      its last workgroup per problem runs the LM controller step (ctl_end_body)
//   k_ba_lin           linearizeOplus + constructQuadraticForm: landmark side (Hll, b_l, the
//                      edge records) and pose side (Hpp, b_p, one wave per pose) in one launch;
//                      its last workgroup per problem starts the trial (ctl_begin_body)
//   k_ba_schur_points  setLambda on Hll, Dinv (Eigen 3x3 cofactor inverse), db
//   k_ba_schur_items   S_ij = [i==j](Hpp_i + lambda I) - sum W_a Hpl_b^T over shared landmarks,
//                      matrix-free; its trailing workgroups compute b_schur = b_p - sum Hpl db
//                      (a block of several items: its last item adds their partials in order)
//   k_chol_dag / k_ba_chol_reg / k_ba_cholesky / k_cb_*   the reduced camera system (ba_chol_*)
//   k_ba_backsub       xl = Dinv (b_l - Hpl^T xp), X += xl (push: old X saved)
//                      and T <- exp(xp) * T (SE3Quat::exp, operator*)   (push: old T saved)
//   k_ba_ctl_init / k_ba_reduce   the initial activeRobustChi2 (k_ba_reduce: a shard's part of it)
//   k_ba_pop           restore the pushed state of problems whose trial was rejected
// The host driver below the kernels is ba_solve_batch: a sequence of named steps over one per-call
// context (BaCall); the host-only problem preparation is ba_prep.cpp.
// The kernels that form an edge's error or Jacobians (k_ba_errors, k_ba_lin, k_ba_schur_items,
// k_ba_backsub, k_ba_backsub_errs) are templates on Stereo: false is the monocular problem
// (EdgeSE3ProjectXYZ alone, every entry point but the stereo ones), true adds the third row of
// EdgeStereoSE3ProjectXYZ on the edges with e_ur >= 0 (orbhip_ba_solve_stereo*, DESIGN.md §4
// "Stereo bundle adjustment").
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "orbhip_ba.h"
#include "dev_attr.h"
#include "ba_chol.h"
#include "ba_chol_blocked.h"
#include "ba_chol_dag.h"
#include "ba_nd.h"
#include "ba_args.h"
#include "ba_prep.h"
#include "ba_chol_reg.h"
#include "ba_se3.h"

namespace orbhip {


// struct BaArgs: ba_args.h


// Grid (X work-groups per problem, Y problems). Work-groups are dispatched round-robin over the
// 8 XCDs in linear order, so the plain (blockIdx.x, blockIdx.y) spreads every problem over all
// XCDs and each XCD's L2 streams every problem's arrays. Remapped, the X work-groups of problem p
// run on XCD p % 8 (for the first 8 floor(Y / 8) problems; the tail keeps the plain order), so a
// problem's Hpl / W / S stay in one L2. Speed only: correctness never depends on the placement.
__device__ __forceinline__ void ba_xcd_map(int& bx, int& by) {
    const int X = gridDim.x, Y = gridDim.y;
    const int id = blockIdx.x + X * blockIdx.y;
    const int Yf = Y & ~7;
    if (id < X * Yf) {
        const int k = id & 7, s = id >> 3;
        by = 8 * (s / X) + k;
        bx = s - (s / X) * X;
    } else {
        by = id / X;
        bx = id - by * X;
    }
}
#define BA_PROLOGUE                                 \
    int bx_, by_;                                   \
    ba_xcd_map(bx_, by_);                           \
    const BaArgs& a = args[act[by_]];

// A kernel runs for a problem only in the phase it belongs to (build: linearisation; trial: Schur /
// solve / update / errors); every problem has its controller (a.ctl).
__device__ __forceinline__ bool in_phase(const BaArgs& a, int ph) { return a.ctl->phase == ph; }
#define BA_PHASE(ph) \
    if (!in_phase(a, ph)) return;

// sum over the workgroup, the same value in every thread (fixed order)
__device__ double block_sum(double v, double* sh) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    double s = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) s += sh[i];
    return s;
}

// Last-arriver hand-off inside one launch (MI355X_MICROARCH.md visibility table, row 1): each
// workgroup of a problem's row stores its partial with an agent-scope (sc1) store, drains it, and
// bumps the problem's counter; the workgroup that arrives last reads every partial with sc1 loads
// and runs the controller step that used to be its own launch. Nobody waits for anybody.
typedef __attribute__((address_space(1))) int ba_gint;
typedef __attribute__((address_space(1))) double ba_gdbl;
__device__ __forceinline__ void st_agent(double* p, double v) {
    __hip_atomic_store((ba_gdbl*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double* p) {
    return __hip_atomic_load((ba_gdbl*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// every workgroup of the row calls it once, after thread 0's partial store; true (uniform) in the
// last one, which also resets the counter for the next launch
__device__ __forceinline__ bool last_arrival(int* counter, int total, int* sh_flag) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add((ba_gint*)counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == total - 1;
        if (last) __hip_atomic_store((ba_gint*)counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *sh_flag = last;
    }
    __syncthreads();
    return *sh_flag != 0;
}
__device__ void ctl_end_body(const BaArgs& a, int prob, int* done_flags, double* sh);
__device__ void ctl_begin_body(const BaArgs& a, int nlin, int* done_flags, int prob, double* sh);

// ---------------------------------------------------------------------------
// errors (when: 0 always, 1 the build's stale-error refresh, 2 a trial's new state); a trial also
// writes each workgroup's sum of the robust chi2 terms to part[bx] (k_ba_ctl_end adds them)
// ---------------------------------------------------------------------------
// one edge: error, chi2, robust rho (EdgeSE3ProjectXYZ::computeError + RobustKernelHuber::robustify);
// returns rho0
// the error terms of edge e from its camera-frame point
// Stereo (template <bool Stereo> below): the problem may hold EdgeStereoSE3ProjectXYZ edges, those
// with e_ur[e] >= 0 (the observation's right coordinate): a third error row
//   e2 = ur - (fx x / z + cx - bf / z), the same information, a Huber delta of its own (delta_s),
// and a third Jacobian row: the first row's formula with j02 replaced by j22 = j02 - bf / z^2.
// A monocular edge of such a problem has a zero third row (error and Jacobian): every sum below
// receives +0 from it. Stereo = false is the monocular code, word for word.
// The terms from the observation's words (o0, o1: the keypoint, ur: its right coordinate, unused
// unless Stereo)
template <bool Stereo>
__device__ __forceinline__ void edge_terms_of(const BaArgs& a, double o0, double o1, double ur, double info, double cx,
                                              double cy, double cz, double& e0, double& e1, double& e2, double& chi2,
                                              double& r0, double& r1) {
    const double u = a.fx * cx / cz + a.cx, v = a.fy * cy / cz + a.cy;
    e0 = o0 - u;
    e1 = o1 - v;
    double delta = a.delta;
    if constexpr (Stereo) {
        const bool st = ur >= 0.0;
        e2 = st ? ur - (u - a.bf / cz) : 0.0;
        chi2 = info * (e0 * e0 + e1 * e1 + e2 * e2);
        delta = st ? a.delta_s : a.delta;
    } else {
        e2 = 0.0;
        chi2 = info * (e0 * e0 + e1 * e1);
    }
    r0 = chi2;
    r1 = 1.0;
    if (delta > 0) {
        const double dsqr = delta * delta;
        if (chi2 > dsqr) {
            const double sq = sqrt(chi2);
            r0 = 2 * sq * delta - dsqr;
            r1 = delta / sq;
        }
    }
}
template <bool Stereo>
__device__ __forceinline__ void edge_terms(const BaArgs& a, int e, double cx, double cy, double cz, double& e0,
                                           double& e1, double& e2, double& chi2, double& r0, double& r1) {
    double ur = -1.0;
    if constexpr (Stereo) ur = a.e_ur[e];
    edge_terms_of<Stereo>(a, a.e_obs[2 * e], a.e_obs[2 * e + 1], ur, a.e_info[e], cx, cy, cz, e0, e1, e2, chi2, r0, r1);
}
template <bool Stereo>
__device__ __forceinline__ void store_terms(const BaArgs& a, int e, double e0, double e1, double e2, double chi2,
                                            double r0, double r1) {
    a.e_err[2 * e] = e0;
    a.e_err[2 * e + 1] = e1;
    if constexpr (Stereo) a.e_err2[e] = e2;
    a.e_chi2[e] = chi2;
    a.e_rho0[e] = r0;
    a.e_rho1[e] = r1;
}
// Plain stores: no launch rewrites these words after another workgroup of the same launch wrote
// them (a rejected small problem's refresh is done by the next build, k_ba_lin, not by the
// trial's last workgroup; r05: the agent-scope stores cost ~4 us per C4 trial)
template <bool Stereo>
__device__ __forceinline__ double edge_error_at(const BaArgs& a, int e, const double* T, const double* X) {
    double cx, cy, cz;
    qrot(load_q(T), X[0], X[1], X[2], cx, cy, cz);
    cx += T[4]; cy += T[5]; cz += T[6];
    double e0, e1, e2, chi2, r0, r1;
    edge_terms<Stereo>(a, e, cx, cy, cz, e0, e1, e2, chi2, r0, r1);
    store_terms<Stereo>(a, e, e0, e1, e2, chi2, r0, r1);
    return r0;
}
template <bool Stereo>
__device__ __forceinline__ double edge_error(const BaArgs& a, int e) {
    return edge_error_at<Stereo>(a, e, a.pose + 8 * a.e_pose[e], a.pts + 3 * a.e_pt[e]);
}

// when == 2 (a trial) ends in the trial's controller step, run by the last workgroup of each
// problem to finish (ctl_end_body; done: the host-mapped done flags).
// when == 1 also opens the device-driven slot (the former k_ba_ctl_pre): workgroup 0 of each
// problem clears the pop request of the previous slot and, at an iteration start, ends the solve
// on the iteration budget or the (host-relayed) stop flag (done[b], host-mapped: the host stops
// queueing slots once every problem is done). Every workgroup derives the same effective phase
// from the controller's fields, so none depends on that transition's store.
// host-mapped words of a device-driven solve, reached through a device-resident pointer pair
// donep = {done, hstop}: done[prob] is set once when the problem's LM run ends (the host stops
// queueing slots once all are set); *hstop is the caller's stop flag as the host relays it while
// it waits (null for sharded solves, whose shards must take the same decisions: they get the
// stop between batches of slots). A store to host memory in every trial put ~5 us in front of
// the next kernel, so the done words are written once per solve and the stop word only read.
__device__ __forceinline__ void post_done(int* done, int prob) {
    if (done) __hip_atomic_store(done + prob, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ int* done_of(int* const* donep) { return donep ? donep[0] : nullptr; }
// The stop word is read over PCIe (~2 us) by an extra workgroup of k_ba_schur_items, off every
// critical path (a read in the controller's tail, or early in a working wave, delays the kernel:
// vmcnt waits in order), and copied into LmCtl::stop, which the controller checks at its trial end
// (this slot) and at the next iteration's start.
// One read per slot (problem row 0's extra workgroup), fanned out to every problem of the launch:
// a read per problem put 256 same-address PCIe reads into every batched slot.
__device__ __forceinline__ void relay_host_stop(const BaArgs* args, const int* act, int* const* donep) {
    const int* hstop = donep ? donep[1] : nullptr;
    if (!hstop || __hip_atomic_load(hstop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) return;
    for (int b = 0; b < (int)gridDim.y; b++) args[act[b]].ctl->stop = 1;
}

template <bool Stereo>
__global__ __launch_bounds__(256) void k_ba_errors(const BaArgs* __restrict__ args, const int* __restrict__ act,
                                                   int when, int* const* donep) {
    BA_PROLOGUE
    int* const done = done_of(donep);
    if (when == 1) {
        LmCtl* c = a.ctl;
        const bool ends = c->phase == kPhBuild && (c->stop || c->it >= c->iterations);
        if (bx_ == 0 && threadIdx.x == 0) {
            c->pop = 0;
            if (ends) {
                c->phase = kPhDone;
                post_done(done, act[by_]);
            }
        }
        if (ends || !(in_phase(a, kPhBuild) && !c->errors_valid)) return;
    }
    if (when == 2 && !in_phase(a, kPhTrial)) return;
    const bool has = bx_ * (int)blockDim.x < a.E;   // uniform
    if (when != 2 && !has) return;
    const int e = bx_ * blockDim.x + threadIdx.x;
    const double r0 = (has && e < a.E) ? edge_error<Stereo>(a, e) : 0.0;
    if (when == 2) {   // uniform: every thread reaches the workgroup sum's barriers once
        __shared__ double sh[4];
        __shared__ int lastf;
        const double t = block_sum(r0, sh);
        if (threadIdx.x == 0 && has) st_agent(a.part + bx_, t);
        // the row's last workgroup runs the trial's controller step (the former k_ba_ctl_end)
        if (!a.sync && last_arrival(&a.ctl->arrive_t, gridDim.x, &lastf)) ctl_end_body(a, act[by_], done, sh);
    }
}

// Jacobians of EdgeSE3ProjectXYZ at the camera-frame point (x, y, z) of a pose with rotation R
// (row-major). The (negated) projection Jacobian J has rows (j00, 0, j02) and (0, j11, j12):
//   j00 = -fx / z, j02 = fx x / z^2, j11 = -fy / z, j12 = fy y / z^2
// A (2x3, landmark) = J R, B (2x6, pose [omega, upsilon]) = J [ -[Pc]x | I ]:
//   B = [[j02 y, j00 z - j02 x, -j00 y, j00, 0, j02], [j12 y - j11 z, -j12 x, j11 x, 0, j11, j12]].
// The linearisation stores (x, y, z, w) per edge; every consumer (Schur, back-substitution)
// rebuilds J, A and B from that record and the pose's R_lin, so Hpl_e = w B^T A (18 doubles per
// edge) is never stored. These consumers are bound by L2 traffic, not flops: storing J too (64
// instead of 32 bytes per edge) measured 20% slower at B = 256.
__device__ __forceinline__ void proj_jac(double fx, double fy, double x, double y, double z, double j[4]) {
    j[0] = -(fx / z);
    j[1] = fx * x / (z * z);
    j[2] = -(fy / z);
    j[3] = fy * y / (z * z);
}
// Stereo: the third row's pair js = (j00, j22 = j02 - bf / z^2) of a stereo edge (ur >= 0), (0, 0)
// of a monocular one; A is then 3x3 (third row js0 R[0,:] + js1 R[2,:]) and B 3x6 (third row
// [js1 y, js0 z - js1 x, -js0 y, js0, 0, js1])
template <bool Stereo>
struct JacDim {
    static constexpr int kA = Stereo ? 9 : 6, kB = Stereo ? 18 : 12;
};
__device__ __forceinline__ void stereo_jac(double bf, double ur, const double j[4], double z, double js[2]) {
    const bool st = ur >= 0.0;
    js[0] = st ? j[0] : 0.0;
    js[1] = st ? j[1] - bf / (z * z) : 0.0;
}
template <bool Stereo>
__device__ __forceinline__ void jac_ab(const double j[4], const double js[2], double x, double y, double z,
                                       const double R[9], double* A, double* B) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        A[c] = j[0] * R[c] + j[1] * R[6 + c];
        A[3 + c] = j[2] * R[3 + c] + j[3] * R[6 + c];
        if constexpr (Stereo) A[6 + c] = js[0] * R[c] + js[1] * R[6 + c];
    }
    B[0] = j[1] * y; B[1] = j[0] * z - j[1] * x; B[2] = -j[0] * y; B[3] = j[0]; B[4] = 0.0; B[5] = j[1];
    B[6] = j[3] * y - j[2] * z; B[7] = -j[3] * x; B[8] = j[2] * x; B[9] = 0.0; B[10] = j[2]; B[11] = j[3];
    if constexpr (Stereo) {
        B[12] = js[1] * y; B[13] = js[0] * z - js[1] * x; B[14] = -js[0] * y; B[15] = js[0]; B[16] = 0.0; B[17] = js[1];
    }
}
// a0 b0 + a1 b1 (+ a2 b2): the rows' sum of one product term
template <bool Stereo>
__device__ __forceinline__ double rows_dot(double a0, double b0, double a1, double b1, double a2, double b2) {
    if constexpr (Stereo) return a0 * b0 + a1 * b1 + a2 * b2;
    else return a0 * b0 + a1 * b1;
}

// camera-frame point of edge e at the current state + the pose's rotation matrix
__device__ __forceinline__ void edge_pc(const BaArgs& a, int e, double& x, double& y, double& z, double R[9]) {
    const double* T = a.pose + 8 * a.e_pose[e];
    const double* X = a.pts + 3 * a.e_pt[e];
    const DQ q = load_q(T);
    qrot(q, X[0], X[1], X[2], x, y, z);
    x += T[4]; y += T[5]; z += T[6];
    qtomat(q, R);
}

// A, B of edge e from its stored linearisation (e_lin) and its pose's R_lin (optimised poses only)
template <bool Stereo>
__device__ __forceinline__ double lin_ab(const BaArgs& a, int e, int oi, double* A, double* B) {
    const double4 l = ((const double4*)a.e_lin)[e];
    double j[4], js[2] = {0.0, 0.0};
    proj_jac(a.fx, a.fy, l.x, l.y, l.z, j);
    if constexpr (Stereo) stereo_jac(a.bf, a.e_ur[e], j, l.z, js);
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = a.R_lin[9 * oi + k];
    jac_ab<Stereo>(j, js, l.x, l.y, l.z, R, A, B);
    return l.w;
}

// ---------------------------------------------------------------------------
// buildSystem
// ---------------------------------------------------------------------------
// four lanes per landmark: Hll, b_l over all its edges (lane sub takes edges sub, sub + 4, ...; the 12
// sums are added over the quad, a butterfly: the same bits in its lanes, and lane 0 stores them);
// stores each edge's linearisation (Pc, w); returns the largest |diagonal| of Hll in every lane of
// the quad (0 for m >= M)
// fresh: the stored errors belong to a rejected trial (an unsharded problem whose iteration ended
// on one): each edge's terms are taken from the restored state here, and stored, instead of read
constexpr int kLinL = 64;   // landmarks per workgroup of k_ba_lin
template <bool Stereo>
__device__ __forceinline__ double lin_point_quad(const BaArgs& a, int m, int sub, bool fresh) {
    if (m >= a.M) return 0.0;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
    for (int k = a.pt_ptr[m] + sub; k < a.pt_ptr[m + 1]; k += 4) {
        const int e = a.pt_edges[k];
        double x, y, z, R[9], j[4], js[2] = {0.0, 0.0}, A[JacDim<Stereo>::kA], B[JacDim<Stereo>::kB];
        edge_pc(a, e, x, y, z, R);
        proj_jac(a.fx, a.fy, x, y, z, j);
        if constexpr (Stereo) stereo_jac(a.bf, a.e_ur[e], j, z, js);
        jac_ab<Stereo>(j, js, x, y, z, R, A, B);
        double r1, er0, er1, er2 = 0.0;
        if (fresh) {   // uniform
            double chi2, r0;
            edge_terms<Stereo>(a, e, x, y, z, er0, er1, er2, chi2, r0, r1);
            store_terms<Stereo>(a, e, er0, er1, er2, chi2, r0, r1);
        } else {
            r1 = a.e_rho1[e];
            er0 = a.e_err[2 * e];
            er1 = a.e_err[2 * e + 1];
            if constexpr (Stereo) er2 = a.e_err2[e];
        }
        const double info = a.e_info[e];
        const double w = r1 * info;
        const double om0 = -info * er0 * r1, om1 = -info * er1 * r1;
        const double om2 = Stereo ? -info * er2 * r1 : 0.0;
        [[maybe_unused]] constexpr int a2 = Stereo ? 6 : 0, b2 = Stereo ? 12 : 0;   // the third rows of A and B (unused unless Stereo)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            bl[r] += rows_dot<Stereo>(A[r], om0, A[3 + r], om1, A[a2 + r], om2);
#pragma unroll
            for (int c = 0; c < 3; c++) H[3 * r + c] += w * rows_dot<Stereo>(A[r], A[c], A[3 + r], A[3 + c], A[a2 + r], A[a2 + c]);
        }
        ((double4*)a.e_lin)[e] = make_double4(x, y, z, w);
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
#pragma unroll
        for (int i = 0; i < 9; i++) H[i] += __shfl_xor(H[i], o, 64);
#pragma unroll
        for (int r = 0; r < 3; r++) bl[r] += __shfl_xor(bl[r], o, 64);
    }
    if (sub == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) a.Hll[9 * m + i] = H[i];
#pragma unroll
        for (int r = 0; r < 3; r++) a.b[a.n + 3 * m + r] = bl[r];
    }
    return fmax(fmax(fabs(H[0]), fabs(H[4])), fabs(H[8]));
}

// one wave per optimised pose: 21 upper Hpp terms + 6 b terms, lanes over the pose's edges; lane 0
// keeps the pose's rotation at the linearisation (R_lin)
// one halving step of a transpose-reduce: a lane with bit m clear keeps values [0, H), set keeps
// [H, 2H); each adds its partner's copy of the values it keeps; the kept values end in [0, H)
template <int H>
__device__ __forceinline__ void reduce_half(double* acc, int lane, int m) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < H; i++) {
        const double send = up ? acc[i] : acc[i + H];
        const double keep = up ? acc[i + H] : acc[i];
        acc[i] = keep + __shfl_xor(send, m, 64);
    }
}

// one wave per pose i; returns (in every lane) the largest |diagonal| of the pose's Hpp block
template <bool Stereo>
__device__ __forceinline__ double lin_pose(const BaArgs& a, int i, int lane, bool fresh = false) {
    if (i >= a.np) return 0.0;   // wave-uniform
    double acc[32];   // 27 sums (21 of the upper Hpp triangle, 6 of b_p), padded to 32
#pragma unroll
    for (int k = 0; k < 32; k++) acc[k] = 0;
    for (int k = a.ps_ptr[i] + lane; k < a.ps_ptr[i + 1]; k += 64) {
        const int e = a.ps_edges[k];
        double x, y, z, R[9], j[4], js[2] = {0.0, 0.0}, A[JacDim<Stereo>::kA], B[JacDim<Stereo>::kB];
        edge_pc(a, e, x, y, z, R);
        proj_jac(a.fx, a.fy, x, y, z, j);
        if constexpr (Stereo) stereo_jac(a.bf, a.e_ur[e], j, z, js);
        jac_ab<Stereo>(j, js, x, y, z, R, A, B);
        double r1, er0, er1, er2 = 0.0;
        if (fresh) {   // uniform; the landmark side stores the same values
            double chi2, r0;
            edge_terms<Stereo>(a, e, x, y, z, er0, er1, er2, chi2, r0, r1);
        } else {
            r1 = a.e_rho1[e];
            er0 = a.e_err[2 * e];
            er1 = a.e_err[2 * e + 1];
            if constexpr (Stereo) er2 = a.e_err2[e];
        }
        const double info = a.e_info[e];
        const double w = r1 * info;
        const double om0 = -info * er0 * r1, om1 = -info * er1 * r1;
        const double om2 = Stereo ? -info * er2 * r1 : 0.0;
        [[maybe_unused]] constexpr int a2 = Stereo ? 6 : 0, b2 = Stereo ? 12 : 0;   // the third rows of A and B (unused unless Stereo)
        int t = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) acc[t++] += w * rows_dot<Stereo>(B[r], B[c], B[6 + r], B[6 + c], B[b2 + r], B[b2 + c]);
#pragma unroll
        for (int r = 0; r < 6; r++) acc[21 + r] += rows_dot<Stereo>(B[r], om0, B[6 + r], om1, B[b2 + r], om2);
    }
    // transpose-reduce over the 64 lanes: at each step a lane keeps half of its values and adds
    // its partner's copy of them (16 + 8 + 4 + 2 + 1 shuffles, then one for the last pair instead
    // of 27 x 6); lane 2k ends with sum k (k = the lane's bits 5..1, most significant first)
    reduce_half<16>(acc, lane, 32);
    reduce_half<8>(acc, lane, 16);
    reduce_half<4>(acc, lane, 8);
    reduce_half<2>(acc, lane, 4);
    reduce_half<1>(acc, lane, 2);
    const double tot = acc[0] + __shfl_xor(acc[0], 1, 64);
    const int k = ((lane >> 5) & 1) << 4 | ((lane >> 4) & 1) << 3 | ((lane >> 3) & 1) << 2 | ((lane >> 2) & 1) << 1 |
                  ((lane >> 1) & 1);
    double dmax = 0.0;
    if ((lane & 1) == 0 && k < 27) {
        double* H = a.Hpp + 36 * i;
        if (k < 21) {   // k-th entry of the upper triangle, row-major
            int r = 0, t = k;
            while (t >= 6 - r) { t -= 6 - r; r++; }
            const int c = r + t;
            H[6 * r + c] = tot;
            H[6 * c + r] = tot;
            if (r == c) dmax = fabs(tot);
        } else {
            a.b[6 * i + k - 21] = tot;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o, 64));
    if (lane < 9 && a.ps_ptr[i] < a.ps_ptr[i + 1]) {   // the pose's rotation, as its edges used it
        {
            const int p = a.e_pose[a.ps_edges[a.ps_ptr[i]]];
            double R[9];
            qtomat(load_q(a.pose + 8 * p), R);
            double r = R[0];
#pragma unroll
            for (int k = 1; k < 9; k++) r = lane == k ? R[k] : r;
            a.R_lin[9 * i + lane] = r;
        }
    }
    return dmax;
}
// the same with the whole work-group on pose i (r06, k_ba_lin with one pose per work-group): its
// four waves take edges lane, lane + 256, ... of the pose, each reduces its 27 sums as above, and
// wave 0 adds the four in wave order; returns the largest |diagonal| in wave 0 (0 in the others)
template <bool Stereo>
__device__ __forceinline__ double lin_pose_wg(const BaArgs& a, int i, bool fresh, double* sh27) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (i >= a.np) return 0.0;   // work-group-uniform
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; k++) acc[k] = 0;
    for (int k = a.ps_ptr[i] + (int)threadIdx.x; k < a.ps_ptr[i + 1]; k += blockDim.x) {
        const int e = a.ps_edges[k];
        double x, y, z, R[9], j[4], js[2] = {0.0, 0.0}, A[JacDim<Stereo>::kA], B[JacDim<Stereo>::kB];
        edge_pc(a, e, x, y, z, R);
        proj_jac(a.fx, a.fy, x, y, z, j);
        if constexpr (Stereo) stereo_jac(a.bf, a.e_ur[e], j, z, js);
        jac_ab<Stereo>(j, js, x, y, z, R, A, B);
        double r1, er0, er1, er2 = 0.0;
        if (fresh) {
            double chi2, r0;
            edge_terms<Stereo>(a, e, x, y, z, er0, er1, er2, chi2, r0, r1);
        } else {
            r1 = a.e_rho1[e];
            er0 = a.e_err[2 * e];
            er1 = a.e_err[2 * e + 1];
            if constexpr (Stereo) er2 = a.e_err2[e];
        }
        const double info = a.e_info[e];
        const double w = r1 * info;
        const double om0 = -info * er0 * r1, om1 = -info * er1 * r1;
        const double om2 = Stereo ? -info * er2 * r1 : 0.0;
        [[maybe_unused]] constexpr int a2 = Stereo ? 6 : 0, b2 = Stereo ? 12 : 0;   // the third rows of A and B (unused unless Stereo)
        int t = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) acc[t++] += w * rows_dot<Stereo>(B[r], B[c], B[6 + r], B[6 + c], B[b2 + r], B[b2 + c]);
#pragma unroll
        for (int r = 0; r < 6; r++) acc[21 + r] += rows_dot<Stereo>(B[r], om0, B[6 + r], om1, B[b2 + r], om2);
    }
    reduce_half<16>(acc, lane, 32);
    reduce_half<8>(acc, lane, 16);
    reduce_half<4>(acc, lane, 8);
    reduce_half<2>(acc, lane, 4);
    reduce_half<1>(acc, lane, 2);
    const double tot = acc[0] + __shfl_xor(acc[0], 1, 64);
    const int k = ((lane >> 5) & 1) << 4 | ((lane >> 4) & 1) << 3 | ((lane >> 3) & 1) << 2 | ((lane >> 2) & 1) << 1 |
                  ((lane >> 1) & 1);
    if ((lane & 1) == 0 && k < 27) sh27[27 * wid + k] = tot;
    __syncthreads();
    double dmax = 0.0;
    if (wid == 0) {
        if (lane < 27) {
            const double v = (sh27[lane] + sh27[27 + lane]) + (sh27[54 + lane] + sh27[81 + lane]);
            double* H = a.Hpp + 36 * i;
            if (lane < 21) {   // lane-th entry of the upper triangle, row-major
                int r = 0, t = lane;
                while (t >= 6 - r) { t -= 6 - r; r++; }
                const int c = r + t;
                H[6 * r + c] = v;
                H[6 * c + r] = v;
                if (r == c) dmax = fabs(v);
            } else {
                a.b[6 * i + lane - 21] = v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o, 64));
        if (lane < 9 && a.ps_ptr[i] < a.ps_ptr[i + 1]) {   // the pose's rotation, as its edges used it
            const int p = a.e_pose[a.ps_edges[a.ps_ptr[i]]];
            double R[9];
            qtomat(load_q(a.pose + 8 * p), R);
            double r = R[0];
#pragma unroll
            for (int kk = 1; kk < 9; kk++) r = lane == kk ? R[kk] : r;
            a.R_lin[9 * i + lane] = r;
        }
    }
    return dmax;
}

// the device-driven build in one launch: workgroups [0, nbp) linearise landmarks (kLinL each,
// four lanes per landmark), the rest poses (one per wave); each stores its largest |diagonal| (sc1), and the
// problem's last workgroup runs the controller's trial start (ctl_begin_body: lambda from the
// maxima on the first iteration)
// ppw: poses per pose work-group, 4 (a wave each) or 1 (the whole work-group, lin_pose_wg)
template <bool Stereo>
__global__ __launch_bounds__(256) void k_ba_lin(const BaArgs* __restrict__ args, const int* __restrict__ act,
                                               int nbp, int ppw, int* const* donep) {
    BA_PROLOGUE
    BA_PHASE(kPhBuild)
    __shared__ double sh[4];
    __shared__ double sh27[4 * 27];
    __shared__ int lastf;
    const int mP = (a.M + kLinL - 1) / kLinL, nP = (a.np + ppw - 1) / ppw;
    // a problem whose iteration ended on a rejected trial: its stored errors are the trial's, so this
    // build takes them from the restored state (a small problem's restored in the trial's launch, a
    // larger one's by k_ba_pop). r06 (late): every unsharded problem, so the larger ones' slots lost
    // their k_ba_errors(1) launch (C5: one launch less per trial); the shards keep it
    const bool fresh = (a.small || !a.sync) && !a.ctl->errors_valid;
    double d;
    int slot;
    if (bx_ < nbp) {
        d = lin_point_quad<Stereo>(a, bx_ * kLinL + (threadIdx.x >> 2), threadIdx.x & 3, fresh);
        slot = bx_ < mP ? bx_ : -1;
    } else {
        const int q = bx_ - nbp;
        d = ppw == 1 ? lin_pose_wg<Stereo>(a, q, fresh, sh27)
                     : lin_pose<Stereo>(a, q * 4 + (threadIdx.x >> 6), threadIdx.x & 63, fresh);
        slot = q < nP ? mP + q : -1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d = fmax(d, __shfl_xor(d, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0 && slot >= 0) {
        double m = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) m = fmax(m, sh[w]);
        st_agent(a.part + slot, m);
    }
    if (!a.sync && last_arrival(&a.ctl->arrive_b, gridDim.x, &lastf))
        ctl_begin_body(a, mP + nP, done_of(donep), act[by_], sh);
}

// ---------------------------------------------------------------------------
// Schur complement
// ---------------------------------------------------------------------------
__device__ __forceinline__ void inv3(const double m[9], double r[9]) {
    const double c0 = m[4] * m[8] - m[5] * m[7];
    const double c1 = m[5] * m[6] - m[3] * m[8];
    const double c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    const double id = 1.0 / det;
    r[0] = c0 * id; r[3] = c1 * id; r[6] = c2 * id;
    r[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    r[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    r[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// Dinv of landmark m = (Hll + lambda I)^-1 (Eigen 3x3 cofactor inverse)
__device__ __forceinline__ void dinv_of(const BaArgs& a, int m, double Di[9]) {
    const double lambda = *a.lambda;
    double D[9];
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = a.Hll[9 * m + k] + (k % 4 == 0 ? lambda : 0.0);
    inv3(D, Di);
}

// one thread per landmark: setLambda on Hll, Dinv (Eigen 3x3 cofactor inverse), db = Dinv b_l.
// Fused trials (BaArgs::fused) skip this launch: every consumer forms Dinv (the same bits) itself
__global__ __launch_bounds__(256) void k_ba_schur_points(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    BA_PROLOGUE
    BA_PHASE(kPhTrial)
    const int m = bx_ * blockDim.x + threadIdx.x;
    if (m >= a.M) return;
    const double lambda = *a.lambda;
    double D[9], Di[9];
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = a.Hll[9 * m + k] + (k % 4 == 0 ? lambda : 0.0);
    inv3(D, Di);
#pragma unroll
    for (int k = 0; k < 9; k++) a.Dinv[9 * m + k] = Di[k];
    const double* bl = a.b + a.n + 3 * m;
#pragma unroll
    for (int r = 0; r < 3; r++) a.db[3 * m + r] = Di[3 * r] * bl[0] + Di[3 * r + 1] * bl[1] + Di[3 * r + 2] * bl[2];
}

__global__ __launch_bounds__(256) void k_ba_zero_s(const BaArgs* __restrict__ args, const int* __restrict__ act,
                                                   int always) {
    BA_PROLOGUE
    if (!always) BA_PHASE(kPhTrial)
    const size_t nn = (size_t)a.n * a.n;
    double2* S2 = (double2*)a.S;
    for (size_t i = (size_t)bx_ * blockDim.x + threadIdx.x; i < nn / 2; i += (size_t)gridDim.x * blockDim.x)
        S2[i] = make_double2(0.0, 0.0);
    if (bx_ == 0 && threadIdx.x == 0 && (nn & 1)) a.S[nn - 1] = 0.0;
}

// Two LANES per Schur work item (a chunk of pairs of one 6x6 block (i, j)): lane half h owns rows
// 3h..3h+2 of the block, 18 sums in registers (the pair prologue is computed by both lanes: the
// register budget, not the flops, bounds this kernel). Matrix-free: for a pair (a, b) of edges of
// landmark m,
//   W_a Hpl_b^T = Hpl_a Dinv_m Hpl_b^T = w_a w_b B_a^T (A_a Dinv_m A_b^T) B_b
// with A, B rebuilt from the edges' stored (Pc, w) and the poses' R_lin: 17 doubles read per pair
// (edge records + Dinv) instead of the 36 of stored W / Hpl blocks, and no W written per trial.
// (kItemsWg Schur work items per work-group: ba_prep.h, whose prepare() lays the items out for it)
template <bool Stereo>
__device__ __forceinline__ void schur_b_pose(const BaArgs& a, int i, int lane);
// work-groups [nbi, gridDim.x - 1) run schur_b_pose on the poses instead (it reads only
// k_ba_schur_points' db and the linearisation: no dependence on the items, one launch less per trial)
// Stereo: A_a, A_b get their third rows (sa, sb: the stereo_jac pairs), so T = A_a Dinv and
// C = w_a w_b A_a Dinv A_b^T are 3x3, and B_b, B_a^T get a third row / column; the same two lanes
// per item and the same 18 sums per lane
template <bool Stereo>
__global__ __launch_bounds__(256) void k_ba_schur_items(const BaArgs* __restrict__ args, const int* __restrict__ act,
                                                        int nbi, int* const* donep) {
    BA_PROLOGUE
    if (donep && bx_ == (int)gridDim.x - 1) {   // the extra workgroup: the relayed stop flag
        if (by_ == 0 && threadIdx.x == 0) relay_host_stop(args, act, donep);
        return;
    }
    BA_PHASE(kPhTrial)
    if (bx_ >= nbi) {
        schur_b_pose<Stereo>(a, (bx_ - nbi) * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
        return;
    }
    const int gt = bx_ * blockDim.x + threadIdx.x;
    const int it = gt >> 1, h = gt & 1;
    const int lane = threadIdx.x & 63;
    const bool valid = it < a.nitems;   // no early exit: the whole wave meets at the ballot below
    const int4 wi = valid ? ((const int4*)a.items)[it] : make_int4(0, 0, 0, -1);
    const int bi = valid && wi.z >= 0 ? a.blk_i[wi.z] : 0, bj = valid && wi.z >= 0 ? a.blk_j[wi.z] : 0;
    double Ri[9], Rj[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { Ri[k] = a.R_lin[9 * bi + k]; Rj[k] = a.R_lin[9 * bj + k]; }
    double s[18];
#pragma unroll
    for (int k = 0; k < 18; k++) s[k] = 0.0;
    const double fx = a.fx, fy = a.fy;
    for (int k = wi.x; k < wi.y; k++) {
        const int2 pr = ((const int2*)a.blk_pairs)[k];
        const double4 la = ((const double4*)a.e_lin)[pr.x], lb = ((const double4*)a.e_lin)[pr.y];
        double Di[9];   // in registers either way (a pointer choice would put a local copy in scratch)
        if (a.fused) {
            dinv_of(a, a.e_pt[pr.x], Di);
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) Di[k] = a.Dinv[9 * a.e_pt[pr.x] + k];
        }
        // the projection Jacobians of both edges (proj_jac); A and B are used through their structure
        double ja[4], jb[4];
        proj_jac(fx, fy, la.x, la.y, la.z, ja);
        proj_jac(fx, fy, lb.x, lb.y, lb.z, jb);
        const double a00 = ja[0], a02 = ja[1], a11 = ja[2], a12 = ja[3];
        const double b00 = jb[0], b02 = jb[1], b11 = jb[2], b12 = jb[3];
        double sa[2] = {0.0, 0.0}, sb[2] = {0.0, 0.0};   // the third rows' (j00, j22) of both edges
        if constexpr (Stereo) {
            stereo_jac(a.bf, a.e_ur[pr.x], ja, la.z, sa);
            stereo_jac(a.bf, a.e_ur[pr.y], jb, lb.z, sb);
        }
        double T[Stereo ? 9 : 6];   // A_a Dinv (2x3), A_a = [a00 Ri0 + a02 Ri2; a11 Ri1 + a12 Ri2] (; sa0 Ri0 + sa1 Ri2)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double d0 = Di[c], d1 = Di[3 + c], d2 = Di[6 + c];
            const double r0 = Ri[0] * d0 + Ri[1] * d1 + Ri[2] * d2;
            const double r1 = Ri[3] * d0 + Ri[4] * d1 + Ri[5] * d2;
            const double r2 = Ri[6] * d0 + Ri[7] * d1 + Ri[8] * d2;
            T[c] = a00 * r0 + a02 * r2;
            T[3 + c] = a11 * r1 + a12 * r2;
            if constexpr (Stereo) T[6 + c] = sa[0] * r0 + sa[1] * r2;
        }
        const double ww = la.w * lb.w;
        constexpr int NR = Stereo ? 3 : 2;   // rows of an edge
        double C[NR * NR];   // w_a w_b A_a Dinv A_b^T (2x2; 3x3)
#pragma unroll
        for (int c = 0; c < NR; c++) {
            const double jb0 = c == 0 ? b00 : c == 1 ? b11 : sb[0], jb2 = c == 0 ? b02 : c == 1 ? b12 : sb[1];
            const int rj = c == 1 ? 3 : 0;   // A_b's row c = jb0 Rj[c == 1 ? 1 : 0, :] + jb2 Rj[2, :]
            double ab[3];
#pragma unroll
            for (int q = 0; q < 3; q++) ab[q] = jb0 * Rj[rj + q] + jb2 * Rj[6 + q];
#pragma unroll
            for (int r = 0; r < NR; r++) C[NR * r + c] = ww * (T[3 * r] * ab[0] + T[3 * r + 1] * ab[1] + T[3 * r + 2] * ab[2]);
        }
        // B_b rows: [b02 y, b00 z - b02 x, -b00 y, b00, 0, b02], [b12 y - b11 z, -b12 x, b11 x, 0, b11, b12]
        // (, [sb1 y, sb0 z - sb1 x, -sb0 y, sb0, 0, sb1])
        const double Bb0[6] = {b02 * lb.y, b00 * lb.z - b02 * lb.x, -b00 * lb.y, b00, 0.0, b02};
        const double Bb1[6] = {b12 * lb.y - b11 * lb.z, -b12 * lb.x, b11 * lb.x, 0.0, b11, b12};
        const double Bb2[6] = {sb[1] * lb.y, sb[0] * lb.z - sb[1] * lb.x, -sb[0] * lb.y, sb[0], 0.0, sb[1]};
        double CB0[6], CB1[6], CB2[6];   // C B_b (2x6; 3x6)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            if constexpr (Stereo) {
                CB0[c] = C[0] * Bb0[c] + C[1] * Bb1[c] + C[2] * Bb2[c];
                CB1[c] = C[3] * Bb0[c] + C[4] * Bb1[c] + C[5] * Bb2[c];
                CB2[c] = C[6] * Bb0[c] + C[7] * Bb1[c] + C[8] * Bb2[c];
            } else {
                CB0[c] = C[0] * Bb0[c] + C[1] * Bb1[c];
                CB1[c] = C[2] * Bb0[c] + C[3] * Bb1[c];
                CB2[c] = 0.0;
                (void)Bb2;
            }
        }
        // this lane's rows of B_a^T: rows 3h..3h+2 of [a02 y, a00 z - a02 x, -a00 y, a00, 0, a02] and
        // [a12 y - a11 z, -a12 x, a11 x, 0, a11, a12]
        // (and of [sa1 y, sa0 z - sa1 x, -sa0 y, sa0, 0, sa1])
        double u0[3], u1[3], u2[3];
        if (h == 0) {
            u0[0] = a02 * la.y; u0[1] = a00 * la.z - a02 * la.x; u0[2] = -a00 * la.y;
            u1[0] = a12 * la.y - a11 * la.z; u1[1] = -a12 * la.x; u1[2] = a11 * la.x;
            u2[0] = sa[1] * la.y; u2[1] = sa[0] * la.z - sa[1] * la.x; u2[2] = -sa[0] * la.y;
        } else {
            u0[0] = a00; u0[1] = 0.0; u0[2] = a02;
            u1[0] = 0.0; u1[1] = a11; u1[2] = a12;
            u2[0] = sa[0]; u2[1] = 0.0; u2[2] = sa[1];
        }
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int cc = 0; cc < 6; cc++) s[6 * rr + cc] -= rows_dot<Stereo>(u0[rr], CB0[cc], u1[rr], CB1[cc], u2[rr], CB2[cc]);
    }
    // r06: a block's chunks (consecutive items, all in this work-group: prepare pads) are summed
    // here, not by a finisher launch: every chunk's 36 values go to LDS at its item position and
    // the pair holding a block's first chunk lists the block (per wave, 32 slots); after the
    // barrier the work-group's threads take the listed blocks' entries, one (block, entry) each:
    // Hpp + lambda (diagonal, pose side), then the chunks in order (the r05 finisher's order),
    // into S. (r06 first tries: the partials handed over through global memory to the block's last
    // arrival, agent-scope stores, an atomic count and loads: 11 + 6 us (items + finisher) ->
    // 26-43 us per C4 trial; a segmented shuffle tree per wave run before an LDS hand-off: 16.5 us,
    // 3.5 of them the tree; each wave summing its own blocks, 36 lanes per block: 15.5 us.)
    __shared__ double parts[kItemsWg * 36];   // partial sums by item position in the work-group
    __shared__ int4 blist[4 * 32];            // per wave: {first item position, chunks, i, j}
    __shared__ int bcnt[4];
    const int li = it & (kItemsWg - 1), wv = threadIdx.x >> 6;
    const int myf = valid && wi.w >= 0 ? a.ifin[it] : -1;
    const bool first = myf >= 0 && h == 0 && wi.w == a.fin[3 * myf + 1];
    const int nch0 = first ? a.fin[3 * myf + 2] : 0;
    if (myf >= 0)
#pragma unroll
        for (int k = 0; k < 18; k++) parts[36 * li + 18 * h + k] = s[k];
    const unsigned long long om = __ballot(first);
    if (first) blist[32 * wv + __popcll(om & ((1ull << lane) - 1))] = make_int4(li, nch0, bi, bj);
    if (lane == 0) bcnt[wv] = __popcll(om);
    __syncthreads();
    if (valid && myf < 0 && wi.z >= 0) {   // a block of one chunk: straight into S (both triangles)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int rr = 3 * h + r;
#pragma unroll
            for (int cc = 0; cc < 6; cc++) {
                a.S[(size_t)(6 * bi + rr) * a.n + 6 * bj + cc] = s[6 * r + cc];
                a.S[(size_t)(6 * bj + cc) * a.n + 6 * bi + rr] = s[6 * r + cc];
            }
        }
    }
    const int n0 = bcnt[0], n1 = n0 + bcnt[1], n2 = n1 + bcnt[2], nb = n2 + bcnt[3];
    if (nb == 0) return;
    const double lambda = *a.lambda;
    for (int q = threadIdx.x; q < 36 * nb; q += blockDim.x) {
        const int g = q / 36, e = q - 36 * g;   // block g of the work-group's list, entry e
        const int w = (g >= n0) + (g >= n1) + (g >= n2);
        const int4 B = blist[32 * w + g - (w == 0 ? 0 : w == 1 ? n0 : w == 2 ? n1 : n2)];
        const int i = B.z, j = B.w, rr = e / 6, cc = e - 6 * rr;
        double acc = i == j && (a.own ? a.own[i] != 0 : a.lead != 0)
                         ? a.Hpp_g[36 * i + 6 * rr + cc] + (rr == cc ? lambda : 0.0) : 0.0;
        const double* pp = parts + 36 * B.x + e;
        for (int c = 0; c < B.y; c++) acc += pp[36 * c];
        a.S[(size_t)(6 * i + rr) * a.n + 6 * j + cc] = acc;
        if (i != j) a.S[(size_t)(6 * j + cc) * a.n + 6 * i + rr] = acc;
    }
}

// one wave per optimised pose: b_schur = b_p - sum_e Hpl_e db, Hpl_e db = w B^T (A db)
template <bool Stereo>
__device__ __forceinline__ void schur_b_pose(const BaArgs& a, int i, int lane) {
    if (i >= a.np) return;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int k = a.ps_ptr[i] + lane; k < a.ps_ptr[i + 1]; k += 64) {
        const int e = a.ps_edges[k];
        double A[JacDim<Stereo>::kA], B[JacDim<Stereo>::kB];
        const double w = lin_ab<Stereo>(a, e, i, A, B);
        [[maybe_unused]] constexpr int a2 = Stereo ? 6 : 0, b2 = Stereo ? 12 : 0;   // the third rows (unused unless Stereo)
        double d0, d1, d2;
        if (a.fused) {   // db = Dinv b_l, formed here
            const int m = a.e_pt[e];
            double Di[9];
            dinv_of(a, m, Di);
            const double* bl = a.b + a.n + 3 * m;
            d0 = Di[0] * bl[0] + Di[1] * bl[1] + Di[2] * bl[2];
            d1 = Di[3] * bl[0] + Di[4] * bl[1] + Di[5] * bl[2];
            d2 = Di[6] * bl[0] + Di[7] * bl[1] + Di[8] * bl[2];
        } else {
            const double* d = a.db + 3 * a.e_pt[e];
            d0 = d[0]; d1 = d[1]; d2 = d[2];
        }
        const double v0 = w * (A[0] * d0 + A[1] * d1 + A[2] * d2), v1 = w * (A[3] * d0 + A[4] * d1 + A[5] * d2);
        const double v2 = Stereo ? w * (A[a2] * d0 + A[a2 + 1] * d1 + A[a2 + 2] * d2) : 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) acc[r] += rows_dot<Stereo>(B[r], v0, B[6 + r], v1, B[b2 + r], v2);
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double v = acc[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) a.bs[6 * i + r] = a.b[6 * i + r] - v;
    }
}

// ---------------------------------------------------------------------------
// dense Cholesky of S (n x n, lower, in place) + solve S xp = bs; one workgroup (8 waves).
// Right-looking, 32-column panels:
//  (a) 32x32 diagonal block factored by ONE wavefront in registers (no block barrier per
//      pivot): lane = column c (+ row parity), 16 rows per lane, the block kept as a full
//      symmetric square so every cross-lane operand is one ds_bpermute. Gaussian elimination
//      on [D | I | y] gives L_u (unit LDL^T factor), L_u^{-1} and the forward-solve slice;
//      L11 = L_u diag(sqrt piv), L11^{-1} = diag(1/sqrt piv) L_u^{-1} at the panel end.
//  (b) the panel L21 = A21 Linv^T and the
//      trailing update C -= L21_I L21_J^T run on v_mfma_f64_16x16x4f64
//      (operand map: lane l holds A[l&15][k=l>>4], B[k=l>>4][l&15]; C/D col = l&15,
//      row = (l>>4) + 4*reg). Panel rows live in LDS (stride 34 doubles: conflict-free).
//  (c) backward solve panel by panel: x_p = Linv^T (y_p - L21^T x_below) (Linv saved per panel).
// ---------------------------------------------------------------------------
constexpr int kNB = 32;
constexpr int kCholSmallN = 480;   // largest n of the single-workgroup solver (LDS envelope)
constexpr int kPS = 34;   // panel row stride in doubles

__host__ __device__ inline size_t chol_lds_doubles(int n) {
    const int np = (n + 31) & ~31;
    return (size_t)(2 + 32 * 33 + np + (size_t)np * kPS + 4 * 32 + 32 * 33);
}


__device__ __forceinline__ void chol_solve(double* __restrict__ S, const double* __restrict__ bs, double* __restrict__ x, int n,
                           int* __restrict__ flag, double* __restrict__ Lsave, unsigned long long* __restrict__ dbg) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int npad = (n + 31) & ~31;
    int& bad = *(int*)lds;                   // control word
    double* Li = lds + 2;                    // 32 x 33 L11^{-1}
    double* y = Li + 32 * 33;                // npad
    double* Pn = y + npad;                   // npad x kPS panel rows
    double* invp = Pn + (size_t)npad * kPS;  // 1/piv (raw pivot) per column of the panel
    double* dval = invp + 32;                // sqrt(piv)
    double* invd = dval + 32;                // 1/sqrt(piv)
    double* red = invd + 32;                 // 32 x 33 scratch (back-solve partial sums)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int wid = tid >> 6, lane = tid & 63, nw = nt >> 6;
    unsigned long long tprev = 0;
    auto stamp = [&](int ph) {
        if (dbg && tid == 0) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if (ph >= 0) dbg[ph] += t - tprev;
            tprev = t;
        }
    };
    stamp(-1);
    if (tid == 0) bad = 0;
    for (int i = tid; i < npad; i += nt) y[i] = i < n ? bs[i] : 0.0;
    __syncthreads();
    for (int k0 = 0; k0 < n; k0 += kNB) {
        const int kb = min(kNB, n - k0);
        // ---- (a) diagonal block: wave 0, registers only ----
        if (wid == 0) chol_diag_wave(S, n, k0, kb, Li, Lsave, &bad);
        __syncthreads();
        // forward-solve slice y_p = L11^{-1} y_p (elimination applied to y)
        if (tid < 32) {
            double s2 = 0.0;
#pragma unroll 8
            for (int k = 0; k < 32; k++) s2 += Li[tid * 33 + k] * (k < kb ? y[k0 + k] : 0.0);
            invp[tid] = s2;
        }
        __syncthreads();
        if (tid < kb) y[k0 + tid] = invp[tid];
        stamp(0);
        if (bad) break;
        // ---- (b2) stage A21 rows into Pn ----
        const int r0 = k0 + kb;
        const int nr = n - r0;
        const int nr_pad = (nr + 15) & ~15;
        for (int t = tid; t < nr_pad * 32; t += nt) {
            const int rr = t >> 5, cI = t & 31;
            Pn[rr * kPS + cI] = (rr < nr && cI < kb) ? S[(size_t)(r0 + rr) * n + k0 + cI] : 0.0;
        }
        __syncthreads();
        // ---- (b3) L21 = A21 Linv^T on MFMA: one wave per 16-row block, both column halves ----
        const int cc = lane & 15, rq = lane >> 4;
        for (int R = wid; R < nr_pad / 16; R += nw) {
            double4_t acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 8; kk++) {
                const double av = Pn[(16 * R + cc) * kPS + 4 * kk + rq];
                const double b0 = Li[cc * 33 + 4 * kk + rq];
                const double b1 = Li[(16 + cc) * 33 + 4 * kk + rq];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
            }
            // all lanes' A reads of this row block are done before any write (wave-synchronous)
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rr = 16 * R + rq + 4 * q;
                Pn[rr * kPS + cc] = acc0[q];
                Pn[rr * kPS + 16 + cc] = acc1[q];
            }
        }
        __syncthreads();
        // ---- (b4) L21 back to S (coalesced rows); y_r -= L21[r] . y_panel (half-wave per row) ----
        for (int t = tid; t < nr * 32; t += nt) {
            const int rr = t >> 5, cI = t & 31;
            const double lv = Pn[rr * kPS + cI];
            if (cI < kb) S[(size_t)(r0 + rr) * n + k0 + cI] = lv;
            double dot = cI < kb ? lv * y[k0 + cI] : 0.0;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 32);
            if (cI == 0) y[r0 + rr] -= dot;
        }
        stamp(1);
        // ---- (c) trailing update, lower 16x16 tiles, 4 tiles per wave per round ----
        const int T = nr_pad / 16;
        const int ntile = T * (T + 1) / 2;
        for (int base = wid; base < ntile; base += 4 * nw) {
            double4_t acc[4];
            int ti[4], tj[4];
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int tile = base + u * nw;
                on[u] = tile < ntile;
                const int tt = on[u] ? tile : 0;
                int I = (int)((sqrtf(8.0f * (float)tt + 1.0f) - 1.0f) * 0.5f);
                while ((I + 1) * (I + 2) / 2 <= tt) I++;
                while (I * (I + 1) / 2 > tt) I--;
                ti[u] = I;
                tj[u] = tt - I * (I + 1) / 2;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int rr = r0 + 16 * ti[u] + rq + 4 * q, col = r0 + 16 * tj[u] + cc;
                    acc[u][q] = (on[u] && rr < n && col < n) ? S[(size_t)rr * n + col] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int kk = 0; kk < kNB / 4; kk++) {
                    const double av = -Pn[(16 * ti[u] + cc) * kPS + 4 * kk + rq];
                    const double bv = Pn[(16 * tj[u] + cc) * kPS + 4 * kk + rq];
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[u], 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int rr = r0 + 16 * ti[u] + rq + 4 * q, col = r0 + 16 * tj[u] + cc;
                    if (on[u] && rr < n && col < n) S[(size_t)rr * n + col] = acc[u][q];
                }
            }
        }
        __syncthreads();
        stamp(2);
    }
    if (bad) {
        if (tid == 0) flag[0] = 0;
        for (int i = tid; i < n; i += nt) x[i] = 0.0;
        return;
    }
    // ---- (d) backward: x_p = Linv_p^T (y_p - L21_p^T x_below), panels from the last ----
    const int npan = (n + kNB - 1) / kNB;
    const int G = nt >> 5;
    for (int pb = npan - 1; pb >= 0; pb--) {
        const int k0 = pb * kNB, kb = min(kNB, n - k0);
        const int r0 = k0 + kb;
        {
            const int cI = tid & 31, g = tid >> 5;   // g = 0..G-1
            double s2 = 0.0;
            if (cI < kb)
                for (int r = r0 + g; r < n; r += G) s2 += S[(size_t)r * n + k0 + cI] * y[r];
            red[g * 33 + cI] = s2;
        }
        for (int t = tid; t < 32 * 32; t += nt) Li[(t >> 5) * 33 + (t & 31)] = Lsave[(size_t)pb * 1024 + t];
        __syncthreads();
        if (tid < 32) {
            double w = 0.0;
            if (tid < kb) {
                double s2 = 0.0;
                for (int g = 0; g < G; g++) s2 += red[g * 33 + tid];
                w = y[k0 + tid] - s2;
            }
            invp[tid] = w;                       // reuse as the 32-vector w
        }
        __syncthreads();
        if (tid < kb) {
            double s2 = 0.0;
#pragma unroll
            for (int k = 0; k < 32; k++) s2 += Li[k * 33 + tid] * invp[k];
            y[k0 + tid] = s2;
        }
        __syncthreads();
    }
    stamp(3);
    for (int i = tid; i < n; i += nt) x[i] = y[i];
    if (tid == 0) flag[0] = 1;
}

__global__ __launch_bounds__(512) void k_ba_cholesky(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    const BaArgs& a = args[act[blockIdx.x]];
    BA_PHASE(kPhTrial)
    if (a.n == 0) {
        if (threadIdx.x == 0) a.flag[0] = 1;
        return;
    }
    chol_solve(a.S, a.bs, a.x, a.n, a.flag, a.Lsave, nullptr);
}

__global__ __launch_bounds__(512) void k_chol_test(double* S, const double* bs, double* x, int n, int* flag,
                                                   double* Lsave, unsigned long long* dbg) {
    chol_solve(S, bs, x, n, flag, Lsave, dbg);
}

// ---------------------------------------------------------------------------
// back-substitution + updates (push saves the old state)
// ---------------------------------------------------------------------------
// landmark m: xl = Dinv (b_l - Hpl^T xp), X += xl (old X saved); returns xl (lambda xl + b_l)
template <bool Stereo>
__device__ __forceinline__ double backsub_point(const BaArgs& a, int m) {
    const double* bl = a.b + a.n + 3 * m;
    double c[3] = {bl[0], bl[1], bl[2]};
    for (int k = a.pt_ptr[m]; k < a.pt_ptr[m + 1]; k++) {
        const int e = a.pt_edges[k];
        const int oi = a.opt[a.e_pose[e]];
        if (oi < 0) continue;
        double A[JacDim<Stereo>::kA], B[JacDim<Stereo>::kB];
        const double w = lin_ab<Stereo>(a, e, oi, A, B);   // Hpl_e^T xp = w A^T (B xp)
        [[maybe_unused]] constexpr int a2 = Stereo ? 6 : 0, b2 = Stereo ? 12 : 0;   // the third rows (unused unless Stereo)
        const double* xp = a.x + 6 * oi;
        double u0 = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            u0 += B[r] * xp[r]; u1 += B[6 + r] * xp[r];
            if constexpr (Stereo) u2 += B[b2 + r] * xp[r];
        }
        u0 *= w; u1 *= w; u2 *= w;
#pragma unroll
        for (int cc = 0; cc < 3; cc++) c[cc] -= rows_dot<Stereo>(A[cc], u0, A[3 + cc], u1, A[a2 + cc], u2);
    }
    double Di[9];
    if (a.fused) {
        dinv_of(a, m, Di);
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) Di[k] = a.Dinv[9 * m + k];
    }
    double* X = a.pts + 3 * m;
    const double lambda = *a.lambda;
    double sc = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double xl = Di[3 * r] * c[0] + Di[3 * r + 1] * c[1] + Di[3 * r + 2] * c[2];
        a.x[a.n + 3 * m + r] = xl;
        const double xo = X[r];
        // sc1 for a small problem: its trial's last workgroup may restore pts from pts_bak in
        // the same launch (ctl_end_body); the others' k_ba_pop runs in a launch of its own
        if (a.small) {
            st_agent(a.pts_bak + 3 * m + r, xo);
            st_agent(X + r, xo + xl);
        } else {
            a.pts_bak[3 * m + r] = xo;
            X[r] = xo + xl;
        }
        sc += xl * (lambda * xl + bl[r]);
    }
    return sc;
}

// one thread per landmark (back-substitution) and, in the first workgroups, one per pose
// (T <- exp(xp) T, the former k_ba_update_poses: it reads xp and writes the poses, which the
// landmarks' back-substitution does not touch)
template <bool Stereo>
__global__ __launch_bounds__(256) void k_ba_backsub(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    BA_PROLOGUE
    BA_PHASE(kPhTrial)
    if (bx_ * (int)blockDim.x >= max(a.M, a.P)) return;   // uniform
    const int m = bx_ * blockDim.x + threadIdx.x;
    if (m < a.P) {
        double* T = a.pose + 8 * m;
#pragma unroll
        for (int k = 0; k < 8; k++) a.pose_bak[8 * m + k] = T[k];
        const int oi = a.opt[m];
        if (oi >= 0) se3_update(a.x + 6 * oi, T);
    }
    // the landmark part of computeScale, sum of xl (lambda xl + b_l), per workgroup (uniform: every
    // thread reaches the workgroup sum's barriers once)
    __shared__ double sh[4];
    const double t = block_sum(m < a.M ? backsub_point<Stereo>(a, m) : 0.0, sh);
    if (threadIdx.x == 0) a.part[a.npart_e + bx_] = t;
    if (bx_ == 0)   // the scale slots past this launch's workgroups (npart_m counts k_ba_backsub_errs')
        for (int i = (max(a.M, a.P) + 255) / 256 + (int)threadIdx.x; i < a.npart_m; i += blockDim.x)
            a.part[a.npart_e + i] = 0.0;
}

// the fused trial (BaArgs::fused; every unsharded problem since r06, small ones only before): the
// back-substitution and the trial's errors in ONE launch, no k_ba_schur_points before it and no
// k_ba_errors(2) after it. The trial's poses go to pose_bak (pose keeps the accepted state until
// the controller commits). Every workgroup forms all P new poses in LDS (P <= kFusedMaxP: a few
// se3 updates per thread, overlapping its landmark loads) and takes kBsL landmarks, four lanes per
// landmark (r06; one thread per landmark and 256 per workgroup before: 8 workgroups at C4): the
// lanes split the landmark's edges for Hpl^T xp (summed over the quad), each forms the new point
// (the same bits in all four) and then the errors of its own edges with it. chi2 and the landmark
// scale terms leave as workgroup partials and the problem's last workgroup runs the controller
// step (ctl_end_body: commit the poses or take the points back)
constexpr int kFusedMaxP = 512;
constexpr int kBsL = 64;   // landmarks per workgroup of k_ba_backsub_errs
template <bool Stereo>
__global__ __launch_bounds__(256) void k_ba_backsub_errs(const BaArgs* __restrict__ args, const int* __restrict__ act,
                                                         int* const* donep) {
    BA_PROLOGUE
    int* const done = done_of(donep);
    BA_PHASE(kPhTrial)
    __shared__ double Tn[8 * kFusedMaxP];   // the trial's poses
    __shared__ double sh[4];
    __shared__ int lastf;
    const int nwg = (max(a.M, a.P) + kBsL - 1) / kBsL;   // this problem's partial slots (<= npart_e, npart_m)
    const int m = bx_ * kBsL + (threadIdx.x >> 2), sub = threadIdx.x & 3;
    // this lane's edges of landmark m: its back-substitution terms (their loads go out first)
    int k0 = 0, k1 = 0;
    if (m < a.M) { k0 = a.pt_ptr[m]; k1 = a.pt_ptr[m + 1]; }
    // r06: the landmark's own words and this lane's first two edges' observation words are loaded
    // here, with the first loop's: after the barrier below everything would be loaded again, two
    // dependent round trips (edge list -> edge words) in front of the errors
    double Hm[9] = {}, blv[3] = {}, Xo[3] = {};
    if (m < a.M) {
#pragma unroll
        for (int k = 0; k < 9; k++) Hm[k] = a.Hll[9 * m + k];
#pragma unroll
        for (int r = 0; r < 3; r++) { blv[r] = a.b[a.n + 3 * m + r]; Xo[r] = a.pts[3 * m + r]; }
    }
    int ce[2] = {-1, -1}, cp[2] = {0, 0};
    double co0[2] = {0, 0}, co1[2] = {0, 0}, ci[2] = {0, 0};
    double cur[2] = {-1.0, -1.0};   // Stereo: the preloaded edges' right coordinates
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;   // - sum_e Hpl_e^T xp over this lane's edges
    for (int k = k0 + sub, j = 0; k < k1; k += 4, j++) {
        const int e = a.pt_edges[k];
        const int pe = a.e_pose[e];
        if (j < 2) {
            ce[j] = e; cp[j] = pe;
            co0[j] = a.e_obs[2 * e]; co1[j] = a.e_obs[2 * e + 1]; ci[j] = a.e_info[e];
            if constexpr (Stereo) cur[j] = a.e_ur[e];
        }
        const int oi = a.opt[pe];
        if (oi < 0) continue;
        double A[JacDim<Stereo>::kA], B[JacDim<Stereo>::kB];
        const double w = lin_ab<Stereo>(a, e, oi, A, B);   // Hpl_e^T xp = w A^T (B xp)
        [[maybe_unused]] constexpr int a2 = Stereo ? 6 : 0, b2 = Stereo ? 12 : 0;   // the third rows (unused unless Stereo)
        const double* xp = a.x + 6 * oi;
        double u0 = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            u0 += B[r] * xp[r]; u1 += B[6 + r] * xp[r];
            if constexpr (Stereo) u2 += B[b2 + r] * xp[r];
        }
        u0 *= w; u1 *= w; u2 *= w;
        c0 -= rows_dot<Stereo>(A[0], u0, A[3], u1, A[a2], u2);
        c1 -= rows_dot<Stereo>(A[1], u0, A[4], u1, A[a2 + 1], u2);
        c2 -= rows_dot<Stereo>(A[2], u0, A[5], u1, A[a2 + 2], u2);
    }
    for (int p = threadIdx.x; p < a.P; p += blockDim.x) {
        double T[8];
#pragma unroll
        for (int k = 0; k < 8; k++) T[k] = a.pose[8 * p + k];
        const int oi = a.opt[p];
        if (oi >= 0) se3_update(a.x + 6 * oi, T);
#pragma unroll
        for (int k = 0; k < 8; k++) Tn[8 * p + k] = T[k];
        if (bx_ == 0) {   // sc1: read back by the problem's last workgroup in this launch
#pragma unroll
            for (int k = 0; k < 8; k++) st_agent(a.pose_bak + 8 * p + k, T[k]);
        }
    }
    // the quad's sum (butterfly: the same bits in its four lanes)
    c0 += __shfl_xor(c0, 1, 64); c1 += __shfl_xor(c1, 1, 64); c2 += __shfl_xor(c2, 1, 64);
    c0 += __shfl_xor(c0, 2, 64); c1 += __shfl_xor(c1, 2, 64); c2 += __shfl_xor(c2, 2, 64);
    double sc = 0.0, Xn[3] = {0.0, 0.0, 0.0};
    if (m < a.M) {   // xl = Dinv (b_l - Hpl^T xp), X += xl (old X saved): every lane of the quad
        const double cv[3] = {blv[0] + c0, blv[1] + c1, blv[2] + c2};
        const double lambda = *a.lambda;
        double D[9], Di[9];   // dinv_of's expressions on the preloaded Hll
#pragma unroll
        for (int k = 0; k < 9; k++) D[k] = Hm[k] + (k % 4 == 0 ? lambda : 0.0);
        inv3(D, Di);
        double* X = a.pts + 3 * m;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double xl = Di[3 * r] * cv[0] + Di[3 * r + 1] * cv[1] + Di[3 * r + 2] * cv[2];
            const double xo = Xo[r];
            Xn[r] = xo + xl;
            if (sub == 0) {
                a.x[a.n + 3 * m + r] = xl;
                // sc1 for a small problem: its trial's last workgroup may restore pts from pts_bak
                // in this launch (ctl_end_body)
                st_agent(a.pts_bak + 3 * m + r, xo);
                st_agent(X + r, Xn[r]);
                sc += xl * (lambda * xl + blv[r]);
            }
        }
    }
    __syncthreads();   // the trial's poses in Tn
    double chi = 0.0;
    for (int k = k0 + sub, j = 0; k < k1; k += 4, j++) {
        if (j < 2) {   // from the preloaded words (edge_error_at's expressions)
            const int e = ce[j];
            const double* T = Tn + 8 * cp[j];
            double cx, cy, cz;
            qrot(load_q(T), Xn[0], Xn[1], Xn[2], cx, cy, cz);
            cx += T[4]; cy += T[5]; cz += T[6];
            double e0, e1, e2, chi2, r0, r1;
            edge_terms_of<Stereo>(a, co0[j], co1[j], cur[j], ci[j], cx, cy, cz, e0, e1, e2, chi2, r0, r1);
            store_terms<Stereo>(a, e, e0, e1, e2, chi2, r0, r1);
            chi += r0;
        } else {
            const int e = a.pt_edges[k];
            chi += edge_error_at<Stereo>(a, e, Tn + 8 * a.e_pose[e], Xn);
        }
    }
    const double tc = block_sum(chi, sh);
    const double ts = block_sum(sc, sh);
    if (threadIdx.x == 0 && bx_ < nwg) {
        st_agent(a.part + bx_, tc);
        st_agent(a.part + a.npart_e + bx_, ts);
    }
    if (bx_ == 0) {   // the slots past this problem's workgroups
        for (int i = nwg + (int)threadIdx.x; i < a.npart_e; i += blockDim.x) st_agent(a.part + i, 0.0);
        for (int i = nwg + (int)threadIdx.x; i < a.npart_m; i += blockDim.x) st_agent(a.part + a.npart_e + i, 0.0);
    }
    if (last_arrival(&a.ctl->arrive_t, gridDim.x, &lastf)) ctl_end_body(a, act[by_], done, sh);
}

// restore the pushed state of every problem whose controller flagged its trial rejected (ctl->pop);
// launched once per slot unless every problem of the call is small (those restore in ctl_end_body)
__global__ __launch_bounds__(256) void k_ba_pop(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    BA_PROLOGUE
    if (!a.ctl->pop) return;
    const int i = bx_ * blockDim.x + threadIdx.x;
    // (a fused trial left the poses unmoved: pose_bak holds the rejected trial's)
    if (i < 8 * a.P && !a.fused) a.pose[i] = a.pose_bak[i];
    if (i < 3 * a.M) a.pts[i] = a.pts_bak[i];
}

// Envelope packing of S for the sharded all-reduce: 32-row tile R keeps columns [32 rf[R],
// 32 R + 32) (the lower envelope, which is all any Cholesky here reads; outside it every shard's
// S is zero), packed row-major per tile at toff[R]. pack (dir 0) S -> buf, unpack (dir 1) buf -> S.
__global__ __launch_bounds__(256) void k_ba_env_pack(double* __restrict__ S, int n, const int* __restrict__ rf,
                                                     const long long* __restrict__ toff, double* __restrict__ buf,
                                                     int dir) {
    const int R = blockIdx.y;
    const int c0 = 32 * rf[R], c1 = min(32 * R + 32, n), w = c1 - c0;
    const int rows = min(32, n - 32 * R);
    double* tb = buf + toff[R];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * w; i += gridDim.x * blockDim.x) {
        const int r = i / w, c = i - r * w;
        double* e = S + (size_t)(32 * R + r) * n + c0 + c;
        if (dir == 0) tb[i] = *e;
        else *e = tb[i];
    }
}

// red[0] = the sum of the robust chi2 terms over the problem's edges (one workgroup, fixed order)
__device__ void ba_reduce_body(const BaArgs& a, double* sh) {
    double v = 0;
    for (int e = threadIdx.x; e < a.E; e += blockDim.x) v += a.e_rho0[e];
    v = block_sum(v, sh);
    if (threadIdx.x == 0) a.red[0] = v;
}

// a shard's part of the initial activeRobustChi2 (summed over the shards before k_ba_sh_init)
__global__ __launch_bounds__(1024) void k_ba_reduce(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    __shared__ double sh[16];
    ba_reduce_body(args[act[blockIdx.x]], sh);
}

// ---------------------------------------------------------------------------
// Levenberg-Marquardt control on the device: one slot = the build kernels, the trial start
// (ctl_begin_*), the trial kernels, the trial end (ctl_end_*), pop. The rules are g2o's
// (OptimizationAlgorithmLevenberg::solve + SparseOptimizer::optimize, U:Thirdparty/g2o), applied
// per problem on the device so that a whole solve needs no host round trip per trial: unsharded,
// in the last workgroup of k_ba_lin and of the trial's error kernel; sharded, in the k_ba_sh_*
// launches around the collectives.
// ---------------------------------------------------------------------------
// initial activeRobustChi2 (errors computed by the preceding k_ba_errors)
__global__ __launch_bounds__(1024) void k_ba_ctl_init(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    __shared__ double sh[16];
    const BaArgs& a = args[act[blockIdx.x]];
    ba_reduce_body(a, sh);
    if (threadIdx.x == 0) {
        LmCtl& c = *a.ctl;
        c.currentChi = a.red[0];
        c.initChi = a.red[0];
    }
}

// the host's stop request (LocalMapping mbAbortBA): a problem between iterations ends now, one in a
// trial at the end of its iteration (ctl_end_decide)
__global__ void k_ba_ctl_stop(LmCtl* __restrict__ ctl, int B, int* const* donep) {
    int* const done = done_of(donep);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    ctl[b].stop = 1;
    if (ctl[b].phase == kPhBuild) {
        ctl[b].phase = kPhDone;
        post_done(done, b);
    }
}

// after the build: lambda initialisation on the first iteration (1e-5 max diagonal, from k_ba_lin's
// per-workgroup maxima: sc1 loads), then trials. Run by the last workgroup of k_ba_lin.
__device__ void ctl_begin_apply(const BaArgs& a, double maxdiag) {
    LmCtl& c = *a.ctl;
    if (c.it == 0) {
        *const_cast<double*>(a.lambda) = 1e-5 * maxdiag;
        c.ni = 2;
        c.nBad = 0;
    }
    c.qmax = 0;
    c.rho = 0;
    c.errors_valid = 1;   // the build just done used the current state's errors
    c.phase = kPhTrial;
}
// every thread of the work-group calls it: on the first iteration the largest diagonal over the
// build's nlin work-group maxima is a block reduction (r06: thread 0 alone read them one after
// another, 94 us of the first C5 build for its 712 partials)
__device__ void ctl_begin_body(const BaArgs& a, int nlin, int* done_flags, int prob, double* sh) {
    double m = 0.0;
    if (a.ctl->it == 0) {   // block-uniform: written by an earlier launch
        for (int i = threadIdx.x; i < nlin; i += blockDim.x) m = fmax(m, ld_agent(a.part + i));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
        __syncthreads();
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) m = fmax(m, sh[w]);
    }
    if (threadIdx.x != 0) return;
    if (a.ctl->stop) {   // a stop relayed before this iteration: g2o's terminate() check, no trial
        LmCtl& c = *a.ctl;
        c.phase = kPhDone;
        post_done(done_flags, prob);
        return;
    }
    ctl_begin_apply(a, m);
}

// after a trial: chi2 and scale, rho, accept (lambda shrink) or reject (lambda *= ni, pop), and
// the end-of-iteration rules. Run by the last workgroup of k_ba_errors(2) of the problem: the chi2
// partials are that launch's (sc1 loads), the scale partials k_ba_backsub's.
__device__ void ctl_end_sums(const BaArgs& a, double* sh) {
    {   // chi2 and the scale from the trial kernels' workgroup partials (k_ba_errors, k_ba_backsub)
        double v = 0.0;
        for (int i = threadIdx.x; i < a.npart_e; i += blockDim.x) v += ld_agent(a.part + i);
        v = block_sum(v, sh);
        if (threadIdx.x == 0) a.red[0] = v;
        const double lambda = *a.lambda, lam_pose = a.lead ? lambda : 0.0;
        v = 0.0;
        for (int j = threadIdx.x; j < a.n; j += blockDim.x) v += a.x[j] * (lam_pose * a.x[j] + a.b[j]);
        for (int i = threadIdx.x; i < a.npart_m; i += blockDim.x) v += ld_agent(a.part + a.npart_e + i);
        v = block_sum(v, sh);
        if (threadIdx.x == 0) a.red[1] = v;
    }
}
// thread 0: the g2o rules on red[0] (chi2) and red[1] (scale)
__device__ void ctl_end_decide(const BaArgs& a, int prob, int* done_flags) {
    LmCtl& c = *a.ctl;
    double* lambda = const_cast<double*>(a.lambda);
    const bool ok2 = a.flag[0] != 0;
    const double tempChi = ok2 ? a.red[0] : DBL_MAX;
    double rho = c.currentChi - tempChi;
    rho /= (a.red[1] + 1e-3);
    if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - pow((2 * rho - 1), 3.0);
        alpha = fmin(alpha, 2. / 3.);
        *lambda *= fmax(1. / 3., alpha);
        c.ni = 2;
        if (c.early_stop) {
            if ((c.currentChi - tempChi) < 1e-3 * c.currentChi) c.nBad++;
            else c.nBad = 0;
        }
        c.currentChi = tempChi;
        c.pop = 0;
    } else {
        *lambda *= c.ni;
        c.ni *= 2;
        c.pop = 1;
    }
    c.rho = rho;
    c.qmax++;
    c.trials++;
    if (rho < 0 && c.qmax < 10 && !c.stop) return;   // another trial of this iteration
    c.it++;
    c.errors_valid = rho > 0;   // rejected: the device errors belong to the popped trial
    bool done = (c.qmax == 10 || rho == 0) || c.stop;   // stop: SparseOptimizer's force-stop, at the iteration end
    if (c.early_stop && c.nBad >= 3) done = true;
    if (c.it >= c.iterations) done = true;   // the budget (a sharded slot's k_ba_errors(1) checks it too), no idle slot
    c.phase = done ? kPhDone : kPhBuild;
    if (done) post_done(done_flags, prob);
}
__device__ void ctl_end_body(const BaArgs& a, int prob, int* done_flags, double* sh) {
    ctl_end_sums(a, sh);
    if (threadIdx.x == 0) ctl_end_decide(a, prob, done_flags);
    if (!a.small && !a.fused) return;
    // a small problem: this workgroup restores a rejected trial's state (k_ba_pop), so that needs
    // no launch of its own (the restored state's errors, g2o's computeActiveErrors at the next
    // iteration's start, come from the next k_ba_lin).
    // Fused trials (k_ba_backsub_errs) left the poses unmoved and the new ones in pose_bak: an
    // accepted trial commits them, a rejected one only takes the points back
    __syncthreads();
    // The backups and the trial's points / errors were stored by other workgroups of this launch
    // (other XCDs) with sc1 stores drained before their arrival: sc1 loads here see them, and the
    // sc1 stores below are the last writes of those words.
    const LmCtl& c = *a.ctl;
    if (a.fused) {
        if (!c.pop) {
            for (int i = threadIdx.x; i < 8 * a.P; i += blockDim.x) st_agent(a.pose + i, ld_agent(a.pose_bak + i));
            return;
        }
        // r06: larger problems take the fused trial too; their points come back in k_ba_pop (3M
        // words are too many for this one work-group)
        if (!a.small) return;
    } else {
        if (!c.pop) return;
        for (int i = threadIdx.x; i < 8 * a.P; i += blockDim.x) st_agent(a.pose + i, ld_agent(a.pose_bak + i));
    }
    for (int i = threadIdx.x; i < 3 * a.M; i += blockDim.x) st_agent(a.pts + i, ld_agent(a.pts_bak + i));
    // the restored state's errors, when the iteration ended here, are taken by the next build
    // (k_ba_lin's fresh terms): rewritten here, in this launch, they raced the other workgroups'
    // plain stores of the trial's errors
}

// ---- sharded device-driven rounds (BaArgs::sync): the controller's reductions, a collective
// over the shards, then its decisions, each a launch of one workgroup per problem ----
// build: red[2] = the largest |diagonal| (landmarks: k_ba_lin's workgroup maxima; poses: the
// summed Hpp_g, since a shard's own Hpp holds only its edges' terms)
__global__ __launch_bounds__(256) void k_ba_sh_maxdiag(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    const BaArgs& a = args[act[blockIdx.x]];
    if (!in_phase(a, kPhBuild)) return;
    const int mP = (a.M + kLinL - 1) / kLinL;   // k_ba_lin's landmark workgroups
    double m = 0.0;
    for (int i = threadIdx.x; i < mP; i += blockDim.x) m = fmax(m, ld_agent(a.part + i));
    for (int i = threadIdx.x; i < 6 * a.np; i += blockDim.x) m = fmax(m, fabs(a.Hpp_g[36 * (i / 6) + 7 * (i % 6)]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) a.red[2] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
__global__ void k_ba_sh_init(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    const BaArgs& a = args[act[blockIdx.x]];
    if (threadIdx.x == 0) { a.ctl->currentChi = a.red[0]; a.ctl->initChi = a.red[0]; }
}
__global__ void k_ba_sh_begin(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    const BaArgs& a = args[act[blockIdx.x]];
    if (threadIdx.x == 0 && in_phase(a, kPhBuild)) ctl_begin_apply(a, a.red[2]);
}
__global__ __launch_bounds__(1024) void k_ba_sh_sums(const BaArgs* __restrict__ args, const int* __restrict__ act) {
    __shared__ double sh[16];
    const BaArgs& a = args[act[blockIdx.x]];
    if (in_phase(a, kPhTrial)) ctl_end_sums(a, sh);
}
__global__ void k_ba_sh_end(const BaArgs* __restrict__ args, const int* __restrict__ act, int* const* donep) {
    int* const done = done_of(donep);
    const BaArgs& a = args[act[blockIdx.x]];
    if (threadIdx.x == 0 && in_phase(a, kPhTrial)) ctl_end_decide(a, act[blockIdx.x], done);
}
// the in-process form of a collective over B shards: dst[s][i] = sum (op 0) / max (op 1) over the
// shards of src[s'][i], in shard order (deterministic); dst may alias src
// sum (op 0) or max (op 1) of nsrc buffers into each of ndst buffers (a destination may alias a
// source: every element is read before it is written, by the same thread)
__global__ __launch_bounds__(256) void k_ba_multi_reduce(const double* const* __restrict__ src, int nsrc,
                                                         double* const* __restrict__ dst, int ndst, size_t count, int op) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        double acc = op ? -1.0e300 : 0.0;
        for (int b = 0; b < nsrc; b++) {
            const double v = src[b][i];
            acc = op ? fmax(acc, v) : acc + v;
        }
        for (int b = 0; b < ndst; b++) dst[b][i] = acc;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
#define BAOK(x)                                                                                    \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            std::fprintf(stderr, "orbhip ba: %s: %s\n", #x, hipGetErrorString(e_));                \
            return ORBHIP_ERR_DEVICE;                                                              \
        }                                                                                          \
    } while (0)

namespace {

inline void se3_from_float(const float* q, const float* t, double* out) {
    double x = q[0], y = q[1], z = q[2], w = q[3];
    if (w < 0) { x = -x; y = -y; z = -z; w = -w; }
    const double nn = std::sqrt(x * x + y * y + z * z + w * w);
    out[0] = x / nn; out[1] = y / nn; out[2] = z / nn; out[3] = w / nn;
    out[4] = t[0]; out[5] = t[1]; out[6] = t[2]; out[7] = 0;
}

template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t c) {
        if (p && c <= n) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(c, 1) * sizeof(T));
        if (e == hipSuccess) n = c;
        return e;
    }
};

template <typename T>
struct HBuf {   // pinned host staging
    T* p = nullptr;
    size_t n = 0;
    ~HBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t c) {
        if (p && c <= n) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
        c = std::max<size_t>(c + c / 4, 64);   // grow geometrically: pinning is expensive
        hipError_t e = hipHostMalloc((void**)&p, c * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = c;
        return e;
    }
};

}  // namespace

struct BaWorkspace {
    DBuf<double> dbl;      // all fp64 per-problem arrays, packed (segment map at place_problem)
    DBuf<int> act;         // active problem lists (several slots)
    DBuf<double> lam;      // per-problem lambda
    DBuf<LmCtl> ctl;       // per-problem LM state
    HBuf<LmCtl> hctl;      // its pinned staging (initial state up, final state down)
    HBuf<double> hdbl;     // staging: [e_chi2 | pose,pts | obs,info | the int arrays | BaArgs] of every problem
    HBuf<int> h_act;       // pinned: the active lists' staging
    // sharded solve over RCCL (orbhip_comm_init): landmarks partitioned, poses replicated
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    DBuf<int> dstop;           // stop-flag consensus (all-reduce max)
    DBuf<double> envbuf;       // S's union envelope, packed for the all-reduce (k_ba_env_pack)
    DBuf<long long> envoff;    // its per-32-row-tile offsets
    HBuf<int> h_stop;          // pinned
    int* h_done = nullptr;     // pinned, mapped: per problem, set by the device when its LM run ends
    int* d_done = nullptr;     // its device address
    DBuf<int*> d_donep;        // ... stored in device memory: what the kernels get
    size_t done_cap = 0;
    HBuf<int> hto;             // pinned: the persistent solver's hand-off timeout count per problem
    long long dag_timeouts = 0, dag_reruns = 0;
    std::vector<Prep> prep;    // the per-problem host preparations of the last call (capacity reused)
    NdWorkspace* nd = nullptr; // nested-dissection solves (created on first use)
    std::vector<NdWorkspace*> nds;   // sharded solves by segments: one per shard of this process
    DBuf<double*> ptab;        // in-process shards: the collectives' pointer tables
    DBuf<int> dint4;           // RCCL: small consensus all-reduces (plan, stop)
    DBuf<unsigned char> uadj;  // RCCL, replicated form: the union pose adjacency (all-reduce max)
    HBuf<int> h_int4;          // pinned
};

BaWorkspace* ba_create() { return new BaWorkspace(); }

void ba_destroy(BaWorkspace* w) {
    if (!w) return;
    if (w->comm) (void)ncclCommDestroy(w->comm);
    if (w->nd) nd_destroy(w->nd);
    for (NdWorkspace* q : w->nds) nd_destroy(q);
    if (w->h_done) (void)hipHostFree(w->h_done);
    delete w;
}

// ---------------------------------------------------------------------------
// ba_solve_batch: the steps below, in the order they run, over one BaCall on its stack
// ---------------------------------------------------------------------------
namespace {

// Every environment switch of a call, read in one place at its top (read_switches).
struct BaSwitches {
    // read once per process
    bool timing;          // ORBHIP_BA_TIMING: one line of host phase times per call
    int chunk;            // ORBHIP_SCHUR_CHUNK: pairs per Schur work item (0: chosen per call)
    int prep_threads;     // ORBHIP_PREP_THREADS=k: one large problem's pair lists on k host threads (1)
    bool force_blocked;   // ORBHIP_CHOL_BLOCKED: the one-launch-per-panel blocked solver for the large problems
    int dag_min;          // ORBHIP_CHOL_DAG_MIN: the smallest n a lone problem takes the DAG solver at (128)
    // read on every call (the tests flip them)
    long small_words;     // ORBHIP_BA_SMALL_WORDS: see BaArgs::small (32768)
    bool nd;              // ORBHIP_ND=0: no nested dissection
    int nd_k;             // ORBHIP_ND_K=k: k segments (0: the planner's choice)
    int nd_min;           // ORBHIP_ND_MIN: the smallest n considered for dissection (960)
    bool shard_nd;        // ORBHIP_SHARD_ND=0: sharded solves take the replicated form
    bool shard_full_s;    // ORBHIP_SHARD_FULL_S: RCCL all-reduces the whole S, not its packed envelope
    int lin_ppw;          // ORBHIP_LIN_PPW=1/4: poses per pose work-group of k_ba_lin (0: by batch size)
    bool fused;           // ORBHIP_BA_FUSED=0: separate k_ba_backsub + k_ba_errors(2) trials
    bool dag_rerun;       // ORBHIP_DAG_RERUN=0: a DAG hand-off timeout is reported, not re-run
};

BaSwitches read_switches() {
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    auto off = [](const char* name) { const char* s = std::getenv(name); return s && s[0] == '0'; };
    auto num = [](const char* name, int dflt) { const char* s = std::getenv(name); return s ? std::atoi(s) : dflt; };
    static const BaSwitches once = {set("ORBHIP_BA_TIMING"), num("ORBHIP_SCHUR_CHUNK", 0), num("ORBHIP_PREP_THREADS", 1),
                                    set("ORBHIP_CHOL_BLOCKED"), num("ORBHIP_CHOL_DAG_MIN", 128)};
    BaSwitches s = once;
    const char* sw = std::getenv("ORBHIP_BA_SMALL_WORDS");
    s.small_words = sw ? std::atol(sw) : 32768;
    s.nd = !off("ORBHIP_ND");
    s.nd_k = num("ORBHIP_ND_K", 0);
    s.nd_min = num("ORBHIP_ND_MIN", 960);
    s.shard_nd = !off("ORBHIP_SHARD_ND");
    s.shard_full_s = set("ORBHIP_SHARD_FULL_S");
    const char* ppw = std::getenv("ORBHIP_LIN_PPW");
    s.lin_ppw = ppw ? (std::atoi(ppw) == 1 ? 1 : 4) : 0;
    s.fused = !off("ORBHIP_BA_FUSED");
    s.dag_rerun = !off("ORBHIP_DAG_RERUN");
    return s;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
unsigned gx(int n_, int b_) { return (unsigned)std::max(1, (n_ + b_ - 1) / b_); }

// The collectives of a sharded slot: site s sums (or maxes) src[b] into dst[b] over the shards
enum { kHpp, kRed0, kRed2, kRed01, kRepS, kRepBs, kNdPack, kNdBz, kNdX, kSites };
struct Site { std::vector<double*> src, dst; size_t count = 0; int op = 0; size_t tab = 0; };

// A step's request to run the call again (ba_solve_batch re-enters itself, after its last use of
// this frame's preparations: the re-entered call reuses the workspace)
enum { kRerunNoNd = -1001, kRerunNoDag = -1002 };

// What one call's steps share; lives on the stack of ba_solve_batch
struct BaCall {
    // the call's arguments
    BaWorkspace* ws; const orbhip_ba_problem* const* probs; int B; orbhip_ba_result* const* res;
    const volatile int* stop; hipStream_t st; int shard_mode; bool no_dag, no_nd; const BaStereoExt* sx;
    BaSwitches sw;
    bool stereo = false;    // some edge is a stereo edge: the Stereo = true kernels on every problem
    bool sharded = false, rccl = false;
    int nth = 1;            // host threads
    double t_start = 0, t_prepare = 0, t_prep = 0, t_pack = 0, t_solve = 0;
    Prep* pp = nullptr;     // ws->prep: the per-problem preparations
    int local_bad = 0;      // RCCL: this rank's shards are invalid (its verdict travels in the first collective)
    int dag_helpers = 0;
    // the sharded plan
    int seg0 = 0;           // segment of problem 0
    NdPlan ndp;             // the segments of a solve by keyframe segments (nd_sh)
    bool nd_sh = false;
    std::vector<int> ubi, ubj;   // the replicated form's union block structure (when dissected)
    // the packed buffers: sizes and starts (doubles) of the segments, device and staging bases
    size_t nC = 0, nA = 0, nR = 0, sC = 0, sA = 0, sU = 0, sI = 0, sG = 0, sR = 0;
    double* D = nullptr; int* I = nullptr; double* hd = nullptr; int* hi = nullptr;
    BaArgs* ha = nullptr; BaArgs* dArgs = nullptr;
    std::vector<DagDev> dd;
    size_t env_total = 0;   // RCCL, replicated, B == 1: doubles of S's packed union envelope (0: the whole S)
    // launch widths and forms
    int maxM = 0, maxE = 0, maxP = 0, maxNp = 0, maxN = 0, maxItems = 0, maxPM = 0;
    bool s_readonly = false;   // S is zeroed once, not per trial
    size_t chol_lds = 0;
    int ns = 0;             // problems on the single-workgroup solvers (act slot 3)
    bool all_small = true;  // every problem restores / refreshes in its trial's last workgroup
    bool fused = false;     // the fused trial (k_ba_backsub_errs)
    unsigned gbs = 1;       // ... its work-groups
    int lin_ppw = 4;        // poses per pose work-group of k_ba_lin
    int* d_act = nullptr; int* h_act = nullptr; LmCtl* dctl = nullptr;
    std::vector<const int*> tw;   // the timeout words of every persistent solve of this call (ndag of them)
    int ndag = 0;
    std::vector<Site> sites;
    int* const* donep = nullptr;  // {done, stop} of post_done / relay_host_stop, on the device
    int* h_stopw = nullptr;       // the host's side of the relayed stop word (null: nothing to relay)
    bool stop_sent = false;
    bool outputs_in = false;      // the speculative copies behind the last slots brought the outputs

    // "large": solved on its own (dissection, DAG or blocked); the rest share one single-workgroup launch
    bool large(int b) const { return pp[b].use_nd || pp[b].use_nd_sh || pp[b].use_dag || pp[b].n > kCholSmallN; }
    NdWorkspace* nd_of(int b) const { return B == 1 ? ws->nd : ws->nds[b]; }
};

// n values of `host` up to `dev`, all-reduced (max or min) over the ranks, back into `host`; the
// stream is synchronised. ORBHIP_ERR_DEVICE on any failure.
template <typename T>
int rccl_consensus(const BaCall& c, T* host, T* dev, size_t n, ncclRedOp_t op) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 1, "ints or bytes");
    const ncclDataType_t ty = sizeof(T) == 1 ? ncclUint8 : ncclInt32;
    if (hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, c.st) != hipSuccess ||
        ncclAllReduce(dev, dev, n, ty, op, c.ws->comm, c.st) != ncclSuccess ||
        hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c.st) != hipSuccess ||
        hipStreamSynchronize(c.st) != hipSuccess)
        return ORBHIP_ERR_DEVICE;
    return ORBHIP_OK;
}

// ---- step 1: arguments; a call with stereo edges (orbhip_ba_solve_stereo*: some edge_ur >= 0) runs
// the Stereo = true kernels on every problem of it, every other call the monocular kernels ----
int ba_validate(const BaWorkspace* ws, const orbhip_ba_problem* const* probs, int B, orbhip_ba_result* const* res,
                int shard_mode, const BaStereoExt* sx, bool& stereo) {
    if (B <= 0 || !probs || !res) return ORBHIP_ERR_ARG;
    if (sx && shard_mode != kShardNone) return ORBHIP_ERR_ARG;   // the sharded forms have no stereo edges
    // RCCL: this rank holds B consecutive shards (segments rank*B .. rank*B+B-1 of nranks*B), the
    // same B on every rank; the shards of one rank are summed on the device before the all-reduce
    if (shard_mode == kShardRccl && !ws->comm) return ORBHIP_ERR_ARG;
    for (int b = 0; b < B; b++)
        if (!probs[b] || !res[b]) return ORBHIP_ERR_ARG;
    stereo = false;
    if (sx) {
        for (int b = 0; b < B; b++) {
            const int E = probs[b]->n_edges;
            if (E > 0 && !sx[b].edge_ur) return ORBHIP_ERR_ARG;
            bool any = false;
            for (int e = 0; e < E && !any; e++) any = sx[b].edge_ur[e] >= 0.0f;
            if (any && !(sx[b].bf > 0.0f)) return ORBHIP_ERR_ARG;
            stereo = stereo || any;
        }
    }
    return ORBHIP_OK;
}

// ---- step 2: the per-problem preparations, kept in the workspace across calls (their vectors'
// capacity: no allocation on the hot path); the shards of one problem must agree in shape and
// share the union envelope ----
int ba_prepare_all(BaCall& c) {
    const int B = c.B;
    if (c.ws->prep.size() < (size_t)B) c.ws->prep.resize(B);
    Prep* pp = c.pp = c.ws->prep.data();
    for (int b = 0; b < B; b++) prep_reset(pp[b]);
    // Schur work-item size: a batch fills the chip with 16 pairs per lane; a few problems alone
    // would leave it mostly idle, so their items are cut to 4 pairs (4x the lanes), 3 for the
    // LBA sizes (r06, alternating runs: C4 1.323 -> 1.309 ms with 3, 1.31-1.33 with 2, 1.34-1.35
    // with 1; the C5 GBA 5.18 -> 5.58 ms with 2)
    int maxE_in = 0;
    for (int b = 0; b < B; b++) maxE_in = std::max(maxE_in, c.probs[b]->n_edges);
    const int chunk = c.sw.chunk > 0 ? c.sw.chunk : (B >= 32 ? kSchurChunk : (maxE_in <= 32768 ? 3 : 4));
    // one problem: its Schur pair lists on the host threads (off by default: on the MI355X box's
    // EPYC the C5 build went 0.62 -> 0.55 ms at 16 threads, 0.71 at 4 in r05, and 0.63 -> 1.09-1.26 ms
    // on the r06 tree: its scattered fill does not scale); a batch: one problem per thread
    const int prep_par = B == 1 ? c.sw.prep_threads : 1;
    parallel_for(B, c.nth, [&](int b) { pp[b].rc = prepare(c.probs[b], pp[b], chunk, prep_par); });
    c.t_prepare = now_ms();
    // RCCL shards: a rank whose shards are invalid must not return before the first collective
    // (the other ranks would wait in it forever); its verdict travels in that all-reduce and every
    // rank returns together
    for (int b = 0; b < B && !c.local_bad; b++)
        if (pp[b].rc) {
            if (!c.rccl) return pp[b].rc;
            c.local_bad = pp[b].rc;
        }
    if (!c.sharded || B == 1 || c.local_bad) return ORBHIP_OK;
    for (int b = 1; b < B; b++)
        if (pp[b].P != pp[0].P || pp[b].np != pp[0].np) {
            if (!c.rccl) return ORBHIP_ERR_ARG;
            c.local_bad = ORBHIP_ERR_ARG;
            return ORBHIP_OK;
        }
    // every shard factors the SUMMED S: the blocked Cholesky needs the union envelope
    for (int b = 1; b < B; b++)
        for (size_t R = 0; R < pp[0].row_first.size(); R++)
            pp[0].row_first[R] = std::min(pp[0].row_first[R], pp[b].row_first[R]);
    for (int b = 1; b < B; b++) pp[b].row_first = pp[0].row_first;
    return ORBHIP_OK;
}

// ---- step 3: the Cholesky of each problem: the persistent DAG solver for the GBA sizes and for a
// problem solved alone (one LBA), the register / LDS single-workgroup solvers for batches of
// small problems, the blocked solver for the large ones when forced; a lone large problem whose S
// is a narrow (cyclic) block band (a GBA's keyframe loop): nested dissection, when the plan's
// chain is shorter ----
void ba_choose_solvers(BaCall& c) {
    Prep* pp = c.pp;
    c.dag_helpers = dag_max_helpers();
    for (int b = 0; b < c.B; b++)
        pp[b].use_dag = !c.no_dag && !c.sw.force_blocked && pp[b].n > 0 &&
                        (pp[b].n > kCholSmallN || (c.B == 1 && pp[b].n >= c.sw.dag_min));
    if (!c.sharded && c.B == 1 && !c.no_nd && pp[0].use_dag && pp[0].n >= c.sw.nd_min && c.sw.nd) {
        Prep& p = pp[0];
        if (nd_plan(p.np, p.blk_i.data(), p.blk_j.data(), p.nblk, c.sw.nd_k, p.nd)) {
            p.use_nd = true;
            p.use_dag = false;
        }
    }
}

// ---- step 4: sharded solves by keyframe segments (the distributed form of the
// dissection): shard r is segment r when every shard's landmarks lie inside its segment's matrix
// (sharding.shard_problem_nd); then each shard eliminates its interior, the separator system is
// summed over the shards, every shard solves it, and the shards' x are summed. Otherwise the
// shards sum S itself and every shard solves it (replicated). The decision is agreed over the
// ranks. Collectives of this step, in order (RCCL only): the band and shard count (5 ints, the
// first collective of a call: an invalid rank reaches it), whether every rank's landmarks fit
// (1 int), and, for a replicated form that may be dissected, the union pose adjacency (np^2 bytes) ----
int ba_plan_replicated_nd(BaCall& c);
int ba_plan_shards(BaCall& c) {
    BaWorkspace* ws = c.ws;
    Prep* pp = c.pp;
    const int B = c.B;
    c.seg0 = c.rccl ? ws->rank * B : 0;
    const int K = c.shard_mode == kShardLocal ? B : ws->nranks * B;
    int wl = 0, wc = 0;
    for (int b = 0; b < B && !c.local_bad; b++) {
        int l = 0, w = 0;
        nd_bandwidth(pp[b].np, pp[b].blk_i.data(), pp[b].blk_j.data(), pp[b].nblk, l, w);
        wl = std::max(wl, l);
        wc = std::max(wc, w);
    }
    const bool ok_base = !c.no_dag && !c.sw.force_blocked && pp[0].n >= c.sw.nd_min;
    int ok = (ok_base && c.sw.shard_nd) ? 1 : 0;
    if (c.rccl) {   // the band over every rank's landmarks; the same B everywhere
        // words 3 / 4: the max of B and of -B agree only when every rank has the same B and
        // valid shards (an invalid rank sends INT_MAX)
        int* h = ws->h_int4.p;
        h[0] = wl; h[1] = wc; h[2] = -ok;
        h[3] = c.local_bad ? std::numeric_limits<int>::max() : B; h[4] = -B;
        if (rccl_consensus(c, h, ws->dint4.p, 5, ncclMax)) return ORBHIP_ERR_DEVICE;
        if (h[3] != B || -h[4] != B) return c.local_bad ? c.local_bad : ORBHIP_ERR_ARG;
        wl = h[0]; wc = h[1]; ok = -h[2];
    }
    ok = ok && nd_plan_band(pp[0].np, wl, wc, K, c.ndp);
    for (int b = 0; b < B && ok; b++)
        ok = nd_blocks_fit(c.ndp, c.seg0 + b, pp[b].blk_i.data(), pp[b].blk_j.data(), pp[b].nblk);
    if (c.rccl) {   // every rank's landmarks fit its segment
        int* h = ws->h_int4.p;
        h[0] = ok ? 0 : 1;
        if (rccl_consensus(c, h, ws->dint4.p, 1, ncclMax)) return ORBHIP_ERR_DEVICE;
        ok = h[0] == 0;
    }
    c.nd_sh = ok != 0;
    if (c.nd_sh)
        for (int b = 0; b < B; b++) {
            Prep& p = pp[b];
            p.use_nd_sh = true;
            p.use_dag = false;
            const int r = c.seg0 + b;
            p.own.assign(p.np, 0);
            for (int q = c.ndp.seg[r]; q < c.ndp.seg[r + 1]; q++) p.own[q] = 1;   // interior + own separator
        }
    if (!c.nd_sh && ok_base && !c.no_nd && c.sw.nd) return ba_plan_replicated_nd(c);
    return ORBHIP_OK;
}
// r06: the replicated form (landmark shards, or segments whose landmarks cross) solves the summed S
// by nested dissection too when that pays, planned on the union of the shards' pose adjacencies
// (every rank derives the same plan from the same union); ORBHIP_ND=0 keeps the plain DAG solve on
// the union envelope
int ba_plan_replicated_nd(BaCall& c) {
    Prep* pp = c.pp;
    const int B = c.B, np = pp[0].np;
    std::vector<unsigned char> adj((size_t)np * np, 0);   // [max(i, j)][min(i, j)]
    for (int b = 0; b < B; b++)
        for (int k = 0; k < pp[b].nblk; k++) {
            const int i = pp[b].blk_i[k], j = pp[b].blk_j[k];
            adj[(size_t)std::max(i, j) * np + std::min(i, j)] = 1;
        }
    if (c.rccl) {
        BAOK(c.ws->uadj.ensure(adj.size()));
        if (rccl_consensus(c, adj.data(), c.ws->uadj.p, adj.size(), ncclMax)) return ORBHIP_ERR_DEVICE;
    }
    for (int i = 0; i < np; i++)
        for (int j = 0; j <= i; j++)
            if (adj[(size_t)i * np + j]) { c.ubi.push_back(j); c.ubj.push_back(i); }
    NdPlan up;
    if (nd_plan(np, c.ubi.data(), c.ubj.data(), (int)c.ubi.size(), 0, up))
        for (int b = 0; b < B; b++) {
            pp[b].nd = up;
            pp[b].use_nd = true;
            pp[b].use_dag = false;
        }
    else
        c.ubi.clear(), c.ubj.clear();
    return ORBHIP_OK;
}

// the per-panel tile lists / the DAG plans (RCCL shards: the envelope is the union over the
// ranks, known after a collective; their DAG plan is made then, into reserved space)
void ba_plan_factors(BaCall& c) {
    parallel_for(c.B, c.nth, [&](int b) {
        Prep& p = c.pp[b];
        if (p.use_nd || p.use_nd_sh) {
            // planned above; its device data is set up with the problem's buffers (nd_setup)
        } else if (p.use_dag) {
            if (c.rccl) {
                const size_t NT = (p.n + kDagTile - 1) / kDagTile;
                p.dag_task_cap = (size_t)c.dag_helpers + 1 + NT * (NT + 1) / 2 + 2 * NT;   // + the copy tasks, the column counts
            } else {
                dag_plan(p.row_first.data(), p.n, c.dag_helpers, p.dag);
                p.dag_task_cap = p.dag.toff.size() + p.dag.tasks.size();
            }
        } else if (p.n > kCholSmallN && !c.rccl) {
            cb_envelope_tiles(p.row_first.data(), p.n, p.cb_tiles, p.cb_off);
        }
    });
}

// A cursor over one packed segment: take(count, align) is the address of the segment's next
// `count` elements, aligned to `align` elements from the segment's start. The sizing pass runs
// over a zero base (only `at` matters there), the packing pass over the segment's device address.
template <typename T>
struct Carve {
    uintptr_t base = 0;
    size_t at = 0;
    T* take(size_t count, size_t align = 1) {
        at = (at + align - 1) & ~(align - 1);
        T* p = reinterpret_cast<T*>(base + at * sizeof(T));
        at += count;
        return p;
    }
};
// the int segment's cursor also fills the pinned staging copy (host: null in the sizing pass)
struct CarveInt : Carve<int> {
    int* host = nullptr;
    size_t counted = 0;   // ints taken, without the alignment gaps
    int* skip(size_t count, size_t align = 1) {   // taken, not filled
        counted += count;
        return take(count, align);
    }
    // src (null: zeros) copied into the staging; bytes: of src, when not whole ints
    int* put(const void* src, size_t count, size_t align = 1, size_t bytes = ~size_t(0)) {
        int* d = skip(count, align);
        if (bytes == ~size_t(0)) bytes = count * sizeof(int);
        if (host && src) std::memcpy(host + at - count, src, bytes);
        if (host && !src) std::memset(host + at - count, 0, bytes);
        return d;
    }
    int* put(const std::vector<int>& v, size_t align = 1) { return put(v.data(), v.size(), align); }
};
struct Segs {
    Carve<double> C, A, U, R;
    CarveInt I;
};

// ---- the packed layout: ONE device buffer (and its pinned staging twin) of doubles,
//   [ C | A | U | I | G | R ],   every segment contiguous over all problems:
//   C  e_chi2 (E)                 downloaded with A in one transfer (nC + nA doubles from 0)
//   A  pose (8P) + pts (3M)       uploaded, optimised in place, downloaded
//   U  obs (2E) + info (E)        uploaded (a call with stereo edges: + ur (E))
//   I  the int arrays             uploaded; 16-byte aligned
//   G  the BaArgs records         uploaded; 16-byte aligned (one copy uploads A .. G: sA to sR)
//   R  the rest (scratch), 128-byte aligned: per problem the arrays below, then the edge
//      linearisations e_lin (32-byte aligned), S (n*n), the panel inverses Lsave and the trial
//      partials (16-byte aligned), and the DAG solver's buffer (128-byte aligned)
// place_problem is the one description of a problem's arrays: each appears here once, with its
// size and alignment, in the order it lies in memory. ba_layout runs it over zero bases to size
// the segments and record where each problem starts; ba_pack_upload runs it again from those
// starts over the real bases, which fills the problem's BaArgs / DagDev and the int staging. ----
void place_problem(Segs& s, const Prep& p, const orbhip_ba_problem* pr, bool stereo, bool sharded, BaArgs& a,
                   DagDev& dd) {
    const size_t P = p.P, M = p.M, E = p.E, np = p.np, n = p.n;
    a.e_chi2 = s.C.take(E);
    a.pose = s.A.take(8 * P); a.pts = s.A.take(3 * M);
    a.e_obs = s.U.take(2 * E); a.e_info = s.U.take(E);
    a.e_ur = stereo ? s.U.take(E) : nullptr;
    Carve<double>& r = s.R;
    a.pose_bak = r.take(8 * P); a.pts_bak = r.take(3 * M);
    a.e_err = r.take(2 * E); a.e_rho0 = r.take(E); a.e_rho1 = r.take(2 * E);   // (+ pad)
    a.e_err2 = stereo ? r.take(E) : nullptr;
    a.Hpp = r.take(36 * np); a.R_lin = r.take(9 * np);
    a.Hll = r.take(9 * M); a.Dinv = r.take(9 * M); a.db = r.take(3 * M);
    a.Hpp_g = sharded ? r.take(36 * np) : a.Hpp;   // Hpp summed over the shards
    a.b = r.take(n + 3 * M); a.x = r.take(n + 3 * M); a.bs = r.take(n); a.red = r.take(4);
    a.e_lin = r.take(4 * E, 4);
    a.S = r.take(n * n);
    a.Lsave = r.take(1024 * ((n + 31) / 32), 2);
    const size_t npart_e = (E + 255) / 256, npart_m = (std::max(M, P) + kBsL - 1) / kBsL;   // k_ba_backsub_errs' workgroups
    a.npart_e = (int)npart_e; a.npart_m = (int)npart_m;
    a.part = r.take(std::max(npart_e + npart_m, (M + kLinL - 1) / kLinL + np) + 2, 2);
    dd.buf = p.use_dag ? r.take(dag_doubles(p.n), 16) : nullptr;
    CarveInt& q = s.I;
    a.opt = q.put(p.opt);
    a.flag = q.put(nullptr, 4);   // [0] Cholesky ok, [1] blocked backward arrival counter (zero between uses)
    a.e_pose = q.put(pr->edge_pose, E); a.e_pt = q.put(pr->edge_point, E);
    a.pt_ptr = q.put(p.pt_ptr); a.pt_edges = q.put(p.pt_edges);
    a.ps_ptr = q.put(p.ps_ptr); a.ps_edges = q.put(p.ps_edges);
    a.nblk = p.nblk; a.nitems = (int)(p.items.size() / 4); a.nfin = (int)(p.fin.size() / 3);
    a.blk_i = q.put(p.blk_i); a.blk_j = q.put(p.blk_j); a.blk_ptr = q.put(p.blk_ptr);
    a.blk_pairs = q.put(p.blk_pairs, 2);   // int2
    a.items = q.put(p.items, 4);           // int4
    a.fin = q.put(p.fin); a.ifin = q.put(p.ifin);
    a.row_first = q.put(p.row_first);
    a.cb_tiles = p.cb_tiles.empty() ? nullptr : q.put(p.cb_tiles);
    a.own = p.own.empty() ? nullptr   // bytes, in the int staging
                          : (const unsigned char*)q.put(p.own.data(), (p.own.size() + 3) / 4, 1, p.own.size());
    if (p.use_dag) {   // flags + control words (zero), then the plan (or the space reserved for it)
        dd.ints = q.put(nullptr, dag_ints(p.n), 4);
        dd.toff = p.dag.toff.empty() ? q.skip(p.dag_task_cap) : q.put(p.dag.toff);
        // (RCCL: planned after the union envelope, into the space skipped here)
        dd.tasks = p.dag.toff.empty() ? dd.toff + kDagMaxHelpers + 1 : q.put(p.dag.tasks);
        dd.G = p.dag.G; dd.pb = p.dag.pb;
        dd.need_off = p.dag.toff.empty() ? 0 : p.dag.toff[p.dag.G];
    }
}

// ---- step 5a: the sizing pass ----
void ba_layout(BaCall& c) {
    Segs s;
    BaArgs a;
    DagDev d;
    for (int b = 0; b < c.B; b++) {
        Prep& p = c.pp[b];
        p.o_chi2 = s.C.at; p.o_state = s.A.at; p.o_obs = s.U.at; p.o_scr = s.R.at; p.o_int = s.I.at;
        s.I.counted = 0;
        place_problem(s, p, c.probs[b], c.stereo, c.sharded, a, d);
        // the gaps in front of the aligned int arrays depend on where the problem starts (at most
        // 1 + 3 ints in front of the pair list and the items, 3 in front of the DAG words): each
        // problem gets a fixed room above them, so its start depends on the sizes alone
        s.I.at = p.o_int + s.I.counted + 9 + (p.use_dag ? 4 : 0);
    }
    // r06: the int arrays and the BaArgs follow the uploaded doubles in the same device / pinned
    // buffers, so that ONE copy uploads all of it (three blit launches of ~4.4 us each before)
    c.nC = s.C.at; c.nA = s.A.at;
    c.sC = 0; c.sA = c.nC; c.sU = c.sA + c.nA;
    c.sI = (c.sU + s.U.at + 1) & ~size_t(1);                                    // 16-byte aligned
    c.sG = (c.sI + (s.I.at * sizeof(int) + 7) / 8 + 1) & ~size_t(1);            // the BaArgs
    c.sR = (c.sG + (c.B * sizeof(BaArgs) + 7) / 8 + 15) & ~size_t(15);
    c.nR = s.R.at;
}

// ---- step 5b: the buffers, every problem's arrays and BaArgs into the staging, one upload ----
int ba_pack_upload(BaCall& c) {
    BaWorkspace* ws = c.ws;
    const int B = c.B;
    BAOK(ws->dbl.ensure(c.sR + c.nR));
    BAOK(ws->act.ensure(3 * (size_t)B));
    BAOK(ws->lam.ensure(B));
    BAOK(ws->ctl.ensure(B));
    BAOK(ws->hctl.ensure(B));
    BAOK(ws->hdbl.ensure(c.sR));
    BAOK(ws->h_act.ensure(3 * (size_t)B));
    double* const D = c.D = ws->dbl.p;
    double* const hd = c.hd = ws->hdbl.p;
    c.I = reinterpret_cast<int*>(D + c.sI);
    c.hi = reinterpret_cast<int*>(hd + c.sI);
    c.ha = reinterpret_cast<BaArgs*>(hd + c.sG);
    c.dArgs = reinterpret_cast<BaArgs*>(D + c.sG);
    c.dd.assign(B, DagDev{nullptr, nullptr, nullptr, nullptr, 0, 0, 0});
    parallel_for(B, c.nth, [&](int b) {
        const Prep& p = c.pp[b];
        const orbhip_ba_problem* pr = c.probs[b];
        const size_t P = p.P, M = p.M, E = p.E;
        double* st_ = hd + c.sA + p.o_state;
        for (size_t i = 0; i < P; i++) se3_from_float(pr->pose_q + 4 * i, pr->pose_t + 3 * i, st_ + 8 * i);
        for (size_t k = 0; k < 3 * M; k++) st_[8 * P + k] = pr->points[k];
        double* ob = hd + c.sU + p.o_obs;
        // (on the host pool this loop measured slower: C5 pack + upload 0.11 -> 0.21 ms, r06 A/B)
        for (size_t e = 0; e < E; e++) {
            ob[2 * e] = pr->edge_uv[2 * e];
            ob[2 * e + 1] = pr->edge_uv[2 * e + 1];
            ob[2 * E + e] = (double)pr->inv_sigma2[pr->edge_octave[e]];
        }
        if (c.stereo)
            for (size_t e = 0; e < E; e++) ob[3 * E + e] = (double)c.sx[b].edge_ur[e];
        Segs s;
        s.C.base = (uintptr_t)(D + c.sC); s.C.at = p.o_chi2;
        s.A.base = (uintptr_t)(D + c.sA); s.A.at = p.o_state;
        s.U.base = (uintptr_t)(D + c.sU); s.U.at = p.o_obs;
        s.R.base = (uintptr_t)(D + c.sR); s.R.at = p.o_scr;
        s.I.base = (uintptr_t)c.I; s.I.host = c.hi; s.I.at = p.o_int;
        BaArgs& a = c.ha[b];
        place_problem(s, p, pr, c.stereo, c.sharded, a, c.dd[b]);
        a.P = p.P; a.M = p.M; a.E = p.E; a.np = p.np; a.n = p.n;
        a.fx = pr->fx; a.fy = pr->fy; a.cx = pr->cx; a.cy = pr->cy; a.delta = pr->huber_delta;
        a.bf = c.stereo ? c.sx[b].bf : 0.0;
        a.delta_s = c.stereo ? c.sx[b].delta_s : 0.0;
        a.sync = c.sharded ? 1 : 0;
        a.small = (!c.sharded && 8 * P + 3 * M <= (size_t)c.sw.small_words && E <= 65536) ? 1 : 0;
        a.fused = 0;   // set by ba_enqueue_start once the batch's launch width is known
        a.lambda = ws->lam.p + b;
        a.lead = c.shard_mode == kShardLocal ? (b == 0) : (c.rccl ? (ws->rank == 0 && b == 0) : 1);
        a.ctl = ws->ctl.p + b;
    });
    BAOK(hipMemcpyAsync(D + c.sA, hd + c.sA, sizeof(double) * (c.sR - c.sA), hipMemcpyHostToDevice, c.st));
    return ORBHIP_OK;
}

// ---- step 6: RCCL shards solved by the blocked or DAG Cholesky (which read only the lower
// triangle inside the envelope; the one-workgroup solvers also read the mirrored upper triangle)
// all-reduce S over its union envelope only: ~5 MB instead of n^2 doubles (46 MB) at C5.
// One collective: row_first, min over the ranks, in place on the device; then the DAG plan of
// the union envelope into the reserved space ----
int ba_union_envelope(BaCall& c) {
    BaWorkspace* ws = c.ws;
    Prep* pp = c.pp;
    const int B = c.B;
    hipStream_t st = c.st;
    int* rf = const_cast<int*>(c.ha[0].row_first);
    if (ncclAllReduce(rf, rf, pp[0].row_first.size(), ncclInt32, ncclMin, ws->comm, st) != ncclSuccess)
        return ORBHIP_ERR_DEVICE;
    const int nt = (int)pp[0].row_first.size(), n = pp[0].n;
    std::vector<int> urf(nt);
    if (n > kCholSmallN || pp[0].use_dag) {
        BAOK(hipMemcpyAsync(urf.data(), rf, nt * sizeof(int), hipMemcpyDeviceToHost, st));
        BAOK(hipStreamSynchronize(st));
    }
    for (int b = 1; b < B; b++)   // this rank's other shards: the same envelope
        BAOK(hipMemcpyAsync(const_cast<int*>(c.ha[b].row_first), rf, nt * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (pp[0].use_dag) {   // the DAG plan of the union envelope, into the reserved space
        DagPlan& dp = pp[0].dag;
        dag_plan(urf.data(), n, c.dag_helpers, dp);
        for (int b = 0; b < B; b++) {
            DagDev& d = c.dd[b];
            if (dp.toff.size() + dp.tasks.size() > pp[b].dag_task_cap) return ORBHIP_ERR_DEVICE;
            BAOK(hipMemcpy(const_cast<int*>(d.toff), dp.toff.data(), dp.toff.size() * sizeof(int), hipMemcpyHostToDevice));
            d.tasks = d.toff + dp.toff.size();
            if (!dp.tasks.empty())
                BAOK(hipMemcpy(const_cast<int*>(d.tasks), dp.tasks.data(), dp.tasks.size() * sizeof(int),
                               hipMemcpyHostToDevice));
            d.G = dp.G;
            d.pb = dp.pb;
            d.need_off = dp.toff[dp.G];
        }
    }
    // one shard per rank: S all-reduced over its union envelope, packed; several: the full S
    // (summed on the device first, then the all-reduce, then copied to the other shards)
    if (B == 1 && n > kCholSmallN && !c.sw.shard_full_s) {
        std::vector<long long> off(nt + 1, 0);
        for (int R = 0; R < nt; R++)
            off[R + 1] = off[R] + (long long)std::min(32, n - 32 * R) * (std::min(32 * R + 32, n) - 32 * urf[R]);
        c.env_total = (size_t)off[nt];
        BAOK(ws->envbuf.ensure(c.env_total));
        BAOK(ws->envoff.ensure(nt + 1));
        BAOK(hipMemcpyAsync(ws->envoff.p, off.data(), (nt + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    }
    return ORBHIP_OK;
}

// ---- step 7: the launch widths, the controllers' initial state, the dissections' device data
// and the timeout words. kRerunNoNd: the device setup refused a lone problem's plan ----
int ba_init_controllers(BaCall& c) {
    BaWorkspace* ws = c.ws;
    const Prep* pp = c.pp;
    const int B = c.B;
    hipStream_t st = c.st;
    static LdsAttrOnce chol_attr;   // per device, thread-safe (dev_attr.h)
    BAOK(chol_attr.ensure((const void*)k_ba_cholesky, 160 * 1024));
    bool s_written = false;
    for (int b = 0; b < B; b++) {
        const Prep& p = pp[b];
        c.maxM = std::max(c.maxM, p.M); c.maxE = std::max(c.maxE, p.E); c.maxP = std::max(c.maxP, p.P);
        c.maxNp = std::max(c.maxNp, p.np);
        c.maxItems = std::max(c.maxItems, (int)(p.items.size() / 4));
        c.maxPM = std::max(c.maxPM, std::max(8 * p.P, 3 * p.M));
        if (!c.large(b)) c.maxN = std::max(c.maxN, p.n);
        if (!p.use_dag && !p.use_nd && !p.use_nd_sh && p.n > kCholRegMaxN) s_written = true;   // the LDS and blocked solvers factor S in place
    }
    c.chol_lds = sizeof(double) * chol_lds_doubles(c.maxN);
    // every problem on a solver that reads S and never writes it (register / DAG / dissection) and no
    // sum of S over the shards (the replicated form all-reduces S in place): S is zeroed once, the
    // Schur finisher overwrites its blocks every trial (r05: segment shards too, which saved a
    // 46 MB memset per shard and trial at C5)
    c.s_readonly = !s_written && (!c.sharded || c.nd_sh);
    (void)hipGetLastError();
    c.d_act = ws->act.p;
    c.h_act = ws->h_act.p;
    for (int b = 0; b < B; b++) c.h_act[b] = b;   // act slot 0: every problem
    BAOK(hipMemcpyAsync(c.d_act, c.h_act, B * sizeof(int), hipMemcpyHostToDevice, st));
    LmCtl* dctl = c.dctl = ws->ctl.p;
    for (int b = 0; b < B; b++) {
        LmCtl& l = ws->hctl.p[b];
        l = LmCtl{};
        l.ni = 2;
        l.phase = c.probs[b]->iterations > 0 ? kPhBuild : kPhDone;   // optimize(0): nothing to run
        l.errors_valid = 1;
        l.iterations = c.probs[b]->iterations;
        l.early_stop = c.probs[b]->early_stop;
    }
    BAOK(hipMemcpyAsync(dctl, ws->hctl.p, B * sizeof(LmCtl), hipMemcpyHostToDevice, st));
    if (B > 1)   // shards of the replicated form: each solves the summed S in its own workspace
        while (ws->nds.size() < (size_t)B) ws->nds.push_back(nd_create());
    for (int b = 0; b < B; b++)
        if (pp[b].use_nd) {
            if (!ws->nd) ws->nd = nd_create();
            const bool uni = !c.ubi.empty();
            const int rc = nd_setup(c.nd_of(b), pp[b].nd, uni ? c.ubi.data() : pp[b].blk_i.data(),
                                    uni ? c.ubj.data() : pp[b].blk_j.data(), uni ? (int)c.ubi.size() : pp[b].nblk,
                                    c.ha[b].S, c.ha[b].bs, c.ha[b].x, c.ha[b].flag, &dctl[b].phase, st);
            // a plan the device setup refuses (a segment beyond the back-substitution's LDS, a
            // separator system beyond the DAG solver; the planner rejects both, so this is a
            // guard): the same problem again on the plain DAG solve, nothing was run yet
            if (rc == -5) return hipStreamSynchronize(st) != hipSuccess ? (int)ORBHIP_ERR_DEVICE : (int)kRerunNoNd;
            if (rc != 0) return ORBHIP_ERR_DEVICE;
        }
    if (c.nd_sh) {   // one segment per shard
        while (ws->nds.size() < (size_t)B) ws->nds.push_back(nd_create());
        for (int b = 0; b < B; b++)
            if (nd_setup(ws->nds[b], c.ndp, pp[b].blk_i.data(), pp[b].blk_j.data(), pp[b].nblk, c.ha[b].S, c.ha[b].bs,
                         c.ha[b].x, c.ha[b].flag, &dctl[b].phase, st, c.seg0 + b) != 0)
                return ORBHIP_ERR_DEVICE;
    }
    // ---- hand-off timeouts of the persistent solver: a timed-out solve fails its trial (flag 0),
    // which must never pass for a g2o rejection. Counted per problem (control word 3), read with
    // the outputs (no extra synchronisation), agreed over the ranks of a sharded solve. ----
    for (int b = 0; b < B; b++) {
        if (pp[b].use_dag) c.tw.push_back(c.dd[b].ints + 3);
        if (pp[b].use_nd) nd_timeout_words(c.nd_of(b), c.tw);
        if (pp[b].use_nd_sh) nd_timeout_words(ws->nds[b], c.tw);
    }
    c.ndag = (int)c.tw.size();
    if (c.ndag) BAOK(ws->hto.ensure(c.ndag));
    return ORBHIP_OK;
}

// ---- step 8: the collectives of a sharded slot (sites) and, for the in-process sums, their
// pointer tables on the device once ----
int ba_make_sites(BaCall& c) {
    BaWorkspace* ws = c.ws;
    const int B = c.B;
    const BaArgs* ha = c.ha;
    c.sites.assign(kSites, Site{});
    auto site = [&](int id, size_t count, int op, auto src, auto dst) {
        Site& t = c.sites[id];
        t.count = count; t.op = op;
        for (int b = 0; b < B; b++) { t.src.push_back(src(b)); t.dst.push_back(dst(b)); }
    };
    auto inplace = [&](int id, size_t count, int op, auto buf) { site(id, count, op, buf, buf); };
    site(kHpp, 36 * (size_t)c.maxNp, 0, [&](int b) { return ha[b].Hpp; }, [&](int b) { return const_cast<double*>(ha[b].Hpp_g); });
    inplace(kRed0, 1, 0, [&](int b) { return ha[b].red; });
    inplace(kRed2, 1, 1, [&](int b) { return ha[b].red + 2; });
    inplace(kRed01, 2, 0, [&](int b) { return ha[b].red; });
    if (!c.nd_sh) {
        inplace(kRepS, (size_t)c.pp[0].n * c.pp[0].n, 0, [&](int b) { return ha[b].S; });
        inplace(kRepBs, (size_t)c.pp[0].n, 0, [&](int b) { return ha[b].bs; });
    } else {
        const NdSepBufs q0 = nd_sep_bufs(ws->nds[0]);
        inplace(kNdPack, q0.pack_n, 0, [&](int b) { return nd_sep_bufs(ws->nds[b]).pack; });
        inplace(kNdBz, (size_t)q0.nZ, 0, [&](int b) { return nd_sep_bufs(ws->nds[b]).bZ; });
        site(kNdX, (size_t)q0.n + 1, 0, [&](int b) { return nd_sep_bufs(ws->nds[b]).x_loc; },
             [&](int b) { return nd_sep_bufs(ws->nds[b]).xg; });
    }
    if (c.shard_mode == kShardLocal || B > 1) {
        std::vector<double*> tab;
        for (Site& t : c.sites) {
            t.tab = tab.size();
            tab.insert(tab.end(), t.src.begin(), t.src.end());
            tab.insert(tab.end(), t.dst.begin(), t.dst.end());
        }
        BAOK(ws->ptab.ensure(tab.size()));
        BAOK(hipMemcpy(ws->ptab.p, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
    }
    return ORBHIP_OK;
}

// one collective of a sharded slot. kShardLocal: one k_ba_multi_reduce over the shards. RCCL: one
// all-reduce of this rank's buffers (B > 1: this rank's sum first, the result copied to its other
// shards after; S of a lone shard: over its packed union envelope)
int coll(const BaCall& c, int id) {
    BaWorkspace* ws = c.ws;
    const int B = c.B;
    hipStream_t st = c.st;
    const Site& t = c.sites[id];
    if (t.count == 0) return ORBHIP_OK;
    const dim3 gr((unsigned)std::min<size_t>(1024, (t.count + 255) / 256));
    double* const* tab = (c.shard_mode == kShardLocal || B > 1) ? ws->ptab.p + t.tab : nullptr;   // [src | dst]
    if (c.shard_mode == kShardLocal) {
        hipLaunchKernelGGL(k_ba_multi_reduce, gr, dim3(256), 0, st, (const double* const*)tab, B, tab + B, B,
                           t.count, t.op);
        return ORBHIP_OK;
    }
    if (B > 1) {   // RCCL with several shards per rank: this rank's sum into dst[0] first
        hipLaunchKernelGGL(k_ba_multi_reduce, gr, dim3(256), 0, st, (const double* const*)tab, B, tab + B, 1,
                           t.count, t.op);
        if (ncclAllReduce(t.dst[0], t.dst[0], t.count, ncclDouble, t.op ? ncclMax : ncclSum, ws->comm, st) !=
            ncclSuccess)
            return ORBHIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_ba_multi_reduce, gr, dim3(256), 0, st, (const double* const*)(tab + B), 1,
                           tab + B + 1, B - 1, t.count, t.op);
        return ORBHIP_OK;
    }
    if (id == kRepS && c.env_total) {   // RCCL, replicated: S over its union envelope, packed
        const BaArgs& a0 = c.ha[0];
        const dim3 g(8, (unsigned)c.pp[0].row_first.size());
        hipLaunchKernelGGL(k_ba_env_pack, g, dim3(256), 0, st, a0.S, a0.n, a0.row_first, ws->envoff.p,
                           ws->envbuf.p, 0);
        if (ncclAllReduce(ws->envbuf.p, ws->envbuf.p, c.env_total, ncclDouble, ncclSum, ws->comm, st) != ncclSuccess)
            return ORBHIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_ba_env_pack, g, dim3(256), 0, st, a0.S, a0.n, a0.row_first, ws->envoff.p,
                           ws->envbuf.p, 1);
        return ORBHIP_OK;
    }
    if (ncclAllReduce(t.src[0], t.dst[0], t.count, ncclDouble, t.op ? ncclMax : ncclSum, ws->comm, st) != ncclSuccess)
        return ORBHIP_ERR_DEVICE;
    return ORBHIP_OK;
}

// ---- step 8b: what runs once in front of the slots: the single-workgroup solvers' problem
// list, S zeroed (when no solver writes it), the initial errors and chi2 (sharded: summed over
// the shards, collective kRed0), the trial's form, and the host-mapped done / stop words ----
int ba_enqueue_start(BaCall& c) {
    BaWorkspace* ws = c.ws;
    const int B = c.B;
    hipStream_t st = c.st;
    const BaArgs* dA = c.dArgs;
    for (int b = 0; b < B; b++)
        if (!c.large(b)) c.h_act[2 * B + c.ns++] = b;
    if (c.ns) BAOK(hipMemcpyAsync(c.d_act + 2 * B, c.h_act + 2 * B, c.ns * sizeof(int), hipMemcpyHostToDevice, st));
    if (c.s_readonly) hipLaunchKernelGGL(k_ba_zero_s, dim3(64, B), dim3(256), 0, st, dA, c.d_act, 1);
    const auto kErrors = c.stereo ? k_ba_errors<true> : k_ba_errors<false>;
    hipLaunchKernelGGL(kErrors, dim3(gx(c.maxE, 256), B), dim3(256), 0, st, dA, c.d_act, 0, nullptr);
    if (!c.sharded) {
        hipLaunchKernelGGL(k_ba_ctl_init, dim3(B), dim3(1024), 0, st, dA, c.d_act);
    } else {   // the initial chi2 over every shard's edges
        hipLaunchKernelGGL(k_ba_reduce, dim3(B), dim3(1024), 0, st, dA, c.d_act);
        if (coll(c, kRed0)) return ORBHIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_ba_sh_init, dim3(B), dim3(64), 0, st, dA, c.d_act);
    }
    for (int b = 0; b < B; b++) c.all_small = c.all_small && c.ha[b].small;
    // a trial takes its errors inside the back-substitution when every problem's partial slots
    // hold the fused kernel's workgroups (r06: every unsharded problem, small or not; a sharded
    // trial ends in the split controller)
    c.gbs = gx(std::max(c.maxM, c.maxP), kBsL);
    // k_ba_lin's pose work-groups: one pose per work-group (its four waves on its edges) for a
    // lone problem, four (a wave each) for batches
    c.lin_ppw = c.sw.lin_ppw ? c.sw.lin_ppw : (B == 1 ? 1 : 4);
    c.fused = !c.sharded && c.sw.fused;
    for (int b = 0; b < B && c.fused; b++) c.fused = (int)c.gbs <= c.ha[b].npart_e && c.pp[b].P <= kFusedMaxP;
    if (c.fused) {
        for (int b = 0; b < B; b++) c.ha[b].fused = 1;
        BAOK(hipMemcpyAsync(c.dArgs, c.ha, B * sizeof(BaArgs), hipMemcpyHostToDevice, st));
    }
    // the host-mapped words (post_done): B done flags, then the relayed stop flag. The kernels
    // get them through a device-resident pointer pair: {done, stop} for a solve of its own,
    // {done, null} for a sharded one (its shards agree on the stop between batches)
    if (ws->done_cap < (size_t)B) {
        if (ws->h_done) (void)hipHostFree(ws->h_done);
        ws->h_done = nullptr; ws->d_done = nullptr; ws->done_cap = 0;
        BAOK(hipHostMalloc((void**)&ws->h_done, sizeof(int) * (B + 1), hipHostMallocMapped | hipHostMallocCoherent));
        BAOK(hipHostGetDevicePointer((void**)&ws->d_done, ws->h_done, 0));
        int* const ptrs[4] = {ws->d_done, ws->d_done + B, ws->d_done, nullptr};
        BAOK(ws->d_donep.ensure(4));
        BAOK(hipMemcpy(ws->d_donep.p, ptrs, sizeof(ptrs), hipMemcpyHostToDevice));
        ws->done_cap = B;
    }
    const bool relay = !c.sharded && c.stop;   // a caller's stop flag to relay mid-solve
    c.donep = ws->d_donep.p + (relay ? 0 : 2);
    c.h_stopw = relay ? ws->h_done + ws->done_cap : nullptr;
    for (int b = 0; b < B; b++)
        __atomic_store_n(ws->h_done + b, c.probs[b]->iterations > 0 ? 0 : 1, __ATOMIC_RELAXED);
    __atomic_store_n(ws->h_done + ws->done_cap, 0, __ATOMIC_RELAXED);
    return ORBHIP_OK;
}

// the linear solve of a large problem (one the single-workgroup launch does not hold)
int large_solve(const BaCall& c, int b) {
    const Prep& p = c.pp[b];
    const BaArgs& a = c.ha[b];
    const int* gate = &c.dctl[b].phase;
    if (p.use_nd) {   // (the gate was set at nd_setup)
        BAOK(nd_solve(c.nd_of(b), c.st));
    } else if (p.use_dag) {
        BAOK(chol_dag_solve(a.S, p.n, a.row_first, a.bs, a.x, a.flag, c.dd[b], c.st, gate));
    } else {
        chol_blocked_solve(a.S, p.n, a.Lsave, a.bs, a.x, a.flag, a.row_first, c.st, gate, a.cb_tiles,
                           p.cb_off.empty() ? nullptr : p.cb_off.data());
    }
    return ORBHIP_OK;
}

// ---- step 9: one slot = one LM trial of every problem, with the iteration's linearisation in
// front when it starts one; the controller applies the g2o rules per problem on the device, so
// the host only enqueues. Sharded solves run the same slot with their collectives on the stream
// between the kernels (RCCL across ranks, k_ba_multi_reduce across the shards of this process)
// and the controller's reductions split from its decisions (BaArgs::sync): every shard sees the
// same sums, so every shard takes the same decisions. Collectives of a sharded slot, in order:
// kHpp, kRed2, then kNdPack, kNdBz, kNdX (segments) or kRepS, kRepBs (replicated), then kRed01 ----
int enqueue_slot(BaCall& c) {
    BaWorkspace* ws = c.ws;
    const int B = c.B;
    hipStream_t st = c.st;
    const BaArgs* dA = c.dArgs;
    int* d_act = c.d_act;
    int* const* donep = c.donep;
    const dim3 b256(256);
    // the edge kernels of this call
    const auto kErrors = c.stereo ? k_ba_errors<true> : k_ba_errors<false>;
    const auto kLin = c.stereo ? k_ba_lin<true> : k_ba_lin<false>;
    const auto kSchurItems = c.stereo ? k_ba_schur_items<true> : k_ba_schur_items<false>;
    const auto kBacksub = c.stereo ? k_ba_backsub<true> : k_ba_backsub<false>;
    const auto kBacksubErrs = c.stereo ? k_ba_backsub_errs<true> : k_ba_backsub_errs<false>;
    // the sharded slots' error refresh and budget check; an unsharded problem's iteration
    // ends in its controller (ctl_end_decide) and its stale errors are refreshed by k_ba_lin
    if (!c.all_small && c.sharded)
        hipLaunchKernelGGL(kErrors, dim3(gx(c.maxE, 256), B), b256, 0, st, dA, d_act, 1, donep);
    hipLaunchKernelGGL(kLin, dim3(gx(c.maxM, kLinL) + gx(c.maxNp, c.lin_ppw), B), b256, 0, st, dA, d_act,
                       (int)gx(c.maxM, kLinL), c.lin_ppw, donep);
    if (c.sharded) {   // the trial start on the shards' sums: Hpp, then the largest diagonal
        if (coll(c, kHpp)) return ORBHIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_ba_sh_maxdiag, dim3(B), b256, 0, st, dA, d_act);
        if (coll(c, kRed2)) return ORBHIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_ba_sh_begin, dim3(B), dim3(64), 0, st, dA, d_act);
    }
    if (!c.s_readonly) hipLaunchKernelGGL(k_ba_zero_s, dim3(64, B), b256, 0, st, dA, d_act, 0);
    if (!c.fused) hipLaunchKernelGGL(k_ba_schur_points, dim3(gx(c.maxM, 256), B), b256, 0, st, dA, d_act);
    hipLaunchKernelGGL(kSchurItems, dim3(gx(2 * c.maxItems, 256) + gx(c.maxNp, 4) + 1, B), b256, 0, st, dA, d_act,
                       (int)gx(2 * c.maxItems, 256), donep);
    if (c.nd_sh) {   // each shard its segment; the separator system and x summed over the shards
        for (int b = 0; b < B; b++) BAOK(nd_factor_assemble(ws->nds[b], st));
        for (int b = 0; b < B; b++) BAOK(nd_sep_pack(ws->nds[b], 0, st));
        if (coll(c, kNdPack) || coll(c, kNdBz)) return ORBHIP_ERR_DEVICE;
        for (int b = 0; b < B; b++) BAOK(nd_sep_pack(ws->nds[b], 1, st));
        for (int b = 0; b < B; b++) BAOK(nd_separator_backsolve(ws->nds[b], st));
        if (coll(c, kNdX)) return ORBHIP_ERR_DEVICE;
        for (int b = 0; b < B; b++) BAOK(nd_finish(ws->nds[b], st));
    } else {
        if (c.sharded && (coll(c, kRepS) || coll(c, kRepBs))) return ORBHIP_ERR_DEVICE;   // replicated solves
        if (c.ns) {
            if (c.maxN <= kCholRegMaxN) BAOK(chol_reg_launch(c.maxN, c.ns, dA, d_act + 2 * B, st));
            else hipLaunchKernelGGL(k_ba_cholesky, dim3(c.ns), dim3(512), c.chol_lds, st, dA, d_act + 2 * B);
        }
        for (int b = 0; b < B; b++)
            if (c.large(b) && large_solve(c, b)) return ORBHIP_ERR_DEVICE;
    }
    if (c.fused) {
        hipLaunchKernelGGL(kBacksubErrs, dim3(c.gbs, B), b256, 0, st, dA, d_act, donep);
    } else {
        hipLaunchKernelGGL(kBacksub, dim3(gx(std::max(c.maxM, c.maxP), 256), B), b256, 0, st, dA, d_act);
        hipLaunchKernelGGL(kErrors, dim3(gx(c.maxE, 256), B), b256, 0, st, dA, d_act, 2, donep);
    }
    if (c.sharded) {   // the trial's end on the shards' sums of chi2 and the scale
        hipLaunchKernelGGL(k_ba_sh_sums, dim3(B), dim3(1024), 0, st, dA, d_act);
        if (coll(c, kRed01)) return ORBHIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_ba_sh_end, dim3(B), dim3(64), 0, st, dA, d_act, donep);
    }
    if (!c.all_small) hipLaunchKernelGGL(k_ba_pop, dim3(gx(c.maxPM, 256), B), b256, 0, st, dA, d_act);
    BAOK(hipGetLastError());
    return ORBHIP_OK;
}

// stop flag: one consistent decision across ranks (all-reduce max) per batch of slots; a failed
// collective counts as a stop
bool stop_now(const BaCall& c) {
    const bool local = c.stop && *c.stop;
    if (!c.rccl) return local;
    int* h = c.ws->h_stop.p;
    *h = local ? 1 : 0;
    if (rccl_consensus(c, h, c.ws->dstop.p, 1, ncclMax)) return true;
    return *h != 0;
}
// the outputs: the timeout words, e_chi2 of every problem + optimised poses/points (one
// transfer); r06: enqueued behind the slots that may be the last ones, so a solve that ended
// there needs no further host round trip (a wasted copy of ~115 KB at C4 otherwise)
int out_copies(const BaCall& c) {
    for (int i = 0; i < c.ndag; i++)
        BAOK(hipMemcpyAsync(c.ws->hto.p + i, c.tw[i], sizeof(int), hipMemcpyDeviceToHost, c.st));
    BAOK(hipMemcpyAsync(c.hd, c.D, sizeof(double) * (c.nC + c.nA), hipMemcpyDeviceToHost, c.st));
    return ORBHIP_OK;
}
bool all_done(const BaCall& c) {
    for (int b = 0; b < c.B; b++)
        if (!__atomic_load_n(c.ws->h_done + b, __ATOMIC_RELAXED)) return false;
    return true;
}
// with a stop flag to relay: polls, yielding the core between polls (the caller's Tracking
// thread may need it), and relays the flag into the mapped word; without one: blocks in the runtime
int wait_ev(const BaCall& c, hipEvent_t e) {
    if (!c.h_stopw) return hipEventSynchronize(e) == hipSuccess ? ORBHIP_OK : ORBHIP_ERR_DEVICE;
    for (;;) {
        std::this_thread::yield();
        const hipError_t q = hipEventQuery(e);
        if (q == hipSuccess) return ORBHIP_OK;
        if (q != hipErrorNotReady) return ORBHIP_ERR_DEVICE;
        if (c.stop && *c.stop) __atomic_store_n(c.h_stopw, 1, __ATOMIC_RELAXED);
    }
}
int read_ctl(const BaCall& c) {
    return hipMemcpyAsync(c.ws->hctl.p, c.dctl, c.B * sizeof(LmCtl), hipMemcpyDeviceToHost, c.st) == hipSuccess
               ? ORBHIP_OK : ORBHIP_ERR_DEVICE;
}

struct EventPair {   // the two events of the slot loop, destroyed with it
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// ---- step 10: slots go out in chunks of kChunk behind one event each (at most two chunks in
// flight): the host checks the done flags once per chunk, and while it waits it relays the
// caller's stop flag into the mapped word that every trial's Schur launch copies into the
// controller (relay_host_stop; checked at the trial's end and the next iteration's start: g2o's
// force-stop checks), so a stop takes effect within a trial or two however many slots are queued.
// r04: an event or a store to host memory between every two slots put a ~5 us bubble in front of
// every trial (the queue drains for the marker; the kernel that wrote host memory ends with a
// system-scope release).
// Ranks of an RCCL solve must enqueue the same slots (their collectives pair up): they look at
// the stop flag only between batches, agreed by an all-reduce (stop_now, the one collective of
// this loop outside the slots), and never end a batch on the asynchronous done flags; the batch
// length comes from the LM state read back, which every rank holds identically ----
int ba_run_slots(BaCall& c) {
    EventPair ev;
    for (hipEvent_t& x : ev.e) BAOK(hipEventCreateWithFlags(&x, hipEventDisableTiming | hipEventDisableSystemFence));
    constexpr int kChunk = 8;
    const int B = c.B;
    const bool rccl = c.rccl;
    const dim3 gB((unsigned)((B + 255) / 256)), b256(256);
    int rc = ORBHIP_OK;
    int remaining = 0;   // slots every unfinished problem still needs at least
    for (int b = 0; b < B; b++) remaining = std::max(remaining, c.probs[b]->iterations);
    int nchunk = 0;
    bool last_ev_spec = false;   // the last event recorded follows the speculative copies
    bool ctl_with_outputs = false;   // the final LM state is read back with the outputs
    while (remaining > 0) {
        if (rccl && !c.stop_sent && stop_now(c)) {
            hipLaunchKernelGGL(k_ba_ctl_stop, gB, b256, 0, c.st, c.dctl, B, c.donep);
            c.stop_sent = true;
        }
        // RCCL: at most kChunk slots per batch, so the agreed stop is looked at every few trials
        const int batch = rccl ? std::min(remaining, kChunk) : remaining;
        for (int k = 0; k < batch && rc == ORBHIP_OK;) {
            if (!rccl && !c.stop_sent && c.stop && *c.stop) {
                hipLaunchKernelGGL(k_ba_ctl_stop, gB, b256, 0, c.st, c.dctl, B, c.donep);
                c.stop_sent = true;
            }
            const int n = std::min(kChunk, batch - k);
            for (int j = 0; j < n && rc == ORBHIP_OK; j++) rc = enqueue_slot(c);
            k += n;
            bool spec = false;   // this batch's last slots: the LM state and outputs behind them
            if (rc == ORBHIP_OK && !rccl && k == batch) {
                spec = true;
                if (read_ctl(c) != ORBHIP_OK || out_copies(c) != ORBHIP_OK) rc = ORBHIP_ERR_DEVICE;
            }
            if (rc == ORBHIP_OK && hipEventRecord(ev[nchunk & 1], c.st) != hipSuccess) rc = ORBHIP_ERR_DEVICE;
            if (rc != ORBHIP_OK) break;
            last_ev_spec = spec;
            if (nchunk++ >= 1) rc = wait_ev(c, ev[nchunk & 1]);   // the chunk before this one
            if (rc == ORBHIP_OK && !rccl && all_done(c)) break;
        }
        if (rc == ORBHIP_OK) rc = wait_ev(c, ev[(nchunk - 1) & 1]);
        if (rc != ORBHIP_OK) return rc;
        if (!rccl && all_done(c)) {   // every problem ended: its LM state comes with the outputs
            // (already in when the last event followed the speculative copies)
            c.outputs_in = last_ev_spec;
            ctl_with_outputs = !c.outputs_in;
            break;
        }
        if (read_ctl(c) != ORBHIP_OK || hipStreamSynchronize(c.st) != hipSuccess) return ORBHIP_ERR_DEVICE;
        remaining = 0;
        for (int b = 0; b < B; b++) {
            const LmCtl& l = c.ws->hctl.p[b];
            if (l.phase == kPhDone) continue;
            remaining = std::max(remaining, c.stop_sent ? 1 : std::max(1, l.iterations - l.it));
        }
    }
    // the LM state read back with the outputs below (one synchronisation for all of it: each
    // read-back + synchronisation of its own cost ~20-30 us of host round trip at C4)
    return ctl_with_outputs ? read_ctl(c) : (int)ORBHIP_OK;
}

// ---- step 11: the outputs and the LM state in host memory; then the hand-off timeouts of the
// persistent solvers, agreed over the ranks (the last collective of an RCCL call: 1 int, max).
// kRerunNoDag: some solve timed out and the call is to run again on the other solvers ----
int ba_read_back(BaCall& c) {
    BaWorkspace* ws = c.ws;
    if (!c.outputs_in) {   // (else the speculative copies below the last slots brought them)
        if (out_copies(c) != ORBHIP_OK) return ORBHIP_ERR_DEVICE;
        BAOK(hipStreamSynchronize(c.st));
    }
    for (int b = 0; b < c.B; b++) c.res[b]->initial_chi2 = ws->hctl.p[b].initChi;
    int timeouts = 0;
    for (int i = 0; i < c.ndag; i++) timeouts += ws->hto.p[i];
    if (c.rccl) {   // one decision for every rank
        *ws->h_stop.p = timeouts;
        if (rccl_consensus(c, ws->h_stop.p, ws->dstop.p, 1, ncclMax)) return ORBHIP_ERR_DEVICE;
        timeouts = *ws->h_stop.p;
    }
    if (timeouts == 0) return ORBHIP_OK;
    ws->dag_timeouts += timeouts;
    // default: solve again on the non-persistent solvers (blocked / single-workgroup), which
    // reproduce the schedule g2o would have run; ORBHIP_DAG_RERUN=0 reports the timeout
    if (c.no_dag || !c.sw.dag_rerun) return ORBHIP_ERR_TIMEOUT;
    ws->dag_reruns++;
    return kRerunNoDag;
}

// the outputs of problem b, edges [e0, e1) (the poses, points and LM words with the first range)
void write_outputs(const BaCall& c, int b, int e0, int e1) {
    const Prep& p = c.pp[b];
    const orbhip_ba_problem* pr = c.probs[b];
    orbhip_ba_result* r = c.res[b];
    const double* pose_o = c.hd + c.sA + p.o_state;
    const double* pts_o = pose_o + 8 * (size_t)p.P;
    const double* chi2_o = c.hd + c.sC + p.o_chi2;
    if (e0 == 0) {
        const LmCtl& l = c.ws->hctl.p[b];   // read back in the slot loop, or with the outputs
        r->final_chi2 = l.currentChi;
        r->iterations_done = l.it;
        r->lm_trials = l.trials;
        for (int i = 0; i < p.P; i++) {
            if (r->pose_q) for (int k = 0; k < 4; k++) r->pose_q[4 * i + k] = (float)pose_o[8 * i + k];
            if (r->pose_t) for (int k = 0; k < 3; k++) r->pose_t[3 * i + k] = (float)pose_o[8 * i + 4 + k];
        }
        if (r->points) for (int k = 0; k < 3 * p.M; k++) r->points[k] = (float)pts_o[k];
    }
    for (int e = e0; e < e1; e++) {
        if (r->edge_chi2) r->edge_chi2[e] = (float)chi2_o[e];
        if (r->edge_depth_ok) {   // isDepthPositive: (T.map(X)).z > 0
            const double* T = &pose_o[8 * pr->edge_pose[e]];
            const double* X = &pts_o[3 * pr->edge_point[e]];
            double ux = T[1] * X[2] - T[2] * X[1], uy = T[2] * X[0] - T[0] * X[2];
            ux += ux; uy += uy;
            const double uz2 = 2 * (T[0] * X[1] - T[1] * X[0]);
            const double cz = T[0] * uy - T[1] * ux;
            const double z = X[2] + T[3] * uz2 + cz + T[6];
            r->edge_depth_ok[e] = z > 0.0 ? 1 : 0;
        }
    }
}
// ---- step 12: the results, and the timing line ----
void ba_write_results(const BaCall& c) {
    const int B = c.B;
    if (B == 1 && c.pp[0].E >= kPrepParallelE && host_pool_on()) {
        // one large problem (a GBA): its edges in chunks on the host pool (r06, late: the C5 loop's
        // 80k depth tests and conversions took ~0.2 ms on one core)
        const int E = c.pp[0].E, T = std::min(host_threads(), E / 4096 + 1);
        HostPool::get(host_threads() - 1).run(T, [&](int t) {
            write_outputs(c, 0, (int)((long long)E * t / T), (int)((long long)E * (t + 1) / T));
        });
    } else {
        parallel_for(B, c.nth, [&](int b) { write_outputs(c, b, 0, c.pp[b].E); });
    }
    if (c.sw.timing)
        std::fprintf(stderr,
                     "orbhip ba timing B=%d: prep %.3f ms (problem structure %.3f), pack+upload %.3f ms, solve %.3f ms, "
                     "outputs %.3f ms\n",
                     B, c.t_prep - c.t_start, c.t_prepare - c.t_start, c.t_pack - c.t_prep, c.t_solve - c.t_pack,
                     now_ms() - c.t_solve);
}

}  // namespace

int ba_solve_batch(BaWorkspace* ws, const orbhip_ba_problem* const* probs, int B, orbhip_ba_result* const* res,
                   const volatile int* stop, hipStream_t st, int shard_mode, bool no_dag, bool no_nd,
                   const BaStereoExt* sx) {
    BaCall c{ws, probs, B, res, stop, st, shard_mode, no_dag, no_nd, sx};
    int rc = ba_validate(ws, probs, B, res, shard_mode, sx, c.stereo);
    if (rc) return rc;
    c.sw = read_switches();
    c.sharded = shard_mode != kShardNone;
    c.rccl = shard_mode == kShardRccl;
    c.t_start = now_ms();
    c.nth = host_threads();
    if ((rc = ba_prepare_all(c))) return rc;
    ba_choose_solvers(c);
    if (c.sharded && (rc = ba_plan_shards(c))) return rc;
    ba_plan_factors(c);
    c.t_prep = now_ms();
    ba_layout(c);
    if ((rc = ba_pack_upload(c))) return rc;
    if (c.rccl && !c.nd_sh && !c.pp[0].row_first.empty() && (rc = ba_union_envelope(c))) return rc;
    c.t_pack = now_ms();
    rc = ba_init_controllers(c);
    // (the re-runs re-enter with the same workspace, after this frame's last use of its preparations)
    if (rc == kRerunNoNd) return ba_solve_batch(ws, probs, B, res, stop, st, shard_mode, no_dag, true, sx);
    if (rc) return rc;
    if (c.sharded && (rc = ba_make_sites(c))) return rc;
    if ((rc = ba_enqueue_start(c))) return rc;
    if ((rc = ba_run_slots(c))) return rc;
    c.t_solve = now_ms();
    rc = ba_read_back(c);
    if (rc == kRerunNoDag) return ba_solve_batch(ws, probs, B, res, stop, st, shard_mode, true, no_nd, sx);
    if (rc) return rc;
    ba_write_results(c);
    return ORBHIP_OK;
}

int ba_solve(BaWorkspace* ws, const orbhip_ba_problem* prob, orbhip_ba_result* res, const volatile int* stop,
             hipStream_t st) {
    const orbhip_ba_problem* pp[1] = {prob};
    orbhip_ba_result* rr[1] = {res};
    return ba_solve_batch(ws, pp, 1, rr, stop, st, kShardNone);
}

void ba_stats(BaWorkspace* ws, long long* timeouts, long long* reruns) {
    *timeouts = ws ? ws->dag_timeouts : 0;
    *reruns = ws ? ws->dag_reruns : 0;
}

int ba_comm_init(BaWorkspace* ws, int nranks, int rank, const void* id) {
    if (nranks < 1 || rank < 0 || rank >= nranks || !id) return ORBHIP_ERR_ARG;
    if (ws->comm) { (void)ncclCommDestroy(ws->comm); ws->comm = nullptr; }
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    if (ncclCommInitRank(&ws->comm, nranks, uid, rank) != ncclSuccess) { ws->comm = nullptr; return ORBHIP_ERR_DEVICE; }
    ws->nranks = nranks;
    ws->rank = rank;
    BAOK(ws->dstop.ensure(1));
    BAOK(ws->dint4.ensure(8));
    BAOK(ws->h_int4.ensure(8));
    BAOK(ws->h_stop.ensure(1));
    return ORBHIP_OK;
}

int ba_comm_unique_id(void* id) {
    ncclUniqueId uid;
    if (ncclGetUniqueId(&uid) != ncclSuccess) return ORBHIP_ERR_DEVICE;
    std::memcpy(id, &uid, sizeof(uid));
    return ORBHIP_OK;
}

// Diagnostic: factor+solve one SPD system with per-phase cycle stamps (test hook).
// Diagnostic: the register-resident solver on one SPD system (test hook); reps launches timed.
int ba_test_cholesky_reg(const double* A, const double* b, double* x, int n, int reps, float* ms,
                         unsigned long long* phases5) {
    if (n <= 0 || n > kCholRegMaxN || reps < 1) return ORBHIP_ERR_ARG;
    double *dS = nullptr, *db_ = nullptr, *dx = nullptr;
    int *df = nullptr, *dact = nullptr;
    BaArgs* dargs = nullptr;
    BAOK(hipMalloc((void**)&dS, sizeof(double) * n * n));
    BAOK(hipMalloc((void**)&db_, sizeof(double) * n));
    BAOK(hipMalloc((void**)&dx, sizeof(double) * n));
    BAOK(hipMalloc((void**)&df, sizeof(int)));
    BAOK(hipMalloc((void**)&dact, sizeof(int)));
    BAOK(hipMalloc((void**)&dargs, sizeof(BaArgs)));
    BAOK(hipMemcpy(dS, A, sizeof(double) * n * n, hipMemcpyHostToDevice));
    BAOK(hipMemcpy(db_, b, sizeof(double) * n, hipMemcpyHostToDevice));
    BaArgs h{};
    h.n = n; h.S = dS; h.bs = db_; h.x = dx; h.flag = df;
    const int zero = 0;
    BAOK(hipMemcpy(dargs, &h, sizeof(BaArgs), hipMemcpyHostToDevice));
    BAOK(hipMemcpy(dact, &zero, sizeof(int), hipMemcpyHostToDevice));
    BAOK(chol_reg_launch(n, 1, dargs, dact, nullptr));   // warm-up (S is read-only)
    hipEvent_t e0, e1;
    BAOK(hipEventCreate(&e0)); BAOK(hipEventCreate(&e1));
    BAOK(hipEventRecord(e0, nullptr));
    for (int r = 0; r < reps; r++) BAOK(chol_reg_launch(n, 1, dargs, dact, nullptr));
    BAOK(hipEventRecord(e1, nullptr));
    BAOK(hipDeviceSynchronize());
    BAOK(hipEventElapsedTime(ms, e0, e1));
    *ms /= reps;
    if (phases5) {
        unsigned long long* dd = nullptr;
        BAOK(hipMalloc((void**)&dd, sizeof(unsigned long long) * 48));
        BAOK(hipMemset(dd, 0, 48 * 8));
        BAOK(chol_reg_probe(n, dargs, dd, nullptr));
        BAOK(hipMemcpy(phases5, dd, sizeof(unsigned long long) * 48, hipMemcpyDeviceToHost));
        (void)hipFree(dd);
    }
    int fl = 0;
    BAOK(hipMemcpy(&fl, df, sizeof(int), hipMemcpyDeviceToHost));
    BAOK(hipMemcpy(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost));
    (void)hipFree(dS); (void)hipFree(db_); (void)hipFree(dx); (void)hipFree(df); (void)hipFree(dact);
    (void)hipFree(dargs);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return fl ? ORBHIP_OK : ORBHIP_ERR_NOT_PD;
}

int ba_test_cholesky(const double* A, const double* b, double* x, int n, unsigned long long* phases5, float* ms) {
    double *dS = nullptr, *db_ = nullptr, *dx = nullptr;
    int* df = nullptr;
    unsigned long long* dd = nullptr;
    BAOK(hipMalloc((void**)&dS, sizeof(double) * n * n));
    BAOK(hipMalloc((void**)&db_, sizeof(double) * n));
    BAOK(hipMalloc((void**)&dx, sizeof(double) * n));
    BAOK(hipMalloc((void**)&df, sizeof(int)));
    BAOK(hipMalloc((void**)&dd, sizeof(unsigned long long) * 8));
    BAOK(hipMemcpy(dS, A, sizeof(double) * n * n, hipMemcpyHostToDevice));
    BAOK(hipMemcpy(db_, b, sizeof(double) * n, hipMemcpyHostToDevice));
    BAOK(hipMemset(dd, 0, 64));
    BAOK(hipFuncSetAttribute((const void*)k_chol_test, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const size_t lds = sizeof(double) * chol_lds_doubles(n);
    double* dL = nullptr;
    BAOK(hipMalloc((void**)&dL, sizeof(double) * 1024 * ((n + 31) / 32)));
    hipEvent_t e0, e1;
    BAOK(hipEventCreate(&e0)); BAOK(hipEventCreate(&e1));
    BAOK(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(k_chol_test, dim3(1), dim3(512), lds, nullptr, dS, db_, dx, n, df, dL, dd);
    BAOK(hipEventRecord(e1, nullptr));
    BAOK(hipDeviceSynchronize());
    BAOK(hipEventElapsedTime(ms, e0, e1));
    int fl = 0;
    BAOK(hipMemcpy(&fl, df, sizeof(int), hipMemcpyDeviceToHost));
    BAOK(hipMemcpy(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost));
    BAOK(hipMemcpy(phases5, dd, sizeof(unsigned long long) * 5, hipMemcpyDeviceToHost));
    (void)hipFree(dS); (void)hipFree(db_); (void)hipFree(dx); (void)hipFree(df); (void)hipFree(dd);
    (void)hipFree(dL);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return fl ? ORBHIP_OK : ORBHIP_ERR_NOT_PD;
}

}  // namespace orbhip
