// gfx950 ORBmatcher::Fuse (LocalMapping::SearchInNeighbors), B keyframes against one list of
// MapPoints in one call (DESIGN.md "Fuse"):
//   fuse_kf_params    host, fp32, fixed operation order: the grid scales and mOw of a keyframe
//   k_fuse_grid       one 1024-thread work-group per keyframe: PosInGrid of every keypoint, a
//                     3072-bin histogram in LDS (12 KiB), an exclusive scan, then the keypoints
//                     scattered into a cell-ordered array of 16-byte records (x, y, cell << 8 | octave, index)
//                     with cell_start[3073] beside it. The position inside a cell is whatever the LDS
//                     counters hand out: k_fuse_search takes the minimum of (distance, cell, index)
//                     over the gated candidates, which does not depend on the order they are met in.
//   k_fuse_search     grid (tiles of 64 points, B), four lanes per (keyframe, point): the gates of
//                     steps 1-7 with an early exit, the point's descriptor in 8 VGPRs, the walk of
//                     the cell rectangle through cell_start (a column of cells is one span of the
//                     cell-ordered array; the four lanes take its entries in turns) with the level
//                     and chi-square gates ahead of the descriptor load, a u64 minimum of
//                     dist << 32 | cell << 16 | idx, merged over the four lanes at the end.
//                     No pair reads what another pair writes (no `taken`, no stealing, no rotation
//                     histogram), so there is no resolve phase. nfused[b]: one LDS atomic per wave,
//                     one global atomic per work-group.
//                     k_fuse_search<S, false> is the rule of Fuse with a Sim3 (LoopClosing::SearchAndFuse):
//                     the same walk without the chi-square gate.
//                     The stereo forms (k_fuse_grid<true>, k_fuse_search<S, true, true>; DESIGN.md "Stereo
//                     LocalMapping"): the grid also scatters mvuRight into a cell-ordered float array beside
//                     the records, and a candidate with ur >= 0 that passed the window and level gates takes
//                     the three-term chi-square at 7.8 against the point's right projection u - bf / z.
// and LoopClosing's SearchByProjection with a Sim3, one keyframe, upstream's sequential greedy pass
// (DESIGN.md "Sim3 functions of LoopClosing"):
//   k_sim3_search     the walk again, four lanes per point, also testing `claimed` and the distance
//                     threshold; per point the 8 smallest keys (sorted, in registers), their total
//                     count and the window go to global memory
//   k_sim3_resolve    ONE 1024-thread work-group turns the lists into the sequential result as a fixed
//                     point over an owner table in global memory; a list longer than 8 is continued by
//                     walking the window again; rounds <= (points with a list) + 1
// LDS: k_fuse_grid 12 KiB histogram + 12 KiB cursors + scan scratch; k_fuse_search 4 bytes; k_sim3_resolve 12 bytes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "geom.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" fuse", x)

namespace orbhip {

constexpr int kFuseMaxPoints = 65536;  // MapPoints per call
constexpr int kFuseMaxLevels = 256;    // the octave shares a word with the cell
struct FuseKf {                        // one keyframe of the call
    int n, base;                       // its keypoints are entries [base, base + n) of the call's arrays
    float minx, maxx, miny, maxy, invw, invh;
    float q[4], t[3], Ow[3], fx, fy, cx, cy;
};
struct FuseRec { float x, y; int cell_oct, idx; };   // a keypoint in cell order: cell << 8 | octave, its index
struct Sim3Win {                       // what k_sim3_resolve needs to walk a point's window again
    float u, v, r;
    int lvl;                           // -1: the point never reached the walk
    int rect;                          // x0 | x1 << 8 | y0 << 16 | y1 << 24
};
struct Sim3Work {                      // device scratch of one call (n points, nk keypoints)
    Sim3Win* win;                      // n
    unsigned long long* list;          // n x kSim3ListCap, ascending, ~0 = empty
    int32_t* count;                    // n: the full length of the list
    unsigned long long *pick, *pick_new;   // n each
    int32_t* owner;                    // nk
};

// ---- host: per-keyframe constants (all fp32, every operation in the order written; no FMA):
// grid scales and mOw ----
static void fuse_kf_params(const orbhip_frame& f, int base, FuseKf* k) {
    k->n = f.n;
    k->base = base;
    k->minx = f.min_x; k->maxx = f.max_x; k->miny = f.min_y; k->maxy = f.max_y;
    k->invw = (float)kGridCols / (f.max_x - f.min_x);
    k->invh = (float)kGridRows / (f.max_y - f.min_y);
    for (int i = 0; i < 4; i++) k->q[i] = f.pose_q[i];
    for (int i = 0; i < 3; i++) k->t[i] = f.pose_t[i];
    const float qc[4] = {-f.pose_q[0], -f.pose_q[1], -f.pose_q[2], f.pose_q[3]};
    const float mt[3] = {f.pose_t[0] * -1.0f, f.pose_t[1] * -1.0f, f.pose_t[2] * -1.0f};
    quat_rotate(qc, mt, k->Ow);
    k->fx = f.fx; k->fy = f.fy; k->cx = f.cx; k->cy = f.cy;
}

// ---- device ----
constexpr int kFuseGridThreads = 1024;
constexpr int kFuseBinsPerThread = kGridCells / kFuseGridThreads;
static_assert(kFuseBinsPerThread * kFuseGridThreads == kGridCells, "k_fuse_grid scans 3 bins per thread");
struct FuseGridLds {
    int hist[kGridCells];     // keypoints per cell
    int cursor[kGridCells];   // next free slot of a cell while scattering
    int scan[kFuseGridThreads / 64 + 1];
};

// STEREO: ur (mvuRight, in keypoint order like kps) goes to ur_cell in the order of recs
template <bool STEREO>
__global__ __launch_bounds__(kFuseGridThreads) void k_fuse_grid(const FuseKf* __restrict__ kfs,
                                                                const orbhip_kp* __restrict__ kps,
                                                                int32_t* __restrict__ cell_start,
                                                                FuseRec* __restrict__ recs,
                                                                int32_t* __restrict__ nfused,
                                                                const float* __restrict__ ur,
                                                                float* __restrict__ ur_cell) {
    __shared__ FuseGridLds L;
    const int tid = threadIdx.x, b = blockIdx.x;
    const FuseKf f = kfs[b];
    const orbhip_kp* kp = kps + f.base;
    for (int c = tid; c < kGridCells; c += kFuseGridThreads) L.hist[c] = 0;
    if (tid == 0) nfused[b] = 0;
    __syncthreads();
    for (int i = tid; i < f.n; i += kFuseGridThreads) {
        const int c = grid_cell(f.minx, f.miny, f.invw, f.invh, kp[i].x, kp[i].y);
        if (c >= 0) atomicAdd(&L.hist[c], 1);
    }
    __syncthreads();
    int h[kFuseBinsPerThread], sum = 0;
#pragma unroll
    for (int k = 0; k < kFuseBinsPerThread; k++) { h[k] = L.hist[tid * kFuseBinsPerThread + k]; sum += h[k]; }
    int total;
    int pos = block_excl_scan(sum, L.scan, &total);
    int32_t* cs = cell_start + (int64_t)b * (kGridCells + 1);
#pragma unroll
    for (int k = 0; k < kFuseBinsPerThread; k++) {
        const int c = tid * kFuseBinsPerThread + k;
        L.cursor[c] = pos;
        cs[c] = pos;
        pos += h[k];
    }
    if (tid == 0) cs[kGridCells] = total;
    __syncthreads();
    // the slot inside a cell is the order in which the LDS counter is reached: any order serves,
    // k_fuse_search's key minimum does not depend on it
    FuseRec* out = recs + f.base;
    for (int i = tid; i < f.n; i += kFuseGridThreads) {
        const orbhip_kp k = kp[i];
        const int c = grid_cell(f.minx, f.miny, f.invw, f.invh, k.x, k.y);
        if (c >= 0) {
            const int slot = atomicAdd(&L.cursor[c], 1);
            out[slot] = FuseRec{k.x, k.y, (c << 8) | k.octave, i};
            if (STEREO) ur_cell[f.base + slot] = ur[f.base + i];
        }
    }
}

constexpr int kFuseThreads = 256;
// lanes per (keyframe, point). Measured on one MI355X, both kernels of a call, B = 30 x 1000 points x
// 1000 keypoints / B = 1 x 20000 x 1000: 1 lane 27.7 / 19.1 us, 4 lanes 18.6 / 15.8 us, 8 lanes
// 20.9 / 18.1 us
constexpr int kFuseSplit = 4;

// Steps 1-8 of the rule for one (keyframe, point) that is not skipped: false at a gate. lvl is set
// from step 6 on (-1 before it), so a pair rejected by GetFeaturesInArea's early returns keeps it.
// z = Pc.z, read by the stereo form only (set from step 2 on).
struct FuseWin { float u, v, r; int lvl, x0, x1, y0, y1; float z; };
__device__ __forceinline__ bool fuse_gates(const FuseKf& f, const DevPoints& mp, int m,
                                           const float* __restrict__ scale_factors, int n_levels,
                                           const LevelSteps& steps, float th, FuseWin& w) {
    w.lvl = -1;
    const float P[3] = {mp.pts[3 * m], mp.pts[3 * m + 1], mp.pts[3 * m + 2]};
    // 1. Sophus SE3f * p
    float Pc[3];
    quat_rotate(f.q, P, Pc);
    Pc[0] += f.t[0]; Pc[1] += f.t[1]; Pc[2] += f.t[2];
    if (Pc[2] < 0.0f) return false;
    // 2., 3. Pinhole::project, KeyFrame::IsInImage (the maximum is strict)
    const float u = (f.fx * Pc[0]) / Pc[2] + f.cx, v = (f.fy * Pc[1]) / Pc[2] + f.cy;
    w.z = Pc[2];
    if (!(u >= f.minx && u < f.maxx && v >= f.miny && v < f.maxy)) return false;
    // 4. distance range
    const float PO[3] = {P[0] - f.Ow[0], P[1] - f.Ow[1], P[2] - f.Ow[2]};
    const float dist3D = sqrtf((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
    const float maxd = mp.maxd[m];
    if (dist3D < 0.8f * mp.mind[m] || dist3D > 1.2f * maxd) return false;
    // 5. viewing angle
    const float* Pn = mp.nrm + 3 * m;
    if ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2] < 0.5f * dist3D) return false;
    // 6. MapPoint::PredictScale
    const int lvl = predict_scale(maxd / dist3D, steps, scale_factors + n_levels, n_levels);
    w.lvl = lvl;
    // 7. radius
    const float r = th * scale_factors[lvl];
    w.u = u; w.v = v; w.r = r;
    // 8. KeyFrame::GetFeaturesInArea: the cell rectangle with its early returns
    w.x0 = max(0, (int)floorf((u - f.minx - r) * f.invw));
    if (w.x0 >= kGridCols) return false;
    w.x1 = min(kGridCols - 1, (int)ceilf((u - f.minx + r) * f.invw));
    if (w.x1 < 0) return false;
    w.y0 = max(0, (int)floorf((v - f.miny - r) * f.invh));
    if (w.y0 >= kGridRows) return false;
    w.y1 = min(kGridRows - 1, (int)ceilf((v - f.miny + r) * f.invh));
    if (w.y1 < 0) return false;
    return true;
}

__device__ __forceinline__ unsigned fuse_hamming(const uint4& da, const uint4& db, const uint8_t* __restrict__ d) {
    const uint4* d2 = (const uint4*)d;
    return hamming256(da, db, d2[0], d2[1]);
}
__device__ __forceinline__ unsigned long long fuse_key(unsigned dist, const FuseRec& k) {
    return ((unsigned long long)dist << 32) | ((unsigned long long)(k.cell_oct >> 8) << 16) | (unsigned)k.idx;
}

// S neighbouring lanes share a point: each computes the gates of steps 1-7 (the same values, so the
// same exits), they take the candidates of a column span in turns and merge their minima.
// CHI2 = false: the rule of Fuse with a Sim3, which has no chi-square gate (inv_level_sigma2 unread)
// STEREO (with CHI2): ur_cell = mvuRight in the order of recs, kf_bf[b] = mbf; a candidate with
// ur >= 0 takes (ex^2 + ey^2) + er^2 against 7.8, er = (u - bf * (1 / Pc.z)) - ur; the others 5.99
template <int S, bool CHI2, bool STEREO = false>
__global__ __launch_bounds__(kFuseThreads) void k_fuse_search(const FuseKf* __restrict__ kfs, DevPoints mp,
                                                              const uint8_t* __restrict__ pair_skip,
                                                              const float* __restrict__ scale_factors,
                                                              const float* __restrict__ inv_level_sigma2,
                                                              int n_levels, LevelSteps steps, float th,
                                                              const int32_t* __restrict__ cell_start,
                                                              const FuseRec* __restrict__ recs,
                                                              const uint8_t* __restrict__ kf_desc,
                                                              int32_t* __restrict__ best_idx,
                                                              int32_t* __restrict__ best_dist,
                                                              int32_t* __restrict__ level,
                                                              int32_t* __restrict__ nfused,
                                                              const float* __restrict__ ur_cell,
                                                              const float* __restrict__ kf_bf) {
    static_assert(S >= 1 && S <= 64 && (S & (S - 1)) == 0, "the lanes of a point lie in one wave");
    static_assert(CHI2 || !STEREO, "the stereo form is a form of the chi-square gate");
    __shared__ int s_count;
    const int b = blockIdx.y, m = (blockIdx.x * kFuseThreads + threadIdx.x) / S, sub = threadIdx.x % S;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const FuseKf f = kfs[b];
    int outIdx = -1, outDist = 256, outLvl = -1;
    unsigned long long best = ~0ull;
    do {
        if (m >= mp.n) break;
        if (mp.skip[m]) break;
        if (pair_skip && pair_skip[(int64_t)b * mp.n + m]) break;
        FuseWin w;
        const bool in = fuse_gates(f, mp, m, scale_factors, n_levels, steps, th, w);
        outLvl = w.lvl;
        if (!in) break;
        const float u = w.u, v = w.v, r = w.r;
        const int lvl = w.lvl;
        const uint4* dm = (const uint4*)(mp.desc + (int64_t)m * 32);
        const uint4 da = dm[0], db = dm[1];
        const int32_t* cs = cell_start + (int64_t)b * (kGridCells + 1);
        const FuseRec* rc = recs + f.base;
        const uint8_t* kd = kf_desc + (int64_t)f.base * 32;
        float urp = 0.0f;          // the point's projection into the right image
        const float* urc = nullptr;
        if (STEREO) {
            const float invz = 1.0f / w.z;
            urp = u - kf_bf[b] * invz;
            urc = ur_cell + f.base;
        }
        for (int ix = w.x0; ix <= w.x1; ix++) {
            // the cells (ix, y0..y1) are neighbours in the cell-ordered array: one span per column
            const int j0 = cs[ix * kGridRows + w.y0], j1 = cs[ix * kGridRows + w.y1 + 1];
            for (int j = j0 + sub; j < j1; j += S) {
                const FuseRec k = rc[j];
                const float dx = k.x - u, dy = k.y - v;
                if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
                // 9. level gate, chi-square gate, then the descriptor
                const int octave = k.cell_oct & 0xFF;
                if (octave < lvl - 1 || octave > lvl) continue;
                if (CHI2) {
                    const float ex = u - k.x, ey = v - k.y;
                    const float e2 = ex * ex + ey * ey;
                    const float kur = STEREO ? urc[j] : -1.0f;
                    if (STEREO && kur >= 0.0f) {
                        const float er = urp - kur;
                        const float e3 = e2 + er * er;
                        if ((double)(e3 * inv_level_sigma2[octave]) > 7.8) continue;
                    } else if ((double)(e2 * inv_level_sigma2[octave]) > 5.99) continue;
                }
                const unsigned long long key = fuse_key(fuse_hamming(da, db, kd + (int64_t)k.idx * 32), k);
                best = key < best ? key : best;
            }
        }
    } while (false);
#pragma unroll
    for (int w = 1; w < S; w <<= 1) {   // the S lanes of a point took the same gates: all of them are here
        const unsigned long long o = __shfl_xor(best, w);
        best = o < best ? o : best;
    }
    if (best != ~0ull) {
        outDist = (int)(best >> 32);
        // 10. TH_LOW
        if (outDist <= 50) outIdx = (int)(best & 0xFFFF);
    }
    if (m < mp.n && sub == 0) {
        const int64_t o = (int64_t)b * mp.n + m;
        best_idx[o] = outIdx;
        best_dist[o] = outDist;
        level[o] = outLvl;
    }
    const int c = __popcll(__ballot(outIdx >= 0 && sub == 0));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_count, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(&nfused[b], s_count);
}

// ---- SearchByProjection with a Sim3: the lists, then the greedy pass over them ----
constexpr unsigned long long kSim3None = ~0ull;

// A candidate of the sequential pass that can ever be claimed: inside the window, octave in
// [lvl - 1, lvl], not claimed at call time, dist < 256 and (float)dist <= thr. kSim3None otherwise.
__device__ __forceinline__ unsigned long long sim3_candidate(const FuseRec& k, float u, float v, float r, int lvl,
                                                             const uint8_t* __restrict__ claimed, const uint4& da,
                                                             const uint4& db, const uint8_t* __restrict__ kd, float thr) {
    const float dx = k.x - u, dy = k.y - v;
    if (!(fabsf(dx) < r && fabsf(dy) < r)) return kSim3None;
    if (claimed[k.idx]) return kSim3None;
    const int octave = k.cell_oct & 0xFF;
    if (octave < lvl - 1 || octave > lvl) return kSim3None;
    const unsigned dist = fuse_hamming(da, db, kd + (int64_t)k.idx * 32);
    if (!(dist < 256u && (float)dist <= thr)) return kSim3None;
    return fuse_key(dist, k);
}

// The walk of k_fuse_search for one keyframe, without the chi-square gate and with the two tests of
// sim3_candidate. Each of the S lanes of a point keeps the kSim3ListCap smallest keys it met, sorted,
// in registers (an unrolled insertion: static indices only); the lanes' lists are merged into the
// point's list[m] (ascending, kSim3None behind the end), count[m] is the number of candidates met.
// level[m] and win[m] are written for every point; match / match_dist are k_sim3_resolve's.
template <int S>
__global__ __launch_bounds__(kFuseThreads) void k_sim3_search(const FuseKf* __restrict__ kfs, DevPoints mp,
                                                              const uint8_t* __restrict__ claimed,
                                                              const float* __restrict__ scale_factors, int n_levels,
                                                              LevelSteps steps, float th, float thr,
                                                              const int32_t* __restrict__ cell_start,
                                                              const FuseRec* __restrict__ recs,
                                                              const uint8_t* __restrict__ kf_desc, Sim3Work wk,
                                                              int32_t* __restrict__ level) {
    static_assert(S >= 1 && S <= 64 && (S & (S - 1)) == 0, "the lanes of a point lie in one wave");
    constexpr int K = kSim3ListCap;
    const int m = (blockIdx.x * kFuseThreads + threadIdx.x) / S, sub = threadIdx.x % S;
    const FuseKf f = kfs[0];
    unsigned long long a[K];
#pragma unroll
    for (int i = 0; i < K; i++) a[i] = kSim3None;
    int cnt = 0;
    FuseWin w;
    w.lvl = -1; w.u = w.v = w.r = w.z = 0.0f; w.x0 = w.x1 = w.y0 = w.y1 = 0;
    bool in = false;
    if (m < mp.n && !mp.skip[m]) in = fuse_gates(f, mp, m, scale_factors, n_levels, steps, th, w);
    if (in) {
        const uint4* dm = (const uint4*)(mp.desc + (int64_t)m * 32);
        const uint4 da = dm[0], db = dm[1];
        for (int ix = w.x0; ix <= w.x1; ix++) {
            const int j0 = cell_start[ix * kGridRows + w.y0], j1 = cell_start[ix * kGridRows + w.y1 + 1];
            for (int j = j0 + sub; j < j1; j += S) {
                unsigned long long key = sim3_candidate(recs[j], w.u, w.v, w.r, w.lvl, claimed, da, db, kf_desc, thr);
                if (key == kSim3None) continue;
                cnt++;
                if (key < a[K - 1]) {
#pragma unroll
                    for (int i = 0; i < K; i++) {
                        const unsigned long long lo = key < a[i] ? key : a[i];
                        key = key < a[i] ? a[i] : key;
                        a[i] = lo;
                    }
                }
            }
        }
    }
    // merge: K times the least head of the S lanes; keys are distinct (the index is in them), so one
    // lane pops. Lanes of points past n or rejected hold empty lists and take part all the same.
#pragma unroll
    for (int s = 1; s < S; s <<= 1) cnt += __shfl_xor(cnt, s);
    unsigned long long out[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        unsigned long long mn = a[0];
#pragma unroll
        for (int s = 1; s < S; s <<= 1) {
            const unsigned long long o = __shfl_xor(mn, s);
            mn = o < mn ? o : mn;
        }
        out[j] = mn;
        if (a[0] == mn && mn != kSim3None) {
#pragma unroll
            for (int i = 0; i + 1 < K; i++) a[i] = a[i + 1];
            a[K - 1] = kSim3None;
        }
    }
    if (m < mp.n && sub == 0) {
        level[m] = w.lvl;
        wk.win[m] = Sim3Win{w.u, w.v, w.r, in ? w.lvl : -1, w.x0 | (w.x1 << 8) | (w.y0 << 16) | (w.y1 << 24)};
        wk.count[m] = cnt;
#pragma unroll
        for (int j = 0; j < K; j++) wk.list[(int64_t)m * K + j] = out[j];
    }
}

// The owner table lives in global memory (65535 keypoints do not fit LDS as words) and is read and
// written by one work-group only: atomics at agent scope, so no access is served from a stale L1 line.
__device__ __forceinline__ int sim3_owner(const int32_t* owner, int idx) {
    return __hip_atomic_load(owner + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The first entry of L[m] whose keypoint no earlier point holds (owner >= m): from the stored keys,
// and, when all of them are held and the list is longer than what is stored, from a walk of the
// window for the least key above the last stored one.
__device__ unsigned long long sim3_eval(int m, const DevPoints& mp, const uint8_t* __restrict__ claimed,
                                        float thr, const int32_t* __restrict__ cell_start,
                                        const FuseRec* __restrict__ recs, const uint8_t* __restrict__ kf_desc,
                                        const Sim3Work& wk) {
    constexpr int K = kSim3ListCap;
    const int cnt = wk.count[m];
    const unsigned long long* l = wk.list + (int64_t)m * K;
    unsigned long long last = 0;
    for (int j = 0; j < K && j < cnt; j++) {
        last = l[j];
        if (sim3_owner(wk.owner, (int)(last & 0xFFFF)) >= m) return last;
    }
    if (cnt <= K) return kSim3None;
    const Sim3Win w = wk.win[m];
    const int x0 = w.rect & 0xFF, x1 = (w.rect >> 8) & 0xFF, y0 = (w.rect >> 16) & 0xFF, y1 = (w.rect >> 24) & 0xFF;
    const uint4* dm = (const uint4*)(mp.desc + (int64_t)m * 32);
    const uint4 da = dm[0], db = dm[1];
    unsigned long long best = kSim3None;
    for (int ix = x0; ix <= x1; ix++) {
        const int j0 = cell_start[ix * kGridRows + y0], j1 = cell_start[ix * kGridRows + y1 + 1];
        for (int j = j0; j < j1; j++) {
            const unsigned long long key = sim3_candidate(recs[j], w.u, w.v, w.r, w.lvl, claimed, da, db, kf_desc, thr);
            if (key == kSim3None || key <= last || key >= best) continue;
            if (sim3_owner(wk.owner, (int)(key & 0xFFFF)) >= m) best = key;
        }
    }
    return best;
}

constexpr int kSim3ResolveThreads = 1024;
constexpr int kSim3NoOwner = 0x7FFFFFFF;

// The sequential pass as a fixed point, in ONE work-group (no work-group waits for another):
//   pick_{r+1}[m] = the first e of L[m] with min{m' : pick_r[m'] = e.idx} >= m
// from pick_0 = nothing. After round k the k lowest points with a list hold their final keypoint (a
// point's choice depends on the picks of lower points only), so the first round that changes nothing
// is the sequential result and it comes within (points with a list) + 1 rounds: the loop's bound.
// owner[idx] = the lowest point whose pick is idx, rebuilt between rounds (only the entries the old
// picks set are cleared).
__global__ __launch_bounds__(kSim3ResolveThreads) void k_sim3_resolve(DevPoints mp,
                                                                       const uint8_t* __restrict__ claimed, float thr,
                                                                       int nk, const int32_t* __restrict__ cell_start,
                                                                       const FuseRec* __restrict__ recs,
                                                                       const uint8_t* __restrict__ kf_desc, Sim3Work wk,
                                                                       int32_t* __restrict__ match,
                                                                       int32_t* __restrict__ match_dist,
                                                                       int32_t* __restrict__ nmatches) {
    __shared__ int s_active, s_changed, s_matched;
    const int tid = threadIdx.x, n = mp.n;
    if (tid == 0) { s_active = 0; s_changed = 0; s_matched = 0; }
    __syncthreads();
    for (int i = tid; i < nk; i += kSim3ResolveThreads)
        __hip_atomic_store(wk.owner + i, kSim3NoOwner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int mine = 0;
    for (int m = tid; m < n; m += kSim3ResolveThreads) {
        wk.pick[m] = kSim3None;
        mine += wk.count[m] > 0;
    }
    if (mine) atomicAdd(&s_active, mine);
    __syncthreads();
    const int rounds = s_active + 1;
    for (int r = 0; r < rounds; r++) {
        bool diff = false;
        for (int m = tid; m < n; m += kSim3ResolveThreads) {
            if (wk.count[m] == 0) continue;
            const unsigned long long p = sim3_eval(m, mp, claimed, thr, cell_start, recs, kf_desc, wk);
            wk.pick_new[m] = p;
            diff |= p != wk.pick[m];
        }
        if (diff) s_changed = 1;
        __syncthreads();
        const bool changed = s_changed != 0;     // the same value in every thread: the exit is uniform
        if (!changed) break;
        for (int m = tid; m < n; m += kSim3ResolveThreads) {
            const unsigned long long p = wk.pick[m];
            if (p != kSim3None)
                __hip_atomic_store(wk.owner + (int)(p & 0xFFFF), kSim3NoOwner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (tid == 0) s_changed = 0;
        for (int m = tid; m < n; m += kSim3ResolveThreads) {
            if (wk.count[m] == 0) continue;
            const unsigned long long p = wk.pick_new[m];
            wk.pick[m] = p;
            if (p != kSim3None) atomicMin(wk.owner + (int)(p & 0xFFFF), m);
        }
        __syncthreads();
    }
    int got = 0;
    for (int m = tid; m < n; m += kSim3ResolveThreads) {
        const unsigned long long p = wk.pick[m];
        match[m] = p == kSim3None ? -1 : (int)(p & 0xFFFF);
        match_dist[m] = p == kSim3None ? 256 : (int)(p >> 32);
        got += p != kSim3None;
    }
    if (got) atomicAdd(&s_matched, got);
    __syncthreads();
    if (tid == 0) nmatches[0] = s_matched;
}

// ---- host ----
// match / match_dist / level: n, nmatches: 1. cell_start: 3073 + recs: nk (written by k_fuse_grid,
// which also zeroes nmatches)
static void launch_sim3_search(const FuseKf* kf, const DevPoints& mp, const uint8_t* claimed,
                               const float* scale_factors, int n_levels, float log_sf, float th, float thr,
                               const orbhip_kp* kps, const uint8_t* kf_desc, int nk, int32_t* cell_start,
                               FuseRec* recs, const Sim3Work& w, int32_t* match, int32_t* match_dist, int32_t* level,
                               int32_t* nmatches, hipStream_t st) {
    const LevelSteps steps = level_steps(log_sf, n_levels);
    ORBHIP_LAUNCH(k_fuse_grid<false>, dim3(1), dim3(kFuseGridThreads), 0, st, kf, kps, cell_start, recs, nmatches,
                  (const float*)nullptr, (float*)nullptr);
    const unsigned tiles = (unsigned)(((int64_t)mp.n * kFuseSplit + kFuseThreads - 1) / kFuseThreads);
    ORBHIP_LAUNCH(k_sim3_search<kFuseSplit>, dim3(tiles), dim3(kFuseThreads), 0, st, kf, mp, claimed, scale_factors,
                  n_levels, steps, th, thr, (const int32_t*)cell_start, (const FuseRec*)recs, kf_desc, w, level);
    ORBHIP_LAUNCH(k_sim3_resolve, dim3(1), dim3(kSim3ResolveThreads), 0, st, mp, claimed, thr, nk,
                  (const int32_t*)cell_start, (const FuseRec*)recs, kf_desc, w, match, match_dist, nmatches);
}

// cell_start: B x 3073, recs: one per keypoint of the call (both written by k_fuse_grid);
// best_idx / best_dist / level: B x n, nfused: B (zeroed by k_fuse_grid).
// inv_level_sigma2 == nullptr: the rule without the chi-square gate (Fuse with a Sim3)
// ur != nullptr: the stereo form (inv_level_sigma2 is then required)
static void launch_fuse(const FuseKf* kfs, int B, const DevPoints& mp, const uint8_t* pair_skip,
                        const float* scale_factors, const float* inv_level_sigma2, int n_levels, float log_sf,
                        float th, const orbhip_kp* kps, const uint8_t* kf_desc, int32_t* cell_start, FuseRec* recs,
                        int32_t* best_idx, int32_t* best_dist, int32_t* level, int32_t* nfused, hipStream_t st,
                        const float* ur = nullptr, float* ur_cell = nullptr, const float* kf_bf = nullptr) {
    const unsigned tiles = (unsigned)(((int64_t)mp.n * kFuseSplit + kFuseThreads - 1) / kFuseThreads);
    const LevelSteps steps = level_steps(log_sf, n_levels);
    if (ur) {   // the stereo form: ur / ur_cell one per keypoint of the call, kf_bf B
        ORBHIP_LAUNCH(k_fuse_grid<true>, dim3((unsigned)B), dim3(kFuseGridThreads), 0, st, kfs, kps, cell_start, recs,
                      nfused, ur, ur_cell);
        ORBHIP_LAUNCH((k_fuse_search<kFuseSplit, true, true>), dim3(tiles, (unsigned)B), dim3(kFuseThreads), 0, st, kfs,
                      mp, pair_skip, scale_factors, inv_level_sigma2, n_levels, steps, th, (const int32_t*)cell_start,
                      (const FuseRec*)recs, kf_desc, best_idx, best_dist, level, nfused, (const float*)ur_cell, kf_bf);
        return;
    }
    ORBHIP_LAUNCH(k_fuse_grid<false>, dim3((unsigned)B), dim3(kFuseGridThreads), 0, st, kfs, kps, cell_start, recs,
                  nfused, (const float*)nullptr, (float*)nullptr);
    if (inv_level_sigma2)
        ORBHIP_LAUNCH((k_fuse_search<kFuseSplit, true>), dim3(tiles, (unsigned)B), dim3(kFuseThreads), 0, st, kfs, mp,
                      pair_skip, scale_factors, inv_level_sigma2, n_levels, steps, th, (const int32_t*)cell_start,
                      (const FuseRec*)recs, kf_desc, best_idx, best_dist, level, nfused, (const float*)nullptr,
                      (const float*)nullptr);
    else
        ORBHIP_LAUNCH((k_fuse_search<kFuseSplit, false>), dim3(tiles, (unsigned)B), dim3(kFuseThreads), 0, st, kfs, mp,
                      pair_skip, scale_factors, inv_level_sigma2, n_levels, steps, th, (const int32_t*)cell_start,
                      (const FuseRec*)recs, kf_desc, best_idx, best_dist, level, nfused, (const float*)nullptr,
                      (const float*)nullptr);
}

// The envelope and argument checks Fuse and the Sim3 searches share: the keyframes of a call have one
// scale pyramid, at most 65535 keypoints each and octaves inside it. nk_total: their keypoints.
static int fuse_check_keyframes(const orbhip_frame* kfs, int B, size_t* nk_total) {
    const int L = kfs[0].n_levels;
    if (L <= 0 || !kfs[0].scale_factors) return ORBHIP_ERR_ARG;
    if (L > kFuseMaxLevels) return ORBHIP_ERR_UNSUPPORTED;
    *nk_total = 0;
    for (int b = 0; b < B; b++) {
        const orbhip_frame& f = kfs[b];
        if (f.n < 0) return ORBHIP_ERR_ARG;
        if (f.n > 65535) return ORBHIP_ERR_UNSUPPORTED;
        if (f.n && (!f.kps || !f.desc)) return ORBHIP_ERR_ARG;
        // one scale pyramid per call
        if (f.n_levels != L || !f.scale_factors || f.log_scale_factor != kfs[0].log_scale_factor) return ORBHIP_ERR_ARG;
        if (std::memcmp(f.scale_factors, kfs[0].scale_factors, (size_t)L * 4) != 0) return ORBHIP_ERR_ARG;
        for (int i = 0; i < f.n; i++)
            if (f.kps[i].octave < 0 || f.kps[i].octave >= L) return ORBHIP_ERR_ARG;
        *nk_total += (size_t)f.n;
    }
    return ORBHIP_OK;
}

int fuse_search(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_frame* kfs, int B,
                const orbhip_local_points* mps, const uint8_t* pair_skip, bool chi2, const float* inv_level_sigma2,
                float th, int32_t* best_idx, int32_t* best_dist, int32_t* level, int32_t* nfused,
                const FuseStereo* sx) {
    if (B < 0 || !mps || mps->n < 0) return ORBHIP_ERR_ARG;
    if (B == 0) return 0;
    if (B > kFuseMaxKf || mps->n > kFuseMaxPoints) return ORBHIP_ERR_UNSUPPORTED;
    if (!kfs || !nfused) return ORBHIP_ERR_ARG;
    const int n = mps->n, L = kfs[0].n_levels;
    if (chi2 && !inv_level_sigma2) return ORBHIP_ERR_ARG;
    if (sx && (!chi2 || !sx->u_right || !sx->bf)) return ORBHIP_ERR_ARG;   // (per keyframe: the caller's checks)
    size_t nk_total = 0;
    if (const int rc = fuse_check_keyframes(kfs, B, &nk_total)) return rc;
    for (int b = 0; b < B; b++) nfused[b] = 0;
    if (n == 0) return 0;
    if (!best_idx || !mps->points || !mps->normals || !mps->min_dist || !mps->max_dist || !mps->desc)
        return ORBHIP_ERR_ARG;
    // one block, the same layout on the host (pinned) and the device:
    // [keyframes B | scale factors, level steps | inv sigma2 | points normals min max desc skip | pair_skip B x n |
    //  keypoints | keyframe descriptors | stereo: mvuRight, mbf B], then device only [cell_start B x 3073 |
    //  records | stereo: mvuRight in cell order | nfused B, best_idx B x n, best_dist B x n, level B x n];
    //  the last segment is read back
    StageLayout lay(16);
    const size_t bn = (size_t)B * (size_t)n;
    const size_t o_kf = lay.take((size_t)B * sizeof(FuseKf));
    const size_t o_sf = lay.take((size_t)L * 8), o_s2 = lay.take(chi2 ? (size_t)L * 4 : 0);   // + PredictScale's steps
    const PointsLayout o_mp(lay, (size_t)n);
    const size_t o_pskip = lay.take(pair_skip ? bn : 0);
    const size_t o_kps = lay.take(nk_total * sizeof(orbhip_kp)), o_kdesc = lay.take(nk_total * 32);
    const size_t o_ur = lay.take(sx ? nk_total * 4 : 0), o_bf = lay.take(sx ? (size_t)B * 4 : 0);
    const size_t up_bytes = lay.total();
    const size_t o_cs = lay.take((size_t)B * (kGridCells + 1) * 4), o_rec = lay.take(nk_total * sizeof(FuseRec));
    const size_t o_urc = lay.take(sx ? nk_total * 4 : 0);
    const size_t nf_bytes = ((size_t)B * 4 + 15) & ~size_t(15);   // best_idx starts 16-byte aligned behind nfused
    const size_t n_out = level ? 3 : (best_dist ? 2 : 1);         // arrays read back: a prefix of idx, dist, level
    const size_t back_bytes = nf_bytes + n_out * bn * 4;
    const size_t o_back = lay.take(nf_bytes + 3 * bn * 4);
    HIPOK(S.ensure(lay.total(), up_bytes + back_bytes + 16));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    FuseKf* hk = (FuseKf*)(h + o_kf);
    size_t base = 0;
    for (int b = 0; b < B; b++) {
        const orbhip_frame& f = kfs[b];
        fuse_kf_params(f, (int)base, &hk[b]);
        put_keyframe(S, o_kps, o_kdesc, base, f.kps, f.desc, (size_t)f.n);
        if (sx && f.n > 0) S.put(o_ur + base * 4, sx->u_right[b], (size_t)f.n * 4);
        base += (size_t)f.n;
    }
    if (sx) S.put(o_bf, sx->bf, (size_t)B * 4);
    S.put(o_sf, kfs[0].scale_factors, (size_t)L * 4);
    S.put(o_sf + (size_t)L * 4, level_thresholds(kfs[0].log_scale_factor, L), (size_t)L * 4);
    if (chi2) S.put(o_s2, inv_level_sigma2, (size_t)L * 4);
    const DevPoints mp = o_mp.put(S, *mps, true);   // the kernels read skip unconditionally
    if (pair_skip) S.put(o_pskip, pair_skip, bn);
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    int32_t* const d_nf = (int32_t*)(d + o_back);
    int32_t* const d_idx = (int32_t*)(d + o_back + nf_bytes);
    {
        const StageScope scope(timer);
        timer.begin(8, st);
        launch_fuse((const FuseKf*)(d + o_kf), B, mp, pair_skip ? d + o_pskip : nullptr, (const float*)(d + o_sf),
                    chi2 ? (const float*)(d + o_s2) : nullptr, L, kfs[0].log_scale_factor, th,
                    (const orbhip_kp*)(d + o_kps), d + o_kdesc,
                    (int32_t*)(d + o_cs), (FuseRec*)(d + o_rec), d_idx, d_idx + bn, d_idx + 2 * bn, d_nf, st,
                    sx ? (const float*)(d + o_ur) : nullptr, sx ? (float*)(d + o_urc) : nullptr,
                    sx ? (const float*)(d + o_bf) : nullptr);
        timer.end(8, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + o_back, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    std::memcpy(nfused, hb, (size_t)B * 4);
    std::memcpy(best_idx, hb + nf_bytes, bn * 4);
    if (best_dist) std::memcpy(best_dist, hb + nf_bytes + bn * 4, bn * 4);
    if (level) std::memcpy(level, hb + nf_bytes + 2 * bn * 4, bn * 4);
    int total = 0;
    for (int b = 0; b < B; b++) total += nfused[b];
    return total;
}

int sim3_search(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_frame* kf,
                const orbhip_local_points* mps, float th, float ratio_hamming, int32_t* match, int32_t* match_dist,
                int32_t* level) {
    if (!kf || !mps || mps->n < 0) return ORBHIP_ERR_ARG;
    if (!(ratio_hamming > 0.0f) || !std::isfinite(ratio_hamming)) return ORBHIP_ERR_ARG;
    if (mps->n > kFuseMaxPoints) return ORBHIP_ERR_UNSUPPORTED;
    size_t nk = 0;
    if (const int rc = fuse_check_keyframes(kf, 1, &nk)) return rc;
    const int n = mps->n, L = kf->n_levels;
    if (n == 0) return 0;
    if (!match || !mps->points || !mps->normals || !mps->min_dist || !mps->max_dist || !mps->desc) return ORBHIP_ERR_ARG;
    const float thr = 50.0f * ratio_hamming;
    // one block, the same layout on the host (pinned) and the device:
    // [keyframe | scale factors, level steps | points normals min max desc skip | claimed | keypoints | descriptors],
    // then device only [cell_start 3073 | records | windows n | lists n x 8 | counts n | picks 2 x n |
    //  owners | nmatches, match n, match_dist n, level n]; the last segment is read back
    StageLayout lay(16);
    const size_t o_kf = lay.take(sizeof(FuseKf)), o_sf = lay.take((size_t)L * 8);   // + PredictScale's steps
    const PointsLayout o_mp(lay, (size_t)n);
    const size_t o_claimed = lay.take(nk), o_kps = lay.take(nk * sizeof(orbhip_kp)), o_kdesc = lay.take(nk * 32);
    const size_t up_bytes = lay.total();
    const size_t o_cs = lay.take((size_t)(kGridCells + 1) * 4), o_rec = lay.take(nk * sizeof(FuseRec));
    const size_t o_win = lay.take((size_t)n * sizeof(Sim3Win)), o_list = lay.take((size_t)n * kSim3ListCap * 8);
    const size_t o_cnt = lay.take((size_t)n * 4), o_pick = lay.take((size_t)n * 8), o_pnew = lay.take((size_t)n * 8);
    const size_t o_own = lay.take(nk * 4);
    const size_t n_out = level ? 3 : (match_dist ? 2 : 1);   // arrays read back: a prefix of match, dist, level
    const size_t back_bytes = 16 + n_out * (size_t)n * 4;     // match starts 16-byte aligned behind nmatches
    const size_t o_back = lay.take(16 + 3 * (size_t)n * 4);
    HIPOK(S.ensure(lay.total(), up_bytes + back_bytes + 16));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    fuse_kf_params(*kf, 0, (FuseKf*)(h + o_kf));
    S.put(o_sf, kf->scale_factors, (size_t)L * 4);
    S.put(o_sf + (size_t)L * 4, level_thresholds(kf->log_scale_factor, L), (size_t)L * 4);
    const DevPoints mp = o_mp.put(S, *mps, true);   // the kernels read skip unconditionally
    S.put_or_zero(o_claimed, kf->claimed, nk);
    put_keyframe(S, o_kps, o_kdesc, 0, kf->kps, kf->desc, nk);
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    int32_t* const d_nm = (int32_t*)(d + o_back);
    int32_t* const d_match = (int32_t*)(d + o_back + 16);
    {
        const StageScope scope(timer);
        timer.begin(9, st);
        const Sim3Work w{(Sim3Win*)(d + o_win), (unsigned long long*)(d + o_list), (int32_t*)(d + o_cnt),
                         (unsigned long long*)(d + o_pick), (unsigned long long*)(d + o_pnew), (int32_t*)(d + o_own)};
        launch_sim3_search((const FuseKf*)(d + o_kf), mp, d + o_claimed, (const float*)(d + o_sf), L,
                           kf->log_scale_factor, th, thr, (const orbhip_kp*)(d + o_kps), d + o_kdesc, (int)nk,
                           (int32_t*)(d + o_cs), (FuseRec*)(d + o_rec), w, d_match, d_match + n, d_match + 2 * (size_t)n,
                           d_nm, st);
        timer.end(9, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + o_back, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    std::memcpy(match, hb + 16, (size_t)n * 4);
    if (match_dist) std::memcpy(match_dist, hb + 16 + (size_t)n * 4, (size_t)n * 4);
    if (level) std::memcpy(level, hb + 16 + 2 * (size_t)n * 4, (size_t)n * 4);
    int32_t nm;
    std::memcpy(&nm, hb, 4);
    return nm;
}

}  // namespace orbhip
