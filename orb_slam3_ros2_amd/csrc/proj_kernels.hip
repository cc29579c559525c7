// Projection-guided matching:
//   U:src/ORBmatcher.cc::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
//   U:src/Frame.cc::Frame::isInFrustum + ORBmatcher::SearchByProjection(Frame& F,
//       const vector<MapPoint*>& vpMapPoints, th, bFarPoints, thFarPoints)
// with the frame grid of U:src/Frame.cc (AssignFeaturesToGrid, PosInGrid, GetFeaturesInArea).
//
// MI355X formulation. The grid walk "cells ix (outer), iy, then cell order" is a total order on
// the frame's keypoints: key = (cell = px * 48 + py) << 16 | index, and a keypoint is visited
// iff its cell lies in the query's cell rectangle. So instead of CSR cell lists, ONE WAVEFRONT
// PER QUERY scans the frame's keypoints (lanes over keypoints, the query descriptor in
// registers), applies the rectangle / level / |dx|,|dy| < r tests, and keeps the lexicographic
// (distance, key) top-2 with levels; a wave merge then gives exactly the reference's best and
// second best (strict <, first in walk order wins).
// The reference is greedy: a current keypoint matched by an earlier query is skipped by later
// ones. That sequential dependence is resolved by a fixed point over parallel rounds: every round
// recomputes all queries with the exclusion "claimed by an earlier query in the previous round's
// picks" (owner[k] < i, an atomicMin over the picks); query i is final once queries < i are, and
// a round that changes nothing is exactly the sequential result (each pick equals its greedy
// definition given the picks before it). Typically 2-3 rounds.
// Rectified-stereo frames (the stereo branches of both functions): the query also carries its
// projection into the right image, a candidate with a right coordinate further than the window
// radius from it is skipped (stereo_gate, in every device form), and the last-frame search takes
// its level window from the direction of motion (proj_direction, decided on the host).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/orbhip.h"
#include "dev_attr.h"
#include "geom.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "proj.h"
#include "proj_ws.h"
#include "rot_filter.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" proj", x)

namespace orbhip {

ORBHIP_TRACE_UNIT(proj)   // kernel id 7: k_proj_lists (phases 1-3), its resolving work-group (16-20)

namespace {

constexpr int kThHigh = 100;

struct ProjFrame {     // the current Frame
    int n;
    float minx, maxx, miny, maxy, invw, invh;
    float q[4], t[3], fx, fy, cx, cy;
    float R[9], Ow[3];   // mRcw, mOw (isInFrustum)
    float bf;            // mbf of a rectified-stereo Frame (0: monocular, ur = u)
};
struct Query {         // one projected MapPoint: GetFeaturesInArea(u, v, r, minL, maxL)
    float u, v, r;
    int minL, maxL, valid;
    float ur;          // its projection into the right image, u - bf / z (the stereo gate)
};
// The stereo gate of both searches, a property of the (query, keypoint) pair: a keypoint with a
// right coordinate (mvuRight > 0) further than the window radius from the query's is skipped.
// u_right < 0 (or no u_right array: the monocular searches) never gates.
__device__ __forceinline__ bool stereo_gate(const Query& Q, float u_right) {
    return u_right > 0.0f && fabsf(Q.ur - u_right) > Q.r;
}
// GetFeaturesInArea's cell rectangle of a query (nMinCellX .. nMaxCellY), whether it meets the
// grid at all, and whether the walk tests levels
struct CellRect {
    int x0, x1, y0, y1;
    bool any, bCheckLevels;
    __device__ __forceinline__ CellRect(const ProjFrame& f, const Query& Q) {
        x0 = max(0, (int)floorf((Q.u - f.minx - Q.r) * f.invw));
        x1 = min(kGridCols - 1, (int)ceilf((Q.u - f.minx + Q.r) * f.invw));
        y0 = max(0, (int)floorf((Q.v - f.miny - Q.r) * f.invh));
        y1 = min(kGridRows - 1, (int)ceilf((Q.v - f.miny + Q.r) * f.invh));
        any = x0 < kGridCols && x1 >= 0 && y0 < kGridRows && y1 >= 0;
        bCheckLevels = (Q.minL > 0) || (Q.maxL >= 0);
    }
    // cell = px * kGridRows + py (0xFFFF, k_proj_lists' "no cell": px = 1365, outside)
    __device__ __forceinline__ bool contains(int c) const {
        const int px = c / kGridRows, py = c - px * kGridRows;
        return px >= x0 && px <= x1 && py >= y0 && py <= y1;
    }
};

__global__ void k_proj_cells(ProjFrame f, const orbhip_kp* __restrict__ kps, int* __restrict__ cell) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= f.n) return;
    cell[k] = grid_cell(f.minx, f.miny, f.invw, f.invh, kps[k].x, kps[k].y);
}

// SearchByProjection(CurrentFrame, LastFrame, th, bMono): window th * scale[lastOctave], levels
// lastOctave - 1 .. lastOctave + 1; !bMono and the camera moved forward (dir 1): lastOctave and up,
// backward (dir -1): 0 .. lastOctave
struct PrepLast {
    const float* pts;
    const int* oct;
    const float* scale;
    float th;
    int dir;
};
__device__ __forceinline__ Query prep_last(const ProjFrame& f, const PrepLast& a, int i) {
    Query Q{0, 0, 0, 0, 0, 0};
    const float P[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
    float Xc[3];
    quat_rotate(f.q, P, Xc);
    Xc[0] += f.t[0]; Xc[1] += f.t[1]; Xc[2] += f.t[2];
    const float invzc = (float)(1.0 / (double)Xc[2]);
    if (!(invzc < 0)) {
        const float u = f.fx * Xc[0] / Xc[2] + f.cx, v = f.fy * Xc[1] / Xc[2] + f.cy;
        if (!(u < f.minx || u > f.maxx || v < f.miny || v > f.maxy)) {
            const int lo = a.oct[i];
            const float ur = u - f.bf * invzc;
            const int minL = a.dir > 0 ? lo : a.dir < 0 ? 0 : lo - 1;
            const int maxL = a.dir > 0 ? -1 : a.dir < 0 ? lo : lo + 1;
            Q = Query{u, v, a.th * a.scale[lo], minL, maxL, 1, ur};
        }
    }
    return Q;
}
__global__ void k_proj_prep_last(ProjFrame f, int nq, PrepLast a, Query* __restrict__ qs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    qs[i] = prep_last(f, a, i);
}

// Frame::isInFrustum(pMP, viewCosLimit) + the window of SearchByProjection(F, vpMapPoints, ...)
struct PrepLocal {
    const float *pts, *nrm, *mind, *maxd;
    const uint8_t* skip;
    const float* scale;   // the scale factors, then PredictScale's steps (level_thresholds)
    int n_levels;
    float view_cos_limit, th;
    int far_points;
    float th_far;
    LevelSteps steps;     // the first of them, in the kernel arguments
};
__device__ __forceinline__ Query prep_local(const ProjFrame& f, const PrepLocal& a, int m, uint8_t* iv_out,
                                            int* lvl_out, float* xr_out) {
    Query Q{0, 0, 0, 0, 0, 0};
    uint8_t iv = 0;
    int lvl = -1;
    float xr = 0.0f;
    do {
        if (a.skip && a.skip[m]) break;
        const float* P = a.pts + 3 * m;
        const float* R = f.R;
        const float Pc[3] = {R[0] * P[0] + R[1] * P[1] + R[2] * P[2] + f.t[0],
                             R[3] * P[0] + R[4] * P[1] + R[5] * P[2] + f.t[1],
                             R[6] * P[0] + R[7] * P[1] + R[8] * P[2] + f.t[2]};
        const float Pc_dist = sqrtf(Pc[0] * Pc[0] + Pc[1] * Pc[1] + Pc[2] * Pc[2]);
        if (Pc[2] < 0.0f) break;
        const float u = f.fx * Pc[0] / Pc[2] + f.cx, v = f.fy * Pc[1] / Pc[2] + f.cy;
        if (u < f.minx || u > f.maxx) break;
        if (v < f.miny || v > f.maxy) break;
        const float PO[3] = {P[0] - f.Ow[0], P[1] - f.Ow[1], P[2] - f.Ow[2]};
        const float dist = sqrtf(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]);
        const float maxDistance = 1.2f * a.maxd[m], minDistance = 0.8f * a.mind[m];
        if (dist < minDistance || dist > maxDistance) break;
        const float* Pn = a.nrm + 3 * m;
        const float viewCos = (PO[0] * Pn[0] + PO[1] * Pn[1] + PO[2] * Pn[2]) / dist;
        if (viewCos < a.view_cos_limit) break;
        const float ratio = a.maxd[m] / dist;
        const int nScale = predict_scale(ratio, a.steps, a.scale + a.n_levels, a.n_levels);
        iv = 1;
        lvl = nScale;
        const float invz = 1.0f / Pc[2];
        xr = u - f.bf * invz;   // mTrackProjXR
        if (a.far_points && Pc_dist > a.th_far) break;
        float r = viewCos > 0.998 ? 2.5f : 4.0f;   // RadiusByViewingCos
        if (a.th != 1.0f) r *= a.th;
        Q = Query{u, v, r * a.scale[nScale], nScale - 1, nScale, 1, xr};
    } while (false);
    *iv_out = iv;
    *lvl_out = lvl;
    *xr_out = xr;
    return Q;
}
__global__ void k_proj_prep_local(ProjFrame f, int nq, PrepLocal a, Query* __restrict__ qs,
                                  uint8_t* __restrict__ in_view, int* __restrict__ level,
                                  float* __restrict__ proj_xr) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nq) return;
    uint8_t iv;
    int lvl;
    float xr;
    qs[m] = prep_local(f, a, m, &iv, &lvl, &xr);
    in_view[m] = iv;
    level[m] = lvl;
    if (proj_xr) proj_xr[m] = xr;
}

// lexicographic (dist, key) top-2 with the level of each
struct Top2 { int d1, k1, l1, d2, k2, l2; };
__device__ __forceinline__ bool lt(int da, int ka, int db, int kb) { return da < db || (da == db && ka < kb); }
__device__ __forceinline__ void top2_add(Top2& a, int d, int k, int l) {
    if (lt(d, k, a.d1, a.k1)) { a.d2 = a.d1; a.k2 = a.k1; a.l2 = a.l1; a.d1 = d; a.k1 = k; a.l1 = l; }
    else if (lt(d, k, a.d2, a.k2)) { a.d2 = d; a.k2 = k; a.l2 = l; }
}
// the wave's top-2 in every lane (lexicographic: the order of the merge does not matter)
__device__ __forceinline__ void top2_wave_merge(Top2& t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int d1 = __shfl_xor(t.d1, o, 64), k1 = __shfl_xor(t.k1, o, 64), l1 = __shfl_xor(t.l1, o, 64);
        const int d2 = __shfl_xor(t.d2, o, 64), k2 = __shfl_xor(t.k2, o, 64), l2 = __shfl_xor(t.l2, o, 64);
        top2_add(t, d1, k1, l1);
        top2_add(t, d2, k2, l2);
    }
}
// the pick of a query from its top-2. mode 0: LastFrame (best <= TH_HIGH); mode 1: local points
// (best/second, ratio test when both are on the same level)
__device__ __forceinline__ int proj_decide(const Top2& t, int mode, float nnratio) {
    if (t.d1 > kThHigh) return -1;
    if (mode == 0) return t.k1 & 0xFFFF;
    const bool same = t.l1 == t.l2;
    const bool reject = same && (float)t.d1 > nnratio * (float)t.d2;
    return (!reject && (!same || (float)t.d1 <= nnratio * (float)t.d2)) ? (t.k1 & 0xFFFF) : -1;
}

// Round r of the fixed point, one wave per query. mode 0: LastFrame (best <= TH_HIGH); mode 1:
// local points (best/second, ratio test when both on the same level). owner[k] < i excludes
// keypoints claimed earlier. The owner table rotates through three buffers: round r reads
// own[r % 3] (built from round r-1's picks), builds own[(r+1) % 3] by atomicMin, and clears
// own[(r+2) % 3] for round r+1, so a round is one launch. chg[r] = some pick changed in round r;
// a round whose predecessor changed nothing exits at once (the host launches rounds ahead).
__global__ __launch_bounds__(256) void k_proj_round(ProjFrame f, int nq, int mode, float nnratio, int r,
                                                    const Query* __restrict__ qs, const orbhip_kp* __restrict__ kps,
                                                    const uint8_t* __restrict__ kdesc, const int* __restrict__ cell,
                                                    const uint8_t* __restrict__ claimed, int* __restrict__ own3,
                                                    const uint8_t* __restrict__ qdesc, int* __restrict__ pick,
                                                    int* __restrict__ chg, const float* __restrict__ u_right) {
    if (r > 0 && chg[r - 1] == 0) return;   // converged: uniform over the grid
    const int n = f.n;
    const int* __restrict__ owner = own3 + (size_t)(r % 3) * n;
    int* own_next = own3 + (size_t)((r + 1) % 3) * n;
    int* own_clear = own3 + (size_t)((r + 2) % 3) * n;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) own_clear[k] = INT_MAX;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nq) return;
    const Query Q = qs[i];
    int p = -1;
    if (Q.valid) {
        const CellRect rect(f, Q);
        const uint4* qd4 = (const uint4*)(qdesc + 32 * (size_t)i);
        const uint4 qa = qd4[0], qb = qd4[1];
        Top2 t{256, INT_MAX, -1, 256, INT_MAX, -1};
        if (rect.any) {
            for (int k = lane; k < f.n; k += 64) {
                const int c = cell[k];
                if (c < 0 || !rect.contains(c)) continue;
                const orbhip_kp kp = kps[k];
                if (rect.bCheckLevels) {
                    if (kp.octave < Q.minL) continue;
                    if (Q.maxL >= 0 && kp.octave > Q.maxL) continue;
                }
                if (!(fabsf(kp.x - Q.u) < Q.r && fabsf(kp.y - Q.v) < Q.r)) continue;
                if ((claimed && claimed[k]) || owner[k] < i) continue;
                if (u_right && stereo_gate(Q, u_right[k])) continue;
                const uint4* kd4 = (const uint4*)(kdesc + 32 * (size_t)k);
                const uint4 ka = kd4[0], kb = kd4[1];
                const int d = hamming256(qa, qb, ka, kb);
                if (d == 256) continue;   // never best (dist < 256) nor second (dist < bestDist2 <= 256)
                top2_add(t, d, (c << 16) | k, kp.octave);
            }
        }
        top2_wave_merge(t);
        p = proj_decide(t, mode, nnratio);
    }
    if (lane == 0) {
        if (pick[i] != p) chg[r] = 1;
        pick[i] = p;
        if (p >= 0) atomicMin(&own_next[p], i);   // owner[k] = the first query whose pick is k
    }
}

// the rotation-consistency filter of SearchByProjection(CurrentFrame, LastFrame) and the count
__global__ __launch_bounds__(1024) void k_proj_finish(int nq, int check_orientation, const float* __restrict__ qangle,
                                                      const orbhip_kp* __restrict__ kps, const int* __restrict__ pick,
                                                      int* __restrict__ match, int* __restrict__ nmatch) {
    __shared__ int hist[32], keep[3], cnt;
    if (threadIdx.x < 32) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    auto bin_of = [&](int i, int k) { return rot_bin(qangle[i], kps[k].angle); };
    if (check_orientation) {
        for (int i = threadIdx.x; i < nq; i += blockDim.x)
            if (pick[i] >= 0) atomicAdd(&hist[bin_of(i, pick[i])], 1);
        __syncthreads();
        if (threadIdx.x < 64) three_maxima_wave(hist, keep);   // wave 0 of 1024 threads
        __syncthreads();
    }
    int c = 0;
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        int k = pick[i];
        if (k >= 0 && check_orientation && !rot_kept(bin_of(i, k), keep)) k = -1;
        match[i] = k;
        c += k >= 0;
    }
    atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) *nmatch = cnt;
}


// ---------------------------------------------------------------------------
// Two-launch form (the default while every candidate list fits kProjCap entries):
//   k_proj_lists    one wave per query: the query's window (prep_last / prep_local), then the
//                   round kernel's tests (cell rectangle, levels, |dx|,|dy| < r, pre-claimed
//                   keypoints, distance < 256) over the frame's keypoints ONCE, the passing
//                   keypoints appended by ballot as (dist << 32 | key << 4 | octave), key =
//                   cell << 16 | index: a u64 compare is the (dist, key) walk order
//   k_proj_resolve  ONE work-group: the fixed point of k_proj_round over the lists (owner tables
//                   in LDS, one barrier per round: a round walks a few list entries per query
//                   instead of scanning the frame), then k_proj_finish's rotation filter / count
// so the search is one upload, two launches and one download. A longer list (status word) sends
// the search to the round kernels with the inputs already on the device.
// ---------------------------------------------------------------------------
constexpr int kProjCap = 128;     // list entries per query
constexpr int kProjMaxN = 8192;   // frame keypoints: staged in LDS (16 B each), 3 owner tables of n ints
constexpr int kProjMaxQ = 8192;   // queries: list offsets in LDS
// queries per k_proj_lists work-group (one per wave of its first kListQ waves; the other waves
// only help stage the frame): one query wave per SIMD, so the scans do not share issue slots
constexpr int kListQ = 4;
// resolve_body's LDS head: 3 owner tables (n), list offsets (nq + 1), picks (nq); the lists follow
__host__ __device__ inline size_t resolve_head_bytes(int n, int nq) {
    return ((size_t)(3 * n + 2 * nq + 1) * 4 + 15) & ~size_t(15);
}
constexpr int kRectCap = 512;   // keypoints in a query's cell rectangle listed per wave (more: every keypoint)
constexpr size_t kListIdxBytes = kListQ * (kProjCap + kRectCap) * 2;   // k_proj_lists' per-wave index lists (LDS)

typedef __attribute__((address_space(1))) int pj_gint;
typedef __attribute__((address_space(1))) unsigned long long pj_gull;
__device__ __forceinline__ void st_ag(uint64_t* p, uint64_t v) {
    __hip_atomic_store((pj_gull*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_ag(const uint64_t* p) {
    return __hip_atomic_load((pj_gull*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_ag(int* p, int v) {
    __hip_atomic_store((pj_gint*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_ag(const int* p) {
    return __hip_atomic_load((pj_gint*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the one-launch form: the last work-group of k_proj_lists runs resolve_body (arrive: a counter,
// 0 between launches; fuse 0: the resolve runs as its own launch)
struct ResolveArgs {
    int fuse, check_orientation, ent_cap;
    const float* qangle;
    int* match;
    int* res;
    int* arrive;
};
template <int MODE>
__device__ void resolve_body(unsigned char* rsm, int n, int nq, float nnratio, int check_orientation, int cap,
                             int ent_cap, const float* __restrict__ qangle, const orbhip_kp* __restrict__ kps,
                             const uint64_t* __restrict__ lists, const int* __restrict__ lcnt,
                             const int* __restrict__ pick0, int* __restrict__ match, int* __restrict__ res,
                             unsigned long long* tr = nullptr);

// the frame's keypoints are staged once per work-group in LDS as (x, y, cell << 16 | claimed << 8 |
// octave, u_right or -1): PosInGrid computed as k_proj_cells does, a 16-byte read per lane and keypoint. The
// query's window is computed first, so its loads overlap the staging. A list entry is written for
// every keypoint passing the window tests (distance 256 included, skipped by the rounds): the
// ballot does not wait on the descriptor load, so the loads of all the scan's steps overlap.
// Round 0 of the fixed point (no exclusions) is the wave's own top-2: pick0[i].
template <int MODE>
__global__ __launch_bounds__(1024) void k_proj_lists(ProjFrame f, int nq, PrepLast pl, PrepLocal pc, int cap,
                                                     float nnratio, const orbhip_kp* __restrict__ kps,
                                                     const uint8_t* __restrict__ kdesc,
                                                     const uint8_t* __restrict__ claimed,
                                                     const uint8_t* __restrict__ qdesc,
                                                     uint64_t* __restrict__ lists, int* __restrict__ lcnt,
                                                     int* __restrict__ pick0, uint8_t* __restrict__ in_view,
                                                     int* __restrict__ level, ResolveArgs ra,
                                                     const float* __restrict__ u_right,
                                                     float* __restrict__ proj_xr) {
    extern __shared__ uint4 kl[];
    TR_BEGIN()
    const int n = f.n, nt = blockDim.x;
    const int w = threadIdx.x >> 6;
    const int i = w < kListQ ? blockIdx.x * kListQ + w : nq;   // nq: no query
    const int lane = threadIdx.x & 63;
    // LDS (list_lds_bytes): kl[n] | kc[n256] cells (u16, 0xFFFF past n) | per-wave index lists
    const int n256 = (n + 255) & ~255;
    uint16_t* kc = (uint16_t*)(kl + n);
    uint16_t* wl = kc + n256 + min(w, kListQ - 1) * kProjCap;
    uint16_t* wr = kc + n256 + kListQ * kProjCap + min(w, kListQ - 1) * kRectCap;
    Query Q{0, 0, 0, 0, 0, 0};
    uint4 qa{0u, 0u, 0u, 0u}, qb{0u, 0u, 0u, 0u};
    uint8_t iv = 0;
    int lvl = 0;
    float xr = 0.0f;
    if (i < nq) {
        if constexpr (MODE == 0) Q = prep_last(f, pl, i);
        else Q = prep_local(f, pc, i, &iv, &lvl, &xr);
        const uint4* qd4 = (const uint4*)(qdesc + 32 * (size_t)i);
        qa = qd4[0];
        qb = qd4[1];
    }
    // staging: two keypoints per thread with their loads in flight together (1250 keypoints: one
    // round trip); the cell of each keypoint also into kc
    for (int k0 = threadIdx.x; k0 < n; k0 += 2 * nt) {
        orbhip_kp kp[2];
        uint32_t cl[2];
        float kur[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int k = min(k0 + u * nt, n - 1);
            kp[u] = kps[k];
            cl[u] = (claimed && claimed[k]) ? 1u : 0u;
            kur[u] = u_right ? u_right[k] : -1.0f;
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int k = k0 + u * nt;
            if (k >= n) break;
            const int c = grid_cell(f.minx, f.miny, f.invw, f.invh, kp[u].x, kp[u].y, 0xFFFF);
            kl[k] = uint4{__float_as_uint(kp[u].x), __float_as_uint(kp[u].y), ((uint32_t)c << 16) | (cl[u] << 8) |
                          (uint32_t)(kp[u].octave & 0xFF), __float_as_uint(kur[u])};
            kc[k] = (uint16_t)c;
        }
    }
    for (int k = n + threadIdx.x; k < n256; k += nt) kc[k] = 0xFFFF;
    __syncthreads();
    TR_PHASE(7, 1)
    int cnt = 0;
    Top2 t{256, INT_MAX, -1, 256, INT_MAX, -1};
    if (i < nq && Q.valid) {
        const CellRect rect(f, Q);
        const bool any = rect.any;
        uint64_t* out = lists + (size_t)i * cap;
        // pass 1, LDS only: the indices of the keypoints passing the window tests into the wave's
        // slice of the index buffer (the first `cap`; the count goes on). Four keypoints per lane
        // and step: their cells are one 8-byte read, and only the few inside the cell rectangle
        // read their 16-byte record for the level / radius / claimed tests
        const uint64_t* kc8 = (const uint64_t*)kc;
        const uint64_t lt = (1ull << lane) - 1ull;
        TR_PHASE(7, 5)
        // 1a: the cell rectangle alone, four cells per lane from one 8-byte read
        int nr = 0;
        for (int s0 = 0; any && s0 < n; s0 += 256) {
            const uint64_t v = kc8[(s0 >> 2) + lane];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const bool r = rect.contains((int)((v >> (16 * u)) & 0xFFFF));
                const uint64_t m = __ballot(r);
                const int pos = nr + __popcll(m & lt);
                if (r && pos < kRectCap) wr[pos] = (uint16_t)(s0 + 4 * lane + u);
                nr += __popcll(m);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // 1b: the level / radius / claimed tests and the stereo gate on the rectangle's keypoints
        // (every keypoint when the rectangle held more than kRectCap), compacted into wl
        const bool all = nr > kRectCap;
        const int nb = all ? n : nr;
        for (int j0 = 0; any && j0 < nb; j0 += 64) {
            const int j = j0 + lane;
            bool ok = false;
            int k = 0;
            if (j < nb) {
                k = all ? j : (int)wr[j];
                const uint4 e = kl[k];
                const uint32_t oct = e.z & 0xFF;
                const float x = __uint_as_float(e.x), y = __uint_as_float(e.y);
                ok = !all || rect.contains((int)(e.z >> 16));
                if (ok && rect.bCheckLevels) ok = (int)oct >= Q.minL && !(Q.maxL >= 0 && (int)oct > Q.maxL);
                ok = ok && fabsf(x - Q.u) < Q.r && fabsf(y - Q.v) < Q.r && !((e.z >> 8) & 1u) &&
                     !stereo_gate(Q, __uint_as_float(e.w));
            }
            const uint64_t m = __ballot(ok);
            const int pos = cnt + __popcll(m & lt);
            if (ok && pos < cap) wl[pos] = (uint16_t)k;
            cnt += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        TR_PHASE(7, 2)
        // pass 2: the descriptor loads of every listed keypoint in flight at once (one round trip
        // instead of one per 64-keypoint step that had a passing lane)
        const int nl = min(cnt, cap);
        int kk[kProjCap / 64];
        uint4 ka[kProjCap / 64], kb[kProjCap / 64];
#pragma unroll
        for (int u = 0; u < kProjCap / 64; u++) {
            const int j = lane + 64 * u;
            kk[u] = j < nl ? (int)wl[j] : -1;
            if (kk[u] >= 0) {
                const uint4* kd4 = (const uint4*)(kdesc + 32 * (size_t)kk[u]);
                ka[u] = kd4[0];
                kb[u] = kd4[1];
            }
        }
#pragma unroll
        for (int u = 0; u < kProjCap / 64; u++) {
            if (kk[u] < 0) continue;
            const int k = kk[u];
            const uint32_t z = kl[k].z, oct = z & 0xFF, key = ((z >> 16) << 16) | (uint32_t)k;
            const int d = hamming256(qa, qb, ka[u], kb[u]);
            st_ag(out + lane + 64 * u, ((uint64_t)d << 32) | (uint64_t)((key << 4) | (oct & 15u)));
            if (d != 256) top2_add(t, d, (int)key, (int)(oct & 15u));
        }
    }
    top2_wave_merge(t);
    if (lane == 0 && i < nq) {
        st_ag(lcnt + i, cnt);
        st_ag(pick0 + i, proj_decide(t, MODE, nnratio));
    }
    TR_PHASE(7, 3)
    // the in_view / level outputs live in host memory: stored after the arrival's vmcnt drain (and
    // after the resolve in the resolving work-group, whose barriers drain stores), not before it
    auto host_outputs = [&]() {
        if constexpr (MODE == 1)
            if (lane == 0 && i < nq) {
                in_view[i] = iv;
                level[i] = lvl;
                if (proj_xr) proj_xr[i] = xr;
            }
    };
    if (!ra.fuse) { host_outputs(); TR_END(7) return; }   // uniform
    // one launch: every wave's list stores drained, then the last work-group to arrive resolves
    __shared__ int lastf;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int old = __hip_atomic_fetch_add((pj_gint*)ra.arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lastf = old == (int)gridDim.x - 1;
        if (lastf) __hip_atomic_store((pj_gint*)ra.arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    TR_PHASE(7, 4)
    if (lastf)
        resolve_body<MODE>((unsigned char*)kl, n, nq, nnratio, ra.check_orientation, cap, ra.ent_cap, ra.qangle, kps,
                           lists, lcnt, pick0, ra.match, ra.res,
                           tr_buf ? tr_buf + 7 * kTraceStride + 8192 + 16 : nullptr);
    host_outputs();
    TR_END(7)
}

// res[0] = matches, res[1] = status (1: a list overflowed, nothing else written), res[2] = rounds,
// res[3] = the list entries in all (orbhip_test_proj_stats).
// LDS rsm: 3 owner tables (n ints), the list offsets (nq ints), then the lists themselves when
// they fit the rest (`ent_cap` entries; else the rounds read them from global memory). The lists,
// their counts and pick0 are read with agent-scope (sc1) loads: in the one-launch form they were
// written by the other work-groups of the same launch.
template <int MODE>
__device__ void resolve_body(unsigned char* rsm, int n, int nq, float nnratio, int check_orientation, int cap,
                             int ent_cap, const float* __restrict__ qangle, const orbhip_kp* __restrict__ kps,
                             const uint64_t* __restrict__ lists, const int* __restrict__ lcnt,
                             const int* __restrict__ pick0, int* __restrict__ match, int* __restrict__ res,
                             unsigned long long* tr) {
    // tr (diagnostics): s_memtime cycles of the resolve's phases, written by thread 0
    unsigned long long tr_p = tr && threadIdx.x == 0 ? __builtin_amdgcn_s_memtime() : 0ull;
    auto mark = [&](int ph) {
        if (tr && threadIdx.x == 0) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            tr[ph] = t - tr_p;
            tr_p = t;
        }
    };
    int* own = (int*)rsm;                        // 3 x n
    int* qoff = own + 3 * n;                     // nq + 1: list i = entries [qoff[i], qoff[i + 1])
    int* pk = qoff + nq + 1;                     // nq: the current picks
    uint64_t* ent = (uint64_t*)(rsm + resolve_head_bytes(n, nq));
    __shared__ int flag[4], hist[32], keep[3], cnt, scan[16];
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid < 4) flag[tid] = 0;
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) cnt = 0;
    for (int k = tid; k < 3 * n; k += nt) own[k] = INT_MAX;
    // list offsets (block scan of the counts, nt queries at a time)
    int over = 0, run = 0;
    for (int i0 = 0; i0 < nq; i0 += nt) {
        const int i = i0 + tid;
        const int c = i < nq ? ld_ag(lcnt + i) : 0;
        const int p0 = i < nq ? ld_ag(pick0 + i) : 0;
        over |= c > cap;
        int tot;
        const int ex = block_excl_scan(c, scan, &tot);
        if (i < nq) { qoff[i] = run + ex; pk[i] = p0; }
        run += tot;
    }
    if (tid == 0) qoff[nq] = run;
    if (over) flag[3] = 1;
    __syncthreads();
    mark(0);
    if (flag[3]) {
        if (tid == 0) res[1] = 1;
        return;
    }
    const bool in_lds = run <= ent_cap;
    // round 0 was k_proj_lists' (pick0): its claims build own[1]
    for (int i = tid; i < nq; i += nt) {
        const int p = pk[i];
        if (p >= 0) atomicMin(&own[n + p], i);
        if (in_lds) {   // 8 loads in flight before their stores (one round trip per 8 entries)
            const int o = qoff[i], c = qoff[i + 1] - o;
            const uint64_t* L = lists + (size_t)i * cap;
            for (int j0 = 0; j0 < c; j0 += 8) {
                uint64_t v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = j0 + u < c ? ld_ag(L + j0 + u) : 0ull;
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (j0 + u < c) ent[o + j0 + u] = v[u];
            }
        }
    }
    __syncthreads();
    mark(1);
    // round r >= 1: reads own[r % 3], builds own[(r+1) % 3], clears own[(r+2) % 3]; flag[r % 3] =
    // some pick changed, and flag[(r+1) % 3] (last read before round r-1's barrier) is reset here
    int r = 1;
    for (; r < nq + 2; r++) {
        const int* owner = own + (r % 3) * n;
        int* own_next = own + ((r + 1) % 3) * n;
        int* own_clear = own + ((r + 2) % 3) * n;
        for (int k = tid; k < n; k += nt) own_clear[k] = INT_MAX;
        if (tid == 0) flag[(r + 1) % 3] = 0;
        int ch = 0;
        for (int i = tid; i < nq; i += nt) {
            const int o = qoff[i], c = qoff[i + 1] - o;
            const uint64_t* L = in_lds ? ent + o : lists + (size_t)i * cap;
            Top2 t{256, INT_MAX, -1, 256, INT_MAX, -1};
            for (int j = 0; j < c; j++) {
                const uint64_t e = in_lds ? L[j] : ld_ag(L + j);
                const uint32_t lo = (uint32_t)e;
                const int d = (int)(e >> 32);
                if (d == 256 || owner[(lo >> 4) & 0xFFFF] < i) continue;
                top2_add(t, d, (int)(lo >> 4), (int)(lo & 15));
            }
            const int p = proj_decide(t, MODE, nnratio);
            ch |= p != pk[i];
            pk[i] = p;
            if (p >= 0) atomicMin(&own_next[p], i);
        }
        if (ch) flag[r % 3] = 1;
        __syncthreads();
        if (!flag[r % 3]) break;
    }
    mark(2);
    // ---- the rotation filter of SearchByProjection(CurrentFrame, LastFrame), the count ----
    auto bin_of = [&](int i, int k) { return rot_bin(qangle[i], kps[k].angle); };
    const bool rot = MODE == 0 && check_orientation;
    if (rot) {
        for (int i = tid; i < nq; i += nt)
            if (pk[i] >= 0) atomicAdd(&hist[bin_of(i, pk[i])], 1);
        __syncthreads();
        if (tid < 64) three_maxima_wave(hist, keep);   // wave 0 of 1024 threads
        __syncthreads();
        for (int i = tid; i < nq; i += nt)   // each thread rewrites only its own queries
            if (pk[i] >= 0 && !rot_kept(bin_of(i, pk[i]), keep)) pk[i] = -1;
    }
    // the count first, then the stores (match / res may be host memory: no barrier waits on them)
    int c = 0;
    for (int i = tid; i < nq; i += nt) c += pk[i] >= 0;
    c = wave_sum_i32(c);   // one LDS atomic per wave: 1024 same-address atomics serialise
    if ((tid & 63) == 0) atomicAdd(&cnt, c);
    __syncthreads();
    mark(4);
    for (int i = tid; i < nq; i += nt) match[i] = pk[i];
    if (tid == 0) {
        res[0] = cnt;
        res[1] = 0;
        res[2] = r + 1;
        res[3] = run;
    }
    mark(5);
}

template <int MODE>
__global__ __launch_bounds__(1024) void k_proj_resolve(int n, int nq, float nnratio, int check_orientation, int cap,
                                                       int ent_cap, const float* __restrict__ qangle,
                                                       const orbhip_kp* __restrict__ kps,
                                                       const uint64_t* __restrict__ lists,
                                                       const int* __restrict__ lcnt, const int* __restrict__ pick0,
                                                       int* __restrict__ match, int* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm_[];
    resolve_body<MODE>(rsm_, n, nq, nnratio, check_orientation, cap, ent_cap, qangle, kps, lists, lcnt, pick0, match,
                       res);
}

}  // namespace

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
ProjWorkspace* proj_ws_create() { return new ProjWorkspace(); }
void proj_ws_destroy(ProjWorkspace* w) { delete w; }

namespace {

ProjFrame make_frame(const orbhip_frame* F) {
    ProjFrame f{};
    f.n = F->n;
    f.minx = F->min_x; f.maxx = F->max_x; f.miny = F->min_y; f.maxy = F->max_y;
    f.invw = (float)kGridCols / (f.maxx - f.minx);
    f.invh = (float)kGridRows / (f.maxy - f.miny);
    for (int k = 0; k < 4; k++) f.q[k] = F->pose_q[k];
    for (int k = 0; k < 3; k++) f.t[k] = F->pose_t[k];
    f.fx = F->fx; f.fy = F->fy; f.cx = F->cx; f.cy = F->cy;
    // mRcw = q.toRotationMatrix(); mOw = conj(q)._transformVector(-t) (Sophus SE3f::inverse)
    const float* q = f.q;
    quat_to_matrix(q, f.R);
    const float qc[4] = {-q[0], -q[1], -q[2], q[3]};
    const float v[3] = {f.t[0] * -1.0f, f.t[1] * -1.0f, f.t[2] * -1.0f};
    quat_rotate(qc, v, f.Ow);
    return f;
}

// the two-launch form applies: every octave fits the list entry's 4 bits, the owner tables fit LDS
constexpr size_t kResolveLds = 150 * 1024;   // k_proj_resolve's dynamic LDS
// (the sizes and the switch alone: orbhip_test_proj_route asks this with the largest octave given)
bool onepass_sizes_ok(int n, int nq) {
    const char* e = std::getenv("ORBHIP_PROJ_ROUNDS");   // A/B switch (read per call: tests flip it)
    return !((e && e[0] == '1') || n > kProjMaxN || nq > kProjMaxQ || resolve_head_bytes(n, nq) > kResolveLds);
}
bool octave_fits(int octave) { return octave >= 0 && octave <= 15; }
bool onepass_ok(const orbhip_frame* F, int nq) {
    if (!onepass_sizes_ok(F->n, nq)) return false;
    for (int k = 0; k < F->n; k++)
        if (!octave_fits(F->kps[k].octave)) return false;
    return true;
}
// k_proj_lists' LDS: keypoint records, cells (padded to 256), the waves' index lists
size_t list_lds_bytes(int n) { return 16 * (size_t)n + 2 * (size_t)((n + 255) & ~255) + kListIdxBytes; }
static_assert(18 * (size_t)kProjMaxN + kListIdxBytes <= kResolveLds, "k_proj_lists' staging exceeds its LDS");
hipError_t proj_lds_attr() {   // beyond the default 64 KiB of dynamic LDS; per device (dev_attr.h)
    static LdsAttrOnce attr;
    static const void* const fs[] = {(const void*)k_proj_resolve<0>, (const void*)k_proj_resolve<1>,
                                     (const void*)k_proj_lists<0>, (const void*)k_proj_lists<1>};
    return attr.ensure(fs, 4, kResolveLds);
}
// list entries the resolve kernel holds in LDS next to its owner tables and list offsets
int resolve_ent_cap(int n, int nq) {
    const size_t head = resolve_head_bytes(n, nq);
    return head >= kResolveLds ? 0 : (int)((kResolveLds - head) / 8);
}
// one launch (the list kernel's last work-group resolves) unless ORBHIP_PROJ_TWO=1 (read per call)
bool proj_fused() {
    const char* e = std::getenv("ORBHIP_PROJ_TWO");
    return !(e && e[0] == '1');
}
int proj_cap() {
    const char* e = std::getenv("ORBHIP_PROJ_CAP");   // tests shrink it to force the round path
    return e ? std::max(1, std::min(kProjCap, std::atoi(e))) : kProjCap;
}

// outputs in one block (one download): match (nq ints), level (nq ints), in_view (nq bytes), res
struct OutBlock {
    size_t match, lvl, iv, res, bytes;
    explicit OutBlock(int nq) {
        match = 0;
        lvl = 4 * (size_t)nq;
        iv = 8 * (size_t)nq;
        res = (iv + (size_t)nq + 15) & ~size_t(15);
        bytes = res + 16;
    }
};

// What both searches decide from a call's sizes before they lay out their block, and the
// device-only tail of that block behind the caller's uploaded inputs:
//  [cells | owners x 3 | queries | changed flags | picks | outputs (OutBlock) | lists | list counts |
//   first picks]
struct ProjPlan {
    int n, nq;
    bool onepass;   // the list form applies (else the rounds alone)
    int cap;        // list entries per query
    OutBlock ob;
    size_t o_cell = 0, o_own = 0, o_q = 0, o_chg = 0, o_pick = 0, o_out = 0, o_list = 0, o_lcnt = 0, o_pick0 = 0;
    ProjPlan(const orbhip_frame* F, int nq_) : n(F->n), nq(nq_), onepass(onepass_ok(F, nq_)), cap(proj_cap()), ob(nq_) {}
    void take_tail(StageLayout& lay) {
        o_cell = lay.take(4 * (size_t)n);
        o_own = lay.take(12 * (size_t)std::max(n, 1));
        o_q = lay.take(sizeof(Query) * nq);
        o_chg = lay.take(4 * ((size_t)nq + 2));
        o_pick = lay.take(4 * (size_t)nq);
        o_out = lay.take(ob.bytes);
        o_list = onepass ? lay.take(8 * (size_t)nq * cap) : 0;
        o_lcnt = lay.take(4 * (size_t)nq);
        o_pick0 = lay.take(4 * (size_t)nq);
    }
};

// One search as its caller staged it: where the kernels find the uploaded inputs, and the
// arguments of the call's mode (0: LastFrame, 1: local points; the other mode's stay empty)
struct ProjCall {
    ProjFrame f;
    size_t o_kps, o_kd, o_qd;
    const uint8_t* dcl;     // the frame's claimed flags on the device, or null
    const float* dur;       // mvuRight on the device (null: no stereo gate)
    PrepLast pl{};
    PrepLocal pc{};
    float nnratio = 0.f;
    int check_orientation = 0;
    const float* qangle = nullptr;   // the queries' angles on the device (mode 0)
    bool want_xr = false;            // mode 1: mTrackProjXR wanted, o_xr its nq floats
    size_t o_xr = 0;
};

// The fixed-point rounds, launched `ws->ahead` at a time with the finishing work (`tail`: the
// finish kernel and the result downloads) behind them and ONE host sync per batch: rounds after
// convergence exit on the device, so the common case is a single round trip. Returns the number
// of rounds that did work (< 0 on error).
template <typename Tail>
int run_rounds(ProjWorkspace* ws, const ProjPlan& p, const ProjCall& c, int mode, hipStream_t st, Tail&& tail) {
    char* D = (char*)ws->s.d;
    char* H = (char*)ws->s.h;
    const int nq = p.nq;
    const dim3 gq((unsigned)std::max(1, (nq + 3) / 4));
    const int cap = nq + 2;   // a fixed point is reached within nq + 1 rounds
    int* chg = (int*)(D + p.o_chg);
    const int* hchg = (const int*)(H + p.o_chg);
    HIPOK(hipMemsetAsync(D + p.o_own, 0x7F, 3 * sizeof(int) * (size_t)std::max(p.n, 1), st));   // > any query
    HIPOK(hipMemsetAsync(chg, 0, sizeof(int) * (size_t)cap, st));
    int r = 0;
    for (;;) {
        const int R = std::min(ws->ahead, cap - r);
        for (int j = 0; j < R; j++)
            hipLaunchKernelGGL(k_proj_round, gq, dim3(256), 0, st, c.f, nq, mode, c.nnratio, r + j,
                               (const Query*)(D + p.o_q), (const orbhip_kp*)(D + c.o_kps),
                               (const uint8_t*)(D + c.o_kd), (const int*)(D + p.o_cell), c.dcl, (int*)(D + p.o_own),
                               (const uint8_t*)(D + c.o_qd), (int*)(D + p.o_pick), chg, c.dur);
        HIPOK(hipGetLastError());
        if (int rc = tail()) return rc;
        HIPOK(hipMemcpyAsync(H + p.o_chg + sizeof(int) * r, chg + r, sizeof(int) * R, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        for (int j = 0; j < R; j++)
            if (hchg[r + j] == 0) {
                const int rounds = r + j + 1;
                ws->ahead = std::min(16, std::max(2, rounds + 1));
                return rounds;
            }
        r += R;
        if (r >= cap) return r;
        ws->ahead = std::min(16, 2 * ws->ahead);
    }
}

// The search itself, with the inputs uploaded: the list form (one launch, or two), and when it does
// not apply or a list overflowed (status word) the rounds, which find the inputs on the device.
// (proj_stats_reset and proj_begin first: the last search's statistics start empty, the kernels may use their LDS.)
// Either way the outputs end in the pinned image (OutBlock at o_out, mTrackProjXR at o_xr) for the
// caller to copy out. Returns the number of matches (< 0 on error).
void proj_stats_reset(ProjWorkspace* ws) {
    ws->st_form = -1;
    ws->st_rounds = ws->st_entries = ws->st_ent_cap = 0;
}
int proj_begin(const ProjPlan& p) {
    if (p.onepass) HIPOK(proj_lds_attr());
    return ORBHIP_OK;
}
template <int MODE>
int proj_search(ProjWorkspace* ws, const ProjPlan& p, const ProjCall& c, int* rounds_out, hipStream_t st) {
    char* H = (char*)ws->s.h;
    char* HD = (char*)ws->s.hd;   // the list form writes its results straight into H
    char* D = (char*)ws->s.d;
    const int n = p.n, nq = p.nq;
    const OutBlock& ob = p.ob;
    const orbhip_kp* dkps = (const orbhip_kp*)(D + c.o_kps);
    const int* hres = (const int*)(H + p.o_out + ob.res);
    if (p.onepass) {
        const bool fused = proj_fused();
        const ResolveArgs ra{fused ? 1 : 0, c.check_orientation, resolve_ent_cap(n, nq), c.qangle,
                             (int*)(HD + p.o_out + ob.match), (int*)(HD + p.o_out + ob.res), ws->arrive};
        hipLaunchKernelGGL(k_proj_lists<MODE>, dim3((unsigned)((nq + kListQ - 1) / kListQ)), dim3(1024),
                           fused ? kResolveLds : list_lds_bytes(n), st, c.f, nq, c.pl, c.pc, p.cap, c.nnratio, dkps,
                           (const uint8_t*)(D + c.o_kd), c.dcl, (const uint8_t*)(D + c.o_qd),
                           (uint64_t*)(D + p.o_list), (int*)(D + p.o_lcnt), (int*)(D + p.o_pick0),
                           MODE == 1 ? (uint8_t*)(HD + p.o_out + ob.iv) : nullptr,
                           MODE == 1 ? (int*)(HD + p.o_out + ob.lvl) : nullptr, ra, c.dur,
                           c.want_xr ? (float*)(HD + c.o_xr) : nullptr);
        if (!fused)
            hipLaunchKernelGGL(k_proj_resolve<MODE>, dim3(1), dim3(1024), kResolveLds, st, n, nq, c.nnratio,
                               c.check_orientation, p.cap, ra.ent_cap, ra.qangle, dkps,
                               (const uint64_t*)(D + p.o_list), (const int*)(D + p.o_lcnt),
                               (const int*)(D + p.o_pick0), ra.match, ra.res);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(st));
        ws->st_ent_cap = ra.ent_cap;
        if (hres[1] == 0) {
            if (rounds_out) *rounds_out = hres[2];
            ws->st_form = 0; ws->st_rounds = hres[2]; ws->st_entries = hres[3];
            return hres[0];
        }
    }
    HIPOK(hipMemsetAsync(D + p.o_pick, 0xFF, 4 * (size_t)nq, st));   // -1: the first round always "changes"
    if (n) hipLaunchKernelGGL(k_proj_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c.f, dkps,
                              (int*)(D + p.o_cell));
    if constexpr (MODE == 0)
        hipLaunchKernelGGL(k_proj_prep_last, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, c.f, nq, c.pl,
                           (Query*)(D + p.o_q));
    else
        hipLaunchKernelGGL(k_proj_prep_local, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, c.f, nq, c.pc,
                           (Query*)(D + p.o_q), (uint8_t*)(D + p.o_out + ob.iv), (int*)(D + p.o_out + ob.lvl),
                           c.want_xr ? (float*)(D + c.o_xr) : nullptr);
    auto tail = [&]() -> int {
        hipLaunchKernelGGL(k_proj_finish, dim3(1), dim3(1024), 0, st, nq, c.check_orientation, c.qangle, dkps,
                           (const int*)(D + p.o_pick), (int*)(D + p.o_out + ob.match), (int*)(D + p.o_out + ob.res));
        HIPOK(hipMemcpyAsync(H + p.o_out, D + p.o_out, ob.bytes, hipMemcpyDeviceToHost, st));
        if (c.want_xr) HIPOK(hipMemcpyAsync(H + c.o_xr, D + c.o_xr, 4 * (size_t)nq, hipMemcpyDeviceToHost, st));
        return 0;
    };
    const int rounds = run_rounds(ws, p, c, MODE, st, tail);
    if (rounds < 0) return rounds;
    if (rounds_out) *rounds_out = rounds;
    ws->st_form = p.onepass ? 1 : 2; ws->st_rounds = rounds;
    return hres[0];
}

}  // namespace

// orbhip_test_proj_route: the decisions both searches take from a call's sizes, from the functions
// they call. out4 = {list form applies, ent_cap, list capacity, one launch}
int proj_test_route(int n, int nq, int max_octave, int32_t* out4) {
    if (!out4 || n < 0 || nq < 0 || n > 65535 || max_octave < 0) return ORBHIP_ERR_ARG;
    out4[0] = onepass_sizes_ok(n, nq) && octave_fits(max_octave) ? 1 : 0;
    out4[1] = resolve_ent_cap(n, nq);
    out4[2] = proj_cap();
    out4[3] = proj_fused() ? 1 : 0;
    return ORBHIP_OK;
}
// orbhip_test_proj_stats: the last projection search on this workspace (ProjWorkspace::st_*)
int proj_test_stats(const ProjWorkspace* ws, int32_t* out4) {
    if (!out4) return ORBHIP_ERR_ARG;
    out4[0] = ws ? ws->st_form : -1;
    out4[1] = ws ? ws->st_rounds : 0;
    out4[2] = ws ? ws->st_entries : 0;
    out4[3] = ws ? ws->st_ent_cap : 0;
    return ORBHIP_OK;
}

namespace {
// predict_scale over the floats of bit patterns [lo, hi] against the host's levels
__global__ void k_predict_scale_sweep(uint32_t lo, uint32_t hi, LevelSteps steps, const float* __restrict__ thr,
                                      int n_levels, const int8_t* __restrict__ ref, unsigned long long* mism) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > hi - lo) return;
    if (predict_scale(__uint_as_float(lo + i), steps, thr, n_levels) != (int)ref[i]) atomicAdd(mism, 1ull);
}
}  // namespace
void launch_predict_scale_sweep(uint32_t lo_bits, uint32_t hi_bits, float log_sf, const float* thr, int n_levels,
                                const int8_t* ref, unsigned long long* mismatches, hipStream_t st) {
    const uint64_t n = (uint64_t)hi_bits - lo_bits + 1;
    hipLaunchKernelGGL(k_predict_scale_sweep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, lo_bits, hi_bits,
                       level_steps(log_sf, n_levels), thr, n_levels, ref, mismatches);
}

// twc = -Rcw^T tcw, tlc = Rlw twc + tlw (float, in the order written); forward: tlc.z > b,
// backward: -tlc.z > b. Decided on the host and passed to the kernels as a uniform.
int proj_direction(const float cur_q[4], const float cur_t[3], const float last_q[4], const float last_t[3], float b) {
    float Rc[9], Rl[9];
    quat_to_matrix(cur_q, Rc);
    quat_to_matrix(last_q, Rl);
    float twc[3];
    for (int j = 0; j < 3; j++) twc[j] = -(Rc[j] * cur_t[0] + Rc[3 + j] * cur_t[1] + Rc[6 + j] * cur_t[2]);
    const float tlcz = Rl[6] * twc[0] + Rl[7] * twc[1] + Rl[8] * twc[2] + last_t[2];
    return tlcz > b ? 1 : (-tlcz > b ? -1 : 0);
}

int proj_search_last(ProjWorkspace* ws, const orbhip_frame* F, const orbhip_proj_last* L, float th,
                     int check_orientation, int32_t* match, int* rounds_out, hipStream_t st, const ProjStereo* sx) {
    if (!ws || !F || !L || !match || F->n < 0 || L->n < 0 || F->n > 65535 || !F->scale_factors ||
        (F->n && (!F->kps || !F->desc)) || (L->n && (!L->points || !L->desc || !L->octave || !L->angle)))
        return ORBHIP_ERR_ARG;
    if (sx && ((F->n && !sx->u_right) || !(sx->bf > 0.0f))) return ORBHIP_ERR_ARG;
    for (int i = 0; i < L->n; i++)
        if (L->octave[i] < 0 || L->octave[i] >= F->n_levels) return ORBHIP_ERR_ARG;
    const int n = F->n, nq = L->n;
    proj_stats_reset(ws);
    if (nq == 0) return 0;
    ProjPlan p(F, nq);
    if (int rc = proj_begin(p)) return rc;
    // uploaded: [keypoints | descriptors | claimed | scale factors | points | point descriptors |
    //  octaves | angles | mvuRight], then the device-only tail
    StageLayout lay(256);
    const size_t o_kps = lay.take(sizeof(orbhip_kp) * n), o_kd = lay.take(32 * (size_t)n), o_cl = lay.take(n);
    const size_t o_scale = lay.take(sizeof(float) * F->n_levels);
    const size_t o_pts = lay.take(12 * (size_t)nq), o_qd = lay.take(32 * (size_t)nq), o_oct = lay.take(4 * (size_t)nq);
    const size_t o_ang = lay.take(4 * (size_t)nq), o_ur = lay.take(sx ? 4 * (size_t)n : 0), o_in_end = lay.total();
    p.take_tail(lay);
    if (int rc = proj_ws_ensure(ws, lay.total())) return rc;
    StageBlock& S = ws->s;
    char* D = (char*)S.d;
    put_keyframe(S, o_kps, o_kd, 0, F->kps, F->desc, n);
    if (F->claimed) S.put(o_cl, F->claimed, n);
    S.put(o_scale, F->scale_factors, sizeof(float) * F->n_levels);
    S.put(o_pts, L->points, 12 * (size_t)nq);
    S.put(o_qd, L->desc, 32 * (size_t)nq);
    S.put(o_oct, L->octave, 4 * (size_t)nq);
    S.put(o_ang, L->angle, 4 * (size_t)nq);
    if (sx) S.put(o_ur, sx->u_right, 4 * (size_t)n);
    HIPOK(upload_inputs(S.hd, D, (char*)S.h, o_in_end, st));
    ProjCall c{make_frame(F), o_kps, o_kd, o_qd, F->claimed ? (const uint8_t*)(D + o_cl) : nullptr,
               sx ? (const float*)(D + o_ur) : nullptr};
    if (sx) c.f.bf = sx->bf;
    c.pl = PrepLast{(const float*)(D + o_pts), (const int*)(D + o_oct), (const float*)(D + o_scale), th,
                    sx ? sx->dir : 0};
    c.check_orientation = check_orientation;
    c.qangle = (const float*)(D + o_ang);
    const int nmatches = proj_search<0>(ws, p, c, rounds_out, st);
    if (nmatches < 0) return nmatches;
    std::memcpy(match, S.h + p.o_out + p.ob.match, 4 * (size_t)nq);
    return nmatches;
}

int proj_search_local(ProjWorkspace* ws, const orbhip_frame* F, const orbhip_local_points* M, float view_cos_limit,
                      float th, float nnratio, int far_points, float th_far, uint8_t* in_view, int32_t* level,
                      int32_t* match, int* rounds_out, hipStream_t st, const ProjStereo* sx) {
    if (!ws || !F || !M || !match || !in_view || !level || F->n < 0 || M->n < 0 || F->n > 65535 ||
        !F->scale_factors || (F->n && (!F->kps || !F->desc)) ||
        (M->n && (!M->points || !M->normals || !M->min_dist || !M->max_dist || !M->desc)))
        return ORBHIP_ERR_ARG;
    if (sx && ((F->n && !sx->u_right) || !(sx->bf > 0.0f))) return ORBHIP_ERR_ARG;
    const int n = F->n, nq = M->n;
    proj_stats_reset(ws);
    if (nq == 0) return 0;
    ProjPlan p(F, nq);
    if (int rc = proj_begin(p)) return rc;
    // uploaded: [keypoints | descriptors | claimed | scale factors, level steps | points normals min max
    //  desc skip | mvuRight], then the device-only tail and mTrackProjXR (an output of its own)
    StageLayout lay(256);
    const size_t o_kps = lay.take(sizeof(orbhip_kp) * n), o_kd = lay.take(32 * (size_t)n), o_cl = lay.take(n);
    const size_t o_scale = lay.take(sizeof(float) * 2 * F->n_levels);   // + PredictScale's steps
    const PointsLayout o_mp(lay, (size_t)nq);
    const size_t o_ur = lay.take(sx ? 4 * (size_t)n : 0), o_in_end = lay.total();
    p.take_tail(lay);
    const bool want_xr = sx && sx->proj_xr;
    const size_t o_xr = lay.take(want_xr ? 4 * (size_t)nq : 0);
    if (int rc = proj_ws_ensure(ws, lay.total())) return rc;
    StageBlock& S = ws->s;
    char* D = (char*)S.d;
    put_keyframe(S, o_kps, o_kd, 0, F->kps, F->desc, n);
    if (F->claimed) S.put(o_cl, F->claimed, n);
    S.put(o_scale, F->scale_factors, sizeof(float) * F->n_levels);
    S.put(o_scale + sizeof(float) * F->n_levels, level_thresholds(F->log_scale_factor, F->n_levels),
          sizeof(float) * F->n_levels);
    const DevPoints mp = o_mp.put(S, *M, false);   // no skip array: a null pointer
    if (sx) S.put(o_ur, sx->u_right, 4 * (size_t)n);
    HIPOK(upload_inputs(S.hd, D, (char*)S.h, o_in_end, st));
    ProjCall c{make_frame(F), o_kps, o_kd, o_mp.desc, F->claimed ? (const uint8_t*)(D + o_cl) : nullptr,
               sx ? (const float*)(D + o_ur) : nullptr};
    if (sx) c.f.bf = sx->bf;
    c.pc = PrepLocal{mp.pts, mp.nrm, mp.mind, mp.maxd, mp.skip, (const float*)(D + o_scale), F->n_levels,
                     view_cos_limit, th, far_points, th_far, level_steps(F->log_scale_factor, F->n_levels)};
    c.nnratio = nnratio;
    c.want_xr = want_xr;
    c.o_xr = o_xr;
    const int nmatches = proj_search<1>(ws, p, c, rounds_out, st);
    if (nmatches < 0) return nmatches;
    const uint8_t* H = S.h + p.o_out;
    std::memcpy(match, H + p.ob.match, 4 * (size_t)nq);
    std::memcpy(level, H + p.ob.lvl, 4 * (size_t)nq);
    std::memcpy(in_view, H + p.ob.iv, nq);
    if (want_xr) {   // only where in view: the rest of the caller's array stays as it was
        const float* hx = (const float*)(S.h + o_xr);
        for (int m = 0; m < nq; m++)
            if (in_view[m]) sx->proj_xr[m] = hx[m];
    }
    return nmatches;
}

}  // namespace orbhip
