// gfx950 ORBmatcher::SearchForTriangulation (LocalMapping::CreateNewMapPoints), one keyframe
// against B covisible neighbours in one launch (DESIGN.md "SearchForTriangulation"):
//   tri_geometry      host, fp32, fixed operation order: F12 and the epipole of a pair
//   k_tri_order       pre-pass, once for all pairs: KF1's FeatureVector entries without a MapPoint
//                     as keys (node << 16 | idx), rank-sorted; every 256-thread work-group compacts
//                     the keys into LDS and ranks its own 256 of them
//   k_tri_search      one 1024-thread work-group per neighbour. The neighbour's unclaimed
//                     FeatureVector entries are dealt into per-node buckets in LDS (a binary search
//                     of the node among KF1's sorted nodes, an LDS counter per node, one scan);
//                     KF1's sorted features are dealt to lanes, so neighbouring lanes share a node
//                     and their KF2 descriptor / keypoint reads hit the same lines. Each lane walks
//                     its node's bucket with the reference's gates (distance, epipole, epipolar
//                     line). No gate depends on the running state, so the walk's result is the
//                     accepted candidate of least distance, the largest index among equals, whatever
//                     the order inside a bucket. Nothing is sequential across KF1 features
//                     (vbMatched2 is never set upstream): only the rotation histogram and the count
//                     are per-pair reductions.
//   k_tri_points, k_tri_claim   the triangulation of the matches and the list of new points
//                     (CreateNewMapPoints; the second half of this file)
// LDS of k_tri_search: 3 x 8 KiB (KF1 nodes, bucket counts, bucket starts) + 4 KiB bucket entries +
// 4 KiB matches + 2 KiB bins + counters = 34.2 KiB static (k_tri_order: 16 KiB), below the 64 KiB a
// kernel gets without the dynamic-LDS attribute (160 KiB per CU).
#include <hip/hip_runtime.h>

#include <vector>

#include "geom.h"
#include "jacobi4.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "rot_filter.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" triangulation", x)

namespace orbhip {

constexpr int kTriMax = 2048;     // features per keyframe (LDS-resident keys, 16-bit indices)
struct TriSide {                  // one keyframe in the call's staging block (device pointers)
    const orbhip_kp* kps;
    const uint8_t* desc;          // n x 32
    const int32_t* node;
    const double* weight;
    const uint8_t* has_mp;
    int n, pad;                   // pad: stereo calls, where this keyframe's [mvuRight n | mvDepth n] starts in sx
};
struct TriGeom { float F[9]; float ep[2]; float pad; };   // F12 row-major, epipole in image 2

// ---- host: per-pair geometry (all fp32, every operation in the order written; no FMA) ----
void tri_geometry(const orbhip_tri_keyframe& k1, const orbhip_tri_keyframe& k2, float* F, float* ep) {
    float R1[9], R2[9], R12[9], t12[3], Cw[3], C2[3], E[9], G[9];
    quat_to_matrix(k1.pose_q, R1);
    quat_to_matrix(k2.pose_q, R2);
    const float* t1 = k1.pose_t;
    const float* t2 = k2.pose_t;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)   // R12 = R1w R2w^T
            R12[3 * i + j] = (R1[3 * i] * R2[3 * j] + R1[3 * i + 1] * R2[3 * j + 1]) + R1[3 * i + 2] * R2[3 * j + 2];
    for (int i = 0; i < 3; i++)
        t12[i] = t1[i] - ((R12[3 * i] * t2[0] + R12[3 * i + 1] * t2[1]) + R12[3 * i + 2] * t2[2]);
    for (int i = 0; i < 3; i++) Cw[i] = -((R1[i] * t1[0] + R1[3 + i] * t1[1]) + R1[6 + i] * t1[2]);
    for (int i = 0; i < 3; i++) C2[i] = ((R2[3 * i] * Cw[0] + R2[3 * i + 1] * Cw[1]) + R2[3 * i + 2] * Cw[2]) + t2[i];
    ep[0] = (k2.fx * C2[0]) / C2[2] + k2.cx;
    ep[1] = (k2.fy * C2[1]) / C2[2] + k2.cy;
    for (int j = 0; j < 3; j++) {   // E = [t12]x R12
        E[j] = t12[1] * R12[6 + j] - t12[2] * R12[3 + j];
        E[3 + j] = t12[2] * R12[j] - t12[0] * R12[6 + j];
        E[6 + j] = t12[0] * R12[3 + j] - t12[1] * R12[j];
    }
    // closed-form inverses: K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1]
    const float ifx1 = 1.0f / k1.fx, ify1 = 1.0f / k1.fy, mcx1 = (-k1.cx) / k1.fx, mcy1 = (-k1.cy) / k1.fy;
    const float ifx2 = 1.0f / k2.fx, ify2 = 1.0f / k2.fy, mcx2 = (-k2.cx) / k2.fx, mcy2 = (-k2.cy) / k2.fy;
    for (int j = 0; j < 3; j++) {   // G = K1^-T E
        G[j] = ifx1 * E[j];
        G[3 + j] = ify1 * E[3 + j];
        G[6 + j] = (mcx1 * E[j] + mcy1 * E[3 + j]) + E[6 + j];
    }
    for (int i = 0; i < 3; i++) {   // F12 = G K2^-1
        F[3 * i] = G[3 * i] * ifx2;
        F[3 * i + 1] = G[3 * i + 1] * ify2;
        F[3 * i + 2] = (G[3 * i] * mcx2 + G[3 * i + 1] * mcy2) + G[3 * i + 2];
    }
}

// ---- device ----
constexpr int kTriOrderThreads = 256;
struct TriOrderLds {
    unsigned long long raw[kTriMax];
    int scan[kTriOrderThreads / 64 + 1];
    int cnt;
};

__global__ __launch_bounds__(kTriOrderThreads) void k_tri_order(const TriSide* __restrict__ sides,
                                                                unsigned long long* __restrict__ keys1,
                                                                int32_t* __restrict__ m1_out) {
    __shared__ TriOrderLds L;
    const TriSide s = sides[0];
    const int tid = threadIdx.x;
    if (tid == 0) L.cnt = 0;
    __syncthreads();
    for (int i0 = 0; i0 < s.n; i0 += blockDim.x) {
        const int i = i0 + tid;
        const bool in = i < s.n && s.node[i] >= 0 && s.weight[i] > 0.0 && !s.has_mp[i];
        int tot;
        const int pos = block_excl_scan(in ? 1 : 0, L.scan, &tot);
        if (in) L.raw[L.cnt + pos] = ((unsigned long long)s.node[i] << 16) | (unsigned)i;
        __syncthreads();
        if (tid == 0) L.cnt += tot;
        __syncthreads();
    }
    const int m = L.cnt;
    if (blockIdx.x == 0 && tid == 0) *m1_out = m;
    const int i = blockIdx.x * blockDim.x + tid;
    if (i < m) {   // keys are distinct: the rank is the position
        const unsigned long long x = L.raw[i];
        int r = 0;
        for (int j = 0; j < m; j++) r += L.raw[j] < x ? 1 : 0;
        keys1[r] = x;
    }
}

constexpr int kTriThreads = 1024;
static_assert(kTriMax == 2 * kTriThreads, "k_tri_search keeps two neighbour features per thread");
struct TriLds {
    int node1[kTriMax];              // nodes of KF1's sorted keys
    int cnt[kTriMax];                // bucket p = the first position of a node in node1: its candidates
    int start[kTriMax];              // exclusive scan of cnt
    unsigned short bucket[kTriMax];  // neighbour feature indices, bucket by bucket
    short match[kTriMax];            // by KF1 index
    int8_t bin[kTriMax];
    int scan[kTriThreads / 64 + 1];
    int hist[32];
    int keep[3];
    int total;
};

// first position in the ascending a[0, m) that is not below v
__device__ __forceinline__ int tri_lower_bound(const int* a, int m, int v) {
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// STEREO: sx holds every keyframe's [mvuRight | mvDepth] (TriSide::pad); the epipole exclusion then
// applies only when neither feature is stereo (mvuRight >= 0)
template <bool STEREO>
__global__ __launch_bounds__(kTriThreads) void k_tri_search(const TriSide* __restrict__ sides,
                                                            const TriGeom* __restrict__ geom,
                                                            const float* __restrict__ scale_factors,
                                                            const float* __restrict__ level_sigma2,
                                                            const unsigned long long* __restrict__ keys1,
                                                            const int32_t* __restrict__ m1_in, int check_orientation,
                                                            int32_t* __restrict__ match12,
                                                            int32_t* __restrict__ nmatches,
                                                            const float* __restrict__ sx) {
    __shared__ TriLds S;
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const TriSide A = sides[0], N = sides[1 + b];
    const int n1 = A.n, m1 = *m1_in;
    if (tid < 32) S.hist[tid] = 0;
    if (tid == 0) S.total = 0;
    for (int i = tid; i < n1; i += kTriThreads) { S.match[i] = -1; S.bin[i] = 127; }
    for (int t = tid; t < m1; t += kTriThreads) { S.node1[t] = (int)(keys1[t] >> 16); S.cnt[t] = 0; }
    __syncthreads();
    // ---- 1. the neighbour's unclaimed FeatureVector entries, counted into KF1's node buckets ----
    int bs[2], bp[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int i = tid + r * kTriThreads;
        bs[r] = -1; bp[r] = 0;
        if (i < N.n && N.node[i] >= 0 && N.weight[i] > 0.0 && !N.has_mp[i]) {
            const int nd = N.node[i];
            const int p = tri_lower_bound(S.node1, m1, nd);
            if (p < m1 && S.node1[p] == nd) { bs[r] = p; bp[r] = atomicAdd(&S.cnt[p], 1); }
        }
    }
    __syncthreads();
    int carry = 0;
    for (int t0 = 0; t0 < m1; t0 += kTriThreads) {
        const int t = t0 + tid;
        int tot;
        const int pos = block_excl_scan(t < m1 ? S.cnt[t] : 0, S.scan, &tot);
        if (t < m1) S.start[t] = carry + pos;
        carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; r++)
        if (bs[r] >= 0) S.bucket[S.start[bs[r]] + bp[r]] = (unsigned short)(tid + r * kTriThreads);
    __syncthreads();
    // ---- 2. lane = a KF1 feature in (node, index) order: the walk over its node's bucket ----
    const TriGeom g = geom[b];
    const float* F = g.F;
    const float ex = g.ep[0], ey = g.ep[1];
    const int kThLow = 50;
    for (int t = tid; t < m1; t += kTriThreads) {
        const int p = tri_lower_bound(S.node1, m1, S.node1[t]);
        const int c0 = S.start[p], c1 = c0 + S.cnt[p];
        if (c0 == c1) continue;
        const int idx1 = (int)(keys1[t] & 0xFFFF);
        const uint4* d1 = (const uint4*)(A.desc + (int64_t)idx1 * 32);
        const uint4 da = d1[0], db = d1[1];
        const orbhip_kp kp1 = A.kps[idx1];
        const float x1 = kp1.x, y1 = kp1.y;
        const float la = (x1 * F[0] + y1 * F[3]) + F[6];
        const float lb = (x1 * F[1] + y1 * F[4]) + F[7];
        const float lc = (x1 * F[2] + y1 * F[5]) + F[8];
        const float den = la * la + lb * lb;
        const bool stereo1 = STEREO && sx[A.pad + idx1] >= 0.0f;
        // (distance, -index): the least key is the reference's result in any visiting order
        int bestDist = kThLow, bestKey = 0x7fffffff;
        // four candidates' descriptors in flight at once (the loads of one candidate after the
        // other are a chain of L2 latencies); few pass the distance gates and read a keypoint
        for (int c = c0; c < c1; c += 4) {
            int idx2v[4], distv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {   // past the bucket's end: its last entry again, not used below
                idx2v[k] = S.bucket[min(c + k, c1 - 1)];
                const uint4* d2 = (const uint4*)(N.desc + (int64_t)idx2v[k] * 32);
                distv[k] = hamming256(da, db, d2[0], d2[1]);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int idx2 = idx2v[k], dist = distv[k];
                if (c + k >= c1 || dist > kThLow || dist > bestDist) continue;
                const orbhip_kp kp2 = N.kps[idx2];
                const float dex = ex - kp2.x, dey = ey - kp2.y;
                const bool either = STEREO && (stereo1 || sx[N.pad + idx2] >= 0.0f);
                if (!either && dex * dex + dey * dey < 100.0f * scale_factors[kp2.octave]) continue;
                const float num = (la * kp2.x + lb * kp2.y) + lc;
                if (den == 0.0f) continue;
                const float dsqr = (num * num) / den;
                if (!((double)dsqr < 3.84 * (double)level_sigma2[kp2.octave])) continue;
                const int key = (dist << 16) | (0xFFFF - idx2);
                if (key < bestKey) { bestKey = key; bestDist = dist; }
            }
        }
        if (bestKey != 0x7fffffff) {
            const int bestIdx2 = 0xFFFF - (bestKey & 0xFFFF);
            S.match[idx1] = (short)bestIdx2;
            if (check_orientation) {
                const int bin = rot_bin(kp1.angle, N.kps[bestIdx2].angle);
                if ((unsigned)bin < (unsigned)kHistoLength) { atomicAdd(&S.hist[bin], 1); S.bin[idx1] = (int8_t)bin; }
            }
        }
    }
    __syncthreads();
    // ---- 3. rotation consistency: ComputeThreeMaxima over the 30 bins (as k_search_bow) ----
    if (check_orientation && tid < 64) three_maxima_wave(S.hist, S.keep);   // wave 0 of kTriThreads
    __syncthreads();
    int c = 0;
    int32_t* out = match12 + (int64_t)b * n1;
    for (int i = tid; i < n1; i += kTriThreads) {
        int m = S.match[i];
        if (m >= 0 && check_orientation) {
            const int bin = S.bin[i];
            if (!rot_kept(bin, S.keep)) m = -1;
        }
        out[i] = m;
        c += m >= 0;
    }
    c = wave_sum_i32(c);
    if (lane == 0 && c) atomicAdd(&S.total, c);
    __syncthreads();
    if (tid == 0) nmatches[b] = S.total;
}

// ---- host ----
// sides[0] = KF1, sides[1 + b] = neighbour b; keys1: kTriMax entries, m1: 1 (both written by the pre-pass)
static void launch_tri_search(const TriSide* sides, const TriGeom* geom, int n1, int B, const float* scale_factors,
                              const float* level_sigma2, unsigned long long* keys1, int32_t* m1,
                              int check_orientation, int32_t* match12, int32_t* nmatches, hipStream_t st,
                              const float* sx = nullptr) {
    const unsigned order_wgs = (unsigned)((n1 + kTriOrderThreads - 1) / kTriOrderThreads);
    ORBHIP_LAUNCH(k_tri_order, dim3(order_wgs), dim3(kTriOrderThreads), 0, st, sides, keys1, m1);
    if (sx)
        ORBHIP_LAUNCH(k_tri_search<true>, dim3((unsigned)B), dim3(kTriThreads), 0, st, sides, geom, scale_factors,
                      level_sigma2, (const unsigned long long*)keys1, (const int32_t*)m1, check_orientation, match12,
                      nmatches, sx);
    else
        ORBHIP_LAUNCH(k_tri_search<false>, dim3((unsigned)B), dim3(kTriThreads), 0, st, sides, geom, scale_factors,
                      level_sigma2, (const unsigned long long*)keys1, (const int32_t*)m1, check_orientation, match12,
                      nmatches, (const float*)nullptr);
}

// The stereo arrays of a call in its staging block: one segment of [mvuRight n | mvDepth n] per
// keyframe of `ks` in order (TriSide::pad = where a keyframe's part starts, in floats), and (mbf, mb)
// per keyframe. ks[0] = KF1.
static size_t tri_stereo_floats(const orbhip_tri_keyframe* const* ks, int count) {
    size_t n = 0;
    for (int s = 0; s < count; s++) n += 2 * (size_t)ks[s]->n;
    return n;
}
static void tri_put_stereo(StageBlock& S, size_t o_sx, size_t o_sb, const TriStereo& x, const int* which, int count,
                           TriSide* sides) {
    size_t at = 0;
    float* sb = (float*)(S.h + o_sb);
    for (int s = 0; s < count; s++) {
        const int k = which[s];
        const size_t n = (size_t)sides[s].n;
        sides[s].pad = (int)at;
        if (n) {
            S.put(o_sx + at * 4, x.u_right[k], n * 4);
            S.put(o_sx + (at + n) * 4, x.depth[k], n * 4);
        }
        at += 2 * n;
        sb[2 * s] = x.bf[k];
        sb[2 * s + 1] = x.b[k];
    }
}

static int tri_check_side(const orbhip_tri_keyframe& k, int n_levels) {
    if (k.n < 0) return ORBHIP_ERR_ARG;
    if (k.n > kTriMax) return ORBHIP_ERR_UNSUPPORTED;
    if (k.n == 0) return ORBHIP_OK;
    if (!k.kps || !k.desc || !k.node || !k.weight || !k.has_mp) return ORBHIP_ERR_ARG;
    for (int i = 0; i < k.n; i++)
        if (k.kps[i].octave < 0 || k.kps[i].octave >= n_levels) return ORBHIP_ERR_ARG;
    return ORBHIP_OK;
}

// A keyframe's segments in the staging block: the keypoints, and for the search (full) its
// descriptors, FeatureVector and MapPoint flags; tri_put_side copies them in and returns the
// device's view of them.
struct TriSideOff { size_t kps, desc, node, weight, mp; };
static TriSideOff tri_take_side(StageLayout& lay, size_t n, bool full) {
    TriSideOff o{lay.take(n * sizeof(orbhip_kp)), 0, 0, 0, 0};
    if (full) o = {o.kps, lay.take(n * 32), lay.take(n * 4), lay.take(n * 8), lay.take(n)};
    return o;
}
static TriSide tri_put_side(StageBlock& S, const TriSideOff& o, const orbhip_tri_keyframe& k, bool full) {
    const size_t n = (size_t)k.n;
    uint8_t* const d = S.d;
    S.put(o.kps, k.kps, n * sizeof(orbhip_kp));
    if (!full) return {(const orbhip_kp*)(d + o.kps), nullptr, nullptr, nullptr, nullptr, k.n, 0};
    S.put(o.desc, k.desc, n * 32);
    S.put(o.node, k.node, n * 4);
    S.put(o.weight, k.weight, n * 8);
    S.put(o.mp, k.has_mp, n);
    return {(const orbhip_kp*)(d + o.kps), d + o.desc, (const int32_t*)(d + o.node), (const double*)(d + o.weight),
            d + o.mp, k.n, 0};
}

int tri_search(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_tri_keyframe* kf1,
               const orbhip_tri_keyframe* nbrs, int B, const float* scale_factors, const float* level_sigma2,
               int n_levels, int check_orientation, int32_t* match12, int32_t* nmatches, const TriStereo* sx) {
    if (!kf1 || B < 0) return ORBHIP_ERR_ARG;
    if (B == 0) return 0;
    if (B > kTriMaxPairs) return ORBHIP_ERR_UNSUPPORTED;
    if (!nbrs || !nmatches || !scale_factors || !level_sigma2 || n_levels <= 0) return ORBHIP_ERR_ARG;
    int rc = tri_check_side(*kf1, n_levels);
    for (int b = 0; b < B && rc == ORBHIP_OK; b++) rc = tri_check_side(nbrs[b], n_levels);
    if (rc != ORBHIP_OK) return rc;
    const int n1 = kf1->n;
    for (int b = 0; b < B; b++) nmatches[b] = 0;
    if (n1 == 0) return 0;
    if (!match12) return ORBHIP_ERR_ARG;
    // one block, the same layout on the host (pinned) and the device:
    // [sides (1 + B) | geometry B | scale factors | sigma2 | per keyframe: kps desc node weight has_mp]
    // then device only [KF1 keys | m1 | match12 B x n1, nmatches B]; the last segment is read back
    StageLayout lay(16);
    const size_t o_sides = lay.take((size_t)(1 + B) * sizeof(TriSide));
    const size_t o_geom = lay.take((size_t)B * sizeof(TriGeom));
    const size_t o_sf = lay.take((size_t)n_levels * 4), o_s2 = lay.take((size_t)n_levels * 4);
    std::vector<TriSideOff> so(1 + B);
    for (int s = 0; s <= B; s++) so[s] = tri_take_side(lay, (size_t)(s ? nbrs[s - 1].n : n1), true);
    const orbhip_tri_keyframe* ks[1 + kTriMaxPairs];
    int which[1 + kTriMaxPairs];
    for (int s = 0; s <= B; s++) { ks[s] = s ? &nbrs[s - 1] : kf1; which[s] = s; }
    const size_t o_sx = lay.take(sx ? tri_stereo_floats(ks, 1 + B) * 4 : 0);   // stereo: [mvuRight | mvDepth] per keyframe
    const size_t o_sb = lay.take(sx ? (size_t)(1 + B) * 8 : 0);                // and (mbf, mb)
    const size_t up_bytes = lay.total();
    const size_t o_keys = lay.take((size_t)kTriMax * 8), o_m1 = lay.take(4);
    const size_t back_bytes = (size_t)B * n1 * 4 + (size_t)B * 4;   // nmatches directly behind match12
    const size_t o_match = lay.take(back_bytes);
    HIPOK(S.ensure(lay.total(), up_bytes + back_bytes + 16));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    TriSide* sides = (TriSide*)(h + o_sides);
    TriGeom* geom = (TriGeom*)(h + o_geom);
    for (int s = 0; s <= B; s++) {
        const orbhip_tri_keyframe& k = s ? nbrs[s - 1] : *kf1;
        sides[s] = tri_put_side(S, so[s], k, true);
        if (s) {
            geom[s - 1].pad = 0.f;
            tri_geometry(*kf1, k, geom[s - 1].F, geom[s - 1].ep);
        }
    }
    if (sx) tri_put_stereo(S, o_sx, o_sb, *sx, which, 1 + B, sides);
    S.put(o_sf, scale_factors, (size_t)n_levels * 4);
    S.put(o_s2, level_sigma2, (size_t)n_levels * 4);
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    {
        const StageScope scope(timer);
        timer.begin(7, st);
        launch_tri_search((const TriSide*)(d + o_sides), (const TriGeom*)(d + o_geom), n1, B, (const float*)(d + o_sf),
                          (const float*)(d + o_s2), (unsigned long long*)(d + o_keys), (int32_t*)(d + o_m1),
                          check_orientation, (int32_t*)(d + o_match), (int32_t*)(d + o_match + (size_t)B * n1 * 4), st,
                          sx ? (const float*)(d + o_sx) : nullptr);
        timer.end(7, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + o_match, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    std::memcpy(match12, hb, (size_t)B * n1 * 4);
    std::memcpy(nmatches, hb + (size_t)B * n1 * 4, (size_t)B * 4);
    int total = 0;
    for (int b = 0; b < B; b++) total += nmatches[b];
    return total;
}

// =====================================================================================
// CreateNewMapPoints: the triangulation of the matches (DESIGN.md "CreateNewMapPoints")
//   tri_camera   host, fp32, fixed operation order: R, t, Ow and the intrinsics of a keyframe
//   k_tri_points one lane per (neighbour, KF1 feature): rays, parallax, the 4x4 system, its null
//                vector by an fp64 one-sided Jacobi held in registers (U and V: 32 doubles, every
//                index a constant), depth, reprojection, distance and scale-ratio checks
//   k_tri_claim  one 1024-thread work-group: first[idx1] = the first neighbour that accepts the
//                feature, the counts per neighbour, and the list in (neighbour, idx1) order: a
//                wave per neighbour walks idx1 in 64s, a lane's place is the number of set lanes
//                below it in the ballot (no atomics decide a position)
// =====================================================================================
struct TriCam { float R[9], t[3], Ow[3], fx, fy, cx, cy, pad; };

static void tri_camera(const orbhip_tri_keyframe& k, TriCam& c) {
    quat_to_matrix(k.pose_q, c.R);
    for (int i = 0; i < 3; i++) c.t[i] = k.pose_t[i];
    for (int i = 0; i < 3; i++) c.Ow[i] = -((c.R[i] * c.t[0] + c.R[3 + i] * c.t[1]) + c.R[6 + i] * c.t[2]);
    c.fx = k.fx; c.fy = k.fy; c.cx = k.cx; c.cy = k.cy; c.pad = 0.f;
}

// The stereo members of one feature and its keyframe (DESIGN.md "Stereo LocalMapping")
struct TriFeatStereo { float ur, depth, bf, b; };

// upstream's cos(2 atan2(mb / 2, mvDepth)) as (D^2 - h^2) / (D^2 + h^2), h = mb / 2, in fp64 (each
// operation rounded once: no FMA), rounded once to fp32
__device__ __forceinline__ float tri_stereo_cos(float b, float d) {
    const double h = (double)b * 0.5, D = (double)d;
    const double DD = D * D, hh = h * h;
    return (float)((DD - hh) / (DD + hh));
}

// KeyFrame::UnprojectStereo of a feature with depth z > 0
__device__ __forceinline__ void tri_unproject(const TriCam& c, const orbhip_kp& kp, float z, float X[3]) {
    const float x = ((kp.x - c.cx) * z) * (1.0f / c.fx), y = ((kp.y - c.cy) * z) * (1.0f / c.fy);
#pragma unroll
    for (int j = 0; j < 3; j++) X[j] = ((c.R[j] * x + c.R[3 + j] * y) + c.R[6 + j] * z) + c.Ow[j];
}

// the reprojection test of a stereo feature: (eX, eY, eR) against 7.8 sigma2
__device__ __forceinline__ bool tri_reproj_stereo_fails(const TriCam& c, const orbhip_kp& kp, const TriFeatStereo& f,
                                                        float px, float py, float z, float sigma2) {
    const float invz = 1.0f / z;
    const float u = ((c.fx * px) * invz) + c.cx, v = ((c.fy * py) * invz) + c.cy;
    const float u_r = u - f.bf * invz;
    const float eX = u - kp.x, eY = v - kp.y, eR = u_r - f.ur;
    return (double)((eX * eX + eY * eY) + eR * eR) > 7.8 * (double)sigma2;
}

// status of one matched pair (include/orbhip.h); X receives the point once it exists. STEREO: f1 / f2
// are the features' stereo members, source receives the branch that made the point (0 none, 1
// triangulated, 2 / 3 unprojected from KF1 / KF2)
template <bool STEREO>
__device__ __forceinline__ int tri_point(const TriCam& c1, const TriCam& c2, const orbhip_kp& kp1, const orbhip_kp& kp2,
                                         const float* __restrict__ scale_factors,
                                         const float* __restrict__ level_sigma2, double cos_max, float ratio_factor,
                                         float far, float X[3], const TriFeatStereo& f1, const TriFeatStereo& f2,
                                         int& source) {
    const float xn1x = (kp1.x - c1.cx) / c1.fx, xn1y = (kp1.y - c1.cy) / c1.fy;
    const float xn2x = (kp2.x - c2.cx) / c2.fx, xn2y = (kp2.y - c2.cy) / c2.fy;
    float r1[3], r2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        r1[i] = (c1.R[i] * xn1x + c1.R[3 + i] * xn1y) + c1.R[6 + i];
        r2[i] = (c2.R[i] * xn2x + c2.R[3 + i] * xn2y) + c2.R[6 + i];
    }
    const float dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2];
    const float nn1 = (r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2];
    const float nn2 = (r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2];
    const float cosP = dot / (sqrtf(nn1) * sqrtf(nn2));
    const bool st1 = STEREO && f1.ur >= 0.0f, st2 = STEREO && f2.ur >= 0.0f;
    int branch = 1;
    if (!STEREO) {
        if (!(cosP > 0.0f)) return 2;
        if (!((double)cosP < cos_max)) return 3;
    } else {
        float cosS1 = cosP + 1.0f, cosS2 = cosP + 1.0f;
        if (st1) cosS1 = tri_stereo_cos(f1.b, f1.depth);
        else if (st2) cosS2 = tri_stereo_cos(f2.b, f2.depth);
        const float cosS = cosS2 < cosS1 ? cosS2 : cosS1;
        if (cosP < cosS && cosP > 0.0f && (st1 || st2 || (double)cosP < cos_max)) branch = 1;
        else if (st1 && cosS1 < cosS2) branch = 2;
        else if (st2 && cosS2 < cosS1) branch = 3;
        else return !(cosP > 0.0f) ? 2 : 3;
        source = branch;
        if (branch != 1) {
            const float zs = branch == 2 ? f1.depth : f2.depth;
            if (!(zs > 0.0f)) return 12;
            tri_unproject(branch == 2 ? c1 : c2, branch == 2 ? kp1 : kp2, zs, X);
        }
    }
    if (!STEREO || branch == 1) {
    double U[16], V[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {   // T = [R | t]
        const float a0 = j < 3 ? c1.R[j] : c1.t[0], a1 = j < 3 ? c1.R[3 + j] : c1.t[1], a2 = j < 3 ? c1.R[6 + j] : c1.t[2];
        const float b0 = j < 3 ? c2.R[j] : c2.t[0], b1 = j < 3 ? c2.R[3 + j] : c2.t[1], b2 = j < 3 ? c2.R[6 + j] : c2.t[2];
        U[j] = (double)(xn1x * a2 - a0);
        U[4 + j] = (double)(xn1y * a2 - a1);
        U[8 + j] = (double)(xn2x * b2 - b0);
        U[12 + j] = (double)(xn2y * b2 - b1);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 6; sweep++) {
        tri_jacobi_pair<0, 1>(U, V);
        tri_jacobi_pair<0, 2>(U, V);
        tri_jacobi_pair<0, 3>(U, V);
        tri_jacobi_pair<1, 2>(U, V);
        tri_jacobi_pair<1, 3>(U, V);
        tri_jacobi_pair<2, 3>(U, V);
    }
    double best = ((U[0] * U[0] + U[4] * U[4]) + U[8] * U[8]) + U[12] * U[12];
    double v0 = V[0], v1 = V[4], v2 = V[8], v3 = V[12];
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const double nk = ((U[k] * U[k] + U[4 + k] * U[4 + k]) + U[8 + k] * U[8 + k]) + U[12 + k] * U[12 + k];
        if (nk < best) { best = nk; v0 = V[k]; v1 = V[4 + k]; v2 = V[8 + k]; v3 = V[12 + k]; }
    }
    if (v3 == 0.0) return 4;
    X[0] = (float)(v0 / v3); X[1] = (float)(v1 / v3); X[2] = (float)(v2 / v3);
    }
    const float x = X[0], y = X[1], z = X[2];
    const float z1 = ((c1.R[6] * x + c1.R[7] * y) + c1.R[8] * z) + c1.t[2];
    if (z1 <= 0.0f) return 5;
    const float z2 = ((c2.R[6] * x + c2.R[7] * y) + c2.R[8] * z) + c2.t[2];
    if (z2 <= 0.0f) return 6;
    {
        const float px = ((c1.R[0] * x + c1.R[1] * y) + c1.R[2] * z) + c1.t[0];
        const float py = ((c1.R[3] * x + c1.R[4] * y) + c1.R[5] * z) + c1.t[1];
        if (st1) {
            if (tri_reproj_stereo_fails(c1, kp1, f1, px, py, z1, level_sigma2[kp1.octave])) return 7;
        } else {
        const float e = ((c1.fx * px) / z1 + c1.cx) - kp1.x;
        const float f = ((c1.fy * py) / z1 + c1.cy) - kp1.y;
        if ((double)(e * e + f * f) > 5.991 * (double)level_sigma2[kp1.octave]) return 7;
        }
    }
    {
        const float px = ((c2.R[0] * x + c2.R[1] * y) + c2.R[2] * z) + c2.t[0];
        const float py = ((c2.R[3] * x + c2.R[4] * y) + c2.R[5] * z) + c2.t[1];
        if (st2) {
            if (tri_reproj_stereo_fails(c2, kp2, f2, px, py, z2, level_sigma2[kp2.octave])) return 8;
        } else {
        const float e = ((c2.fx * px) / z2 + c2.cx) - kp2.x;
        const float f = ((c2.fy * py) / z2 + c2.cy) - kp2.y;
        if ((double)(e * e + f * f) > 5.991 * (double)level_sigma2[kp2.octave]) return 8;
        }
    }
    const float d1x = x - c1.Ow[0], d1y = y - c1.Ow[1], d1z = z - c1.Ow[2];
    const float d2x = x - c2.Ow[0], d2y = y - c2.Ow[1], d2z = z - c2.Ow[2];
    const float dist1 = sqrtf((d1x * d1x + d1y * d1y) + d1z * d1z);
    const float dist2 = sqrtf((d2x * d2x + d2y * d2y) + d2z * d2z);
    if (dist1 == 0.0f || dist2 == 0.0f) return 9;
    if (far > 0.0f && (dist1 >= far || dist2 >= far)) return 10;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = scale_factors[kp1.octave] / scale_factors[kp2.octave];
    if (ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor) return 11;
    return 1;
}

constexpr int kTriPointsThreads = 256;
// pair = b * n1 + idx1 over the npairs = B x n1 pairs of the call; cams[0] = KF1, cams[1 + b] = neighbour b
// STEREO: sx = every keyframe's [mvuRight | mvDepth] (TriSide::pad), sb = (mbf, mb) per keyframe, source per pair
template <bool STEREO>
__global__ __launch_bounds__(kTriPointsThreads) void k_tri_points(
    const TriSide* __restrict__ sides, const TriCam* __restrict__ cams, const float* __restrict__ scale_factors,
    const float* __restrict__ level_sigma2, const int32_t* __restrict__ match12, int n1, int npairs, double cos_max,
    float ratio_factor, float far, uint8_t* __restrict__ status, float* __restrict__ x3d_all,
    const float* __restrict__ sx, const float* __restrict__ sb, uint8_t* __restrict__ source) {
    const int pair = blockIdx.x * kTriPointsThreads + threadIdx.x;
    if (pair >= npairs) return;
    const int b = pair / n1, idx1 = pair - b * n1;
    const int idx2 = match12[pair];
    int st = 0;
    float X[3] = {0.f, 0.f, 0.f};
    int src = 0;
    if (idx2 >= 0) {
        TriFeatStereo f1{-1.f, 0.f, 0.f, 0.f}, f2{-1.f, 0.f, 0.f, 0.f};
        if (STEREO) {
            const TriSide A = sides[0], N = sides[1 + b];
            f1 = TriFeatStereo{sx[A.pad + idx1], sx[A.pad + A.n + idx1], sb[0], sb[1]};
            f2 = TriFeatStereo{sx[N.pad + idx2], sx[N.pad + N.n + idx2], sb[2 * (1 + b)], sb[2 * (1 + b) + 1]};
        }
        st = tri_point<STEREO>(cams[0], cams[1 + b], sides[0].kps[idx1], sides[1 + b].kps[idx2], scale_factors,
                               level_sigma2, cos_max, ratio_factor, far, X, f1, f2, src);
    }
    if (STEREO) source[pair] = (uint8_t)src;
    status[pair] = (uint8_t)st;
    x3d_all[3 * (int64_t)pair] = X[0];
    x3d_all[3 * (int64_t)pair + 1] = X[1];
    x3d_all[3 * (int64_t)pair + 2] = X[2];
}

// head: [first n1 | nnew B | total 1]; the lists hold n1 entries each (new_x3d: n1 x 3)
__global__ __launch_bounds__(kTriThreads) void k_tri_claim(const uint8_t* __restrict__ status,
                                                           const int32_t* __restrict__ match12,
                                                           const float* __restrict__ x3d_all, int n1, int B,
                                                           int32_t* __restrict__ first_out, int32_t* __restrict__ nnew,
                                                           int32_t* __restrict__ total_out, int32_t* __restrict__ new_nbr,
                                                           int32_t* __restrict__ new_idx1, int32_t* __restrict__ new_idx2,
                                                           float* __restrict__ new_x3d) {
    __shared__ short first[kTriMax];
    __shared__ int cnt[kTriMaxPairs], base[kTriMaxPairs];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid < kTriMaxPairs) cnt[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n1; i += kTriThreads) {
        int f = -1;
        for (int b = 0; b < B; b++)
            if (status[(int64_t)b * n1 + i] == 1) { f = b; break; }
        first[i] = (short)f;
        first_out[i] = f;
        if (f >= 0) atomicAdd(&cnt[f], 1);   // a count: the same whatever the order
    }
    __syncthreads();
    if (tid < 64) {
        const int c = tid < B ? cnt[tid] : 0;
        const int inc = wave_incl_scan(c);
        base[tid] = inc - c;
        if (tid < B) nnew[tid] = c;
        if (tid == 63) *total_out = inc;
    }
    __syncthreads();
    for (int b = wid; b < B; b += kTriThreads / 64) {   // b is wave-uniform
        int run = base[b];
        if (cnt[b] == 0) continue;
        for (int i0 = 0; i0 < n1; i0 += 64) {
            const int i = i0 + lane;
            const bool mine = i < n1 && first[i] == b;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                const int pos = run + __popcll(m & ((1ull << lane) - 1ull));
                const int64_t pair = (int64_t)b * n1 + i;
                new_nbr[pos] = b;
                new_idx1[pos] = i;
                new_idx2[pos] = match12[pair];
                new_x3d[3 * pos] = x3d_all[3 * pair];
                new_x3d[3 * pos + 1] = x3d_all[3 * pair + 1];
                new_x3d[3 * pos + 2] = x3d_all[3 * pair + 2];
            }
            run += __popcll(m);
        }
    }
}

// the keypoints alone (orbhip_triangulate_matches reads nothing else of a keyframe)
static int tri_check_kps(const orbhip_tri_keyframe& k, int n_levels) {
    if (k.n < 0) return ORBHIP_ERR_ARG;
    if (k.n > kTriMax) return ORBHIP_ERR_UNSUPPORTED;
    if (k.n == 0) return ORBHIP_OK;
    if (!k.kps) return ORBHIP_ERR_ARG;
    for (int i = 0; i < k.n; i++)
        if (k.kps[i].octave < 0 || k.kps[i].octave >= n_levels) return ORBHIP_ERR_ARG;
    return ORBHIP_OK;
}

int tri_new_points(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_tri_keyframe* kf1,
                   const orbhip_tri_keyframe* nbrs, int B, const int32_t* match12_in, const float* median_depth,
                   const float* scale_factors, const float* level_sigma2, int n_levels, int check_orientation,
                   const orbhip_tri_params* params, orbhip_new_points* out, const TriStereo* sx, uint8_t* source) {
    const bool search = match12_in == nullptr;
    if (!kf1 || B < 0 || !params || !out) return ORBHIP_ERR_ARG;
    if (B > kTriMaxPairs) return ORBHIP_ERR_UNSUPPORTED;
    if ((B > 0 && (!nbrs || !out->nmatches || !out->gated || !out->nnew)) || !scale_factors || !level_sigma2 ||
        n_levels <= 0)
        return ORBHIP_ERR_ARG;
    int rc = search ? tri_check_side(*kf1, n_levels) : tri_check_kps(*kf1, n_levels);
    for (int b = 0; b < B && rc == ORBHIP_OK; b++)
        rc = search ? tri_check_side(nbrs[b], n_levels) : tri_check_kps(nbrs[b], n_levels);
    if (rc != ORBHIP_OK) return rc;
    const int n1 = kf1->n;
    if (n1 > 0 && (!out->first || !out->new_nbr || !out->new_idx1 || !out->new_idx2 || !out->new_x3d))
        return ORBHIP_ERR_ARG;
    if (!search)   // an index past the neighbour's keypoints would be read on the device
        for (int b = 0; b < B; b++)
            for (int i = 0; i < n1; i++) {
                const int32_t m = match12_in[(size_t)b * n1 + i];
                if (m < -1 || m >= nbrs[b].n) return ORBHIP_ERR_ARG;
            }
    const size_t pairs_all = (size_t)B * n1;
    for (int b = 0; b < B; b++) out->nmatches[b] = out->nnew[b] = 0, out->gated[b] = 0;
    for (int i = 0; i < n1; i++) out->first[i] = out->new_nbr[i] = out->new_idx1[i] = out->new_idx2[i] = -1;
    if (n1) std::memset(out->new_x3d, 0, (size_t)n1 * 12);
    if (out->match12) for (size_t i = 0; i < pairs_all; i++) out->match12[i] = -1;
    if (out->status && pairs_all) std::memset(out->status, 0, pairs_all);
    if (out->x3d_all && pairs_all) std::memset(out->x3d_all, 0, pairs_all * 12);
    if (source && pairs_all) std::memset(source, 0, pairs_all);
    if (B == 0 || n1 == 0) return 0;
    // the cameras, and the neighbours the baseline gate leaves (act): B scalar evaluations on the host
    std::vector<TriCam> cam(1 + B);
    tri_camera(*kf1, cam[0]);
    int act[kTriMaxPairs], Ba = 0;
    for (int b = 0; b < B; b++) {
        tri_camera(nbrs[b], cam[1 + b]);
        if (search && (median_depth || sx)) {
            const float dx = cam[1 + b].Ow[0] - cam[0].Ow[0], dy = cam[1 + b].Ow[1] - cam[0].Ow[1],
                        dz = cam[1 + b].Ow[2] - cam[0].Ow[2];
            const float baseline = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (sx) {   // the stereo gate: the neighbour's own stereo baseline mb
                if (baseline < sx->b[1 + b]) { out->gated[b] = 1; continue; }
            } else {
                const float r = baseline / median_depth[b];
                if ((double)r < 0.01) { out->gated[b] = 1; continue; }
            }
        }
        act[Ba++] = b;
    }
    if (Ba == 0) return 0;
    const size_t npairs = (size_t)Ba * n1;
    // upload: [sides (1 + Ba) | geometry Ba | cameras (1 + Ba) | scale factors | sigma2 | per keyframe: kps (and,
    // for the search, desc node weight has_mp) | the given matches]; device only: [KF1 keys | m1];
    // read back, as far as the caller asks: [first n1, nnew Ba, total | nmatches Ba | new_nbr | new_idx1 | new_idx2 |
    // new_x3d | match12 (of the search) | status | x3d_all]
    StageLayout lay(16);
    const size_t o_sides = lay.take((size_t)(1 + Ba) * sizeof(TriSide));
    const size_t o_geom = lay.take(search ? (size_t)Ba * sizeof(TriGeom) : 0);
    const size_t o_cams = lay.take((size_t)(1 + Ba) * sizeof(TriCam));
    const size_t o_sf = lay.take((size_t)n_levels * 4), o_s2 = lay.take((size_t)n_levels * 4);
    std::vector<TriSideOff> so(1 + Ba);
    for (int s = 0; s <= Ba; s++) so[s] = tri_take_side(lay, (size_t)(s ? nbrs[act[s - 1]].n : n1), search);
    const size_t o_min = lay.take(search ? 0 : npairs * 4);
    const orbhip_tri_keyframe* ks[1 + kTriMaxPairs];
    int which[1 + kTriMaxPairs];
    for (int s = 0; s <= Ba; s++) { ks[s] = s ? &nbrs[act[s - 1]] : kf1; which[s] = s ? 1 + act[s - 1] : 0; }
    const size_t o_sx = lay.take(sx ? tri_stereo_floats(ks, 1 + Ba) * 4 : 0);   // stereo: [mvuRight | mvDepth] per keyframe
    const size_t o_sb = lay.take(sx ? (size_t)(1 + Ba) * 8 : 0);                // and (mbf, mb)
    const size_t up_bytes = lay.total();
    const size_t o_keys = lay.take(search ? (size_t)kTriMax * 8 : 0), o_m1 = lay.take(search ? 4 : 0);
    const size_t o_head = lay.take((size_t)(n1 + Ba + 1) * 4);
    const size_t o_nm = lay.take((size_t)Ba * 4);
    const size_t o_nbr = lay.take((size_t)n1 * 4), o_i1 = lay.take((size_t)n1 * 4), o_i2 = lay.take((size_t)n1 * 4);
    const size_t o_x = lay.take((size_t)n1 * 12);
    size_t back_end = lay.off;
    const size_t o_match = search ? lay.take(npairs * 4) : o_min;
    if (search && out->match12) back_end = lay.off;
    const size_t o_status = lay.take(npairs);
    if (out->status) back_end = lay.off;
    const size_t o_x3d = lay.take(npairs * 12);
    if (out->x3d_all) back_end = lay.off;
    const size_t o_src = lay.take(sx ? npairs : 0);
    if (sx && source) back_end = lay.off;
    const size_t back_bytes = back_end - o_head;
    HIPOK(S.ensure(lay.total(), up_bytes + back_bytes + 16));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    TriSide* sides = (TriSide*)(h + o_sides);
    TriCam* cams = (TriCam*)(h + o_cams);
    for (int s = 0; s <= Ba; s++) {
        const orbhip_tri_keyframe& k = s ? nbrs[act[s - 1]] : *kf1;
        cams[s] = cam[s ? 1 + act[s - 1] : 0];
        sides[s] = tri_put_side(S, so[s], k, search);
        if (search && s) {
            TriGeom* geom = (TriGeom*)(h + o_geom);
            geom[s - 1].pad = 0.f;
            tri_geometry(*kf1, k, geom[s - 1].F, geom[s - 1].ep);
        }
    }
    if (sx) tri_put_stereo(S, o_sx, o_sb, *sx, which, 1 + Ba, sides);
    S.put(o_sf, scale_factors, (size_t)n_levels * 4);
    S.put(o_s2, level_sigma2, (size_t)n_levels * 4);
    if (!search) S.put(o_min, match12_in, npairs * 4);   // no neighbour is gated: the rows are the caller's
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    int32_t* const d_head = (int32_t*)(d + o_head);
    {
        const StageScope scope(timer);
        if (search) {
            timer.begin(7, st);
            launch_tri_search((const TriSide*)(d + o_sides), (const TriGeom*)(d + o_geom), n1, Ba,
                              (const float*)(d + o_sf), (const float*)(d + o_s2), (unsigned long long*)(d + o_keys),
                              (int32_t*)(d + o_m1), check_orientation, (int32_t*)(d + o_match), (int32_t*)(d + o_nm),
                              st, sx ? (const float*)(d + o_sx) : nullptr);
            timer.end(7, st);
        }
        timer.begin(10, st);
        const unsigned wgs = (unsigned)((npairs + kTriPointsThreads - 1) / kTriPointsThreads);
        if (sx)
            ORBHIP_LAUNCH(k_tri_points<true>, dim3(wgs), dim3(kTriPointsThreads), 0, st, (const TriSide*)(d + o_sides),
                          (const TriCam*)(d + o_cams), (const float*)(d + o_sf), (const float*)(d + o_s2),
                          (const int32_t*)(d + o_match), n1, (int)npairs, params->cos_parallax_max,
                          params->ratio_factor, params->far_threshold, d + o_status, (float*)(d + o_x3d),
                          (const float*)(d + o_sx), (const float*)(d + o_sb), d + o_src);
        else
            ORBHIP_LAUNCH(k_tri_points<false>, dim3(wgs), dim3(kTriPointsThreads), 0, st, (const TriSide*)(d + o_sides),
                          (const TriCam*)(d + o_cams), (const float*)(d + o_sf), (const float*)(d + o_s2),
                          (const int32_t*)(d + o_match), n1, (int)npairs, params->cos_parallax_max,
                          params->ratio_factor, params->far_threshold, d + o_status, (float*)(d + o_x3d),
                          (const float*)nullptr, (const float*)nullptr, (uint8_t*)nullptr);
        ORBHIP_LAUNCH(k_tri_claim, dim3(1), dim3(kTriThreads), 0, st, (const uint8_t*)(d + o_status),
                      (const int32_t*)(d + o_match), (const float*)(d + o_x3d), n1, Ba, d_head, d_head + n1,
                      d_head + n1 + Ba, (int32_t*)(d + o_nbr), (int32_t*)(d + o_i1), (int32_t*)(d + o_i2),
                      (float*)(d + o_x));
        timer.end(10, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + o_head, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    auto back = [&](size_t o) { return hb + (o - o_head); };
    const int32_t* r_head = (const int32_t*)back(o_head);
    int total = r_head[n1 + Ba];
    if (total < 0 || total > n1) return ORBHIP_ERR_DEVICE;
    const int32_t *r_nm = (const int32_t*)back(o_nm), *r_nbr = (const int32_t*)back(o_nbr);
    for (int i = 0; i < n1; i++) out->first[i] = (unsigned)r_head[i] >= (unsigned)Ba ? -1 : act[r_head[i]];
    for (int a = 0; a < Ba; a++) {
        const int b = act[a];
        out->nnew[b] = r_head[n1 + a];
        if (search) {
            out->nmatches[b] = r_nm[a];
        } else {
            int c = 0;
            for (int i = 0; i < n1; i++) c += match12_in[(size_t)b * n1 + i] >= 0;
            out->nmatches[b] = c;
        }
        if (out->match12)
            std::memcpy(out->match12 + (size_t)b * n1, search ? (const void*)(back(o_match) + (size_t)a * n1 * 4)
                                                               : (const void*)(match12_in + (size_t)b * n1),
                        (size_t)n1 * 4);
        if (out->status) std::memcpy(out->status + (size_t)b * n1, back(o_status) + (size_t)a * n1, (size_t)n1);
        if (sx && source) std::memcpy(source + (size_t)b * n1, back(o_src) + (size_t)a * n1, (size_t)n1);
        if (out->x3d_all)
            std::memcpy(out->x3d_all + (size_t)b * n1 * 3, back(o_x3d) + (size_t)a * n1 * 12, (size_t)n1 * 12);
    }
    for (int k = 0; k < total; k++) {
        if ((unsigned)r_nbr[k] >= (unsigned)Ba) return ORBHIP_ERR_DEVICE;
        out->new_nbr[k] = act[r_nbr[k]];
    }
    std::memcpy(out->new_idx1, back(o_i1), (size_t)total * 4);
    std::memcpy(out->new_idx2, back(o_i2), (size_t)total * 4);
    std::memcpy(out->new_x3d, back(o_x), (size_t)total * 12);
    return total;
}

}  // namespace orbhip
