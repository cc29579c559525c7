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
// LDS of k_tri_search: 3 x 8 KiB (KF1 nodes, bucket counts, bucket starts) + 4 KiB bucket entries +
// 4 KiB matches + 2 KiB bins + counters = 34.2 KiB static (k_tri_order: 16 KiB), below the 64 KiB a
// kernel gets without the dynamic-LDS attribute (160 KiB per CU).
#include <hip/hip_runtime.h>

#include <vector>

#include "geom.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" triangulation", x)

namespace orbhip {

constexpr int kTriMax = 2048;     // features per keyframe (LDS-resident keys, 16-bit indices)
constexpr int kTriMaxPairs = 64;  // neighbours per call
struct TriSide {                  // one keyframe in the call's staging block (device pointers)
    const orbhip_kp* kps;
    const uint8_t* desc;          // n x 32
    const int32_t* node;
    const double* weight;
    const uint8_t* has_mp;
    int n, pad;
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

__global__ __launch_bounds__(kTriThreads) void k_tri_search(const TriSide* __restrict__ sides,
                                                            const TriGeom* __restrict__ geom,
                                                            const float* __restrict__ scale_factors,
                                                            const float* __restrict__ level_sigma2,
                                                            const unsigned long long* __restrict__ keys1,
                                                            const int32_t* __restrict__ m1_in, int check_orientation,
                                                            int32_t* __restrict__ match12,
                                                            int32_t* __restrict__ nmatches) {
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
    const float factor = 1.0f / 30;
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
                if (dex * dex + dey * dey < 100.0f * scale_factors[kp2.octave]) continue;
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
                float rot = kp1.angle - N.kps[bestIdx2].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == 30) bin = 0;
                if ((unsigned)bin < 30u) { atomicAdd(&S.hist[bin], 1); S.bin[idx1] = (int8_t)bin; }
            }
        }
    }
    __syncthreads();
    // ---- 3. rotation consistency: ComputeThreeMaxima over the 30 bins (as k_search_bow) ----
    if (check_orientation && tid == 0) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < 30; i++) {
            const int s = S.hist[i];
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
        S.keep[0] = ind1; S.keep[1] = ind2; S.keep[2] = ind3;
    }
    __syncthreads();
    int c = 0;
    int32_t* out = match12 + (int64_t)b * n1;
    for (int i = tid; i < n1; i += kTriThreads) {
        int m = S.match[i];
        if (m >= 0 && check_orientation) {
            const int bin = S.bin[i];
            if (bin != S.keep[0] && bin != S.keep[1] && bin != S.keep[2]) m = -1;
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
                              int check_orientation, int32_t* match12, int32_t* nmatches, hipStream_t st) {
    const unsigned order_wgs = (unsigned)((n1 + kTriOrderThreads - 1) / kTriOrderThreads);
    ORBHIP_LAUNCH(k_tri_order, dim3(order_wgs), dim3(kTriOrderThreads), 0, st, sides, keys1, m1);
    ORBHIP_LAUNCH(k_tri_search, dim3((unsigned)B), dim3(kTriThreads), 0, st, sides, geom, scale_factors, level_sigma2,
                  (const unsigned long long*)keys1, (const int32_t*)m1, check_orientation, match12, nmatches);
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

int tri_search(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_tri_keyframe* kf1,
               const orbhip_tri_keyframe* nbrs, int B, const float* scale_factors, const float* level_sigma2,
               int n_levels, int check_orientation, int32_t* match12, int32_t* nmatches) {
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
    struct SideOff { size_t kps, desc, node, weight, mp; };
    std::vector<SideOff> so(1 + B);
    for (int s = 0; s <= B; s++) {
        const size_t n = (size_t)(s ? nbrs[s - 1].n : n1);
        so[s] = {lay.take(n * sizeof(orbhip_kp)), lay.take(n * 32), lay.take(n * 4), lay.take(n * 8), lay.take(n)};
    }
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
        const size_t n = (size_t)k.n;
        sides[s] = {(const orbhip_kp*)(d + so[s].kps), d + so[s].desc, (const int32_t*)(d + so[s].node),
                    (const double*)(d + so[s].weight), d + so[s].mp, k.n, 0};
        put_keyframe(S, so[s].kps, so[s].desc, 0, k.kps, k.desc, n);
        S.put(so[s].node, k.node, n * 4);
        S.put(so[s].weight, k.weight, n * 8);
        S.put(so[s].mp, k.has_mp, n);
        if (s) {
            geom[s - 1].pad = 0.f;
            tri_geometry(*kf1, k, geom[s - 1].F, geom[s - 1].ep);
        }
    }
    S.put(o_sf, scale_factors, (size_t)n_levels * 4);
    S.put(o_s2, level_sigma2, (size_t)n_levels * 4);
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    {
        const StageScope scope(timer);
        timer.begin(7, st);
        launch_tri_search((const TriSide*)(d + o_sides), (const TriGeom*)(d + o_geom), n1, B, (const float*)(d + o_sf),
                          (const float*)(d + o_s2), (unsigned long long*)(d + o_keys), (int32_t*)(d + o_m1),
                          check_orientation, (int32_t*)(d + o_match), (int32_t*)(d + o_match + (size_t)B * n1 * 4), st);
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

}  // namespace orbhip
