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
// LDS: k_fuse_grid 12 KiB histogram + 12 KiB cursors + scan scratch; k_fuse_search 4 bytes.
#include <hip/hip_runtime.h>

#include "orbhip_device.h"
#include "orbhip_kernels.h"

namespace orbhip {

// ---- host: per-keyframe constants (all fp32, every operation in the order written; no FMA) ----
static void fuse_qrot(const float q[4], const float v[3], float o[3]) {   // Eigen _transformVector
    float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    o[0] = v[0] + q[3] * uv[0] + c[0];
    o[1] = v[1] + q[3] * uv[1] + c[1];
    o[2] = v[2] + q[3] * uv[2] + c[2];
}

void fuse_kf_params(const orbhip_frame& f, int base, FuseKf* k) {
    k->n = f.n;
    k->base = base;
    k->minx = f.min_x; k->maxx = f.max_x; k->miny = f.min_y; k->maxy = f.max_y;
    k->invw = (float)kFuseCols / (f.max_x - f.min_x);
    k->invh = (float)kFuseRows / (f.max_y - f.min_y);
    for (int i = 0; i < 4; i++) k->q[i] = f.pose_q[i];
    for (int i = 0; i < 3; i++) k->t[i] = f.pose_t[i];
    const float qc[4] = {-f.pose_q[0], -f.pose_q[1], -f.pose_q[2], f.pose_q[3]};
    const float mt[3] = {f.pose_t[0] * -1.0f, f.pose_t[1] * -1.0f, f.pose_t[2] * -1.0f};
    fuse_qrot(qc, mt, k->Ow);
    k->fx = f.fx; k->fy = f.fy; k->cx = f.cx; k->cy = f.cy;
}

// ---- device ----
__device__ __forceinline__ void fuse_qrot_dev(const float q[4], const float v[3], float o[3]) {
    float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    o[0] = v[0] + q[3] * uv[0] + c[0];
    o[1] = v[1] + q[3] * uv[1] + c[1];
    o[2] = v[2] + q[3] * uv[2] + c[2];
}

// PosInGrid: cell = px * 48 + py, -1 outside the grid (as k_proj_cells)
__device__ __forceinline__ int fuse_cell(const FuseKf& f, float x, float y) {
    const int px = (int)roundf((x - f.minx) * f.invw);
    const int py = (int)roundf((y - f.miny) * f.invh);
    return (px < 0 || px >= kFuseCols || py < 0 || py >= kFuseRows) ? -1 : px * kFuseRows + py;
}

constexpr int kFuseGridThreads = 1024;
constexpr int kFuseBinsPerThread = kFuseCells / kFuseGridThreads;
static_assert(kFuseBinsPerThread * kFuseGridThreads == kFuseCells, "k_fuse_grid scans 3 bins per thread");
struct FuseGridLds {
    int hist[kFuseCells];     // keypoints per cell
    int cursor[kFuseCells];   // next free slot of a cell while scattering
    int scan[kFuseGridThreads / 64 + 1];
};

__global__ __launch_bounds__(kFuseGridThreads) void k_fuse_grid(const FuseKf* __restrict__ kfs,
                                                                const orbhip_kp* __restrict__ kps,
                                                                int32_t* __restrict__ cell_start,
                                                                FuseRec* __restrict__ recs,
                                                                int32_t* __restrict__ nfused) {
    __shared__ FuseGridLds L;
    const int tid = threadIdx.x, b = blockIdx.x;
    const FuseKf f = kfs[b];
    const orbhip_kp* kp = kps + f.base;
    for (int c = tid; c < kFuseCells; c += kFuseGridThreads) L.hist[c] = 0;
    if (tid == 0) nfused[b] = 0;
    __syncthreads();
    for (int i = tid; i < f.n; i += kFuseGridThreads) {
        const int c = fuse_cell(f, kp[i].x, kp[i].y);
        if (c >= 0) atomicAdd(&L.hist[c], 1);
    }
    __syncthreads();
    int h[kFuseBinsPerThread], sum = 0;
#pragma unroll
    for (int k = 0; k < kFuseBinsPerThread; k++) { h[k] = L.hist[tid * kFuseBinsPerThread + k]; sum += h[k]; }
    int total;
    int pos = block_excl_scan(sum, L.scan, &total);
    int32_t* cs = cell_start + (int64_t)b * (kFuseCells + 1);
#pragma unroll
    for (int k = 0; k < kFuseBinsPerThread; k++) {
        const int c = tid * kFuseBinsPerThread + k;
        L.cursor[c] = pos;
        cs[c] = pos;
        pos += h[k];
    }
    if (tid == 0) cs[kFuseCells] = total;
    __syncthreads();
    // the slot inside a cell is the order in which the LDS counter is reached: any order serves,
    // k_fuse_search's key minimum does not depend on it
    FuseRec* out = recs + f.base;
    for (int i = tid; i < f.n; i += kFuseGridThreads) {
        const orbhip_kp k = kp[i];
        const int c = fuse_cell(f, k.x, k.y);
        if (c >= 0) out[atomicAdd(&L.cursor[c], 1)] = FuseRec{k.x, k.y, (c << 8) | k.octave, i};
    }
}

constexpr int kFuseThreads = 256;
// lanes per (keyframe, point). Measured on one MI355X, both kernels of a call, B = 30 x 1000 points x
// 1000 keypoints / B = 1 x 20000 x 1000: 1 lane 27.7 / 19.1 us, 4 lanes 18.6 / 15.8 us, 8 lanes
// 20.9 / 18.1 us
constexpr int kFuseSplit = 4;

// S neighbouring lanes share a point: each computes the gates of steps 1-7 (the same values, so the
// same exits), they take the candidates of a column span in turns and merge their minima
template <int S>
__global__ __launch_bounds__(kFuseThreads) void k_fuse_search(const FuseKf* __restrict__ kfs, FusePoints mp,
                                                              const uint8_t* __restrict__ pair_skip,
                                                              const float* __restrict__ scale_factors,
                                                              const float* __restrict__ inv_level_sigma2,
                                                              int n_levels, float log_sf, float th,
                                                              const int32_t* __restrict__ cell_start,
                                                              const FuseRec* __restrict__ recs,
                                                              const uint8_t* __restrict__ kf_desc,
                                                              int32_t* __restrict__ best_idx,
                                                              int32_t* __restrict__ best_dist,
                                                              int32_t* __restrict__ level,
                                                              int32_t* __restrict__ nfused) {
    static_assert(S >= 1 && S <= 64 && (S & (S - 1)) == 0, "the lanes of a point lie in one wave");
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
        const float P[3] = {mp.pts[3 * m], mp.pts[3 * m + 1], mp.pts[3 * m + 2]};
        // 1. Sophus SE3f * p
        float Pc[3];
        fuse_qrot_dev(f.q, P, Pc);
        Pc[0] += f.t[0]; Pc[1] += f.t[1]; Pc[2] += f.t[2];
        if (Pc[2] < 0.0f) break;
        // 2., 3. Pinhole::project, KeyFrame::IsInImage (the maximum is strict)
        const float u = (f.fx * Pc[0]) / Pc[2] + f.cx, v = (f.fy * Pc[1]) / Pc[2] + f.cy;
        if (!(u >= f.minx && u < f.maxx && v >= f.miny && v < f.maxy)) break;
        // 4. distance range
        const float PO[3] = {P[0] - f.Ow[0], P[1] - f.Ow[1], P[2] - f.Ow[2]};
        const float dist3D = sqrtf((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
        const float maxd = mp.maxd[m];
        if (dist3D < 0.8f * mp.mind[m] || dist3D > 1.2f * maxd) break;
        // 5. viewing angle
        const float* Pn = mp.nrm + 3 * m;
        if ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2] < 0.5f * dist3D) break;
        // 6. MapPoint::PredictScale (clamped before the conversion: the same for every finite value)
        const float fl = ceilf(logf(maxd / dist3D) / log_sf);
        const int lvl = !(fl > 0.0f) ? 0 : (fl >= (float)n_levels ? n_levels - 1 : (int)fl);
        outLvl = lvl;
        // 7. radius
        const float r = th * scale_factors[lvl];
        // 8. KeyFrame::GetFeaturesInArea: the cell rectangle with its early returns
        const int x0 = max(0, (int)floorf((u - f.minx - r) * f.invw));
        if (x0 >= kFuseCols) break;
        const int x1 = min(kFuseCols - 1, (int)ceilf((u - f.minx + r) * f.invw));
        if (x1 < 0) break;
        const int y0 = max(0, (int)floorf((v - f.miny - r) * f.invh));
        if (y0 >= kFuseRows) break;
        const int y1 = min(kFuseRows - 1, (int)ceilf((v - f.miny + r) * f.invh));
        if (y1 < 0) break;
        const uint4* dm = (const uint4*)(mp.desc + (int64_t)m * 32);
        const uint4 da = dm[0], db = dm[1];
        const int32_t* cs = cell_start + (int64_t)b * (kFuseCells + 1);
        const FuseRec* rc = recs + f.base;
        const uint8_t* kd = kf_desc + (int64_t)f.base * 32;
        for (int ix = x0; ix <= x1; ix++) {
            // the cells (ix, y0..y1) are neighbours in the cell-ordered array: one span per column
            const int j0 = cs[ix * kFuseRows + y0], j1 = cs[ix * kFuseRows + y1 + 1];
            for (int j = j0 + sub; j < j1; j += S) {
                const FuseRec k = rc[j];
                const float dx = k.x - u, dy = k.y - v;
                if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
                // 9. level gate, chi-square gate, then the descriptor
                const int octave = k.cell_oct & 0xFF;
                if (octave < lvl - 1 || octave > lvl) continue;
                const float ex = u - k.x, ey = v - k.y;
                const float e2 = ex * ex + ey * ey;
                if ((double)(e2 * inv_level_sigma2[octave]) > 5.99) continue;
                const uint4* d2 = (const uint4*)(kd + (int64_t)k.idx * 32);
                const uint4 ea = d2[0], eb = d2[1];
                const unsigned dist = __popc(da.x ^ ea.x) + __popc(da.y ^ ea.y) + __popc(da.z ^ ea.z) +
                                      __popc(da.w ^ ea.w) + __popc(db.x ^ eb.x) + __popc(db.y ^ eb.y) +
                                      __popc(db.z ^ eb.z) + __popc(db.w ^ eb.w);
                const unsigned long long key =
                    ((unsigned long long)dist << 32) | ((unsigned long long)(k.cell_oct >> 8) << 16) | (unsigned)k.idx;
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

void launch_fuse(const FuseKf* kfs, int B, const FusePoints& mp, const uint8_t* pair_skip, const float* scale_factors,
                 const float* inv_level_sigma2, int n_levels, float log_sf, float th, const orbhip_kp* kps,
                 const uint8_t* kf_desc, int32_t* cell_start, FuseRec* recs, int32_t* best_idx, int32_t* best_dist,
                 int32_t* level, int32_t* nfused, hipStream_t st) {
    ORBHIP_LAUNCH(k_fuse_grid, dim3((unsigned)B), dim3(kFuseGridThreads), 0, st, kfs, kps, cell_start, recs, nfused);
    const unsigned tiles = (unsigned)(((int64_t)mp.n * kFuseSplit + kFuseThreads - 1) / kFuseThreads);
    ORBHIP_LAUNCH(k_fuse_search<kFuseSplit>, dim3(tiles, (unsigned)B), dim3(kFuseThreads), 0, st, kfs, mp, pair_skip,
                  scale_factors, inv_level_sigma2, n_levels, log_sf, th, (const int32_t*)cell_start,
                  (const FuseRec*)recs, kf_desc, best_idx, best_dist, level, nfused);
}

}  // namespace orbhip
