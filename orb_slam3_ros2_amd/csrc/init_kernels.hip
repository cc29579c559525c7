// SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
//   (U:src/ORBmatcher.cc; monocular initialisation, Tracking::MonocularInitialization)
//
// The reference walks the F1 keypoints of octave 0 in index order; each reads and writes the
// per-F2-keypoint state (vMatchedDistance, vnMatches21), so query i depends on every earlier
// query. The device splits that into the state-free part and the chain:
//   k_init_prep     one WG: F2 octave-0 keypoints with a grid cell, ranked in walk order
//                   (cell = px * 48 + py, then index); F1 octave-0 keypoints -> query slots
//   k_init_cands    one wave per query: GetFeaturesInArea(prev, windowSize, 0, 0) as a
//                   rectangle/level/|d| < r test over the ranked F2 keypoints, Hamming distance,
//                   ballot-compacted list of (dist << 21 | rank << 5 | rotation bin), and the
//                   list's 16 smallest entries (per-lane sorted top-4, 16 wave-min extractions)
//   k_init_greedy   one WG: wave 0 runs the chain with the state in LDS. Per query: the
//                   eligible entries (dist < vMatchedDistance[rank]) among its 16 smallest by one
//                   ballot; the first two set bits are the reference's best and second best
//                   whenever two are eligible or the list has <= 16 entries (else the whole list
//                   is scanned, a DPP/permlane top-2 butterfly); TH_LOW / ratio test; the steal
//                   update. Four queries share a 64-lane register, blocks of four are in flight.
//                   Then the whole WG applies the rotation histogram (ComputeThreeMaxima over the
//                   pushes, stale ones included) and writes vnMatches12 / vbPrevMatched.
// (dist, rank) order is the walk order tie-break of "dist < bestDist", and the second-best
// distance is the second element of the multiset, so the chain is exact. The bin of the pair
// (the rotHist push) rides in the low bits, so the chain never touches the keypoints.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "../../include/orbhip.h"
#include "dev_attr.h"
#include "geom.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "proj.h"
#include "proj_ws.h"
#include "rot_filter.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" init", x)

namespace orbhip {

namespace {

constexpr int kThLow = 50;
constexpr int kInitK = 16;   // smallest list entries per query handed to the chain
constexpr int kInitR = 4;    // ring of 4-query blocks in flight in the chain
constexpr int kInitMaxRounds = 64;   // parallel rounds before the chain takes over

// min over the wave, every lane gets it
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true));   // row_mirror
    const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = min(a[0], a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return min(b[0], b[1]);
}

struct InitGeom {
    int n1, n2;
    float minx, maxx, miny, maxy, invw, invh, r;
    int list_cap;    // entries per query list (>= number of ranked F2 keypoints, multiple of 64)
};

// counts[0] = queries (F1 octave 0), counts[1] = ranked F2 keypoints, counts[2] = nmatches
__global__ __launch_bounds__(1024) void k_init_prep(InitGeom g, const orbhip_kp* __restrict__ kps1,
                                                    const orbhip_kp* __restrict__ kps2, int* __restrict__ slot,
                                                    int* __restrict__ qlist, int* __restrict__ counts,
                                                    int* __restrict__ cnt3, int* __restrict__ flags, int nflags) {
    __shared__ int cnt[kGridCells], start[kGridCells], scratch[20], tot;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int c = tid; c < kGridCells; c += nt) cnt[c] = 0;
    __syncthreads();
    for (int k = tid; k < g.n2; k += nt) {
        const orbhip_kp kp = kps2[k];
        const int c = kp.octave == 0 ? grid_cell(g.minx, g.miny, g.invw, g.invh, kp.x, kp.y) : -1;
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan of the 3072 cell counts (3 per thread, in order)
    {
        int v[3], s = 0;
        for (int j = 0; j < 3; j++) { const int c = tid * 3 + j; v[j] = c < kGridCells ? cnt[c] : 0; s += v[j]; }
        int total;
        int base = block_excl_scan(s, scratch, &total);
        for (int j = 0; j < 3; j++) { const int c = tid * 3 + j; if (c < kGridCells) start[c] = base; base += v[j]; }
        if (tid == 0) tot = total;
    }
    __syncthreads();
    for (int c = tid; c < kGridCells; c += nt) cnt[c] = 0;
    __syncthreads();
    for (int k = tid; k < g.n2; k += nt) {
        const orbhip_kp kp = kps2[k];
        const int c = kp.octave == 0 ? grid_cell(g.minx, g.miny, g.invw, g.invh, kp.x, kp.y) : -1;
        if (c >= 0) slot[start[c] + atomicAdd(&cnt[c], 1)] = k;
    }
    __syncthreads();
    // index order inside each cell (cells hold a handful of keypoints)
    for (int c = tid; c < kGridCells; c += nt) {
        int* a = slot + start[c];
        const int m = cnt[c];
        for (int i = 1; i < m; i++) {
            const int v = a[i];
            int j = i - 1;
            while (j >= 0 && a[j] > v) { a[j + 1] = a[j]; j--; }
            a[j + 1] = v;
        }
    }
    // F1 octave-0 keypoints in index order
    int run = 0;
    for (int k0 = 0; k0 < g.n1; k0 += nt) {
        const int k = k0 + tid;
        const int f = (k < g.n1 && kps1[k].octave == 0) ? 1 : 0;   // level1 > 0 -> skipped
        int total;
        const int pos = block_excl_scan(f, scratch, &total);
        if (f) qlist[run + pos] = k;
        run += total;
    }
    if (tid == 0) { counts[0] = run; counts[1] = tot; }
    // the parallel rounds' first two claim tables and flags start empty
    for (int k = tid; k < 2 * tot; k += nt) cnt3[k] = 0;
    for (int k = tid; k < nflags; k += nt) flags[k] = 0;
}

// one wave per query slot: the candidate list of GetFeaturesInArea(prev[i1], r, 0, 0)
__global__ __launch_bounds__(256) void k_init_cands(InitGeom g, const orbhip_kp* __restrict__ kps1,
                                                    const uint8_t* __restrict__ desc1,
                                                    const orbhip_kp* __restrict__ kps2,
                                                    const uint8_t* __restrict__ desc2, const float* __restrict__ prev,
                                                    const int* __restrict__ slot, const int* __restrict__ qlist,
                                                    const int* __restrict__ counts, uint32_t* __restrict__ lists,
                                                    int* __restrict__ lens, uint32_t* __restrict__ topk,
                                                    int* __restrict__ need) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int nq = counts[0], nr = counts[1];
    if (q >= nq) {
        // the slots that fill the last block of four: the chain loads their rows too (empty, not stale)
        if (lane < kInitK) topk[(size_t)q * kInitK + lane] = ~0u;
        return;
    }
    const int i1 = qlist[q];
    const float x = prev[2 * i1], y = prev[2 * i1 + 1], r = g.r;
    const int nMinCellX = max(0, (int)floorf((x - g.minx - r) * g.invw));
    const int nMaxCellX = min(kGridCols - 1, (int)ceilf((x - g.minx + r) * g.invw));
    const int nMinCellY = max(0, (int)floorf((y - g.miny - r) * g.invh));
    const int nMaxCellY = min(kGridRows - 1, (int)ceilf((y - g.miny + r) * g.invh));
    const bool any = nMinCellX < kGridCols && nMaxCellX >= 0 && nMinCellY < kGridRows && nMaxCellY >= 0;
    uint32_t* out = lists + (size_t)q * g.list_cap;
    const float a1 = kps1[i1].angle;
    int n = 0, seen = 0;
    uint32_t t0 = ~0u, t1 = ~0u, t2 = ~0u, t3 = ~0u;
    if (any) {
        const uint4* qd4 = (const uint4*)(desc1 + 32 * (size_t)i1);
        const uint4 qa = qd4[0], qb = qd4[1];
        for (int b = 0; b < nr; b += 64) {
            const int rk = b + lane;
            bool ok = false;
            uint32_t v = 0;
            if (rk < nr) {
                const int k = slot[rk];
                const orbhip_kp kp = kps2[k];
                const int c = grid_cell(g.minx, g.miny, g.invw, g.invh, kp.x, kp.y);
                const int px = c / kGridRows, py = c - px * kGridRows;
                if (px >= nMinCellX && px <= nMaxCellX && py >= nMinCellY && py <= nMaxCellY &&
                    fabsf(kp.x - x) < r && fabsf(kp.y - y) < r) {
                    const uint4* kd4 = (const uint4*)(desc2 + 32 * (size_t)k);
                    const uint4 ka = kd4[0], kb = kd4[1];
                    const int d = hamming256(qa, qb, ka, kb);
                    v = ((uint32_t)d << 21) | ((uint32_t)rk << 5) | (uint32_t)rot_bin(a1, kp.angle);
                    ok = true;
                }
            }
            const uint64_t m = __ballot(ok);
            if (ok) out[n + __popcll(m & ((1ull << lane) - 1ull))] = v;
            n += __popcll(m);
            // per-lane sorted top-4 (branch-free insert)
            const uint32_t w = ok ? v : ~0u;
            t3 = min(t3, max(t2, w)); t2 = min(t2, max(t1, w)); t1 = min(t1, max(t0, w)); t0 = min(t0, w);
            seen += ok;
        }
    }
    // the list's 16 smallest entries: 16 rounds of wave-min over the lane heads, the winning lane
    // pops. A lane that pops all 4 of its kept entries while it had more may have lost one of
    // the 16: then the chain scans the whole list (need = 2).
    uint32_t mine = ~0u;
    int popped = 0;
#pragma unroll
    for (int j = 0; j < kInitK; j++) {
        const uint32_t mn = wave_min_u32(t0);
        if (lane == j) mine = mn;
        if (t0 == mn && mn != ~0u) { t0 = t1; t1 = t2; t2 = t3; t3 = ~0u; popped++; }
    }
    const bool lost = __ballot(popped == 4 && seen > 4) != 0;
    if (lane < kInitK) topk[(size_t)q * kInitK + lane] = mine;
    if (lane == 0) {
        lens[q] = n;
        need[q] = lost ? 2 : (n > kInitK ? 1 : 0);
    }
}

// (m1, m2) = the two smallest values of the multiset union of two disjoint lane sets
__device__ __forceinline__ void top2_merge(uint32_t& m1, uint32_t& m2, uint32_t o1, uint32_t o2) {
    const uint32_t hi = max(m1, o1);
    m1 = min(m1, o1);
    m2 = min(hi, min(m2, o2));
}
template <int CTRL>
__device__ __forceinline__ void top2_dpp(uint32_t& m1, uint32_t& m2) {
    const uint32_t o1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)m1, CTRL, 0xF, 0xF, true);
    const uint32_t o2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)m2, CTRL, 0xF, 0xF, true);
    top2_merge(m1, m2, o1, o2);
}
// butterfly over the wave: xor 1, xor 2, half-row mirror, row mirror (each pairs lanes whose
// sets are disjoint), then rows 0<->1, 2<->3 and halves by permlane swaps; every lane ends with
// the wave's top-2
__device__ __forceinline__ void wave_top2(uint32_t& m1, uint32_t& m2) {
    top2_dpp<0xB1>(m1, m2);
    top2_dpp<0x4E>(m1, m2);
    top2_dpp<0x141>(m1, m2);
    top2_dpp<0x140>(m1, m2);
    {
        const auto a = __builtin_amdgcn_permlane16_swap(m1, m1, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(m2, m2, false, false);
        m1 = a[0]; m2 = b[0];
        top2_merge(m1, m2, a[1], b[1]);
    }
    {
        const auto a = __builtin_amdgcn_permlane32_swap(m1, m1, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(m2, m2, false, false);
        m1 = a[0]; m2 = b[0];
        top2_merge(m1, m2, a[1], b[1]);
    }
}


// LDS: ST u32[nr] = vMatchedDistance (low 16 bits, 0xFFFF = INT_MAX) | vnMatches21 as a query
// slot (high 16, 0xFFFF none); CL u32[nq] = the rank query q claimed | its rotHist push bin << 16
// (~0u none). vnMatches12 is implied: the claim of q survives iff ST[rank].hi == q at the end (a
// steal only ever replaces it), so the chain never reads a match back.
__global__ __launch_bounds__(256) void k_init_greedy(InitGeom g, float nnratio, int check_orientation,
                                                     const orbhip_kp* __restrict__ kps2, const int* __restrict__ slot,
                                                     const int* __restrict__ qlist, const int* __restrict__ counts,
                                                     const uint32_t* __restrict__ lists, const int* __restrict__ lens,
                                                     const uint32_t* __restrict__ topk, const int* __restrict__ need,
                                                     int32_t* __restrict__ matches12, float* __restrict__ prev,
                                                     int* __restrict__ nmatch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int hist[32], keep[3], cnt;
    const int nq = counts[0], nr = counts[1];
    uint32_t* ST = (uint32_t*)smem;
    uint32_t* CL = ST + nr;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    for (int k = tid; k < nr; k += nt) ST[k] = ~0u;
    for (int q = tid; q < nq; q += nt) CL[q] = ~0u;
    for (int i = tid; i < g.n1; i += nt) matches12[i] = -1;
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) cnt = 0;
    __syncthreads();
    if (tid < 64 && nq > 0) {
        // blocks of 4 queries: lane 16j + e holds entry e of query 4b + j's top-16 (one 256-byte
        // row per block), and lane j < 4 its `need`. A ring of kInitR blocks is in flight; the
        // loads are unconditional (clamped block) so the waits count only the oldest block.
        // vMatchedDistance of a block's entries is read from LDS one block ahead (mdv) and kept
        // current by forwarding (the chain is the only writer, one rank per accepted query): a
        // block's own updates go into its mdv at once and into the next block's at its start.
        const int nb = (nq + 3) >> 2;
        uint32_t tk[kInitR];
        int nd[kInitR], mdv[kInitR];
        auto load = [&](int b, int r) {
            const int bb = min(b, nb - 1);
            tk[r] = topk[(size_t)bb * 64 + lane];
            nd[r] = need[min(4 * bb + (lane & 3), nq - 1)];
        };
        auto rank_of = [&](uint32_t v) { return v == ~0u ? 0 : (int)((v >> 5) & 0xFFFF); };
#pragma unroll
        for (int r = 0; r < kInitR; r++) load(r, r);
        mdv[0] = (int)(ST[rank_of(tk[0])] & 0xFFFF);
        for (int b0 = 0; b0 < nb; b0 += kInitR) {
#pragma unroll
            for (int r = 0; r < kInitR; r++) {
                const int b = b0 + r;
                const int rn = (r + 1) % kInitR;
                mdv[rn] = (int)(ST[rank_of(tk[rn])] & 0xFFFF);   // next block, before this block's writes
                const int rk_c = rank_of(tk[r]), rk_n = rank_of(tk[rn]);
                int upd_rk[4] = {-1, -1, -1, -1}, upd_d[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int q = 4 * b + j;
                    if (q < nq) {
                        const uint32_t v = tk[r];
                        const bool elig = v != ~0u && (int)(v >> 21) < mdv[r];
                        const uint32_t mask = (uint32_t)(__ballot(elig) >> (16 * j)) & 0xFFFFu;
                        const int nq_need = __builtin_amdgcn_readlane(nd[r], j);
                        uint32_t m1 = ~0u, m2 = ~0u;
                        if (nq_need == 0 || (nq_need == 1 && __popc(mask) >= 2)) {
                            // the two smallest eligible entries are among the list's 16 smallest
                            if (mask) m1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16 * j + __ffs(mask) - 1);
                            const uint32_t rest = mask & (mask - 1);
                            if (rest) m2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16 * j + __ffs(rest) - 1);
                        } else {
                            // whole-list scan (fewer than two eligible among the 16, or a lost entry)
                            const int lc = lens[q];
                            const uint32_t* lq = lists + (size_t)q * g.list_cap;
                            for (int e = lane; e < lc; e += 64) {
                                const uint32_t w0 = lq[e];
                                const uint32_t w = (w0 >> 21) < (ST[(w0 >> 5) & 0xFFFF] & 0xFFFF) ? w0 : ~0u;
                                m2 = min(m2, max(m1, w));
                                m1 = min(m1, w);
                            }
                            wave_top2(m1, m2);
                            m1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)m1);
                            m2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)m2);
                        }
                        if (m1 != ~0u) {
                            const int d1 = (int)(m1 >> 21);
                            const int d2 = m2 == ~0u ? INT_MAX : (int)(m2 >> 21);
                            if (d1 <= kThLow && (float)d1 < (float)d2 * nnratio) {
                                const int rk = (int)((m1 >> 5) & 0xFFFF);
                                if (lane == 0) {
                                    CL[q] = (uint32_t)rk | ((m1 & 31) << 16);
                                    ST[rk] = (uint32_t)d1 | ((uint32_t)q << 16);
                                }
                                // forward into this block's registers now, the next block's later
                                mdv[r] = rk_c == rk ? d1 : mdv[r];
                                upd_rk[j] = rk;
                                upd_d[j] = d1;
                                // a wave's LDS operations complete in order: only keep the compiler
                                // from moving later MD reads above these writes
                                asm volatile("" ::: "memory");
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) mdv[rn] = rk_n == upd_rk[j] ? upd_d[j] : mdv[rn];
                load(b + kInitR, r);
            }
        }
    }
    __syncthreads();
    if (check_orientation) {
        for (int q = tid; q < nq; q += nt)
            if (CL[q] != ~0u) atomicAdd(&hist[CL[q] >> 16], 1);   // every push, stolen ones included
        __syncthreads();
        if (tid < 64) three_maxima_wave(hist, keep);   // wave 0 of 256 threads, converged again after the barrier
        __syncthreads();
    }
    int c = 0;
    for (int q = tid; q < nq; q += nt) {
        int rk = CL[q] == ~0u ? -1 : (int)(CL[q] & 0xFFFF);
        if (rk >= 0 && (int)(ST[rk] >> 16) != q) rk = -1;   // stolen by a later query
        if (rk >= 0 && check_orientation) {
            const int b = (int)(CL[q] >> 16);
            if (!rot_kept(b, keep)) rk = -1;
        }
        if (rk >= 0) {
            const int i1 = qlist[q], k = slot[rk];
            matches12[i1] = k;
            prev[2 * i1] = kps2[k].x;
            prev[2 * i1 + 1] = kps2[k].y;
            c++;
        }
    }
    atomicAdd(&cnt, c);
    __syncthreads();
    if (tid == 0) *nmatch = cnt;
}

// ---------------------------------------------------------------------------
// The same greedy pass as a parallel fixed point. Round r recomputes every query's pick from the
// picks of round r - 1: query q's vMatchedDistance of rank k is the smallest distance among the
// earlier queries (j < q) that picked k in round r - 1 (in the sequential pass each later claimant
// is strictly closer, so the last write is the minimum). Query 0 is right in round 0, and a query
// is right once every earlier one was right a round before, so a round that changes nothing ends
// at the sequential result. The claims of a round go to a per-rank table (kInitC slots of
// q << 9 | dist); three tables rotate (read r, fill r + 1, clear r + 2), as in k_proj_round. A
// rank with more than kInitC claimants in one round sets the overflow flag and the host runs the
// chain kernel instead. The 16-lane row of a query holds its 16 smallest entries; the selection
// is the chain's (first two eligible bits, or the whole-list scan reduced within the row).
// flags[0] = overflow, flags[1 + r] = "round r changed a pick".
// ---------------------------------------------------------------------------
constexpr int kInitC = 8;

__device__ __forceinline__ int init_md(const int* __restrict__ cnt, const uint32_t* __restrict__ ent, int rk, int q) {
    const int c = min(cnt[rk], kInitC);
    int md = INT_MAX;
    for (int t = 0; t < c; t++) {
        const uint32_t e = ent[(size_t)rk * kInitC + t];
        md = (int)(e >> 9) < q ? min(md, (int)(e & 511)) : md;
    }
    return md;
}

__global__ __launch_bounds__(256) void k_init_round(InitGeom g, float nnratio, int r, const int* __restrict__ counts,
                                                    const uint32_t* __restrict__ lists, const int* __restrict__ lens,
                                                    const uint32_t* __restrict__ topk, const int* __restrict__ need,
                                                    int* __restrict__ cnt3, uint32_t* __restrict__ ent3,
                                                    uint32_t* __restrict__ pick, int* __restrict__ flags) {
    if (flags[0] || (r > 0 && flags[r] == 0)) return;   // overflow, or converged a round ago
    const int nq = counts[0], nr = counts[1];
    const int* cc = cnt3 + (size_t)(r % 3) * nr;
    const uint32_t* ec = ent3 + (size_t)(r % 3) * nr * kInitC;
    int* cn = cnt3 + (size_t)((r + 1) % 3) * nr;
    uint32_t* en = ent3 + (size_t)((r + 1) % 3) * nr * kInitC;
    int* cz = cnt3 + (size_t)((r + 2) % 3) * nr;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nr; k += gridDim.x * blockDim.x) cz[k] = 0;

    const int lane = threadIdx.x & 63, row = lane >> 4, e = lane & 15;
    const int q = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + row;
    const bool qv = q < nq;
    const uint32_t v = qv ? topk[(size_t)q * kInitK + e] : ~0u;
    const int nd = qv ? need[q] : 0;
    const int md = v != ~0u ? init_md(cc, ec, (int)((v >> 5) & 0xFFFF), q) : INT_MAX;
    const bool elig = v != ~0u && (int)(v >> 21) < md;
    const uint32_t mask = (uint32_t)(__ballot(elig) >> (16 * row)) & 0xFFFFu;
    const uint32_t rest = mask & (mask - 1);
    // first two eligible entries of the row (all lanes shuffle, so no source lane is inactive)
    const uint32_t a = (uint32_t)__shfl((int)v, 16 * row + (mask ? __ffs(mask) - 1 : 0));
    const uint32_t b = (uint32_t)__shfl((int)v, 16 * row + (rest ? __ffs(rest) - 1 : 0));
    const bool full = qv && (nd == 2 || (nd == 1 && __popc(mask) < 2));
    uint32_t f1 = ~0u, f2 = ~0u;
    if (full) {   // whole list, 16 lanes of the row
        const int lc = lens[q];
        const uint32_t* lq = lists + (size_t)q * g.list_cap;
        for (int t = e; t < lc; t += 16) {
            const uint32_t w0 = lq[t];
            const uint32_t w = (int)(w0 >> 21) < init_md(cc, ec, (int)((w0 >> 5) & 0xFFFF), q) ? w0 : ~0u;
            f2 = min(f2, max(f1, w));
            f1 = min(f1, w);
        }
    }
    // top-2 within each 16-lane row (rows that did not scan reduce ~0u)
    top2_dpp<0xB1>(f1, f2);
    top2_dpp<0x4E>(f1, f2);
    top2_dpp<0x141>(f1, f2);
    top2_dpp<0x140>(f1, f2);
    const uint32_t m1 = full ? f1 : (mask ? a : ~0u);
    const uint32_t m2 = full ? f2 : (rest ? b : ~0u);
    uint32_t np = ~0u;
    if (m1 != ~0u) {
        const int d1 = (int)(m1 >> 21);
        const int d2 = m2 == ~0u ? INT_MAX : (int)(m2 >> 21);
        if (d1 <= kThLow && (float)d1 < (float)d2 * nnratio) np = m1;
    }
    if (qv && e == 0) {
        const uint32_t was = r == 0 ? ~0u : pick[q];   // round 0 starts from "no picks"
        if (r == 0 || was != np) pick[q] = np;
        if (was != np) flags[1 + r] = 1;
        if (np != ~0u) {
            const int rk = (int)((np >> 5) & 0xFFFF);
            const int s = atomicAdd(&cn[rk], 1);
            if (s < kInitC) en[(size_t)rk * kInitC + s] = ((uint32_t)q << 9) | (np >> 21);
            else flags[0] = 1;
        }
    }
}

// Applies converged picks: the last claimant of each rank keeps it (the steals), the rotation
// histogram counts every pick, as k_init_greedy. Writes matches12 and prev_out for all of F1 (so
// a finish over a not yet converged round, which the host discards, leaves nothing behind).
__global__ __launch_bounds__(1024) void k_init_finish(InitGeom g, int check_orientation, const orbhip_kp* __restrict__ kps2,
                                                      const int* __restrict__ slot, const int* __restrict__ qlist,
                                                      const int* __restrict__ counts, const uint32_t* __restrict__ pick,
                                                      const float* __restrict__ prev_in, int32_t* __restrict__ matches12,
                                                      float* __restrict__ prev_out, int* __restrict__ nmatch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int hist[32], keep[3], cnt;
    int* owner = (int*)smem;
    const int nq = counts[0], nr = counts[1];
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k = tid; k < nr; k += nt) owner[k] = -1;
    for (int i = tid; i < g.n1; i += nt) {
        matches12[i] = -1;
        prev_out[2 * i] = prev_in[2 * i];
        prev_out[2 * i + 1] = prev_in[2 * i + 1];
    }
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (int q = tid; q < nq; q += nt) {
        const uint32_t p = pick[q];
        if (p != ~0u) {
            atomicMax(&owner[(p >> 5) & 0xFFFF], q);
            if (check_orientation) atomicAdd(&hist[p & 31], 1);
        }
    }
    __syncthreads();
    if (check_orientation) {
        if (tid < 64) three_maxima_wave(hist, keep);   // wave 0 of 1024 threads
        __syncthreads();
    }
    int c = 0;
    for (int q = tid; q < nq; q += nt) {
        const uint32_t p = pick[q];
        int rk = p == ~0u ? -1 : (int)((p >> 5) & 0xFFFF);
        if (rk >= 0 && owner[rk] != q) rk = -1;   // stolen by a later query
        if (rk >= 0 && check_orientation) {
            const int b = (int)(p & 31);
            if (!rot_kept(b, keep)) rk = -1;
        }
        if (rk >= 0) {
            const int i1 = qlist[q], k = slot[rk];
            matches12[i1] = k;
            prev_out[2 * i1] = kps2[k].x;
            prev_out[2 * i1 + 1] = kps2[k].y;
            c++;
        }
    }
    atomicAdd(&cnt, c);
    __syncthreads();
    if (tid == 0) *nmatch = cnt;
}

// The envelope of a call from its sizes (n1 / n2 keypoints, nq0 / nr0 of them on octave 0): ranks and
// query slots fit 16 bits, the chain's state (4 bytes per rank and per query + 16) fits 150 KiB of
// dynamic LDS, the lists hold at most 2^28 entries. Decided before anything is allocated.
struct InitEnvelope {
    size_t lds;     // k_init_greedy's dynamic LDS
    int list_cap;   // entries per query list
    int cap;        // parallel rounds before the chain takes over
};
int init_envelope(int n1, int n2, int nq0, int nr0, InitEnvelope* e) {
    if (n1 < 0 || n2 < 0 || n1 > 65535 || n2 > 65535) return ORBHIP_ERR_ARG;
    e->lds = 4 * (size_t)nr0 + 4 * (size_t)nq0 + 16;
    e->list_cap = std::max(64, (nr0 + 63) & ~63);
    e->cap = std::min(kInitMaxRounds, nq0 + 2);
    if (e->lds > 150 * 1024) return ORBHIP_ERR_UNSUPPORTED;
    if ((size_t)std::max(nq0, 1) * e->list_cap > ((size_t)1 << 28)) return ORBHIP_ERR_UNSUPPORTED;
    return ORBHIP_OK;
}

}  // namespace

// orbhip_test_init_route (host only): out4 = {init_envelope's return code, LDS bytes, list_cap, round cap}
int init_test_route(int n1, int n2, int nq0, int nr0, int32_t* out4) {
    if (!out4 || nq0 < 0 || nr0 < 0 || nq0 > n1 || nr0 > n2) return ORBHIP_ERR_ARG;
    InitEnvelope e{};
    out4[0] = init_envelope(n1, n2, nq0, nr0, &e);
    out4[1] = (int32_t)e.lds; out4[2] = e.list_cap; out4[3] = e.cap;
    return ORBHIP_OK;
}

int init_search(ProjWorkspace* ws, const orbhip_init_frame* F1, const orbhip_init_frame* F2, float* prev_matched,
                int window_size, float nnratio, int check_orientation, int32_t* matches12, hipStream_t st) {
    if (!ws) return ORBHIP_ERR_ARG;
    ws->in_form = -1;   // orbhip_test_init_stats: nothing to report until a form has produced a result
    ws->in_round = ws->in_nq0 = ws->in_nr0 = 0;
    if (!F1 || !F2 || !prev_matched || !matches12 || F1->n < 0 || F2->n < 0 || F1->n > 65535 ||
        F2->n > 65535 || (F1->n && (!F1->kps || !F1->desc)) || (F2->n && (!F2->kps || !F2->desc)) ||
        !(F2->max_x > F2->min_x) || !(F2->max_y > F2->min_y))
        return ORBHIP_ERR_ARG;
    const int n1 = F1->n, n2 = F2->n;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0) return 0;
    // capacity from the octave-0 counts (bounds of the device-side queries / ranks)
    // (octaves are >= 0: ORBextractor levels; a negative octave would disable the level check)
    int nq0 = 0, nr0 = 0;
    for (int i = 0; i < n1; i++) {
        if (F1->kps[i].octave < 0) return ORBHIP_ERR_ARG;
        nq0 += F1->kps[i].octave == 0;
    }
    for (int k = 0; k < n2; k++) nr0 += F2->kps[k].octave == 0;
    InitEnvelope env{};
    if (int rc = init_envelope(n1, n2, nq0, nr0, &env)) return rc;
    const size_t lds = env.lds;
    const int list_cap = env.list_cap;
    // the kernel's static LDS (histogram) comes on top of the dynamic 150 KiB envelope
    static LdsAttrOnce attr;   // per device, thread-safe (dev_attr.h)
    static const void* const fs[] = {(const void*)k_init_greedy, (const void*)k_init_finish};
    HIPOK(attr.ensure(fs, 2, 152 * 1024));
    // uploaded: [F1 keypoints | F1 descriptors | F2 keypoints | F2 descriptors | prev_matched], read
    // back: [matches | counts], then device only: the slots, lists and claim tables of the rounds
    StageLayout lay(256);
    const size_t o_k1 = lay.take(sizeof(orbhip_kp) * n1), o_d1 = lay.take(32 * (size_t)n1);
    const size_t o_k2 = lay.take(sizeof(orbhip_kp) * std::max(n2, 1)), o_d2 = lay.take(32 * (size_t)std::max(n2, 1));
    const size_t o_prev = lay.take(8 * (size_t)n1), o_in_end = lay.total();
    const size_t o_match = lay.take(4 * (size_t)n1), o_cnt = lay.take(16), o_out_end = lay.total();
    const size_t o_slot = lay.take(4 * (size_t)std::max(n2, 1)), o_ql = lay.take(4 * (size_t)n1);
    const size_t o_len = lay.take(4 * ((size_t)n1 + 1)), o_list = lay.take(4 * (size_t)std::max(nq0, 1) * list_cap);
    const size_t o_topk = lay.take(4 * (size_t)kInitK * (((size_t)std::max(nq0, 1) + 3) & ~size_t(3)));
    const size_t o_need = lay.take(4 * (size_t)std::max(nq0, 1));
    const int cap = env.cap;
    const size_t o_cnt3 = lay.take(4 * 3 * (size_t)std::max(nr0, 1));
    const size_t o_ent3 = lay.take(4 * 3 * (size_t)std::max(nr0, 1) * kInitC);
    const size_t o_pick = lay.take(4 * (size_t)std::max(nq0, 1));
    const size_t o_pout = lay.take(8 * (size_t)n1);
    const size_t o_flags = lay.take(4 * ((size_t)cap + 1));
    if (int rc = proj_ws_ensure(ws, lay.total())) return rc;
    ws->in_nq0 = nq0; ws->in_nr0 = nr0;
    ws->in_need_off = o_need; ws->in_need_live = true;
    StageBlock& S = ws->s;
    char* H = (char*)S.h;
    char* D = (char*)S.d;
    put_keyframe(S, o_k1, o_d1, 0, F1->kps, F1->desc, n1);
    put_keyframe(S, o_k2, o_d2, 0, F2->kps, F2->desc, n2);
    S.put(o_prev, prev_matched, 8 * (size_t)n1);
    HIPOK(upload_inputs(S.hd, D, H, o_in_end, st));
    InitGeom g{};
    g.n1 = n1; g.n2 = n2;
    g.minx = F2->min_x; g.maxx = F2->max_x; g.miny = F2->min_y; g.maxy = F2->max_y;
    g.invw = (float)kGridCols / (g.maxx - g.minx);
    g.invh = (float)kGridRows / (g.maxy - g.miny);
    g.r = (float)window_size;
    g.list_cap = list_cap;
    const orbhip_kp* dk1 = (const orbhip_kp*)(D + o_k1);
    const orbhip_kp* dk2 = (const orbhip_kp*)(D + o_k2);
    int* counts = (int*)(D + o_cnt);
    int* flags = (int*)(D + o_flags);
    hipLaunchKernelGGL(k_init_prep, dim3(1), dim3(1024), 0, st, g, dk1, dk2, (int*)(D + o_slot), (int*)(D + o_ql),
                       counts, (int*)(D + o_cnt3), flags, cap + 1);
    hipLaunchKernelGGL(k_init_cands, dim3((unsigned)std::max(1, (nq0 + 3) / 4)), dim3(256), 0, st, g, dk1,
                       (const uint8_t*)(D + o_d1), dk2, (const uint8_t*)(D + o_d2), (const float*)(D + o_prev),
                       (const int*)(D + o_slot), (const int*)(D + o_ql), (const int*)counts, (uint32_t*)(D + o_list),
                       (int*)(D + o_len), (uint32_t*)(D + o_topk), (int*)(D + o_need));
    HIPOK(hipGetLastError());
    // parallel rounds, launched init_ahead at a time with the finish and the read-back behind them
    const int* hflags = (const int*)(H + o_flags);
    const dim3 gq((unsigned)std::max(1, (nq0 + 15) / 16));
    bool done = false;
    const bool chain_only = std::getenv("ORBHIP_INIT_CHAIN") != nullptr;
    int form = chain_only ? 3 : 2, rounds = chain_only ? 0 : cap;   // of the chain, unless the rounds end it
    for (int r = 0; r < cap && !done && !chain_only;) {
        const int R = std::min(ws->init_ahead, cap - r);
        for (int j = 0; j < R; j++)
            hipLaunchKernelGGL(k_init_round, gq, dim3(256), 0, st, g, nnratio, r + j, (const int*)counts,
                               (const uint32_t*)(D + o_list), (const int*)(D + o_len),
                               (const uint32_t*)(D + o_topk), (const int*)(D + o_need), (int*)(D + o_cnt3),
                               (uint32_t*)(D + o_ent3), (uint32_t*)(D + o_pick), flags);
        hipLaunchKernelGGL(k_init_finish, dim3(1), dim3(1024), 4 * (size_t)std::max(nr0, 1), st, g,
                           check_orientation, dk2, (const int*)(D + o_slot), (const int*)(D + o_ql),
                           (const int*)counts, (const uint32_t*)(D + o_pick), (const float*)(D + o_prev),
                           (int32_t*)(D + o_match), (float*)(D + o_pout), counts + 2);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(H + o_match, D + o_match, o_out_end - o_match, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(H + o_pout, D + o_pout, 8 * (size_t)n1, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(H + o_flags, flags, 4 * ((size_t)cap + 1), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (hflags[0]) {   // a rank overflowed its claim slots: the chain decides
            form = 1; rounds = r + R;
            break;
        }
        for (int j = 0; j < R && !done; j++)
            if (hflags[1 + r + j] == 0) {
                done = true;
                form = 0; rounds = r + j;
                ws->init_ahead = std::min(16, std::max(3, r + j + 2));
            }
        r += R;
        if (!done) ws->init_ahead = std::min(16, 2 * ws->init_ahead);
    }
    if (done) {
        std::memcpy(matches12, H + o_match, 4 * (size_t)n1);
        std::memcpy(prev_matched, H + o_pout, 8 * (size_t)n1);
        ws->in_form = form; ws->in_round = rounds;
        return ((int*)(H + o_cnt))[2];
    }
    hipLaunchKernelGGL(k_init_greedy, dim3(1), dim3(256), lds, st, g, nnratio, check_orientation, dk2,
                       (const int*)(D + o_slot), (const int*)(D + o_ql), (const int*)counts,
                       (const uint32_t*)(D + o_list), (const int*)(D + o_len), (const uint32_t*)(D + o_topk),
                       (const int*)(D + o_need), (int32_t*)(D + o_match), (float*)(D + o_prev), counts + 2);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(H + o_prev, D + o_prev, o_out_end - o_prev, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    std::memcpy(matches12, H + o_match, 4 * (size_t)n1);
    std::memcpy(prev_matched, H + o_prev, 8 * (size_t)n1);
    ws->in_form = form; ws->in_round = rounds;
    return ((int*)(H + o_cnt))[2];
}

// orbhip_test_init_stats: the last SearchForInitialization on this workspace (ProjWorkspace::in_*).
// out8 = {form, round, init_ahead, nq0, nr0, queries with need == 1, with need == 2, 0}; the two
// counts come from that call's need[] while the block still holds it (-1 each once another call
// has laid the block out, or when no call got as far as the kernels)
int init_test_stats(ProjWorkspace* ws, int32_t* out8, hipStream_t st) {
    if (!out8) return ORBHIP_ERR_ARG;
    for (int i = 0; i < 8; i++) out8[i] = 0;
    out8[0] = ws ? ws->in_form : -1;
    out8[5] = out8[6] = -1;
    if (!ws) return ORBHIP_OK;
    out8[1] = ws->in_round; out8[2] = ws->init_ahead; out8[3] = ws->in_nq0; out8[4] = ws->in_nr0;
    if (ws->in_form < 0 || !ws->in_need_live) return ORBHIP_OK;
    const size_t nq = (size_t)ws->in_nq0;
    if (ws->in_need_off + 4 * nq > ws->s.dcap || ws->in_need_off + 4 * nq > ws->s.hcap) return ORBHIP_ERR_CAPACITY;
    // the pinned image's need segment is unused by the search itself
    int* hn = (int*)(ws->s.h + ws->in_need_off);
    if (nq) HIPOK(hipMemcpyAsync(hn, ws->s.d + ws->in_need_off, 4 * nq, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    out8[5] = out8[6] = 0;
    for (size_t q = 0; q < nq; q++) out8[5] += hn[q] == 1, out8[6] += hn[q] == 2;
    return ORBHIP_OK;
}

}  // namespace orbhip
