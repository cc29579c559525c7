// Frame::ComputeStereoMatches (U:src/Frame.cc) for rectified pairs, DESIGN.md section 4 "Stereo".
// k_stereo_match: one wave per left keypoint. The wave tests every right keypoint of the pair
// (row band, octave, disparity range), computes the Hamming distance of the survivors and
// reduces (distance << 16 | iR), which gives upstream's winner (minimum distance, lowest iR)
// in any order. The same wave then stages the left 11x11 patch and the right 11x21 strip of the
// left keypoint's level in LDS, forms the eleven SADs and applies the parabola and the gates.
// k_stereo_median: one work-group per pair finds the SAD of rank size / 2 by two 256-bin
// histograms (a SAD is below 2^16) and removes the matches at or above 2.1 x that median.
// Integer arithmetic throughout except the single fp32 operations the rule names; the division is
// the correctly rounded one (no fast-math, no contraction).
#include <hip/hip_runtime.h>

#include "stereo.h"

namespace orbhip {
namespace {

constexpr int kW = 5, kL = 5;                    // w, L of the rule
constexpr int kPw = 2 * kW + 1;                  // 11: patch edge
constexpr int kSw = 2 * (kL + kW) + 1;           // 21: right strip width
constexpr int kNs = 2 * kL + 1;                  // 11 SADs
constexpr int kThHigh = 100, kThOrbDist = 75;    // TH_HIGH, (TH_HIGH + TH_LOW) / 2
constexpr int kWaves = 4;                        // left keypoints per work-group

__device__ __forceinline__ const uint8_t* level_ptr(const StereoArgs& a, const ExtractPlan* __restrict__ P, int f,
                                                    int l, int* pitch) {
    if (l == 0) {
        *pitch = a.stride;
        return a.img + (int64_t)f * a.fstride;
    }
    *pitch = P->lv[l].pitch;
    return a.pyr + (int64_t)f * P->pyr_bytes + P->lv[l].pyr_off;
}

__global__ __launch_bounds__(64 * kWaves) void k_stereo_match(StereoArgs a) {
    __shared__ uint8_t s_left[kWaves][kPw * kPw + 7];
    __shared__ uint8_t s_right[kWaves][kPw * kSw + 1];
    __shared__ int s_sad[kWaves][kNs + 1];
    const ExtractPlan* __restrict__ P = a.d_plan;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = blockIdx.y, fl = 2 * p, fr = 2 * p + 1;
    const int nl = min(max(a.n[fl], 0), a.cap), nr = min(max(a.n[fr], 0), min(a.cap, kStereoMaxKp));
    const int iL = blockIdx.x * kWaves + wv;
    const bool live = iL < nl;   // wave-uniform; dead waves only keep the barriers
    const int nlev = P->n_levels, rows = P->lv[0].h;

    int st = 0, best_r = -1, octL = 0;
    float uL = 0.f;
    int suL = 0, svL = 0, suR0 = 0;
    if (lane < kNs + 1) s_sad[wv][lane] = 0;
    if (live) {
        const orbhip_kp kl = a.kps[(int64_t)fl * a.cap + iL];
        octL = kl.octave;
        uL = kl.x;
        const float vL = kl.y;
        if (octL < 0 || octL >= nlev) {
            st = 9;
        } else {
            const int row = (int)vL;
            const bool row_ok = row >= 0 && row < rows;
            const float maxD = a.bf / a.b;   // mbf / minZ, minZ = mb
            const float minU = uL - maxD, maxU = uL - 0.0f;
            const uint32_t* dl = (const uint32_t*)(a.desc + ((int64_t)fl * a.cap + iL) * 32);
            uint32_t d0[8];
#pragma unroll
            for (int k = 0; k < 8; k++) d0[k] = dl[k];
            bool any_row = false;
            uint32_t key = ((uint32_t)kThHigh << 16) | 0xFFFFu;
            const orbhip_kp* kr = a.kps + (int64_t)fr * a.cap;
            const uint8_t* dr = a.desc + (int64_t)fr * a.cap * 32;
            for (int iR = lane; iR < nr; iR += 64) {
                const int oR = kr[iR].octave;
                if (oR < 0 || oR >= nlev || !row_ok) continue;
                const float xR = kr[iR].x, yR = kr[iR].y;
                const float r = 2.0f * P->lv[oR].scale;
                const int lo = max((int)floorf(yR - r), 0), hi = min((int)ceilf(yR + r), rows - 1);
                if (row < lo || row > hi) continue;
                any_row = true;
                if (oR < octL - 1 || oR > octL + 1) continue;
                if (!(xR >= minU && xR <= maxU)) continue;
                const uint32_t* d1 = (const uint32_t*)(dr + (int64_t)iR * 32);
                int dist = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) dist += __popc(d0[k] ^ d1[k]);
                if (dist < kThHigh) key = min(key, ((uint32_t)dist << 16) | (uint32_t)iR);
            }
            any_row = __ballot(any_row) != 0ull;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, m, 64));
            const int best_dist = (int)(key >> 16);
            if (!any_row || maxU < 0.0f) {
                st = 2;
            } else {
                if (best_dist < kThHigh) best_r = (int)(key & 0xFFFFu);
                if (best_dist >= kThOrbDist) st = 3;
            }
            if (st == 0) {
                const float uR0 = kr[best_r].x;
                const float inv = 1.0f / P->lv[octL].scale;   // mvInvScaleFactors[octL]
                suL = (int)roundf(uL * inv);
                svL = (int)roundf(vL * inv);
                suR0 = (int)roundf(uR0 * inv);
                const int wl = P->lv[octL].w, hl = P->lv[octL].h;
                // iniu = scaleduR0 + L - w < 0 || endu = scaleduR0 + L + w + 1 >= cols
                if (suR0 < 0 || suR0 >= wl - (kL + kW + 1)) st = 4;
                // the guard: both windows inside the level, by arithmetic, before any pixel is loaded
                else if (suL < kW || suL >= wl - kW || svL < kW || svL >= hl - kW || suR0 < kL + kW ||
                         suR0 >= wl - (kL + kW))
                    st = 9;
            }
        }
    }
    const bool sadp = live && st == 0;
    if (sadp) {
        int pl, pr;
        const uint8_t* Lp = level_ptr(a, P, fl, octL, &pl);
        const uint8_t* Rp = level_ptr(a, P, fr, octL, &pr);
        for (int i = lane; i < kPw * kPw + kPw * kSw; i += 64) {
            if (i < kPw * kPw) {
                const int r = i / kPw, c = i - r * kPw;
                s_left[wv][i] = Lp[(int64_t)(svL - kW + r) * pl + (suL - kW + c)];
            } else {
                const int j = i - kPw * kPw, r = j / kSw, c = j - r * kSw;
                s_right[wv][j] = Rp[(int64_t)(svL - kW + r) * pr + (suR0 - kL - kW + c)];
            }
        }
    }
    __syncthreads();
    if (sadp) {
        const int lc = a.center_patch ? (int)s_left[wv][kW * kPw + kW] : 0;
        for (int i = lane; i < kNs * kPw; i += 64) {
            const int inc = i / kPw, r = i - inc * kPw;
            const int rc = a.center_patch ? (int)s_right[wv][kW * kSw + inc + kW] : 0;
            int s = 0;
#pragma unroll
            for (int c = 0; c < kPw; c++)
                s += abs(((int)s_left[wv][r * kPw + c] - lc) - ((int)s_right[wv][r * kSw + inc + c] - rc));
            atomicAdd(&s_sad[wv][inc], s);
        }
    }
    __syncthreads();
    if (!live) return;
    float u_right = -1.0f, depth = -1.0f;
    int best_sad = -1;
    if (sadp) {
        int bi = 0;
        best_sad = s_sad[wv][0];
        for (int k = 1; k < kNs; k++) {
            const int d = s_sad[wv][k];
            if (d < best_sad) { best_sad = d; bi = k; }
        }
        const int best_inc = bi - kL;
        if (bi == 0 || bi == kNs - 1) {
            st = 5;
        } else {
            const float d1 = (float)s_sad[wv][bi - 1], d2 = (float)s_sad[wv][bi], d3 = (float)s_sad[wv][bi + 1];
            const float deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
            if (deltaR < -1.0f || deltaR > 1.0f) {
                st = 6;
            } else {
                float bestuR = P->lv[octL].scale * ((float)suR0 + (float)best_inc + deltaR);
                float disparity = uL - bestuR;
                const float maxD = a.bf / a.b;
                if (disparity >= 0.0f && disparity < maxD) {
                    if (disparity <= 0.0f) {
                        disparity = 0.01f;
                        bestuR = (float)((double)uL - 0.01);
                    }
                    depth = a.bf / disparity;
                    u_right = bestuR;
                    st = 1;
                } else {
                    st = 7;
                }
            }
        }
    }
    if (lane == 0) {
        const int64_t o = (int64_t)p * a.cap + iL;
        a.u_right[o] = u_right;
        a.depth[o] = depth;
        a.status[o] = st;
        a.sad[o] = best_sad;
        if (a.best_r) a.best_r[o] = best_r;
    }
}

__global__ __launch_bounds__(1024) void k_stereo_median(StereoArgs a) {
    __shared__ int hist[256];
    __shared__ int s_sel, s_rank, s_count;
    const int p = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int nl = min(max(a.n[2 * p], 0), a.cap);
    int32_t* st = a.status + (int64_t)p * a.cap;
    const int32_t* sad = a.sad + (int64_t)p * a.cap;
    // pass 0: the high byte of every accepted SAD; pass 1: the low byte inside the bin of the rank
    for (int pass = 0; pass < 2; pass++) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < nl; i += nt)
            if (st[i] == 1) {
                const int s = sad[i];
                if (pass == 0) atomicAdd(&hist[(s >> 8) & 255], 1);
                else if (((s >> 8) & 255) == s_sel) atomicAdd(&hist[s & 255], 1);
            }
        __syncthreads();
        if (tid == 0) {
            int rank;
            if (pass == 0) {
                int total = 0;
                for (int k = 0; k < 256; k++) total += hist[k];
                s_count = total;
                rank = total / 2;   // vDistIdx[size / 2]
            } else {
                rank = s_rank;
            }
            int k = 0, cum = 0;
            while (k < 255 && cum + hist[k] <= rank) cum += hist[k++];
            s_rank = rank - cum;
            s_sel = pass == 0 ? k : ((s_sel << 8) | k);
        }
        __syncthreads();
    }
    const int total = s_count;
    const float median = (float)s_sel;
    const float thDist = (1.5f * 1.4f) * median;
    __syncthreads();
    if (tid == 0) s_count = 0;
    __syncthreads();
    int kept = 0;
    for (int i = tid; i < nl; i += nt) {
        int s = st[i];
        if (s == 1 && total > 0) {
            if ((float)sad[i] >= thDist) {
                s = 8;
                st[i] = s;
                a.u_right[(int64_t)p * a.cap + i] = -1.0f;
                a.depth[(int64_t)p * a.cap + i] = -1.0f;
            } else {
                kept++;
            }
        }
        if (a.status_out) a.status_out[(int64_t)p * a.cap + i] = s;
    }
    if (kept) atomicAdd(&s_count, kept);
    __syncthreads();
    if (tid == 0) a.n_stereo[p] = s_count;
}

}  // namespace

void launch_stereo(const StereoArgs& a, hipStream_t st) {
    if (a.P <= 0 || a.cap <= 0) return;
    hipLaunchKernelGGL(k_stereo_match, dim3((a.cap + kWaves - 1) / kWaves, a.P), dim3(64 * kWaves), 0, st, a);
    hipLaunchKernelGGL(k_stereo_median, dim3(a.P), dim3(1024), 0, st, a);
}

void launch_stereo_median(const StereoArgs& a, hipStream_t st) {
    if (a.P <= 0 || a.cap <= 0) return;
    hipLaunchKernelGGL(k_stereo_median, dim3(a.P), dim3(1024), 0, st, a);
}

}  // namespace orbhip
