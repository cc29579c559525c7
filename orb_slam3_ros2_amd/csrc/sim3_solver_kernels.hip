// gfx950 Sim3Solver (LoopClosing::DetectCommonRegionsFromBoW): every RANSAC hypothesis of every
// candidate keyframe in one call (DESIGN.md "Sim3Solver"):
//   k_sim3_ransac   one wavefront per (problem, hypothesis), four per work-group. Every lane computes
//                   the hypothesis itself (Horn's closed form on the triple: fp32 in the written
//                   order, the eigenvector of the 4x4 matrix by an fp64 two-sided cyclic Jacobi held
//                   in registers, every index a constant); then the wave walks the correspondences in
//                   64s, a ballot per step is one word of the hypothesis' inlier mask
//   k_sim3_select   one work-group per problem: upstream's sequential "first that converges / best so
//                   far" rule in its order-free form (a min over the hypotheses above the minimum, a
//                   max over (count, h)), the chosen hypothesis' mask as bytes and its 13 floats
// No work-group waits for another; the two launches are ordered by the stream.
#include <hip/hip_runtime.h>

#include <cmath>

#include "geom.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" sim3 solver", x)

namespace orbhip {

constexpr int kSim3MaxN = 8192;      // correspondences per problem
constexpr int kSim3MaxHyp = 4096;    // hypotheses per problem
constexpr int kSim3Sweeps = 6;       // Jacobi sweeps: the measured need + 1 (tests/test_sim3_solver.py)
constexpr int kSim3HypFloats = 13;   // (s, R row-major, t)
constexpr int kSim3Waves = 4;        // hypotheses per work-group
constexpr int kSim3SelThreads = 256;

struct Sim3Dev {                     // one problem in the call's staging block (device pointers)
    const float *X1, *X2, *e1, *e2;  // n x 3, n x 3, n, n
    const int32_t* tri;              // H x 3
    int32_t* n_inl;                  // H
    float* hyp;                      // H x 13
    unsigned long long* mask;        // H x words
    int32_t* head;                   // [sel 13 floats | converged | best | pad]
    uint8_t* inl;                    // n
    float cam1[4], cam2[4];          // fx, fy, cx, cy
    int n, H, words, fix_scale, min_inliers, pad;
};

// one rotation of the two-sided Jacobi on the symmetric A (4x4, the upper triangle is kept:
// A[4 r + c], r <= c), its eigenvectors accumulated in the columns of V. The rotation is
// tri_jacobi_pair's: zeta, t = +-1 / (|zeta| + sqrt(1 + zeta^2)), c, s; nothing when A[P][Q] == 0
template <int P, int Q>
__device__ __forceinline__ void sim3_jacobi_pair(double (&A)[16], double (&V)[16]) {
    const double g = A[4 * P + Q];
    if (g == 0.0) return;
    const double zeta = (A[5 * Q] - A[5 * P]) / (2.0 * g);
    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    if (zeta < 0.0) t = -t;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    A[5 * P] = A[5 * P] - t * g;
    A[5 * Q] = A[5 * Q] + t * g;
    A[4 * P + Q] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r != P && r != Q) {
            const int ip = r < P ? 4 * r + P : 4 * P + r, iq = r < Q ? 4 * r + Q : 4 * Q + r;
            const double x = A[ip], y = A[iq];
            A[ip] = c * x - s * y;
            A[iq] = s * x + c * y;
        }
        const double vx = V[4 * r + P], vy = V[4 * r + Q];
        V[4 * r + P] = c * vx - s * vy;
        V[4 * r + Q] = s * vx + c * vy;
    }
}

struct Sim3Hyp { float s, R[9], t[3], sR[9], Ri[9], ti[3]; };

// ComputeSim3 on the triple (a, b, c); every operation rounded once, in this order
__device__ __forceinline__ void sim3_hypothesis(const float* __restrict__ X1, const float* __restrict__ X2, int a,
                                                int b, int c, bool fix_scale, Sim3Hyp& h) {
    const int idx[3] = {a, b, c};
    float P1[3][3], P2[3][3], O1[3], O2[3];   // [k][j]: point k, coordinate j
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            P1[k][j] = X1[3 * idx[k] + j];
            P2[k][j] = X2[3 * idx[k] + j];
        }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        O1[j] = ((P1[0][j] + P1[1][j]) + P1[2][j]) / 3.0f;
        O2[j] = ((P2[0][j] + P2[1][j]) + P2[2][j]) / 3.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            P1[k][j] = P1[k][j] - O1[j];
            P2[k][j] = P2[k][j] - O2[j];
        }
    float M[3][3];   // M = Pr2 Pr1^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (P2[0][i] * P1[0][j] + P2[1][i] * P1[1][j]) + P2[2][i] * P1[2][j];
    double A[16], V[16];
    A[0] = (double)((M[0][0] + M[1][1]) + M[2][2]);
    A[1] = (double)(M[1][2] - M[2][1]);
    A[2] = (double)(M[2][0] - M[0][2]);
    A[3] = (double)(M[0][1] - M[1][0]);
    A[5] = (double)((M[0][0] - M[1][1]) - M[2][2]);
    A[6] = (double)(M[0][1] + M[1][0]);
    A[7] = (double)(M[2][0] + M[0][2]);
    A[10] = (double)((-M[0][0] + M[1][1]) - M[2][2]);
    A[11] = (double)(M[1][2] + M[2][1]);
    A[15] = (double)((-M[0][0] - M[1][1]) + M[2][2]);
#pragma unroll
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSim3Sweeps; sweep++) {
        sim3_jacobi_pair<0, 1>(A, V);
        sim3_jacobi_pair<0, 2>(A, V);
        sim3_jacobi_pair<0, 3>(A, V);
        sim3_jacobi_pair<1, 2>(A, V);
        sim3_jacobi_pair<1, 3>(A, V);
        sim3_jacobi_pair<2, 3>(A, V);
    }
    // the column of the largest eigenvalue (in value: N is traceless), the lowest column among equals
    double best = A[0], w = V[0], x = V[4], y = V[8], z = V[12];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (A[5 * k] > best) { best = A[5 * k]; w = V[k]; x = V[4 + k]; y = V[8 + k]; z = V[12 + k]; }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    const float q[4] = {(float)(x / nrm), (float)(y / nrm), (float)(z / nrm), (float)(w / nrm)};
    quat_to_matrix(q, h.R);
    float s = 1.0f;
    if (!fix_scale) {
        float nom = 0.f, den = 0.f;   // column-major over the 3 x 3 matrices: column k, row i
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float p3 = (h.R[3 * i] * P2[k][0] + h.R[3 * i + 1] * P2[k][1]) + h.R[3 * i + 2] * P2[k][2];
                const float a1 = P1[k][i] * p3, a2 = p3 * p3;
                nom = (k == 0 && i == 0) ? a1 : nom + a1;
                den = (k == 0 && i == 0) ? a2 : den + a2;
            }
        s = nom / den;
    }
    h.s = s;
#pragma unroll
    for (int i = 0; i < 9; i++) h.sR[i] = s * h.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
        h.t[i] = O1[i] - ((h.sR[3 * i] * O2[0] + h.sR[3 * i + 1] * O2[1]) + h.sR[3 * i + 2] * O2[2]);
    const float sinv = 1.0f / s;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) h.Ri[3 * i + j] = sinv * h.R[3 * j + i];
#pragma unroll
    for (int i = 0; i < 3; i++)
        h.ti[i] = -((h.Ri[3 * i] * h.t[0] + h.Ri[3 * i + 1] * h.t[1]) + h.Ri[3 * i + 2] * h.t[2]);
}

// |project(cam, Y) - project(cam, A X + t)|^2 as CheckInliers forms it (no depth test upstream;
// the square is the same whichever way round the difference is taken)
__device__ __forceinline__ float sim3_reproj_err(float fx, float fy, float cx, float cy, const float (&A)[9],
                                                 const float (&t)[3], float x, float y, float z, float px, float py,
                                                 float pz) {
    const float X = ((A[0] * x + A[1] * y) + A[2] * z) + t[0];
    const float Y = ((A[3] * x + A[4] * y) + A[5] * z) + t[1];
    const float Z = ((A[6] * x + A[7] * y) + A[8] * z) + t[2];
    const float qu = (fx * X) / Z + cx, qv = (fy * Y) / Z + cy;
    const float pu = (fx * px) / pz + cx, pv = (fy * py) / pz + cy;
    const float du = pu - qu, dv = pv - qv;
    return du * du + dv * dv;
}

__global__ __launch_bounds__(64 * kSim3Waves) void k_sim3_ransac(const Sim3Dev* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * kSim3Waves + (threadIdx.x >> 6);   // wave-uniform
    const Sim3Dev& P = probs[blockIdx.y];
    if (h >= P.H) return;
    const float* __restrict__ X1 = P.X1;
    const float* __restrict__ X2 = P.X2;
    const float* __restrict__ E1 = P.e1;
    const float* __restrict__ E2 = P.e2;
    const float fx1 = P.cam1[0], fy1 = P.cam1[1], cx1 = P.cam1[2], cy1 = P.cam1[3];
    const float fx2 = P.cam2[0], fy2 = P.cam2[1], cx2 = P.cam2[2], cy2 = P.cam2[3];
    const int n = P.n;
    unsigned long long* __restrict__ mask = P.mask + (size_t)h * P.words;
    int32_t* __restrict__ n_inl = P.n_inl;
    float* __restrict__ out = P.hyp + (size_t)h * kSim3HypFloats;
    Sim3Hyp hy;
    sim3_hypothesis(X1, X2, P.tri[3 * h], P.tri[3 * h + 1], P.tri[3 * h + 2], P.fix_scale != 0, hy);
    int cnt = 0;
    for (int i0 = 0, w = 0; i0 < n; i0 += 64, w++) {
        const int i = i0 + lane;
        bool ok = false;
        if (i < n) {
            const float x1 = X1[3 * i], y1 = X1[3 * i + 1], z1 = X1[3 * i + 2];
            const float x2 = X2[3 * i], y2 = X2[3 * i + 1], z2 = X2[3 * i + 2];
            const float e1 = sim3_reproj_err(fx1, fy1, cx1, cy1, hy.sR, hy.t, x2, y2, z2, x1, y1, z1);
            const float e2 = sim3_reproj_err(fx2, fy2, cx2, cy2, hy.Ri, hy.ti, x1, y1, z1, x2, y2, z2);
            ok = e1 < E1[i] && e2 < E2[i];
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) mask[w] = m;
        cnt += __popcll(m);
    }
    if (lane == 0) {
        n_inl[h] = cnt;
        out[0] = hy.s;
#pragma unroll
        for (int i = 0; i < 9; i++) out[1 + i] = hy.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) out[10 + i] = hy.t[i];
    }
}

__global__ __launch_bounds__(kSim3SelThreads) void k_sim3_select(const Sim3Dev* __restrict__ probs) {
    __shared__ int s_conv[kSim3SelThreads / 64];
    __shared__ unsigned long long s_best[kSim3SelThreads / 64];
    __shared__ int s_pick;
    const Sim3Dev& P = probs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int conv = 0x7fffffff;               // the first h above the minimum
    unsigned long long best = 0;         // the largest (count, h): the last h of the largest count
    for (int h = tid; h < P.H; h += kSim3SelThreads) {
        const int c = P.n_inl[h];
        if (c > P.min_inliers) conv = min(conv, h);
        const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)h;
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        conv = min(conv, __shfl_xor(conv, o));
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    if (lane == 0) { s_conv[wid] = conv; s_best[wid] = best; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kSim3SelThreads / 64; k++) {
            conv = min(conv, s_conv[k]);
            best = s_best[k] > best ? s_best[k] : best;
        }
        const int converged = conv == 0x7fffffff ? -1 : conv;
        const int b = converged >= 0 ? converged : (int)(best & 0xffffffffull);
        P.head[kSim3HypFloats] = converged;
        P.head[kSim3HypFloats + 1] = b;
        s_pick = b;
    }
    __syncthreads();
    const int pick = s_pick;
    if (tid < kSim3HypFloats) ((float*)P.head)[tid] = P.hyp[(size_t)pick * kSim3HypFloats + tid];
    const unsigned long long* __restrict__ mask = P.mask + (size_t)pick * P.words;
    for (int i = tid; i < P.n; i += kSim3SelThreads) P.inl[i] = (uint8_t)((mask[i >> 6] >> (i & 63)) & 1ull);
}

// ---- host ----
static int sim3_check(const orbhip_sim3_problem& p, const orbhip_sim3_result& r) {
    if (p.n < 3 || p.n_hyp < 1 || p.min_inliers < 0) return ORBHIP_ERR_ARG;
    if (!p.X1 || !p.X2 || !p.max_err1 || !p.max_err2 || !p.triples || !r.n_inliers) return ORBHIP_ERR_ARG;
    for (int k = 0; k < 2; k++) {
        const float* cam = k ? p.cam2 : p.cam1;
        if (!(cam[0] > 0.0f) || !(cam[1] > 0.0f) || !std::isfinite(cam[0]) || !std::isfinite(cam[1]))
            return ORBHIP_ERR_ARG;
    }
    if (p.n > kSim3MaxN || p.n_hyp > kSim3MaxHyp) return ORBHIP_ERR_UNSUPPORTED;
    for (int h = 0; h < p.n_hyp; h++) {   // an index past the points would be read on the device
        const int32_t a = p.triples[3 * h], b = p.triples[3 * h + 1], c = p.triples[3 * h + 2];
        if ((unsigned)a >= (unsigned)p.n || (unsigned)b >= (unsigned)p.n || (unsigned)c >= (unsigned)p.n || a == b ||
            a == c || b == c)
            return ORBHIP_ERR_ARG;
    }
    return ORBHIP_OK;
}

int sim3_solve_batch(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_sim3_problem* probs, int B,
                     orbhip_sim3_result* res) {
    if (B < 0) return ORBHIP_ERR_ARG;
    if (B == 0) return 0;
    if (!probs || !res) return ORBHIP_ERR_ARG;
    if (B > kSim3MaxBatch) return ORBHIP_ERR_UNSUPPORTED;
    for (int b = 0; b < B; b++)
        if (const int rc = sim3_check(probs[b], res[b])) return rc;
    // one block, the same layout on the host (pinned) and the device:
    // [problems B | per problem: X1 X2 max_err1 max_err2 triples] uploaded; device only [masks];
    // read back as far as the caller asks: [heads B x 16 | n_inliers | inliers | hyp]
    struct Off { size_t X1, X2, e1, e2, tri, mask, n_inl, inl, hyp; };
    Off off[kSim3MaxBatch];
    StageLayout lay(16);
    const size_t o_probs = lay.take((size_t)B * sizeof(Sim3Dev));
    int max_h = 0;
    bool want_hyp = false;
    for (int b = 0; b < B; b++) {
        const size_t n = (size_t)probs[b].n, H = (size_t)probs[b].n_hyp;
        off[b].X1 = lay.take(n * 12); off[b].X2 = lay.take(n * 12);
        off[b].e1 = lay.take(n * 4); off[b].e2 = lay.take(n * 4);
        off[b].tri = lay.take(H * 12);
        max_h = probs[b].n_hyp > max_h ? probs[b].n_hyp : max_h;
        want_hyp = want_hyp || res[b].hyp;
    }
    const size_t up_bytes = lay.total();
    for (int b = 0; b < B; b++)
        off[b].mask = lay.take((size_t)probs[b].n_hyp * (((size_t)probs[b].n + 63) / 64) * 8);
    const size_t o_head = lay.take((size_t)B * 64);
    for (int b = 0; b < B; b++) off[b].n_inl = lay.take((size_t)probs[b].n_hyp * 4);
    for (int b = 0; b < B; b++) off[b].inl = lay.take((size_t)probs[b].n);
    size_t back_end = lay.total();
    for (int b = 0; b < B; b++) off[b].hyp = lay.take((size_t)probs[b].n_hyp * kSim3HypFloats * 4);
    if (want_hyp) back_end = lay.total();
    const size_t back_bytes = back_end - o_head;
    HIPOK(S.ensure(lay.total(), up_bytes + back_bytes + 16));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    Sim3Dev* dev = (Sim3Dev*)(h + o_probs);
    for (int b = 0; b < B; b++) {
        const orbhip_sim3_problem& p = probs[b];
        const size_t n = (size_t)p.n, H = (size_t)p.n_hyp;
        S.put(off[b].X1, p.X1, n * 12);
        S.put(off[b].X2, p.X2, n * 12);
        S.put(off[b].e1, p.max_err1, n * 4);
        S.put(off[b].e2, p.max_err2, n * 4);
        S.put(off[b].tri, p.triples, H * 12);
        Sim3Dev& v = dev[b];
        v.X1 = (const float*)(d + off[b].X1); v.X2 = (const float*)(d + off[b].X2);
        v.e1 = (const float*)(d + off[b].e1); v.e2 = (const float*)(d + off[b].e2);
        v.tri = (const int32_t*)(d + off[b].tri);
        v.n_inl = (int32_t*)(d + off[b].n_inl);
        v.hyp = (float*)(d + off[b].hyp);
        v.mask = (unsigned long long*)(d + off[b].mask);
        v.head = (int32_t*)(d + o_head + (size_t)b * 64);
        v.inl = d + off[b].inl;
        for (int k = 0; k < 4; k++) { v.cam1[k] = p.cam1[k]; v.cam2[k] = p.cam2[k]; }
        v.n = p.n; v.H = p.n_hyp; v.words = (p.n + 63) / 64;
        v.fix_scale = p.fix_scale; v.min_inliers = p.min_inliers; v.pad = 0;
    }
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    {
        const StageScope scope(timer);
        timer.begin(11, st);
        ORBHIP_LAUNCH(k_sim3_ransac, dim3((unsigned)((max_h + kSim3Waves - 1) / kSim3Waves), (unsigned)B),
                      dim3(64 * kSim3Waves), 0, st, (const Sim3Dev*)(d + o_probs));
        ORBHIP_LAUNCH(k_sim3_select, dim3((unsigned)B), dim3(kSim3SelThreads), 0, st, (const Sim3Dev*)(d + o_probs));
        timer.end(11, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + o_head, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    auto back = [&](size_t o) { return hb + (o - o_head); };
    int nconv = 0;
    for (int b = 0; b < B; b++) {   // nothing is written before every problem's head is known to be sane
        const int32_t* head = (const int32_t*)back(o_head + (size_t)b * 64);
        const int32_t conv = head[kSim3HypFloats], best = head[kSim3HypFloats + 1];
        if (conv < -1 || conv >= probs[b].n_hyp || (unsigned)best >= (unsigned)probs[b].n_hyp) return ORBHIP_ERR_DEVICE;
    }
    for (int b = 0; b < B; b++) {
        const size_t n = (size_t)probs[b].n, H = (size_t)probs[b].n_hyp;
        const int32_t* head = (const int32_t*)back(o_head + (size_t)b * 64);
        std::memcpy(res[b].sel, head, kSim3HypFloats * 4);
        res[b].converged = head[kSim3HypFloats];
        res[b].best = head[kSim3HypFloats + 1];
        std::memcpy(res[b].n_inliers, back(off[b].n_inl), H * 4);
        if (res[b].inliers) std::memcpy(res[b].inliers, back(off[b].inl), n);
        if (res[b].hyp) std::memcpy(res[b].hyp, back(off[b].hyp), H * kSim3HypFloats * 4);
        nconv += res[b].converged >= 0;
    }
    return nconv;
}

}  // namespace orbhip
