// Sim3 refinement of a loop candidate: U:src/Optimizer.cc::Optimizer::OptimizeSim3, batched: ONE
// WAVEFRONT GROUP PER PROBLEM runs the whole reference procedure on the device, with no host round
// trip between the rounds (the scheme of pose_opt.hip, restated for one 7-dof vertex):
//   optimize(5) of g2o's Levenberg with Huber (float)sqrt(th2); pairs whose e12 or e21 chi2 (of the
//   last computeActiveErrors that saw the edge) exceeds th2 are removed, the kernels dropped; fewer
//   than 10 pairs left: return 0 with the input S12; optimize(nBad > 0 ? 10 : 5) from a fresh
//   lambda0; pairs whose recomputed chi2 exceeds th2 are cleared, the others counted.
// VertexSim3Expmap (U:Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h): estimate = (q, t, s),
// oplus(u) = Sim3(u) * estimate with u[6] = 0 under fix_scale. EdgeSim3ProjectXYZ: e12 = obs1 -
// cam1.project(S.map(X2c)); EdgeInverseSim3ProjectXYZ: e21 = obs2 - cam2.project(S^-1.map(X1c)).
// Neither edge has an analytic Jacobian: g2o's central differences (U:Thirdparty/g2o/g2o/core/
// base_binary_edge.hpp), column d = (e(oplus(+1e-9 e_d)) - e(oplus(-1e-9 e_d))) / 2e-9. The 14
// perturbed estimates and their inverses are the same for every edge: lanes 0..13 compute one each
// per linearisation and leave them in LDS, every edge maps its two points through them.
// The 7x7 system (H + lambda I) x = b is solved redundantly in every lane (dense LDL^T); edge sums
// are fixed-order LDS reductions (partials -> strip sums -> totals, 18 sums at a time) with the same
// bits in every lane, the per-trial chi2 a DPP/permlane wave sum then the W wave sums in order.
// Every operation is fp64 in the order tests/sim3_opt_numpy.py writes it.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/orbhip.h"
#include "ba_se3.h"
#include "orbhip_kernels.h"
#include "sim3_dev.h"
#include "sim3_opt.h"
#include "stage.h"
#include "wave_f64.h"

#define HIPOK(x) ORBHIP_HIPOK(" sim3opt", x)

namespace orbhip {

namespace {

constexpr int kAcc = 36;     // 28 upper-triangle H + 7 b + chi2
constexpr int kChunk = 18;   // sums reduced per pass of the partial table
constexpr int kPert = 14 * 16;   // 14 perturbed estimates, each (S, S^-1) as 2 x 8 doubles

// e = obs - cam.project(S.map(X)); project = (x / z fx + cx, y / z fy + cy)
__device__ __forceinline__ void proj_err(const S3& S, const double* X, const double* obs, const double* cam, double& e0,
                                         double& e1) {
    double x, y, z;
    qrot(S.q, X[0], X[1], X[2], x, y, z);
    x = S.s * x + S.tx; y = S.s * y + S.ty; z = S.s * z + S.tz;
    e0 = obs[0] - (x / z * cam[0] + cam[2]);
    e1 = obs[1] - (y / z * cam[1] + cam[3]);
}

// a pair record's floats as the doubles the edges compute with (by value: no address of a record
// held in registers is ever taken)
struct PairD {
    double X1[3], X2[3], o1[2], o2[2], i1, i2;
    __device__ __forceinline__ explicit PairD(const Sim3OptEdge& E)
        : X1{(double)E.f[0], (double)E.f[1], (double)E.f[2]}, X2{(double)E.f[3], (double)E.f[4], (double)E.f[5]},
          o1{(double)E.f[6], (double)E.f[7]}, o2{(double)E.f[8], (double)E.f[9]}, i1((double)E.f[10]), i2((double)E.f[11]) {}
};

__device__ __forceinline__ void huber(double chi2, double delta, bool robust, double& rho0, double& rho1) {
    rho0 = chi2; rho1 = 1.0;
    if (robust) {
        const double dsqr = delta * delta;
        if (chi2 > dsqr) {
            const double sq = sqrt(chi2);
            rho0 = 2 * sq * delta - dsqr;
            rho1 = delta / sq;
        }
    }
}

// The W wavefronts that run one problem, and their LDS: partial table [kChunk][RS], strip sums
// [kChunk][S], totals [40], wave sums [2][W] (double-buffered), the perturbed estimates [kPert], the estimate and the cameras [24].
template <int W>
struct Sim3Group {
    static constexpr int T = 64 * W;
    static constexpr int S = W == 1 ? 2 : 8;
    static constexpr int RS = T + S;   // row stride: the S-lane groups of the strip pass hit distinct banks
    static constexpr int kTot = kChunk * RS + kChunk * S;
    static constexpr int kDoubles = kTot + 40 + 2 * W + kPert + 24;
    double* L;
    int tid, par = 0;
    __device__ __forceinline__ void sync() const {
        if constexpr (W == 1) wave_lds_sync();
        else __syncthreads();
    }
    __device__ __forceinline__ double* pert() const { return L + kTot + 40 + 2 * W; }
    // the estimate, its inverse, cam1, cam2: what every pair reads and no pair changes
    __device__ __forceinline__ double* uni() const { return pert() + kPert; }
    // acc[k] <- sum over the group's threads, same bits everywhere
    __device__ __forceinline__ void sum_acc(double* acc) {
        double* L2 = L + kChunk * RS;
        double* L3 = L + kTot;
#pragma unroll
        for (int half = 0; half < kAcc / kChunk; half++) {
#pragma unroll
            for (int k = 0; k < kChunk; k++) L[k * RS + tid] = acc[half * kChunk + k];
            sync();
            if (tid < kChunk * S) {
                const int k = tid / S, s = tid - k * S;
                const double* row = L + k * RS;
                double p0 = 0, p1 = 0;
#pragma unroll 4
                for (int j = s; j < T; j += 2 * S) { p0 += row[j]; p1 += row[j + S]; }
                L2[tid] = p0 + p1;
            }
            sync();
            if (tid < kChunk) {
                double p = 0;
#pragma unroll
                for (int s = 0; s < S; s++) p += L2[tid * S + s];
                L3[half * kChunk + tid] = p;
            }
        }
        sync();
#pragma unroll
        for (int k = 0; k < kAcc; k++) acc[k] = L3[k];
    }
    __device__ __forceinline__ double sum1(double v) {
        v = col4_sum(row16_sum(v));
        if constexpr (W == 1) return v;
        double* Lw = L + kTot + 40 + par * W;
        if ((tid & 63) == 0) Lw[tid >> 6] = v;
        sync();
        double s = 0;
#pragma unroll
        for (int w = 0; w < W; w++) s += Lw[w];
        par ^= 1;
        return s;
    }
};

// dense LDL^T without pivoting, uniform in every lane (pose_opt.hip's ldlt6 with one more row)
__device__ __forceinline__ bool ldlt7(double S[49], const double b[7], double x[7]) {
    double d[7], id[7];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double dj = S[7 * j + j];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= S[7 * j + k] * S[7 * j + k] * d[k];
        if (dj == 0.0 || !isfinite(dj)) return false;
        d[j] = dj;
        id[j] = 1.0 / dj;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = S[7 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= S[7 * i + k] * S[7 * j + k] * d[k];
            S[7 * i + j] = s * id[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) x[i] = b[i];
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int k = 0; k < i; k++) x[i] -= S[7 * i + k] * x[k];
#pragma unroll
    for (int i = 0; i < 7; i++) x[i] *= id[i];
#pragma unroll
    for (int i = 6; i >= 0; i--)
#pragma unroll
        for (int k = i + 1; k < 7; k++) x[i] -= S[7 * k + i] * x[k];
    return true;
}

// g2o optimize(iters) over the pairs that are not removed. c2[2 e], c2[2 e + 1] = the chi2 of e12,
// e21 at the last computeActiveErrors that saw pair e (stale after a rejected final trial, as g2o).
template <int W>
__device__ __forceinline__ void sim3_optimize(Sim3Group<W>& g, S3& S, const Sim3OptHdr& h,
                                              const Sim3OptEdge* __restrict__ ed, const uint8_t* __restrict__ removed,
                                              double* __restrict__ c2, bool robust, int iters, int& trials) {
    constexpr int NT = Sim3Group<W>::T;
    // the first EC pairs of every thread stay in registers for all trials; the rest are re-read
    // (4 in both widths: a chain of selects picks the pass's record; 256 pairs at W = 1, 1024 at W = 4)
    constexpr int EC = 4;
    const int tid = g.tid, n = h.n;
    Sim3OptEdge ec[EC];
    unsigned act = 0;
#pragma unroll
    for (int c = 0; c < EC; c++) {
        const int e = tid + c * NT;
#pragma unroll
        for (int k = 0; k < 12; k++) ec[c].f[k] = e < n ? ed[e].f[k] : 0.0f;
        if (e < n && !removed[e]) act |= 1u << c;
    }
    // one loop body for cached and re-read pairs (pass i < EC: a select over the cached records)
    auto for_pairs = [&](auto&& f) {
#pragma unroll 1
        for (int i = 0, e = tid; e < n; i++, e += NT) {
            if (i < EC ? !(act >> i & 1) : removed[e] != 0) continue;
            Sim3OptEdge E;   // by value, field by field: a select between records would be one between addresses
#pragma unroll
            for (int k = 0; k < 12; k++) E.f[k] = ec[0].f[k];
#pragma unroll
            for (int c = 1; c < EC; c++)
#pragma unroll
                for (int k = 0; k < 12; k++) E.f[k] = i == c ? ec[c].f[k] : E.f[k];
            if (i >= EC) {
#pragma unroll
                for (int k = 0; k < 12; k++) E.f[k] = ed[e].f[k];
            }
            f(E, e);
        }
    };
    double* P = g.pert();
    double* U = g.uni();
    const double scalar = 1.0 / (2 * 1e-9);
    double lambda = 0, ni = 2;
    for (int it = 0; it < iters; it++) {
        // the 14 perturbed estimates of linearizeOplus: lane 2 d + sgn holds oplus((+-)1e-9 e_d)
        if (tid < 14) {
            const int d = tid >> 1;
            const double dl = (tid & 1) ? -1e-9 : 1e-9;
            double u[7];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = k == d ? dl : 0.0;
            if (h.fix_scale) u[6] = 0.0;
            const S3 Sp = s3_mul(s3_exp(u), S);
            s3_store(Sp, P + 16 * tid);
            s3_store(s3_inv(Sp), P + 16 * tid + 8);
        }
        if (tid == 14) {   // the estimate and its inverse, read from LDS by every pair like the perturbed ones
            s3_store(S, U);
            s3_store(s3_inv(S), U + 8);
        }
        g.sync();
        // computeActiveErrors + buildSystem
        double acc[kAcc];
#pragma unroll
        for (int k = 0; k < kAcc; k++) acc[k] = 0.0;
        // one edge of a pair (k = 0: e12, 1: e21): its error at the estimate, its chi2, the numeric
        // Jacobian through the perturbed estimates, its part of every sum
        auto edge = [&](auto K, const PairD& E, int e) {
            constexpr int k = decltype(K)::value;
            const double* X = k ? E.X1 : E.X2;
            const double* obs = k ? E.o2 : E.o1;
            const double info = k ? E.i2 : E.i1;
            const double* cam = U + 16 + 4 * k;
            double e0, e1;
            proj_err(s3_load(U + 8 * k), X, obs, cam, e0, e1);
            const double chi2 = info * (e0 * e0 + e1 * e1);
            c2[2 * e + k] = chi2;
            // rows 0, 1. The component loop stays rolled (unrolled, the compiler reads all fourteen
            // perturbed estimates before it computes, more than the register file holds); a column
            // reaches its registers by selects
            double J[14];
#pragma unroll
            for (int c = 0; c < 14; c++) J[c] = 0.0;
#pragma unroll 1
            for (int d = 0; d < 7; d++) {
                double p0, p1, m0, m1;
                proj_err(s3_load(P + 32 * d + 8 * k), X, obs, cam, p0, p1);
                proj_err(s3_load(P + 32 * d + 16 + 8 * k), X, obs, cam, m0, m1);
                const double j0 = scalar * (p0 - m0), j1 = scalar * (p1 - m1);
#pragma unroll
                for (int c = 0; c < 7; c++) {
                    J[c] = d == c ? j0 : J[c];
                    J[7 + c] = d == c ? j1 : J[7 + c];
                }
            }
            double r0, r1;
            huber(chi2, h.delta, robust, r0, r1);
            acc[35] += r0;
            const double w = r1 * info;
            const double om0 = -(info * e0) * r1, om1 = -(info * e1) * r1;
            int t = 0;
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
                for (int c = r; c < 7; c++) acc[t++] += w * (J[r] * J[c] + J[7 + r] * J[7 + c]);
#pragma unroll
            for (int r = 0; r < 7; r++) acc[28 + r] += J[r] * om0 + J[7 + r] * om1;
        };
        auto build = [&](const Sim3OptEdge& Ef, int e) {
            const PairD E(Ef);
            edge(std::integral_constant<int, 0>{}, E, e);
            edge(std::integral_constant<int, 1>{}, E, e);
        };
        for_pairs(build);
        g.sum_acc(acc);
        double H[49], b[7];
        {
            int t = 0;
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
                for (int c = r; c < 7; c++) { H[7 * r + c] = acc[t]; H[7 * c + r] = acc[t]; t++; }
#pragma unroll
            for (int r = 0; r < 7; r++) b[r] = acc[28 + r];
        }
        double currentChi = acc[35];
        if (it == 0) {
            double md = 0;
#pragma unroll
            for (int j = 0; j < 7; j++) md = fmax(md, fabs(H[8 * j]));
            lambda = 1e-5 * md;
            ni = 2;
        }
        double rho = 0;
        int qmax = 0;
        do {
            double M[49], x[7];
#pragma unroll
            for (int k = 0; k < 49; k++) M[k] = H[k] + (k % 8 == 0 ? lambda : 0.0);
            const bool ok = ldlt7(M, b, x);
            if (!ok) {
#pragma unroll
                for (int k = 0; k < 7; k++) x[k] = 0.0;
            }
            double u[7];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = x[k];
            if (h.fix_scale) u[6] = 0.0;
            const S3 Sn = s3_mul(s3_exp(u), S);
            const S3 Sni = s3_inv(Sn);
            double tc = 0;
            auto chi = [&](const Sim3OptEdge& Ef, int e) {
                const PairD E(Ef);
                double a0, a1, b0, b1, r0, r1;
                proj_err(Sn, E.X2, E.o1, U + 16, a0, a1);
                proj_err(Sni, E.X1, E.o2, U + 20, b0, b1);
                const double ca = E.i1 * (a0 * a0 + a1 * a1), cb = E.i2 * (b0 * b0 + b1 * b1);
                c2[2 * e] = ca;
                c2[2 * e + 1] = cb;
                huber(ca, h.delta, robust, r0, r1);
                tc += r0;
                huber(cb, h.delta, robust, r0, r1);
                tc += r0;
            };
            for_pairs(chi);
            double tempChi = g.sum1(tc);
            if (!ok) tempChi = DBL_MAX;
            double scale = 1e-3;
#pragma unroll
            for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
            rho = (currentChi - tempChi) / scale;
            if (rho > 0 && isfinite(tempChi)) {
                const double t2 = 2 * rho - 1;
                double alpha = 1. - t2 * t2 * t2;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                S = Sn;
            } else {
                lambda *= ni;   // pop: S keeps the pushed state
                ni *= 2;
            }
            qmax++;
            trials++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) break;
    }
}

}  // namespace

// W wavefronts per problem, one problem per work-group
template <int W>
__global__ __launch_bounds__(64 * W) void k_sim3_opt(const Sim3OptHdr* __restrict__ hdr,
                                                     const Sim3OptEdge* __restrict__ edges,
                                                     uint8_t* __restrict__ removed, uint8_t* __restrict__ keep,
                                                     double* __restrict__ chi2_last, Sim3OptOut* __restrict__ out) {
    constexpr int NT = Sim3Group<W>::T;
    __shared__ double sm[Sim3Group<W>::kDoubles];
    Sim3Group<W> g;
    g.L = sm;
    g.tid = threadIdx.x;
    const int tid = g.tid;
    const Sim3OptHdr h = hdr[blockIdx.x];
    const Sim3OptEdge* ed = edges + h.off;
    uint8_t* rm = removed + h.off;
    uint8_t* kp = keep + h.off;
    double* c2 = chi2_last + 2 * (size_t)h.off;
    for (int e = tid; e < h.n; e += NT) { rm[e] = 0; c2[2 * e] = 0.0; c2[2 * e + 1] = 0.0; }
    // cam1 then cam2 (adjacent in the header), read from memory: an index into the register copy h
    // would send it to scratch. Visible to the group after the optimizer's first barrier
    if (tid < 8) g.uni()[16 + tid] = (&hdr[blockIdx.x].cam1[0])[tid];
    S3 S = s3_load(h.S0);
    int trials = 0, nbad = 0, nin = 0;
    bool done = false;
    // one call site for both rounds: the optimizer's code exists once
    for (int round = 0; round < 2 && h.n > 0; round++) {
        sim3_optimize<W>(g, S, h, ed, rm, c2, round == 0, round == 0 || nbad == 0 ? 5 : 10, trials);
        if (round == 0) {
            int nb = 0;
            for (int e = tid; e < h.n; e += NT) {   // each thread only touches its own pairs
                const bool bad = c2[2 * e] > h.th2 || c2[2 * e + 1] > h.th2;
                rm[e] = bad; kp[e] = !bad; nb += bad;
            }
            nbad = (int)g.sum1((double)nb);
            if (h.n - nbad < 10) break;   // return 0: g2oS12 and the rest of the mask stay
        } else {
            const S3 Si = s3_inv(S);
            int ni = 0;
            for (int e = tid; e < h.n; e += NT) {
                if (rm[e]) continue;
                double a0, a1, b0, b1;   // e->computeError() on both edges at the estimate
                const PairD E(ed[e]);
                proj_err(S, E.X2, E.o1, g.uni() + 16, a0, a1);
                proj_err(Si, E.X1, E.o2, g.uni() + 20, b0, b1);
                const double ca = E.i1 * (a0 * a0 + a1 * a1), cb = E.i2 * (b0 * b0 + b1 * b1);
                const bool bad = ca > h.th2 || cb > h.th2;
                if (bad) kp[e] = 0;
                ni += !bad;
            }
            nin = (int)g.sum1((double)ni);
            done = true;
        }
    }
    if (tid == 0) {
        Sim3OptOut& o = out[blockIdx.x];
        if (!done) S = s3_load(h.S0);   // g2oS12 stays untouched
        s3_store(S, o.S);
        o.n_in = nin; o.n_bad = nbad; o.trials = trials; o.pad = 0;
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
int sim3_opt_batch(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_sim3_opt_problem* probs, int B,
                   orbhip_sim3_opt_result* res) {
    if (const int rc = sim3_opt_check(probs, B, res)) return rc;
    if (B == 0) return ORBHIP_OK;
    const Sim3OptLayout L = sim3_opt_layout(probs, B);
    const size_t back_bytes = L.back_end - L.o_out;
    HIPOK(S.ensure(L.total, L.up_bytes + back_bytes));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    sim3_opt_pack(probs, B, L, h);
    HIPOK(hipMemcpyAsync(d, h, L.up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    // W = 4 wavefronts per problem: a call has at most 64 problems, far fewer than the chip's SIMDs
    int W = 4;
    if (const char* s = std::getenv("ORBHIP_SIM3_OPT_WAVES")) W = std::atoi(s) == 1 ? 1 : 4;
    const Sim3OptHdr* dh = (const Sim3OptHdr*)(d + L.o_hdr);
    const Sim3OptEdge* de = (const Sim3OptEdge*)(d + L.o_edge);
    uint8_t* drm = d + L.o_rm;
    uint8_t* dkp = d + L.o_keep;
    double* dc2 = (double*)(d + L.o_c2);
    Sim3OptOut* dout = (Sim3OptOut*)(d + L.o_out);
    {
        const StageScope scope(timer);
        timer.begin(13, st);
        if (W == 4) ORBHIP_LAUNCH(k_sim3_opt<4>, dim3((unsigned)B), dim3(256), 0, st, dh, de, drm, dkp, dc2, dout);
        else ORBHIP_LAUNCH(k_sim3_opt<1>, dim3((unsigned)B), dim3(64), 0, st, dh, de, drm, dkp, dc2, dout);
        timer.end(13, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + L.up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + L.o_out, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const Sim3OptOut* ho = (const Sim3OptOut*)hb;
    const uint8_t* hk = hb + (L.o_keep - L.o_out);
    const Sim3OptHdr* hh = (const Sim3OptHdr*)(h + L.o_hdr);
    for (int b = 0; b < B; b++)   // nothing is written before every problem's counts are known to be sane
        if (ho[b].n_in < 0 || ho[b].n_bad < 0 || ho[b].n_in + ho[b].n_bad > probs[b].n) return ORBHIP_ERR_DEVICE;
    for (int b = 0; b < B; b++) {
        orbhip_sim3_opt_result& r = res[b];
        for (int k = 0; k < 4; k++) r.q[k] = ho[b].S[k];
        for (int k = 0; k < 3; k++) r.t[k] = ho[b].S[4 + k];
        r.s = ho[b].S[7];
        r.n_in = ho[b].n_in; r.n_bad = ho[b].n_bad; r.lm_trials = ho[b].trials;
        if (r.keep && probs[b].n) std::memcpy(r.keep, hk + hh[b].off, (size_t)probs[b].n);
    }
    return ORBHIP_OK;
}

}  // namespace orbhip
