// The 7-dof pose graph of a loop closure: U:src/Optimizer.cc::Optimizer::OptimizeEssentialGraph,
// on the device. VertexSim3Expmap vertices (estimate (q, t, s), oplus(u) = Sim3(u) * estimate with
// u[6] = 0 under fix_scale), EdgeSim3 edges (e = (Sji Si Sj^-1).log(), information I7, no robust
// kernel, g2o's numeric Jacobians), BlockSolver_7_3 + Levenberg with a user lambda0, then the
// map-point correction P' = Swc_corrected.map(Scw_before.map(P)).
// One slot = one Levenberg trial, enqueued by the host without a round trip; the g2o rules run on
// the device and every kernel (and the linear solve) is gated on the phase word of EgCtl:
//   k_eg_lin       (build) 16 lanes per edge: lanes 0..13 one central-difference column each, lane
//                  14 the error and chi2; J and e go to the edge's record (EgEdgeLin)
//   k_eg_assemble  (build) one wavefront per 7x7 block of H's lower triangle: the block's edges
//                  gathered in edge order from the host's lists, no floating-point atomics; the
//                  diagonal blocks also give Hdiag and b
//   k_eg_damp      (build: the fixed-order chi2 sum, lambda0, phase -> trial) S[k][k] = Hdiag[k] + lambda
//   chol_dag_solve / chol_blocked_solve of (H + lambda I) x = b
//   k_eg_apply     St = oplus(S, x) per free vertex (S stays: a rejected trial restores nothing)
//   k_eg_trial     every edge's chi2 at St; the last work-group to arrive sums them in a fixed
//                  order and takes g2o's decision: rho, accept (S <- St) or reject, lambda and ni,
//                  the iteration counter, the stop
//   k_eg_points    after the last slot: one thread per map point
// Every operation is fp64 in the order tests/essential_graph_numpy.py writes it; only the sums over
// edges differ in order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/orbhip.h"
#include "ba_args.h"
#include "ba_chol_blocked.h"
#include "ba_chol_dag.h"
#include "essential_graph.h"
#include "orbhip_kernels.h"
#include "sim3_dev.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" essential_graph", x)

namespace orbhip {

namespace {

constexpr int kEgStage = 15;

// e = (Sji * Si * Sj^-1).log()
__device__ __forceinline__ void eg_error(const S3& M, const S3& Si, const S3& Sj, double* e) {
    s3_log(s3_mul(s3_mul(M, Si), s3_inv(Sj)), e);
}

// sum of v over the work-group's T threads in a fixed order (a tree over LDS), in every thread
template <int T>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = T / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] = sh[t] + sh[t + o];
        __syncthreads();
    }
    return sh[0];
}

}  // namespace

// 16 lanes per edge, 16 edges per work-group
__global__ __launch_bounds__(256) void k_eg_lin(const EgCtl* __restrict__ ctl, const double* __restrict__ S,
                                                const int32_t* __restrict__ vidx, const int32_t* __restrict__ eij,
                                                const double* __restrict__ eS, int E, EgEdgeLin* __restrict__ lin) {
    if (ctl->phase != kPhBuild) return;
    const int e = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    if (e >= E) return;
    const int i = eij[2 * e], j = eij[2 * e + 1];
    const S3 M = s3_load(eS + 8 * (size_t)e), Si = s3_load(S + 8 * (size_t)i), Sj = s3_load(S + 8 * (size_t)j);
    const int side = l >= 7 ? 1 : 0, d = l - 7 * side;
    const bool col = l < 14;
    const bool fixed_v = col && vidx[side ? j : i] < 0;
    double ev[2][7];
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int r = 0; r < 7; r++) ev[p][r] = 0.0;
    // lanes 0..13: e(oplus(+1e-9 e_d)) then e(oplus(-1e-9 e_d)); lane 14: the error at the estimate
    const int npass = col ? (fixed_v ? 0 : 2) : (l == 14 ? 1 : 0);
#pragma unroll 1
    for (int p = 0; p < npass; p++) {
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = (col && k == d) ? (p ? -1e-9 : 1e-9) : 0.0;
        if (ctl->fix_scale) u[6] = 0.0;
        const S3 P = s3_exp(u);
        const S3 Pi = s3_mul(P, Si), Pj = s3_mul(P, Sj);
        S3 A = Si, B = Sj;
        if (col && !side) A = Pi;
        if (col && side) B = Pj;
        double er[7];
        eg_error(M, A, B, er);
#pragma unroll
        for (int r = 0; r < 7; r++) {
            ev[0][r] = p == 0 ? er[r] : ev[0][r];
            ev[1][r] = p == 1 ? er[r] : ev[1][r];
        }
    }
    EgEdgeLin& L = lin[e];
    if (col) {
        const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll
        for (int r = 0; r < 7; r++) L.J[l][r] = fixed_v ? 0.0 : scalar * (ev[0][r] - ev[1][r]);
    } else if (l == 14) {
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < 7; r++) { L.e[r] = ev[0][r]; c += ev[0][r] * ev[0][r]; }
        L.chi2 = c;
    }
}

// One wavefront per block: lanes 0..48 an element of the 7x7 block, lanes 49..55 of a diagonal
// block a row of b. always: also outside the build phase (the blocked solver factors S in place)
__global__ __launch_bounds__(64) void k_eg_assemble(const EgCtl* __restrict__ ctl, const EgBlock* __restrict__ blocks,
                                                    const int32_t* __restrict__ ent,
                                                    const int32_t* __restrict__ bfirst,
                                                    const EgEdgeLin* __restrict__ lin, int n, int always,
                                                    double* __restrict__ Sd, double* __restrict__ hdiag,
                                                    double* __restrict__ b) {
    const int ph = ctl->phase;
    if (ph == kPhDone || (!always && ph != kPhBuild)) return;
    const EgBlock B = blocks[blockIdx.x];
    const int t = threadIdx.x;
    if (t < 49) {
        const int r = t / 7, c = t - 7 * r;
        double acc = 0.0;
        for (int k = B.first; k < B.first + B.count; k++) {
            const int en = ent[k], form = en & 7;
            const EgEdgeLin& L = lin[en >> 3];
            const double* Ja = L.J[(form == 1 || form == 3 ? 7 : 0) + r];
            const double* Jb = L.J[(form == 1 || form == 2 ? 7 : 0) + c];
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 7; q++) v += Ja[q] * Jb[q];
            acc += v;
        }
        Sd[(size_t)(7 * B.br + r) * n + 7 * B.bc + c] = acc;
        if (B.br == B.bc && r == c) hdiag[7 * B.br + r] = acc;
    } else if (t < 56 && B.br == B.bc) {
        const int r = t - 49;
        double acc = 0.0;
        for (int k = bfirst[B.br]; k < bfirst[B.br + 1]; k++) {
            const int en = ent[k];
            const EgEdgeLin& L = lin[en >> 3];
            const double* Ja = L.J[(en & 7 ? 7 : 0) + r];
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 7; q++) v += Ja[q] * L.e[q];
            acc += -v;
        }
        b[7 * B.br + r] = acc;
    }
}

// One work-group. In the build phase: the iteration's chi2 in a fixed order, lambda0 in the first
// iteration, phase -> trial. Then the damped diagonal of this trial.
__global__ __launch_bounds__(1024) void k_eg_damp(EgCtl* __restrict__ ctl, const EgEdgeLin* __restrict__ lin, int E,
                                                  int n, const double* __restrict__ hdiag, double* __restrict__ Sd) {
    __shared__ double sh[1024];
    __shared__ double lam;
    const int ph = ctl->phase;
    if (ph == kPhDone) return;
    const int t = threadIdx.x;
    if (ph == kPhBuild) {
        double c = 0.0;
        for (int e = t; e < E; e += 1024) c += lin[e].chi2;
        const double chi = block_sum<1024>(c, sh);
        if (t == 0) {
            ctl->currentChi = chi;
            if (ctl->it == 0) { ctl->lambda = ctl->lambda_init; ctl->ni = 2.0; }
            ctl->it += 1;
            ctl->qmax = 0;
            ctl->phase = kPhTrial;
        }
    }
    if (t == 0) lam = ctl->lambda;
    __syncthreads();
    const double lambda = lam;
    for (int k = t; k < n; k += 1024) Sd[(size_t)k * n + k] = hdiag[k] + lambda;
}

// St = the trial estimates: oplus(x) on the free vertices, the fixed ones as they are
__global__ __launch_bounds__(256) void k_eg_apply(const EgCtl* __restrict__ ctl, const double* __restrict__ S,
                                                  const int32_t* __restrict__ vidx, const double* __restrict__ x,
                                                  int nv, double* __restrict__ St) {
    if (ctl->phase != kPhTrial) return;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    S3 s = s3_load(S + 8 * (size_t)v);
    const int k = vidx[v];
    if (k >= 0) {
        double u[7];
#pragma unroll
        for (int q = 0; q < 7; q++) u[q] = x[7 * k + q];
        if (ctl->fix_scale) u[6] = 0.0;
        s = s3_mul(s3_exp(u), s);
    }
    s3_store(s, St + 8 * (size_t)v);
}

// mode 0 (before the slots, ungated): every edge's chi2 at S; the last work-group sums them into
// initChi and currentChi. mode 1 (trial phase): at St; the last work-group takes the decision.
// cnt: the arrival counter, 0 between launches
__global__ __launch_bounds__(256) void k_eg_trial(EgCtl* __restrict__ ctl, int mode, double* __restrict__ S,
                                                  const double* __restrict__ St, const int32_t* __restrict__ eij,
                                                  const double* __restrict__ eS, int E, int nv, int n,
                                                  const double* __restrict__ x, const double* __restrict__ b,
                                                  const int* __restrict__ flag, double* __restrict__ chi2,
                                                  int* __restrict__ cnt) {
    __shared__ double sh[256];
    __shared__ int last;
    if (mode == 1 && ctl->phase != kPhTrial) return;
    const double* Sx = mode ? St : S;
    const int t = threadIdx.x, e = blockIdx.x * 256 + t;
    if (e < E) {
        const int i = eij[2 * e], j = eij[2 * e + 1];
        double er[7];
        eg_error(s3_load(eS + 8 * (size_t)e), s3_load(Sx + 8 * (size_t)i), s3_load(Sx + 8 * (size_t)j), er);
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < 7; r++) c += er[r] * er[r];
        chi2[e] = c;
    }
    __threadfence();
    __syncthreads();
    if (t == 0) last = atomicAdd(cnt, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    double c = 0.0;
    for (int k = t; k < E; k += 256) c += __hip_atomic_load(&chi2[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double tempChi = block_sum<256>(c, sh);
    if (mode == 0) {
        if (t == 0) { ctl->initChi = tempChi; ctl->currentChi = tempChi; *cnt = 0; }
        return;
    }
    const double lambda = ctl->lambda;
    double sc = 0.0;
    for (int k = t; k < n; k += 256) sc += x[k] * (lambda * x[k] + b[k]);
    const double scale = 1e-3 + block_sum<256>(sc, sh);
    if (flag[0] == 0) tempChi = DBL_MAX;   // a failed pivot: x = 0, a rejected trial
    const double rho = (ctl->currentChi - tempChi) / scale;
    const bool accept = rho > 0 && isfinite(tempChi);
    if (accept)
        for (int k = t; k < 8 * nv; k += 256) S[k] = St[k];
    __syncthreads();
    if (t == 0) {
        double lam = lambda, ni = ctl->ni;
        if (accept) {
            const double t2 = 2 * rho - 1;
            double alpha = 1. - t2 * t2 * t2;
            alpha = fmin(alpha, 2. / 3.);
            lam *= fmax(1. / 3., alpha);
            ni = 2;
            ctl->currentChi = tempChi;
        } else {
            lam *= ni;
            ni *= 2;
            ctl->rejected += 1;
        }
        ctl->lambda = lam;
        ctl->ni = ni;
        const int qmax = ctl->qmax + 1;
        ctl->qmax = qmax;
        ctl->trials += 1;
        if (!(rho < 0 && qmax < 10)) {   // the iteration ends
            const bool stop = qmax == 10 || rho == 0;
            ctl->phase = (stop || ctl->it >= ctl->iterations) ? kPhDone : kPhBuild;
        }
        *cnt = 0;
    }
}

// P' = Swc_corrected[ref].map(Scw_before[ref].map(P)): one thread per map point
__global__ __launch_bounds__(256) void k_eg_points(const double* __restrict__ S_in, const double* __restrict__ S_out,
                                                   const float* __restrict__ pts, const int32_t* __restrict__ ref,
                                                   int M, float* __restrict__ out) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int v = ref[m];
    const S3 Scw = s3_load(S_in + 8 * (size_t)v);
    const S3 Swc = s3_inv(s3_load(S_out + 8 * (size_t)v));
    double cx, cy, cz, wx, wy, wz;
    s3_map(Scw, (double)pts[3 * (size_t)m], (double)pts[3 * (size_t)m + 1], (double)pts[3 * (size_t)m + 2], cx, cy, cz);
    s3_map(Swc, cx, cy, cz, wx, wy, wz);
    out[3 * (size_t)m] = (float)wx;
    out[3 * (size_t)m + 1] = (float)wy;
    out[3 * (size_t)m + 2] = (float)wz;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <typename T>
struct EgBuf {
    T* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t count) {
        if (count <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const hipError_t e = hipMalloc((void**)&p, sizeof(T) * count);
        if (e == hipSuccess) cap = count;
        return e;
    }
    ~EgBuf() { if (p) (void)hipFree(p); }
};

// what does not live in the staging block: the dense system and the solvers' own storage
struct EgWorkspace {
    EgBuf<double> Sd, dagbuf, Lsave;
    EgBuf<int> ints;          // the DAG solver's control words and flags, then its plan
    EgStructure st;
    DagPlan plan;
    long long timeouts = 0;
};
EgWorkspace* eg_ws_create() { return new EgWorkspace(); }
void eg_ws_destroy(EgWorkspace* ws) { delete ws; }

namespace {

int eg_run(EgWorkspace* ws, StageBlock& SB, StageTimer& timer, hipStream_t st,
           const orbhip_essential_graph_problem* p, orbhip_essential_graph_result* res, bool after_timeout) {
    const int nv = p->n_vertices, E = p->n_edges, M = p->n_points;
    EgStructure& s = ws->st;
    eg_structure(p, s);
    const int n = s.n;
    const EgLayout L = eg_layout(p, s);
    HIPOK(SB.ensure(L.total, L.back_end));
    uint8_t* const d = SB.d;
    uint8_t* const h = SB.h;
    eg_pack(p, s, L, h);
    const bool run = p->iterations > 0 && s.nf > 0 && E > 0;
    const char* env = std::getenv("ORBHIP_EG_BLOCKED");
    const bool forced = env && env[0] == '1';
    const bool blocked = after_timeout || forced || n < kEgDagMinN;
    const int solver = after_timeout ? 2 : (blocked ? 1 : 0);
    const int nt = (n + 31) / 32;
    DagDev dd{};
    int* dflag = (int*)(d + L.o_flag);            // [0] the solver's flag, [1] the blocked solver's counter
    int* dcnt = dflag + 8;                        // k_eg_trial's arrival counter
    int* dto = nullptr;                           // the DAG solver's timeout word
    if (run) {
        HIPOK(ws->Sd.ensure((size_t)n * n));
        HIPOK(hipMemsetAsync(ws->Sd.p, 0, sizeof(double) * (size_t)n * n, st));
        if (blocked) {
            HIPOK(ws->Lsave.ensure((size_t)1024 * nt));
        } else {
            dag_plan(s.row_first.data(), n, dag_max_helpers(), ws->plan);
            const DagPlan& pl = ws->plan;
            const size_t ni = dag_ints(n), ntoff = pl.toff.size(), ntask = std::max<size_t>(1, pl.tasks.size());
            HIPOK(ws->dagbuf.ensure(dag_doubles(n)));
            HIPOK(ws->ints.ensure(ni + ntoff + ntask));
            HIPOK(hipMemsetAsync(ws->ints.p, 0, sizeof(int) * ni, st));
            HIPOK(hipMemcpyAsync(ws->ints.p + ni, pl.toff.data(), sizeof(int) * ntoff, hipMemcpyHostToDevice, st));
            if (!pl.tasks.empty())
                HIPOK(hipMemcpyAsync(ws->ints.p + ni + ntoff, pl.tasks.data(), sizeof(int) * pl.tasks.size(),
                                     hipMemcpyHostToDevice, st));
            dd = DagDev{ws->dagbuf.p, ws->ints.p, ws->ints.p + ni, ws->ints.p + ni + ntoff, pl.G, pl.pb, pl.toff[pl.G]};
            dto = ws->ints.p + 3;
        }
    }
    HIPOK(hipMemcpyAsync(d, h, L.up_bytes, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d + L.o_out_ctl, d + L.o_ctl, sizeof(EgCtl), hipMemcpyDeviceToDevice, st));
    if (nv) HIPOK(hipMemcpyAsync(d + L.o_out_S, d + L.o_S, 64 * (size_t)nv, hipMemcpyDeviceToDevice, st));
    HIPOK(hipMemsetAsync(dflag, 0, 16 * sizeof(int), st));
    (void)hipGetLastError();
    EgCtl* ctl = (EgCtl*)(d + L.o_out_ctl);
    const double* S_in = (const double*)(d + L.o_S);
    double* Sw = (double*)(d + L.o_out_S);
    double* St = (double*)(d + L.o_St);
    const int32_t* vidx = (const int32_t*)(d + L.o_vidx);
    const int32_t* eij = (const int32_t*)(d + L.o_eij);
    const double* eS = (const double*)(d + L.o_eS);
    const EgBlock* blocks = (const EgBlock*)(d + L.o_blocks);
    const int32_t* ent = (const int32_t*)(d + L.o_ent);
    const int32_t* bfirst = (const int32_t*)(d + L.o_bfirst);
    const int* rf = (const int*)(d + L.o_rf);
    EgEdgeLin* lin = (EgEdgeLin*)(d + L.o_lin);
    double* chi2 = (double*)(d + L.o_chi2);
    double* hdiag = (double*)(d + L.o_hdiag);
    double* b = (double*)(d + L.o_b);
    double* x = (double*)(d + L.o_x);
    const dim3 b256(256);
    const unsigned gE = (unsigned)((E + 255) / 256), gE16 = (unsigned)((E + 15) / 16);
    const EgCtl* hctl = (const EgCtl*)(h + L.o_out_ctl);
    int timeouts = 0;
    {
        const StageScope scope(timer);
        timer.begin(kEgStage, st);
        if (E > 0)
            ORBHIP_LAUNCH(k_eg_trial, dim3(gE), b256, 0, st, ctl, 0, Sw, (const double*)St, eij, eS, E, nv, n,
                          (const double*)x, (const double*)b, (const int*)dflag, chi2, dcnt);
        int slots = run ? p->iterations : 0;
        for (;;) {
            for (int k = 0; k < slots; k++) {
                ORBHIP_LAUNCH(k_eg_lin, dim3(gE16), b256, 0, st, (const EgCtl*)ctl, (const double*)Sw, vidx, eij, eS, E,
                              lin);
                if (blocked) HIPOK(hipMemsetAsync(ws->Sd.p, 0, sizeof(double) * (size_t)n * n, st));
                ORBHIP_LAUNCH(k_eg_assemble, dim3((unsigned)s.blocks.size()), dim3(64), 0, st, (const EgCtl*)ctl, blocks,
                              ent, bfirst, (const EgEdgeLin*)lin, n, blocked ? 1 : 0, ws->Sd.p, hdiag, b);
                ORBHIP_LAUNCH(k_eg_damp, dim3(1), dim3(1024), 0, st, ctl, (const EgEdgeLin*)lin, E, n,
                              (const double*)hdiag, ws->Sd.p);
                if (blocked) {
                    chol_blocked_solve(ws->Sd.p, n, ws->Lsave.p, b, x, dflag, rf, st, &ctl->phase);
                } else {
                    HIPOK(chol_dag_solve(ws->Sd.p, n, rf, b, x, dflag, dd, st, &ctl->phase));
                }
                ORBHIP_LAUNCH(k_eg_apply, dim3((unsigned)((nv + 255) / 256)), b256, 0, st, (const EgCtl*)ctl,
                              (const double*)Sw, vidx, (const double*)x, nv, St);
                ORBHIP_LAUNCH(k_eg_trial, dim3(gE), b256, 0, st, ctl, 1, Sw, (const double*)St, eij, eS, E, nv, n,
                              (const double*)x, (const double*)b, (const int*)dflag, chi2, dcnt);
            }
            // the points and the outputs behind the slots that may be the last ones
            if (M > 0)
                ORBHIP_LAUNCH(k_eg_points, dim3((unsigned)((M + 255) / 256)), b256, 0, st, S_in, (const double*)Sw,
                              (const float*)(d + L.o_pts), (const int32_t*)(d + L.o_ref), M, (float*)(d + L.o_out_pts));
            HIPOK(hipGetLastError());
            HIPOK(hipMemcpyAsync(h + L.o_out_ctl, d + L.o_out_ctl, L.back_end - L.o_out_ctl, hipMemcpyDeviceToHost, st));
            if (dto) HIPOK(hipMemcpyAsync(&timeouts, dto, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            if (!run || hctl->phase == kPhDone || timeouts) break;
            if (hctl->phase != kPhBuild && hctl->phase != kPhTrial) return ORBHIP_ERR_DEVICE;
            slots = std::max(1, hctl->iterations - hctl->it);   // rejected trials took their iterations' slots
        }
        timer.end(kEgStage, st);
    }
    if (timeouts) {   // a hand-off of the persistent solver timed out: again on the blocked solver
        ws->timeouts += timeouts;
        return 1;
    }
    if (hctl->trials < 0 || hctl->rejected < 0 || hctl->rejected > hctl->trials || hctl->it > p->iterations)
        return ORBHIP_ERR_DEVICE;
    if (nv) std::memcpy(res->S, h + L.o_out_S, 64 * (size_t)nv);
    if (M) std::memcpy(res->points, h + L.o_out_pts, 12 * (size_t)M);
    res->chi2_initial = hctl->initChi;
    res->chi2_final = hctl->currentChi;
    res->iterations_run = hctl->it;
    res->lm_trials = hctl->trials;
    res->lm_rejected = hctl->rejected;
    res->solver = solver;
    return ORBHIP_OK;
}

}  // namespace

int eg_optimize(EgWorkspace* ws, StageBlock& SB, StageTimer& timer, hipStream_t st,
                const orbhip_essential_graph_problem* prob, orbhip_essential_graph_result* res) {
    if (const int rc = eg_check(prob, res)) return rc;
    if (!ws) return ORBHIP_ERR_ARG;
    const int rc = eg_run(ws, SB, timer, st, prob, res, false);
    return rc == 1 ? eg_run(ws, SB, timer, st, prob, res, true) : rc;
}

}  // namespace orbhip
