// Optimizer::OptimizeSim3 on the device (sim3_opt.hip): one wavefront group per problem, the whole
// procedure in one launch. The records the kernel reads, and the argument check and the packing of
// a batch into the staging block's host image: plain C++, so that a host-only program can include
// this file and run both without the HIP runtime.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/orbhip.h"
#include "stage.h"

namespace orbhip {

constexpr int kSim3OptMaxBatch = 64;   // problems (candidate keyframes) per call
constexpr int kSim3OptMaxN = 8192;     // correspondences per problem

struct Sim3OptHdr {
    double S0[8];                // the initial S12: quaternion (x, y, z, w), t, s
    double cam1[4], cam2[4];     // fx, fy, cx, cy
    double th2, delta;           // delta = (float)sqrt(th2), the Huber width
    int32_t n, off;              // pairs [off, off + n) of the packed arrays
    int32_t fix_scale, pad;
};
struct Sim3OptOut {
    double S[8];
    int32_t n_in, n_bad, trials, pad;
};
struct Sim3OptEdge {             // float inputs as the reference holds them:
    float f[12];                 // X1c[3], X2c[3], obs1[2], obs2[2], inv_sigma2_1, inv_sigma2_2
};

// [hdr B][pairs E] uploaded; [out B][keep E] read back; [chi2 2 E][removed E] device only
struct Sim3OptLayout {
    size_t o_hdr, o_edge, up_bytes, o_out, o_keep, back_end, o_c2, o_rm, total, E;
};

inline bool sim3_opt_pos_finite(double v) { return v > 0.0 && std::isfinite(v); }

// ORBHIP_OK, ORBHIP_ERR_ARG or ORBHIP_ERR_UNSUPPORTED; reads nothing behind the problems' pointers
inline int sim3_opt_check(const orbhip_sim3_opt_problem* probs, int B, const orbhip_sim3_opt_result* res) {
    if (B < 0) return ORBHIP_ERR_ARG;
    if (B == 0) return ORBHIP_OK;
    if (!probs || !res) return ORBHIP_ERR_ARG;
    if (B > kSim3OptMaxBatch) return ORBHIP_ERR_UNSUPPORTED;
    for (int b = 0; b < B; b++) {
        const orbhip_sim3_opt_problem& p = probs[b];
        if (p.n < 0) return ORBHIP_ERR_ARG;
        if (p.n > 0 && (!p.X1c || !p.X2c || !p.obs1 || !p.obs2 || !p.inv_sigma2_1 || !p.inv_sigma2_2))
            return ORBHIP_ERR_ARG;
        if (!sim3_opt_pos_finite(p.cam1[0]) || !sim3_opt_pos_finite(p.cam1[1]) || !sim3_opt_pos_finite(p.cam2[0]) ||
            !sim3_opt_pos_finite(p.cam2[1]) || !sim3_opt_pos_finite(p.th2) || !sim3_opt_pos_finite(p.s))
            return ORBHIP_ERR_ARG;
        for (int k = 0; k < 4; k++)
            if (!std::isfinite(p.q[k])) return ORBHIP_ERR_ARG;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(p.t[k])) return ORBHIP_ERR_ARG;
    }
    for (int b = 0; b < B; b++)
        if (probs[b].n > kSim3OptMaxN) return ORBHIP_ERR_UNSUPPORTED;
    return ORBHIP_OK;
}

inline Sim3OptLayout sim3_opt_layout(const orbhip_sim3_opt_problem* probs, int B) {
    Sim3OptLayout L{};
    for (int b = 0; b < B; b++) L.E += (size_t)probs[b].n;
    StageLayout lay(256);
    L.o_hdr = lay.take(sizeof(Sim3OptHdr) * (size_t)B);
    L.o_edge = lay.take(sizeof(Sim3OptEdge) * L.E);
    L.up_bytes = lay.total();
    L.o_out = lay.take(sizeof(Sim3OptOut) * (size_t)B);
    L.o_keep = lay.take(L.E);
    L.back_end = lay.total();
    L.o_c2 = lay.take(sizeof(double) * 2 * L.E);
    L.o_rm = lay.take(L.E);
    L.total = lay.total();
    return L;
}

// the upload part of a checked batch into the host image h (L.up_bytes bytes)
inline void sim3_opt_pack(const orbhip_sim3_opt_problem* probs, int B, const Sim3OptLayout& L, uint8_t* h) {
    Sim3OptHdr* hh = (Sim3OptHdr*)(h + L.o_hdr);
    Sim3OptEdge* he = (Sim3OptEdge*)(h + L.o_edge);
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        const orbhip_sim3_opt_problem& p = probs[b];
        Sim3OptHdr& H = hh[b];
        for (int k = 0; k < 4; k++) H.S0[k] = p.q[k];
        for (int k = 0; k < 3; k++) H.S0[4 + k] = p.t[k];
        H.S0[7] = p.s;
        for (int k = 0; k < 4; k++) { H.cam1[k] = p.cam1[k]; H.cam2[k] = p.cam2[k]; }
        H.th2 = p.th2;
        H.delta = (double)(float)std::sqrt(p.th2);
        H.n = p.n; H.off = (int32_t)off;
        H.fix_scale = p.fix_scale != 0; H.pad = 0;
        for (int e = 0; e < p.n; e++) {
            Sim3OptEdge& E = he[off + e];
            for (int k = 0; k < 3; k++) { E.f[k] = p.X1c[3 * e + k]; E.f[3 + k] = p.X2c[3 * e + k]; }
            for (int k = 0; k < 2; k++) { E.f[6 + k] = p.obs1[2 * e + k]; E.f[8 + k] = p.obs2[2 * e + k]; }
            E.f[10] = p.inv_sigma2_1[e]; E.f[11] = p.inv_sigma2_2[e];
        }
        off += (size_t)p.n;
    }
}

#ifdef __HIPCC__
struct StageBlock;
struct StageTimer;
// profile stage 13 brackets the launch; returns ORBHIP_OK or an error
int sim3_opt_batch(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_sim3_opt_problem* probs, int B,
                   orbhip_sim3_opt_result* res);
#endif

}  // namespace orbhip
