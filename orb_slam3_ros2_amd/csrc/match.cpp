// Brute-force matching, host side (beside match_kernels.hip): the matcher's scratch and its three
// entry points (orbhip_match_bf, orbhip_match_pairs_device, orbhip_match_frames_device).
#include <algorithm>

#include "devbuf.h"
#include "graph_cache.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" match", x)

namespace orbhip {

struct MatchWorkspace {
    // the host call's staged inputs and results
    DevBuf<uint8_t> d_mq, d_mt;
    DevBuf<float> d_mqa, d_mta;
    DevBuf<int32_t> d_mm, d_mb, d_ms, d_mn;
    DevBuf<uint64_t> d_mpart;   // chunk partials (match_part_entries)
    DevBuf<int> d_msync;        // one-launch matcher counters (zeroed once, reset by every launch)
};
MatchWorkspace* match_ws_create() { return new MatchWorkspace(); }
void match_ws_destroy(MatchWorkspace* ws) { delete ws; }

// chunk partials for the call, and the one-launch matcher's counters: zeroed on the call's stream
// before their first use
static int ensure_scratch(MatchWorkspace* ws, size_t part_entries, hipStream_t st) {
    HIPOK(ws->d_mpart.ensure(part_entries));
    if (ws->d_msync.p) return ORBHIP_OK;
    HIPOK(ws->d_msync.ensure(kMatchSyncInts));
    HIPOK(hipMemsetAsync(ws->d_msync.p, 0, sizeof(int) * kMatchSyncInts, st));
    return ORBHIP_OK;
}

int match_bf_host(MatchWorkspace* ws, const uint8_t* q, const float* qa, int nq, const uint8_t* t, const float* ta,
                  int nt, int th_low, float ratio, int check_orientation, int32_t* match, int32_t* best_d,
                  int32_t* second_d, hipStream_t st) {
    HIPOK(ws->d_mq.ensure((size_t)nq * 32));
    HIPOK(ws->d_mt.ensure((size_t)std::max(nt, 1) * 32));
    HIPOK(ws->d_mqa.ensure(nq));
    HIPOK(ws->d_mta.ensure(std::max(nt, 1)));
    HIPOK(ws->d_mm.ensure(nq));
    HIPOK(ws->d_mb.ensure(nq));
    HIPOK(ws->d_ms.ensure(nq));
    HIPOK(ws->d_mn.ensure(1));
    HIPOK(hipMemcpyAsync(ws->d_mq.p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(ws->d_mqa.p, qa, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    if (nt > 0) {
        HIPOK(hipMemcpyAsync(ws->d_mt.p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(ws->d_mta.p, ta, (size_t)nt * 4, hipMemcpyHostToDevice, st));
    } else {
        // no train descriptors: every query keeps best = second = 256 (no match)
        HIPOK(hipMemsetAsync(ws->d_mm.p, 0xFF, (size_t)nq * 4, st));
    }
    if (int rc = ensure_scratch(ws, match_part_entries(1, nq, nt), st)) return rc;
    (void)hipGetLastError();
    launch_match_bf(ws->d_mq.p, ws->d_mqa.p, nq, ws->d_mt.p, ws->d_mta.p, nt, th_low, ratio, check_orientation,
                    ws->d_mm.p, ws->d_mb.p, ws->d_ms.p, ws->d_mn.p, ws->d_mpart.p, st, ws->d_msync.p);
    HIPOK(hipGetLastError());
    int nm = 0;
    HIPOK(hipMemcpyAsync(match, ws->d_mm.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(best_d, ws->d_mb.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(second_d, ws->d_ms.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&nm, ws->d_mn.p, 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return nm;
}

int match_pairs_device(MatchWorkspace* ws, GraphCache& graphs, StageTimer& timer, const orbhip_kp* d_kps,
                       const uint8_t* d_desc, const int32_t* d_n, int B, int cap, int th_low, float ratio,
                       int check_orientation, int32_t* d_match, int32_t* d_best, int32_t* d_second, int32_t* d_nmatch,
                       hipStream_t st) {
    if (int rc = ensure_scratch(ws, match_part_entries(B - 1, cap, cap), st)) return rc;
    (void)hipGetLastError();
    GraphKey key;
    key.add(3).ptr(d_kps).ptr(d_desc).ptr(d_n).add((uint64_t)B).add((uint64_t)cap).add((uint64_t)th_low).f32(ratio)
        .add((uint64_t)check_orientation).ptr(d_match).ptr(d_best).ptr(d_second).ptr(d_nmatch).ptr(st)
        .ptr(ws->d_mpart.p).ptr(ws->d_msync.p);
    return graphs.run(key, st, timer.stage != 0, [&](hipStream_t st) -> int {
        launch_match_pairs(d_kps, d_desc, d_n, B - 1, cap, th_low, ratio, check_orientation, d_match, d_best,
                           d_second, d_nmatch, ws->d_mpart.p, st, &timer, ws->d_msync.p);
        HIPOK(hipGetLastError());
        return ORBHIP_OK;
    });
}

int match_frames_device(MatchWorkspace* ws, GraphCache& graphs, StageTimer& timer, const orbhip_kp* d_q_kps,
                        const uint8_t* d_q_desc, const int32_t* d_nq, const orbhip_kp* d_t_kps,
                        const uint8_t* d_t_desc, const int32_t* d_nt, int cap, int th_low, float ratio,
                        int check_orientation, int32_t* d_match, int32_t* d_best, int32_t* d_second,
                        int32_t* d_nmatch, hipStream_t st) {
    if (int rc = ensure_scratch(ws, match_part_entries(1, cap, cap), st)) return rc;
    (void)hipGetLastError();
    GraphKey key;
    key.add(2).ptr(d_q_kps).ptr(d_q_desc).ptr(d_nq).ptr(d_t_kps).ptr(d_t_desc).ptr(d_nt).add((uint64_t)cap)
        .add((uint64_t)th_low).f32(ratio).add((uint64_t)check_orientation).ptr(d_match).ptr(d_best).ptr(d_second)
        .ptr(d_nmatch).ptr(st).ptr(ws->d_mpart.p).ptr(ws->d_msync.p);
    return graphs.run(key, st, timer.stage != 0, [&](hipStream_t st) -> int {
        launch_match_frames(d_q_kps, d_q_desc, d_nq, d_t_kps, d_t_desc, d_nt, cap, th_low, ratio, check_orientation,
                            d_match, d_best, d_second, d_nmatch, ws->d_mpart.p, st, &timer, ws->d_msync.p);
        HIPOK(hipGetLastError());
        return ORBHIP_OK;
    });
}

}  // namespace orbhip
