// ORB extraction, host side (extract.h): plan lookup and upload, scratch, the launch sequence of
// one batch, the host-image call, what the stereo stage reads of the workspace and the
// extractor's test hooks.
#include "extract.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "devbuf.h"
#include "graph_cache.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" extract", x)

namespace orbhip {
namespace {

// a host plan and its device image
struct Plan {
    HostPlan hp;
    DevBuf<ExtractPlan> d_plan;
    DevBuf<CellGeom> d_cells;
    DevBuf<int> d_xofs, d_xalpha, d_yofs, d_ybeta, d_disc, d_cone_tab, d_cone_hi_tab, d_bands, d_flow_dep;
    DevBuf<ConeRect> d_cone, d_cone_hi;
    DevBuf<uint16_t> d_otab;
};

// A plan depends only on the device, the frame size, the ORBextractor parameters, the cone tile
// and the test switches read for it, never on a context's buffers: contexts with the same key
// (e.g. the 16 camera streams of the C2 bench) share one, so its tables (the cone's per-tile
// resize tables are ~0.5 MB at 640x480) stay L2-resident once instead of once per context. The
// cache holds weak references: a plan dies with the last context using it.
struct PlanKey {
    int device, w, h, nfeat, nlev, ini, mn;
    float scale;
    PlanSwitches sw;
    bool operator<(const PlanKey& o) const { return std::memcmp(this, &o, sizeof(PlanKey)) < 0; }
};
std::mutex g_plan_m;
std::map<PlanKey, std::weak_ptr<Plan>>& plan_cache() {
    static auto* m = new std::map<PlanKey, std::weak_ptr<Plan>>();   // never destroyed (exit order)
    return *m;
}

// threads per batch-cone tile: ORBHIP_CONE_HI_THREADS (256 / 512 / 1024), else 256
int cone_hi_threads() {
    static const int t = std::getenv("ORBHIP_CONE_HI_THREADS") ? std::atoi(std::getenv("ORBHIP_CONE_HI_THREADS")) : 256;
    return (t == 512 || t == 1024) ? t : 256;
}

template <typename T>
hipError_t upload(DevBuf<T>& d, const std::vector<T>& v) {
    if (v.empty()) return hipSuccess;
    const hipError_t e = d.ensure(v.size());
    return e != hipSuccess ? e : hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

int upload_plan(Plan& pl) {
    const HostPlan& hp = pl.hp;
    HIPOK(pl.d_plan.ensure(1));
    HIPOK(hipMemcpy(pl.d_plan.p, &hp.h, sizeof(ExtractPlan), hipMemcpyHostToDevice));
    HIPOK(upload(pl.d_cells, hp.cells));
    HIPOK(upload(pl.d_xofs, hp.xofs));
    HIPOK(upload(pl.d_xalpha, hp.xalpha));
    HIPOK(upload(pl.d_yofs, hp.yofs));
    HIPOK(upload(pl.d_ybeta, hp.ybeta));
    HIPOK(upload(pl.d_disc, hp.disc));
    HIPOK(upload(pl.d_otab, hp.otab));
    HIPOK(upload(pl.d_bands, hp.bands));
    HIPOK(upload(pl.d_flow_dep, hp.flow_dep));
    HIPOK(upload(pl.d_cone_hi, hp.cone_hi));
    HIPOK(upload(pl.d_cone_hi_tab, hp.cone_hi_tab));
    HIPOK(upload(pl.d_cone, hp.cone));
    HIPOK(upload(pl.d_cone_tab, hp.cone_tab));
    return ORBHIP_OK;
}

// the switches of one run, read per call so that tests can flip them on a live context
struct RunSwitches {
    // octree division engine: ORBHIP_OCTREE_SWEEP=1 runs the sweep path only, ORBHIP_OCTREE_DH=d
    // caps the pyramid depth (a shallow cap forces the pyramid path's fallback to the sweep path)
    int oct_fast, oct_max_dh;
    bool no_cone;   // pyramid engine: ORBHIP_NO_CONE (set) forces the k_resize cascade
    // ORBHIP_CONE_HI=1: batches run levels 3.. as one cone launch behind two k_resize levels.
    // Off by default: at C3 (B = 64, 1280x720) that launch took 255-320 us against the 89 us of
    // the five k_resize launches it replaces (tools/c3_pyr_sweep.sh, tiles 16-48)
    bool cone_hi;
    // ORBHIP_CAND_PACK=1: packed FAST candidates, the octree then reads whole lines. Off: at C3
    // it cut k_octree's traffic 21.8 -> 6.4 MB per launch (PMC), but the atomic each FAST cell
    // waits on held its work-group slot ~1 us longer: k_fast_cells 525 -> 568 us
    bool pack;
    bool flow;      // ORBHIP_RZ_FLOW=1: batches build levels 1..L-1 in one k_pyr_flow launch
};
RunSwitches read_run_switches() {
    auto is1 = [](const char* name) {
        const char* e = std::getenv(name);
        return e && e[0] == '1';
    };
    const char* e_dh = std::getenv("ORBHIP_OCTREE_DH");
    RunSwitches s;
    s.oct_fast = is1("ORBHIP_OCTREE_SWEEP") ? 0 : 1;
    s.oct_max_dh = e_dh ? std::max(1, std::min(6, std::atoi(e_dh))) : 6;
    s.no_cone = std::getenv("ORBHIP_NO_CONE") != nullptr;
    s.cone_hi = is1("ORBHIP_CONE_HI");
    s.pack = is1("ORBHIP_CAND_PACK");
    s.flow = is1("ORBHIP_RZ_FLOW");
    return s;
}

}  // namespace

struct ExtractWorkspace {
    int device = 0;
    const orbhip_orb_params* prm = nullptr;
    const OrbTables* tab = nullptr;
    StageTimer* timer = nullptr;
    GraphCache* graphs = nullptr;
    hipStream_t stream = nullptr;
    std::map<PlanKey, std::shared_ptr<Plan>> plans;   // shared with other contexts (plan_cache)
    int cone_tile = 0, fast_nt = 0;                   // extract_set_hints
    // per-batch scratch (grown on demand)
    DevBuf<uint8_t> d_pyr;
    DevBuf<uint32_t> d_cand, d_kscratch;
    DevBuf<uint32_t> d_cprim;   // FAST candidates' primary slots (kCandPrim per cell)
    DevBuf<uint16_t> d_nscratch;
    DevBuf<int> d_cand_cnt, d_lvl_cnt, d_lvl_nlap, d_err;
    DevBuf<int> d_cand_off, d_cand_fill;   // packed FAST candidates (batches, CandPack)
    DevBuf<int> d_flow;   // k_pyr_flow: kFlowCtl control words + B x nbt band flags, zeroed when (re)allocated
    DevBuf<LevelKp> d_lvl_kp;
    // the one-frame host-image path: the frame and its outputs
    DevBuf<uint8_t> d_in, d_desc;
    DevBuf<orbhip_kp> d_kps;
    DevBuf<int32_t> d_n, d_mono;
    // the stereo stage (stereo.cpp): per-keypoint scratch and the host call's outputs
    DevBuf<int32_t> d_st_status, d_st_sad, d_st_best, d_st_nst;
    DevBuf<float> d_st_u, d_st_depth;
    // Bumped whenever a buffer above is reallocated. A captured launch sequence holds the scratch
    // addresses, so its key (run_extract) names the workspace and this count: a key that lists
    // the pointers is only as sound as the list, and d_flow was once missing from it.
    uint64_t gen = 0;
    template <typename T>
    hipError_t grow(DevBuf<T>& b, size_t count) {
        if (count > b.n || !b.p) gen++;
        return b.ensure(count);
    }
};

ExtractWorkspace* extract_ws_create(int device, const orbhip_orb_params* prm, const OrbTables* tab, StageTimer* timer,
                                    GraphCache* graphs, hipStream_t st) {
    ExtractWorkspace* ws = new ExtractWorkspace();
    ws->device = device; ws->prm = prm; ws->tab = tab; ws->timer = timer; ws->graphs = graphs; ws->stream = st;
    return ws;
}
void extract_ws_destroy(ExtractWorkspace* ws) { delete ws; }
void extract_set_hints(ExtractWorkspace* ws, int cone_tile, int fast_nt) {
    ws->cone_tile = cone_tile;
    ws->fast_nt = fast_nt;
}

// The plan of a frame size under the plan switches as they are now. The workspace's map is keyed
// by the full PlanKey, so a switch changed in the environment takes effect on a live context too.
static int find_plan(ExtractWorkspace* ws, int w, int h, Plan** out) {
    PlanKey k;
    std::memset(&k, 0, sizeof(k));
    const orbhip_orb_params& prm = *ws->prm;
    k.device = ws->device; k.w = w; k.h = h; k.nfeat = prm.n_features; k.nlev = prm.n_levels;
    k.ini = prm.ini_th_fast; k.mn = prm.min_th_fast; k.scale = prm.scale_factor;
    k.sw = read_plan_switches(ws->cone_tile);
    auto it = ws->plans.find(k);
    if (it != ws->plans.end()) { *out = it->second.get(); return ORBHIP_OK; }
    std::lock_guard<std::mutex> g(g_plan_m);
    std::shared_ptr<Plan> sp = plan_cache()[k].lock();
    if (!sp) {
        sp = std::make_shared<Plan>();
        if (int rc = plan_build_host(prm, *ws->tab, w, h, k.sw, sp->hp)) return rc;
        if (int rc = upload_plan(*sp)) return rc;
        plan_cache()[k] = sp;
    }
    *out = sp.get();
    ws->plans[k] = sp;
    return ORBHIP_OK;
}

static int ensure_batch(ExtractWorkspace* ws, const Plan* pl, int B) {
    const ExtractPlan& P = pl->hp.h;
    HIPOK(ws->grow(ws->d_pyr, (size_t)B * P.pyr_bytes));
    HIPOK(ws->grow(ws->d_cand, (size_t)B * P.n_slots_total));
    HIPOK(ws->grow(ws->d_cprim, (size_t)B * P.n_cells_total * kCandPrim));
    HIPOK(ws->grow(ws->d_kscratch, (size_t)B * P.n_slots_total));
    HIPOK(ws->grow(ws->d_nscratch, (size_t)B * P.n_slots_total));
    HIPOK(ws->grow(ws->d_cand_cnt, (size_t)B * P.n_cells_total));
    HIPOK(ws->grow(ws->d_cand_off, (size_t)B * P.n_cells_total));
    HIPOK(ws->grow(ws->d_cand_fill, (size_t)B * kMaxLevels));
    if (pl->hp.flow_nbt) {
        const uint64_t was = ws->gen;
        HIPOK(ws->grow(ws->d_flow, kFlowCtl + (size_t)B * pl->hp.flow_nbt));
        if (ws->gen != was) HIPOK(hipMemset(ws->d_flow.p, 0, ws->d_flow.n * sizeof(int)));
    }
    HIPOK(ws->grow(ws->d_lvl_kp, (size_t)B * P.kp_slots_total));
    HIPOK(ws->grow(ws->d_lvl_cnt, (size_t)B * P.n_levels));
    HIPOK(ws->grow(ws->d_lvl_nlap, (size_t)B * P.n_levels));
    HIPOK(ws->grow(ws->d_err, 4));
    return ORBHIP_OK;
}

// The pyramid stage: levels 1..L-1 of B frames into ws->d_pyr (ensure_batch first). Every route
// writes every level of every frame there, and no later stage of the extraction writes to it.
static void launch_pyramid(ExtractWorkspace* ws, Plan* pl, FrameBufs& fb, int B, const RunSwitches& sw, bool flow_on,
                           hipStream_t st) {
    const ExtractPlan& P = pl->hp.h;
    StageTimer& tm = *ws->timer;
    // the cone recomputes each tile's halo on every level: it pays only while the per-level
    // cascade is launch-latency bound (a few work-groups per CU); big batches keep the cascade
    static const size_t cone_max = std::getenv("ORBHIP_CONE_MAX_WG")
                                       ? (size_t)std::atol(std::getenv("ORBHIP_CONE_MAX_WG"))
                                       : (size_t)1024;
    const bool cone_path = pl->hp.cone_tiles && !sw.no_cone && (size_t)B * pl->hp.cone_tiles <= cone_max;
    const bool cone_hi = !cone_path && pl->hp.cone_hi_tiles && sw.cone_hi;
    // the one-launch pyramid stamps its own execution span for the stage timer
    fb.stamp = (cone_path && tm.stage == 1 && tm.dstamp && tm.n < StageTimer::kCap) ? tm.dstamp + tm.n : nullptr;
    if (cone_path) {
        static const int cone_nt = [] {   // threads per tile (A/B: ORBHIP_CONE_NT = 256 / 512)
            const char* e = std::getenv("ORBHIP_CONE_NT");
            const int v = e ? std::atoi(e) : 1024;
            return (v == 256 || v == 512) ? v : 1024;
        }();
        launch_pyr_cone(pl->d_plan.p, pl->hp.cone_tiles, pl->hp.cone_lds, fb, B, pl->d_cone.p, pl->d_cone_tab.p,
                        pl->hp.cone_tab_stride, st, 0, cone_nt, pl->d_xofs.p, pl->d_xalpha.p, pl->d_yofs.p,
                        pl->d_ybeta.p);
    } else if (flow_on) {
        PyrFlow fa{};
        fa.ctl = ws->d_flow.p;
        fa.flags = ws->d_flow.p + kFlowCtl;
        fa.dep = (const int2*)pl->d_flow_dep.p;
        for (int l = 0; l <= kMaxLevels; l++) fa.boff[l] = pl->hp.flow_boff[l];
        fa.B = B;
        fa.nbt = pl->hp.flow_nbt;
        fa.pyr_limit = (int)((int64_t)B * P.pyr_bytes);
        launch_pyr_flow(pl->d_plan.p, fb, pl->d_xofs.p, pl->d_xalpha.p, pl->d_yofs.p, pl->d_ybeta.p, fa, st);
    } else {
        const bool bands = !cone_hi && pl->hp.nbands > 0;
        const int lr = cone_hi ? kConeHiStart + 1 : (bands ? kBandStart + 1 : P.n_levels);
        for (int l = 1; l < lr; l++)
            launch_resize(pl->d_plan.p, P, fb, B, l, pl->d_xofs.p, pl->d_xalpha.p, pl->d_yofs.p, pl->d_ybeta.p,
                          st);
        if (cone_hi)
            launch_pyr_cone(pl->d_plan.p, pl->hp.cone_hi_tiles, pl->hp.cone_hi_lds, fb, B, pl->d_cone_hi.p,
                            pl->d_cone_hi_tab.p, pl->hp.cone_hi_tab_stride, st, kConeHiStart, cone_hi_threads(),
                            pl->d_xofs.p, pl->d_xalpha.p, pl->d_yofs.p, pl->d_ybeta.p);
        if (bands)
            launch_resize_bands(pl->d_plan.p, pl->hp.nbands, fb, B, kBandStart, (const int2*)pl->d_bands.p,
                                pl->d_xofs.p, pl->d_xalpha.p, pl->d_yofs.p, pl->d_ybeta.p, st);
    }
}

static int run_extract(ExtractWorkspace* ws, Plan* pl, const uint8_t* d_imgs, int B, int stride, int64_t fstride,
                       int lap0, int lap1, orbhip_kp* d_kps, uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono,
                       hipStream_t st) {
    const ExtractPlan& P = pl->hp.h;
    (void)hipGetLastError();   // clear a sticky error of an earlier, already-reported call
    int rc = ensure_batch(ws, pl, B);
    if (rc) return rc;
    const RunSwitches sw = read_run_switches();
    const bool flow_on = sw.flow && pl->hp.flow_nbt > 0 && (int64_t)B * P.pyr_bytes < (1ll << 31);
    GraphKey key;
    key.add(1).add((uint64_t)sw.oct_fast).add((uint64_t)sw.oct_max_dh).add((uint64_t)sw.no_cone)
        .add((uint64_t)sw.cone_hi).add((uint64_t)flow_on).add((uint64_t)sw.pack).add((uint64_t)ws->fast_nt).ptr(pl)
        .ptr(d_imgs).add((uint64_t)B).add((uint64_t)stride).add((uint64_t)fstride).add((uint64_t)lap0)
        .add((uint64_t)lap1).ptr(d_kps).ptr(d_desc).add((uint64_t)cap).ptr(d_n).ptr(d_mono).ptr(st)
        .ptr(ws).add(ws->gen);   // the scratch as a whole (ExtractWorkspace::gen)
    return ws->graphs->run(key, st, ws->timer->stage != 0, [&](hipStream_t st) -> int {
        FrameBufs fb;
        fb.in = d_imgs; fb.in_stride = stride; fb.in_fstride = fstride; fb.pyr = ws->d_pyr.p;
        StageTimer& tm = *ws->timer;
        const StageScope scope(tm);
        tm.begin(1, st);
        launch_pyramid(ws, pl, fb, B, sw, flow_on, st);
        tm.end(1, st);
        tm.begin(2, st);
        CandPack cp;
        cp.prim = ws->d_cprim.p;
        if (sw.pack) {
            HIPOK(hipMemsetAsync(ws->d_cand_fill.p, 0, sizeof(int) * (size_t)B * kMaxLevels, st));
            cp.fill = ws->d_cand_fill.p;
            cp.off = ws->d_cand_off.p;
        }
        launch_fast(pl->d_plan.p, P, pl->d_cells.p, fb, B, ws->d_cand.p, ws->d_cand_cnt.p, ws->d_err.p, st,
                    ws->fast_nt, cp);
        tm.end(2, st);
        OctreeCfg oc = pl->hp.oct;
        oc.lap0 = lap0; oc.lap1 = lap1;
        oc.fast = sw.oct_fast;
        oc.max_dh = sw.oct_max_dh;
        tm.begin(3, st);
        launch_octree(pl->d_plan.p, P, pl->d_cells.p, pl->d_otab.p, ws->d_cand.p, cp.off ? nullptr : cp.prim,
                      ws->d_cand_cnt.p, cp.off, ws->d_kscratch.p, ws->d_nscratch.p, ws->d_lvl_kp.p, ws->d_lvl_cnt.p,
                      ws->d_lvl_nlap.p, oc, ws->d_err.p, B, st,
                      (tm.stage == 3 && tm.dstamp && tm.n < StageTimer::kCap) ? tm.dstamp + tm.n : nullptr);
        tm.end(3, st);
        tm.begin(4, st);
        launch_desc(pl->d_plan.p, P, fb, ws->d_lvl_kp.p, ws->d_lvl_cnt.p, ws->d_lvl_nlap.p, pl->d_disc.p, d_kps,
                    d_desc, cap, d_n, d_mono, B, st);
        tm.end(4, st);
        HIPOK(hipGetLastError());
        return ORBHIP_OK;
    });
}

int extract_max_keypoints(ExtractWorkspace* ws, int w, int h) {
    Plan* pl = nullptr;
    const int rc = find_plan(ws, w, h, &pl);
    return rc ? rc : pl->hp.kp_cap_frame;
}

int extract_batch(ExtractWorkspace* ws, const uint8_t* d_imgs, int B, int w, int h, int stride, int64_t fstride,
                  int lap0, int lap1, orbhip_kp* d_kps, uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono,
                  hipStream_t st) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    return run_extract(ws, pl, d_imgs, B, stride, fstride, lap0, lap1, d_kps, d_desc, cap, d_n, d_mono, st);
}

// B host images (1 or 2) through the workspace's own frame and output buffers, on the context's
// stream; frame f's outputs at f * kp_cap_frame. pyramid_only: the pyramid stage alone.
static int run_host_frames(ExtractWorkspace* ws, Plan* pl, const uint8_t* const* imgs, int B, int w, int h, int stride,
                           int lap0, int lap1, bool pyramid_only = false) {
    const int kcap = pl->hp.kp_cap_frame;
    HIPOK(ws->grow(ws->d_in, (size_t)B * w * h));
    HIPOK(ws->grow(ws->d_kps, (size_t)B * kcap));
    HIPOK(ws->grow(ws->d_desc, (size_t)B * kcap * 32));
    HIPOK(ws->grow(ws->d_n, B));
    HIPOK(ws->grow(ws->d_mono, B));
    for (int f = 0; f < B; f++)
        HIPOK(hipMemcpy2DAsync(ws->d_in.p + (size_t)f * w * h, w, imgs[f], stride, w, h, hipMemcpyHostToDevice,
                               ws->stream));
    if (pyramid_only) {
        (void)hipGetLastError();
        if (int rc = ensure_batch(ws, pl, B)) return rc;
        const RunSwitches sw = read_run_switches();
        const bool flow_on = sw.flow && pl->hp.flow_nbt > 0 && (int64_t)B * pl->hp.h.pyr_bytes < (1ll << 31);
        FrameBufs fb;
        fb.in = ws->d_in.p; fb.in_stride = w; fb.in_fstride = (int64_t)w * h; fb.pyr = ws->d_pyr.p;
        launch_pyramid(ws, pl, fb, B, sw, flow_on, ws->stream);
        HIPOK(hipGetLastError());
        return ORBHIP_OK;
    }
    return run_extract(ws, pl, ws->d_in.p, B, w, (int64_t)w * h, lap0, lap1, ws->d_kps.p, ws->d_desc.p, kcap,
                       ws->d_n.p, ws->d_mono.p, ws->stream);
}
static int run_host_frame(ExtractWorkspace* ws, Plan* pl, const uint8_t* img, int w, int h, int stride, int lap0,
                          int lap1) {
    return run_host_frames(ws, pl, &img, 1, w, h, stride, lap0, lap1);
}

// ---- what the stereo stage (stereo.cpp) needs of the workspace ----
int extract_view(ExtractWorkspace* ws, int w, int h, ExtractView* v) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    v->plan = &pl->hp.h;
    v->d_plan = pl->d_plan.p;
    v->kp_cap = pl->hp.kp_cap_frame;
    v->stream = ws->stream;
    // (the buffers as they are now: read them after the extraction of the same call)
    v->d_pyr = ws->d_pyr.p; v->d_in = ws->d_in.p; v->d_kps = ws->d_kps.p; v->d_desc = ws->d_desc.p;
    v->d_n = ws->d_n.p; v->d_err = ws->d_err.p;
    return ORBHIP_OK;
}

int extract_stereo_scratch(ExtractWorkspace* ws, size_t entries, int pairs, bool outputs, StereoScratch* s) {
    HIPOK(ws->grow(ws->d_st_status, entries));
    HIPOK(ws->grow(ws->d_st_sad, entries));
    if (outputs) {
        HIPOK(ws->grow(ws->d_st_best, entries));
        HIPOK(ws->grow(ws->d_st_u, entries));
        HIPOK(ws->grow(ws->d_st_depth, entries));
        HIPOK(ws->grow(ws->d_st_nst, pairs));
    }
    s->status = ws->d_st_status.p; s->sad = ws->d_st_sad.p; s->best = ws->d_st_best.p;
    s->u_right = ws->d_st_u.p; s->depth = ws->d_st_depth.p; s->n_stereo = ws->d_st_nst.p;
    return ORBHIP_OK;
}

int extract_host_pair(ExtractWorkspace* ws, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                      bool pyramid_only) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    const uint8_t* imgs[2] = {left, right};
    return run_host_frames(ws, pl, imgs, 2, w, h, stride, 0, 0, pyramid_only);
}

int extract_host(ExtractWorkspace* ws, const uint8_t* img, int w, int h, int stride, int lap0, int lap1,
                 orbhip_kp* kps, uint8_t* desc32, int cap, int* n_out, int* mono_index) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    if (int rc = run_host_frame(ws, pl, img, w, h, stride, lap0, lap1)) return rc;
    hipStream_t st = ws->stream;
    int n = 0, mono = 0, err[4] = {0, 0, 0, 0};
    HIPOK(hipMemcpyAsync(&n, ws->d_n.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&mono, ws->d_mono.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(err, ws->d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (err[0]) return ORBHIP_ERR_DEVICE;
    *n_out = n;
    if (mono_index) *mono_index = mono;
    if (n > cap) return ORBHIP_ERR_CAPACITY;
    if (n > 0) {
        HIPOK(hipMemcpyAsync(kps, ws->d_kps.p, (size_t)n * sizeof(orbhip_kp), hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(desc32, ws->d_desc.p, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
    }
    return ORBHIP_OK;
}

// Debug hook: run one frame and return the intermediates (pyramid levels 1.., candidates
// per cell, octree output per level) so a mismatch can be localised offline.
// pyr: sum_{l>=1} w_l*h_l bytes (packed, no pitch); cand: n_slots_total u32; cand_cnt:
// n_cells_total; lvl: kp_slots_total LevelKp (8 B each); lvl_cnt/lvl_nlap: n_levels;
// sizes: n_slots_total, n_cells_total, kp_slots_total, err.
int extract_test_debug(ExtractWorkspace* ws, const uint8_t* img, int w, int h, int lap0, int lap1, uint8_t* pyr,
                       uint32_t* cand, int32_t* cand_cnt, void* lvl, int32_t* lvl_cnt, int32_t* lvl_nlap,
                       int32_t* sizes) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    const ExtractPlan& P = pl->hp.h;
    sizes[0] = P.n_slots_total; sizes[1] = P.n_cells_total; sizes[2] = P.kp_slots_total;
    if (!pyr) return ORBHIP_OK;   // size query
    if (int rc = run_host_frame(ws, pl, img, w, h, w, lap0, lap1)) return rc;
    HIPOK(hipStreamSynchronize(ws->stream));
    size_t off = 0;
    for (int l = 1; l < P.n_levels; l++) {
        const LevelGeom& G = P.lv[l];
        HIPOK(hipMemcpy2D(pyr + off, G.w, ws->d_pyr.p + G.pyr_off, G.pitch, G.w, G.h, hipMemcpyDeviceToHost));
        off += (size_t)G.w * G.h;
    }
    HIPOK(hipMemcpy(cand, ws->d_cand.p, (size_t)P.n_slots_total * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(cand_cnt, ws->d_cand_cnt.p, (size_t)P.n_cells_total * 4, hipMemcpyDeviceToHost));
    {   // each cell's first kCandPrim candidates sit in its primary slots: back into its slot range
        std::vector<uint32_t> prim((size_t)P.n_cells_total * kCandPrim);
        HIPOK(hipMemcpy(prim.data(), ws->d_cprim.p, prim.size() * 4, hipMemcpyDeviceToHost));
        for (int ci = 0; ci < P.n_cells_total; ci++)
            for (int j = 0; j < std::min(cand_cnt[ci], kCandPrim); j++)
                cand[pl->hp.cells[ci].slot_off + j] = prim[(size_t)ci * kCandPrim + j];
    }
    HIPOK(hipMemcpy(lvl, ws->d_lvl_kp.p, (size_t)P.kp_slots_total * sizeof(LevelKp), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(lvl_cnt, ws->d_lvl_cnt.p, (size_t)P.n_levels * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(lvl_nlap, ws->d_lvl_nlap.p, (size_t)P.n_levels * 4, hipMemcpyDeviceToHost));
    int err[4];
    HIPOK(hipMemcpy(err, ws->d_err.p, sizeof(err), hipMemcpyDeviceToHost));
    sizes[3] = err[0];
    return ORBHIP_OK;
}

// FAST candidates of frame `frame` of the context's last extraction at w x h (sum over its cells):
// the octree's input size, for the bench's algorithmic bytes of k_octree
int extract_test_candidates(ExtractWorkspace* ws, int w, int h, int frame, int64_t* n) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    const size_t nc = (size_t)pl->hp.h.n_cells_total;
    if (!ws->d_cand_cnt.p || ws->d_cand_cnt.n < (frame + 1) * nc) return ORBHIP_ERR_ARG;
    std::vector<int> cnt(nc);
    HIPOK(hipStreamSynchronize(ws->stream));
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemcpy(cnt.data(), ws->d_cand_cnt.p + frame * nc, nc * sizeof(int), hipMemcpyDeviceToHost));
    int64_t s = 0;
    for (int v : cnt) s += v;
    *n = s;
    return ORBHIP_OK;
}

// Cell table of a plan (level, x0, y0, wc, hc, slot_off per cell) for offline checks.
int extract_test_cells(ExtractWorkspace* ws, int w, int h, int32_t* out6, int cap) {
    Plan* pl = nullptr;
    if (int rc = find_plan(ws, w, h, &pl)) return rc;
    const int n = (int)pl->hp.cells.size();
    if (n > cap) return n;
    for (int i = 0; i < n; i++) {
        const CellGeom& g = pl->hp.cells[i];
        out6[6 * i + 0] = g.level; out6[6 * i + 1] = g.x0; out6[6 * i + 2] = g.y0;
        out6[6 * i + 3] = g.wc; out6[6 * i + 4] = g.hc; out6[6 * i + 5] = g.slot_off;
    }
    return n;
}

}  // namespace orbhip
