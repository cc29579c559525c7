// The extraction planner: every table of one (image size, ORB params, plan switches)
// configuration, as plain host data. No HIP: extract.cpp uploads a HostPlan, a CPU program can
// build and check one (tests/cpp/extract_plan_check.cpp).
#pragma once
#include <cmath>
#include <vector>

#include "../../include/orbhip.h"
#include "orbhip_plan.h"

namespace orbhip {

constexpr int kConeHiStart = 2;   // batches: k_resize for levels 1..2, one cone launch for the rest
constexpr int kBandStart = 2;     // batches: k_resize for levels 1..2, k_resize_bands for the rest

inline int round_even_f(float v) { return (int)std::nearbyintf(v); }

// ORBextractor ctor tables
struct OrbTables {
    std::vector<float> scale, inv_scale;
    std::vector<int> feat, umax;
    int blurk[7] = {0};
};
OrbTables build_orb_tables(const orbhip_orb_params& prm);

// The environment switches a plan depends on, as read (plan_build_host validates them). They are
// part of the plan's cache key and read per plan lookup, so a change takes effect on a live context.
struct PlanSwitches {
    int cone_tile;      // k_pyr_cone tile edge in last-level pixels: ORBHIP_CONE_TILE, else the
                        // context's hint, else 10 (the one-frame latency optimum)
    int cone_hi_tile;   // the batch cone's: ORBHIP_CONE_HI_TILE (at least 4), else 32
    // row bands per frame of k_resize_bands: ORBHIP_RZ_BANDS, default 0 = every level by k_resize
    // (clamped to the last level's rows). Opt-in: at C3 the band launch measured 400-1200 us for
    // 8-64 bands against the 95 us of the five k_resize launches it replaces (tools/c3_pyr_sweep.sh)
    int rz_bands;
    // ORBHIP_FAST_CLIST_CAP lowers the survivor list (tests force the dense FAST pass with 0);
    // -1 = unset = kClistCap, else clamped to [0, kClistCap]
    int clist_cap;
    // ORBHIP_FAST_NT pins k_fast_cells' threads per cell (A/B and tests): -1 = unset, 128, 256, 512
    // or 1024; any other value is rejected loudly and the batch-size choice stays
    int fast_nt;
};
PlanSwitches read_plan_switches(int cone_tile_hint);

struct HostPlan {
    ExtractPlan h{};
    std::vector<CellGeom> cells;
    std::vector<int> xofs, xalpha, yofs, ybeta, disc;
    std::vector<uint16_t> otab;   // k_octree interval tables (LevelGeom::oct_tab_off)
    std::vector<ConeRect> cone;   // k_pyr_cone tables (empty: per-level k_resize cascade)
    std::vector<int> cone_tab;    // per tile: every level's resize tables in the kernel's LDS layout
    int cone_tab_stride = 0, cone_tiles = 0;
    size_t cone_lds = 0;
    // the same for batches: levels kConeHiStart+1..L-1 in one launch behind the first
    // kConeHiStart k_resize levels (empty: all levels by k_resize)
    std::vector<ConeRect> cone_hi;
    std::vector<int> cone_hi_tab;
    int cone_hi_tab_stride = 0, cone_hi_tiles = 0;
    size_t cone_hi_lds = 0;
    // batches: levels kBandStart+1..L-1 by k_resize_bands, the output rows of each (band, level)
    std::vector<int> bands;   // [nbands][kMaxLevels] (r0, r1) pairs
    int nbands = 0;
    // batches: k_pyr_flow's 16-row bands (level 1 first), the level l-1 bands each band's source
    // rows lie in
    int flow_boff[kMaxLevels + 1] = {0};
    int flow_nbt = 0;
    std::vector<int> flow_dep;   // (b0, b1) per band
    OctreeCfg oct{};
    int kp_cap_frame = 0;   // sum of level caps = max keypoints per frame
};

// ORBHIP_OK, or ORBHIP_ERR_UNSUPPORTED for a size, a parameter set or a table the kernels do not cover
int plan_build_host(const orbhip_orb_params& prm, const OrbTables& tab, int w, int h, const PlanSwitches& sw,
                    HostPlan& out);

}  // namespace orbhip
