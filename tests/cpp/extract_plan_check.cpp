// The extraction planner (csrc/extract_plan.cpp) on the host alone: builds HostPlans for a set of
// frame sizes, ORB parameters and plan switches, checks the invariants the kernels rely on and
// prints the ORBextractor ctor tables per shape. Exits non-zero on any violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "extract_plan.h"

using namespace orbhip;

static int g_fail = 0;
static char g_what[256];
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            if (g_fail++ < 40) std::printf("FAIL %s: %s (line %d)\n", g_what, #cond, __LINE__); \
        }                                                                                   \
    } while (0)

// last_h: rows of the last level (ComputePyramid's rounding), checked for every shape
struct Shape { int w, h, L; float sf; int nfeat; bool ok; int last_h; };
// the largest nfeatures that plans at 320x240, 8 levels, 1.2 (tests/test_extract_cases.py finds the
// same value by bisection over this program's "plan" mode)
constexpr int kNStar = 6158;
static const Shape kShapes[] = {
    // 67 rows is the smallest last level that plans: its cell area (rows 16 .. h - 16) holds one
    // 35-px cell row from 67 rows on (ComputeKeyPointsOctTree's nRows = (h - 32) / 35)
    {320, 240, 8, 1.2f, 1000, true, 67},  {641, 479, 8, 1.2f, 1000, true, 134},
    // One row less has nRows = 0, and so have the two shapes whose last level is exactly 64 rows,
    // the smallest height the level-size check admits: all three return UNSUPPORTED, from the cell
    // grid. The planner must return the same cases as it did inside the C-ABI file, where
    // orbhip_max_keypoints gives ORBHIP_ERR_UNSUPPORTED for each of these sizes.
    {316, 237, 8, 1.2f, 1000, false, 66},  {306, 230, 8, 1.2f, 1000, false, 64},
    {306, 228, 8, 1.2f, 1000, false, 64},
    {320, 240, 2, 2.0f, 1000, false, 120},   // exact 2x: OpenCV's INTER_AREA case
    {320, 240, 1, 1.2f, 1000, true, 240},  {320, 240, 2, 1.2f, 1000, true, 200},
    {320, 240, 3, 1.2f, 1000, true, 167},  {320, 240, 4, 1.2f, 1000, true, 139},
    {641, 481, 5, 1.5f, 1000, true, 95},  {1001, 751, 3, 2.5f, 1000, true, 120},   // the per-row resize path
    // The envelope catalogue of tests/extract_cases.py (the kernels run at these shapes on the GPU).
    // One level: 67x67 is the smallest frame that plans (one 35x35 cell, one root), 101x101 the
    // largest single cell (69x69, window 75), 102x102 the first 2x2 grid, 136x101 two roots.
    {67, 67, 1, 1.2f, 100, true, 67},  {101, 101, 1, 1.2f, 200, true, 101},  {102, 102, 1, 1.2f, 200, true, 102},
    {136, 101, 1, 1.2f, 200, true, 101},
    // box 101x68 (ratio 1.485, one root) against box 102x68 (ratio 1.5, two): std::round in n_ini
    {133, 100, 1, 1.2f, 100, true, 100},  {134, 100, 1, 1.2f, 100, true, 100},
    {240, 240, 8, 1.2f, 1000, true, 67},   // the smallest square 8-level frame
    // strips: one cell row per level; 32 roots; 61 roots and a 4068-px box, next to both limits
    {1000, 100, 2, 1.2f, 500, true, 83},  {2200, 100, 1, 1.2f, 500, true, 100},  {4100, 99, 1, 1.2f, 500, true, 99},
    {640, 480, 8, 1.2f, 1, true, 134},  {640, 480, 8, 1.2f, 7, true, 134},   // levels with a quota of 0
    {320, 240, 8, 1.2f, 7, true, 67},                                         // ... and two roots
    // the octree's LDS budget bounds nfeatures at 320x240: kNStar is the largest that plans
    {320, 240, 8, 1.2f, 5000, true, 67},  {320, 240, 8, 1.2f, kNStar, true, 67},
    {320, 240, 8, 1.2f, kNStar + 1, false, 67},  {320, 240, 8, 1.2f, 20000, false, 67},
    {640, 480, 9, 1.2f, 1000, true, 112},  {640, 480, 12, 1.1f, 1000, true, 168},   // more than 8 levels
    {1920, 1080, 8, 1.2f, 2000, true, 301},
    // rejected: no cell row / column; a portrait strip whose root count rounds to 0; past the root
    // and box limits
    {66, 67, 1, 1.2f, 100, false, 67},  {67, 66, 1, 1.2f, 100, false, 66},  {100, 1000, 1, 1.2f, 100, false, 1000},
    {4400, 99, 1, 1.2f, 500, false, 99},
};
static const PlanSwitches kDefault = {10, 32, 0, -1, -1};

static bool taps_ok(int packed) {
    const int t0 = (int)(short)(packed & 0xFFFF), t1 = (int)(short)(packed >> 16);
    return t0 >= 0 && t1 >= 0 && t0 + t1 <= 2049;
}
static int clampi(int v, int n) { return v < 0 ? 0 : (v < n ? v : n - 1); }

// One cone table set from source level s0: rects (kMaxLevels per tile), per-tile resize tables.
static void check_cone(const HostPlan& hp, int s0, const std::vector<ConeRect>& rects, const std::vector<int>& tab,
                       int stride, int tiles, size_t lds) {
    const ExtractPlan& P = hp.h;
    const int L = P.n_levels;
    if (tiles == 0) {
        CHECK(rects.empty() && tab.empty());
        return;
    }
    CHECK(lds <= 60 * 1024);
    CHECK(rects.size() == (size_t)tiles * kMaxLevels);
    CHECK(tab.size() == (size_t)tiles * stride);
    if (rects.size() != (size_t)tiles * kMaxLevels || tab.size() != (size_t)tiles * stride) return;
    for (int l = s0 + 1; l < L; l++) {   // the own rectangles tile the level exactly once
        const LevelGeom& G = P.lv[l];
        std::vector<uint8_t> cover((size_t)G.w * G.h, 0);
        bool once = true;
        for (int t = 0; t < tiles; t++) {
            const ConeRect& r = rects[(size_t)t * kMaxLevels + l];
            const bool in =
                0 <= r.ox0 && r.ox0 <= r.ox1 && r.ox1 <= G.w && 0 <= r.oy0 && r.oy0 <= r.oy1 && r.oy1 <= G.h;
            CHECK(in);
            if (!in) continue;
            for (int y = r.oy0; y < r.oy1; y++)
                for (int x = r.ox0; x < r.ox1; x++) once &= ++cover[(size_t)y * G.w + x] == 1;
        }
        for (uint8_t c : cover) once &= c == 1;
        CHECK(once);
    }
    for (int t = 0; t < tiles; t++) {
        const ConeRect* R = &rects[(size_t)t * kMaxLevels];
        size_t len = 0;
        for (int l = s0; l < L; l++) {
            const LevelGeom& G = P.lv[l];   // need inside the level (l == s0: the staged source)
            const ConeRect& r = R[l];
            CHECK(0 <= r.nx0 && r.nx0 <= r.nx1 && r.nx1 <= G.w && 0 <= r.ny0 && r.ny0 <= r.ny1 && r.ny1 <= G.h);
            if (l > s0 && r.ox1 > r.ox0 && r.oy1 > r.oy0)   // need contains own
                CHECK(r.nx0 <= r.ox0 && r.ox1 <= r.nx1 && r.ny0 <= r.oy0 && r.oy1 <= r.ny1);
        }
        const int* o = tab.data() + (size_t)t * stride;
        for (int l = s0 + 1; l < L; l++) {   // the tables index inside the source level, in the tile's need of it
            const int sw = P.lv[l - 1].w, sh = P.lv[l - 1].h;
            const ConeRect &r = R[l], &s = R[l - 1];
            const int nw = r.nx1 - r.nx0, nh = r.ny1 - r.ny0;
            len += 2 * (size_t)nw + 3 * (size_t)nh;
            if (len > (size_t)stride) break;
            bool in = true;
            for (int i = 0; i < nw; i++) in &= 0 <= o[i] && o[i] < sw && s.nx0 <= o[i] && o[i] < s.nx1;
            for (int j = 0; j < nh; j++)
                for (int k = 0; k < 2; k++) {
                    const int v = o[2 * nw + 3 * j + k];
                    in &= 0 <= v && v < sh && s.ny0 <= v && v < s.ny1;
                }
            CHECK(in);
            o += 2 * nw + 3 * nh;
        }
        CHECK(len <= (size_t)stride);
    }
}

static void check_plan(const HostPlan& hp, const PlanSwitches& sw) {
    const ExtractPlan& P = hp.h;
    const int L = P.n_levels;
    // cone and cone-hi tables
    check_cone(hp, 0, hp.cone, hp.cone_tab, hp.cone_tab_stride, hp.cone_tiles, hp.cone_lds);
    check_cone(hp, kConeHiStart, hp.cone_hi, hp.cone_hi_tab, hp.cone_hi_tab_stride, hp.cone_hi_tiles, hp.cone_hi_lds);
    if (L < 2) CHECK(hp.cone_tiles == 0);
    if (L < kConeHiStart + 2) CHECK(hp.cone_hi_tiles == 0);
    if (L > 1 && sw.cone_tile == 1000) CHECK(hp.cone_tiles == 0);   // one tile of > 60 KB: dropped
    // bands
    const int nb = hp.nbands;
    CHECK(nb == (L > kBandStart + 1 ? (sw.rz_bands < P.lv[L - 1].h ? sw.rz_bands : P.lv[L - 1].h) : 0));
    CHECK(hp.bands.size() == (nb ? (size_t)nb * kMaxLevels * 2 : 0));
    if (nb && hp.bands.size() == (size_t)nb * kMaxLevels * 2) {
        auto row = [&](int b, int l, int k) { return hp.bands[((size_t)b * kMaxLevels + l) * 2 + k]; };
        for (int l = kBandStart + 1; l < L; l++) {
            const LevelGeom& G = P.lv[l];
            std::vector<uint8_t> cover(G.h, 0);
            for (int b = 0; b < nb; b++) {
                const int r0 = row(b, l, 0), r1 = row(b, l, 1);
                CHECK(0 <= r0 && r0 <= r1 && r1 <= G.h);
                for (int r = r0; r < r1 && r < G.h; r++) cover[r < 0 ? 0 : r] = 1;
                if (l == L - 1) continue;
                const LevelGeom& U = P.lv[l + 1];   // the band's rows of level l + 1 read these rows of level l
                bool in = true;
                for (int r = row(b, l + 1, 0); r < row(b, l + 1, 1); r++)
                    for (int k = 0; k < 2; k++) {
                        const int s = clampi(hp.yofs[U.ytab_off + r] + k, G.h);
                        in &= r0 <= s && s < r1;
                    }
                CHECK(in);
            }
            bool all = true;
            for (uint8_t c : cover) all &= c == 1;
            CHECK(all);
        }
    }
    // flow
    CHECK(hp.flow_dep.size() == (size_t)hp.flow_nbt * 2);
    for (int l = 0; l < kMaxLevels; l++) CHECK(hp.flow_boff[l] <= hp.flow_boff[l + 1]);
    CHECK(hp.flow_boff[kMaxLevels] == hp.flow_nbt && hp.flow_boff[L < 1 ? 0 : L] == hp.flow_nbt);
    if (L < 2) CHECK(hp.flow_nbt == 0);
    for (int l = 2; l < L && hp.flow_dep.size() == (size_t)hp.flow_nbt * 2; l++) {
        const int nprev = hp.flow_boff[l] - hp.flow_boff[l - 1];
        CHECK(hp.flow_boff[l + 1] - hp.flow_boff[l] == (P.lv[l].h + 15) / 16);
        for (int b = hp.flow_boff[l]; b < hp.flow_boff[l + 1]; b++) {
            const int b0 = hp.flow_dep[2 * (size_t)b], b1 = hp.flow_dep[2 * (size_t)b + 1];
            CHECK(0 <= b0 && b0 <= b1 && b1 < nprev);
        }
    }
    // cells, candidate slots, keypoint slots
    CHECK((int)hp.cells.size() == P.n_cells_total);
    int slot = 0, cell = 0, kp = 0;
    for (int l = 0; l < L; l++) {
        const LevelGeom& G = P.lv[l];
        CHECK(G.cell_base == cell && G.slot_base == slot && G.kp_base == kp);
        for (int i = 0; i < G.n_cells && cell + i < (int)hp.cells.size(); i++) {
            const CellGeom& c = hp.cells[cell + i];
            CHECK(c.level == l && c.slot_off == slot && c.wc <= 76 && c.hc <= 76 && c.wc >= 0 && c.hc >= 0);
            const int dc = c.wc > 6 ? c.wc - 6 : 0, dr = c.hc > 6 ? c.hc - 6 : 0;
            slot += ((dc + 1) / 2) * ((dr + 1) / 2);
        }
        CHECK(G.n_slots == slot - G.slot_base);
        cell += G.n_cells;
        kp += G.kp_cap;
    }
    CHECK(slot == P.n_slots_total && cell == P.n_cells_total && kp == P.kp_slots_total && kp == hp.kp_cap_frame);
    // octree configuration
    CHECK(octree_lds_bytes(P, hp.oct) <= 160 * 1024);
    // tap flags: rz_noclamp only where every tap of the level passes
    for (int l = 1; l < L; l++) {
        const LevelGeom& G = P.lv[l];
        bool all = true, xin = true;
        for (int x = 0; x < G.w; x++) {
            all &= taps_ok(hp.xalpha[G.xtab_off + x]);
            xin &= 0 <= hp.xofs[G.xtab_off + x] && hp.xofs[G.xtab_off + x] < P.lv[l - 1].w;
        }
        for (int y = 0; y < G.h; y++) all &= taps_ok(hp.ybeta[G.ytab_off + y]);
        CHECK(xin);
        if (G.rz_noclamp == 1) CHECK(all);
    }
    // the validated switches
    CHECK(P.clist_cap == (sw.clist_cap < 0 || sw.clist_cap > kClistCap ? kClistCap : sw.clist_cap));
    const int nt = sw.fast_nt;
    CHECK(P.fast_nt == (nt == 128 || nt == 256 || nt == 512 || nt == 1024 ? nt : 0));
}

static bool same_level(const LevelGeom& a, const LevelGeom& b) {
#define F(x) if (a.x != b.x) return false;
    F(w) F(h) F(pitch) F(pyr_off) F(scale) F(n_feat) F(min_bx) F(max_bx) F(min_by) F(max_by) F(n_cols) F(n_rows)
    F(w_cell) F(h_cell) F(cell_base) F(n_cells) F(slot_base) F(n_slots) F(n_ini) F(hX) F(kp_cap) F(kp_base)
    F(rz_noclamp) F(oct_tab_off) F(patch_size) F(xtab_off) F(ytab_off) F(xmax) F(vend)
    return true;
}
template <typename T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same_plan(const HostPlan& a, const HostPlan& b) {
    const ExtractPlan &p = a.h, &q = b.h;
    {
        const ExtractPlan &a = p, &b = q;
        F(w) F(h) F(n_levels) F(n_cells_total) F(n_slots_total) F(kp_slots_total) F(pyr_bytes) F(ini_th) F(min_th)
        F(n_disc) F(max_cells_level) F(clist_cap) F(fast_nt) F(fast_win_rows) F(fast_win_cols)
    }
    F(cone_tab_stride) F(cone_tiles) F(cone_lds) F(cone_hi_tab_stride) F(cone_hi_tiles) F(cone_hi_lds) F(nbands)
    F(flow_nbt) F(kp_cap_frame) F(oct.node_cap) F(oct.sort_cap) F(oct.key_cap)
#undef F
    for (int l = 0; l < kMaxLevels; l++)
        if (!same_level(p.lv[l], q.lv[l])) return false;
    return std::memcmp(p.blurk, q.blurk, sizeof(p.blurk)) == 0 &&
           std::memcmp(a.flow_boff, b.flow_boff, sizeof(a.flow_boff)) == 0 && same_bytes(a.cells, b.cells) &&
           same_bytes(a.xofs, b.xofs) && same_bytes(a.xalpha, b.xalpha) && same_bytes(a.yofs, b.yofs) &&
           same_bytes(a.ybeta, b.ybeta) && same_bytes(a.disc, b.disc) && same_bytes(a.otab, b.otab) &&
           same_bytes(a.cone, b.cone) && same_bytes(a.cone_tab, b.cone_tab) && same_bytes(a.cone_hi, b.cone_hi) &&
           same_bytes(a.cone_hi_tab, b.cone_hi_tab) && same_bytes(a.bands, b.bands) &&
           same_bytes(a.flow_dep, b.flow_dep);
}

// "levels w h nfeat scale nlevels | widths | heights | features | scales | umax"
static void print_levels(int w, int h, int nfeat, float sf, int L) {
    const orbhip_orb_params prm = {nfeat, sf, L, 20, 7};
    const OrbTables t = build_orb_tables(prm);
    std::printf("levels %d %d %d %.9g %d |", w, h, nfeat, sf, L);
    for (int l = 0; l < L; l++) std::printf(" %d", round_even_f((float)w * t.inv_scale[l]));
    std::printf(" |");
    for (int l = 0; l < L; l++) std::printf(" %d", round_even_f((float)h * t.inv_scale[l]));
    std::printf(" |");
    for (int l = 0; l < L; l++) std::printf(" %d", t.feat[l]);
    std::printf(" |");
    for (int l = 0; l < L; l++) std::printf(" %.9g", t.scale[l]);
    std::printf(" |");
    for (int v : t.umax) std::printf(" %d", v);
    std::printf("\n");
}

// "plan w h nlevels scale nfeatures": one shape at the default switches. Prints "plan rc" and, when it
// plans, per level "level l w h n_cols n_rows w_cell h_cell n_cells n_ini n_feat kp_cap", the cell
// table as "cell level x0 y0 wc hc slots", and "octree node_cap sort_cap key_cap lds_bytes".
static int print_plan(int w, int h, int L, float sf, int nfeat) {
    const orbhip_orb_params prm = {nfeat, sf, L, 20, 7};
    HostPlan hp;
    const int rc = L < 1 || L > kMaxLevels ? ORBHIP_ERR_ARG : plan_build_host(prm, build_orb_tables(prm), w, h, kDefault, hp);
    std::printf("plan %d\n", rc);
    if (rc != ORBHIP_OK) return 0;
    std::snprintf(g_what, sizeof(g_what), "%dx%d L%d sf%g nfeat%d", w, h, L, sf, nfeat);
    check_plan(hp, kDefault);
    for (int l = 0; l < L; l++) {
        const LevelGeom& G = hp.h.lv[l];
        std::printf("level %d %d %d %d %d %d %d %d %d %d %d\n", l, G.w, G.h, G.n_cols, G.n_rows, G.w_cell, G.h_cell,
                    G.n_cells, G.n_ini, G.n_feat, G.kp_cap);
    }
    for (size_t i = 0; i < hp.cells.size(); i++) {
        const CellGeom& c = hp.cells[i];
        const int next = i + 1 < hp.cells.size() ? hp.cells[i + 1].slot_off : hp.h.n_slots_total;
        std::printf("cell %d %d %d %d %d %d\n", c.level, c.x0, c.y0, c.wc, c.hc, next - c.slot_off);
    }
    std::printf("octree %d %d %d %zu\n", hp.oct.node_cap, hp.oct.sort_cap, hp.oct.key_cap,
                octree_lds_bytes(hp.h, hp.oct));
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && std::strcmp(argv[1], "plan") == 0)
        return print_plan(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), (float)std::atof(argv[5]),
                          std::atoi(argv[6]));
    std::vector<PlanSwitches> sws = {kDefault};
    auto vary = [&](int PlanSwitches::*m, std::initializer_list<int> vals) {
        for (int v : vals) {
            PlanSwitches s = kDefault;
            s.*m = v;
            sws.push_back(s);
        }
    };
    vary(&PlanSwitches::cone_tile, {4, 16, 1000});
    vary(&PlanSwitches::cone_hi_tile, {4});
    vary(&PlanSwitches::rz_bands, {1, 5, 16, 100000});
    vary(&PlanSwitches::clist_cap, {0, 2048, 5000});
    vary(&PlanSwitches::fast_nt, {0, 128, 300});
    int built = 0;
    for (const Shape& s : kShapes) {
        const orbhip_orb_params prm = {s.nfeat, s.sf, s.L, 20, 7};
        const OrbTables tab = build_orb_tables(prm);
        print_levels(s.w, s.h, s.nfeat, s.sf, s.L);
        int rc_default = 0;
        for (const PlanSwitches& sw : sws) {
            std::snprintf(g_what, sizeof(g_what), "%dx%d L%d sf%g tile%d hi%d bands%d cap%d nt%d", s.w, s.h, s.L, s.sf,
                          sw.cone_tile, sw.cone_hi_tile, sw.rz_bands, sw.clist_cap, sw.fast_nt);
            HostPlan a, b;
            const int rc = plan_build_host(prm, tab, s.w, s.h, sw, a);
            // what a shape returns does not depend on the switches: reported once, at the default ones
            if (&sw == &sws[0]) CHECK(rc == (s.ok ? ORBHIP_OK : ORBHIP_ERR_UNSUPPORTED));
            else CHECK(rc == rc_default);
            if (&sw == &sws[0]) rc_default = rc;
            if (rc != ORBHIP_OK) continue;
            CHECK(a.h.lv[s.L - 1].h == s.last_h);
            check_plan(a, sw);
            CHECK(plan_build_host(prm, tab, s.w, s.h, sw, b) == ORBHIP_OK && same_plan(a, b));
            built++;
        }
        std::snprintf(g_what, sizeof(g_what), "%dx%d L%d sf%g last level rows", s.w, s.h, s.L, s.sf);
        CHECK(round_even_f((float)s.h * tab.inv_scale[s.L - 1]) == s.last_h);
    }
    print_levels(640, 480, 1250, 1.2f, 8);
    if (g_fail) {
        std::printf("extract plan FAILED: %d violations\n", g_fail);
        return 1;
    }
    std::printf("extract plan OK: %d plans\n", built);
    return 0;
}
