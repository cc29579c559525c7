// The extraction planner (extract_plan.h): host arithmetic only, no device calls.
//
// It restates the table logic of the reference (it is the product's own code, not the oracle's):
//   U:src/ORBextractor.cc::ORBextractor::ORBextractor  scale / feature / umax tables
//   U:src/ORBextractor.cc::ComputePyramid               level sizes
//   OCV:imgproc/src/resize.cpp hal::resize              xofs/alpha/yofs/beta fixed-point tables
//   U:src/ORBextractor.cc::ComputeKeyPointsOctTree      35-px cell grid
//   U:src/ORBextractor.cc::DistributeOctTree            root count nIni, root width hX
//   OCV:imgproc smooth.dispatch.cpp getGaussianKernelBitExact + fixed-point ED  (7x7, sigma 2)
#include "extract_plan.h"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>

namespace orbhip {

static int round_even_d(double v) { return (int)std::nearbyint(v); }
static int floor_f(float v) { int i = (int)v; return i - (i > v); }
static short sat_s16(int v) { return (short)std::min(std::max(v, -32768), 32767); }

OrbTables build_orb_tables(const orbhip_orb_params& prm) {
    OrbTables t;
    const int L = prm.n_levels;
    const double sf = (double)prm.scale_factor;
    t.scale.assign(L, 1.f);
    t.inv_scale.assign(L, 1.f);
    for (int i = 1; i < L; i++) t.scale[i] = (float)(t.scale[i - 1] * sf);
    for (int i = 0; i < L; i++) t.inv_scale[i] = 1.0f / t.scale[i];
    t.feat.assign(L, 0);
    const float factor = (float)(1.0f / sf);
    float nd = prm.n_features * (1 - factor) / (1 - (float)std::pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        t.feat[l] = round_even_f(nd);
        sum += t.feat[l];
        nd *= factor;
    }
    t.feat[L - 1] = std::max(prm.n_features - sum, 0);
    // umax (HALF_PATCH_SIZE 15)
    const int H = 15;
    t.umax.assign(H + 1, 0);
    int vmax = (int)std::floor(H * std::sqrt(2.f) / 2 + 1);
    int vmin = (int)std::ceil(H * std::sqrt(2.f) / 2);
    const double hp2 = H * H;
    for (int v = 0; v <= vmax; ++v) t.umax[v] = round_even_d(std::sqrt(hp2 - v * v));
    for (int v = H, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    // bit-exact 7-tap Gaussian, sigma 2, 8 fractional bits, error diffusion
    const int n = 7, n2 = 3;
    double vals[3], s = 0, scale2X = -0.125 / (2.0 * 2.0);
    for (int i = 0, x = 1 - n; i < n2; i++, x += 2) { vals[i] = std::exp((double)(x * x) * scale2X); s += vals[i]; }
    s = s * 2 + 1.0;
    const double mul1 = 1.0 / s;
    double err = 0;
    long tot = 0;
    for (int i = 0; i < n2; i++) {
        double adj = vals[i] * mul1 * 256.0 + err;
        long v0 = round_even_d(adj);
        err = adj - (double)v0;
        t.blurk[i] = t.blurk[n - 1 - i] = (int)v0;
        tot += v0;
    }
    t.blurk[n2] = (int)(256 - 2 * tot);
    return t;
}

PlanSwitches read_plan_switches(int cone_tile_hint) {
    // a set variable gives at least `lo`, so -1 stays "unset" for the last two
    auto env = [](const char* name, int unset, int lo) {
        const char* e = std::getenv(name);
        return e ? std::max(lo, std::atoi(e)) : unset;
    };
    PlanSwitches s{};
    const int ts = env("ORBHIP_CONE_TILE", 0, 0);
    s.cone_tile = ts > 0 ? ts : (cone_tile_hint > 0 ? cone_tile_hint : 10);
    s.cone_hi_tile = env("ORBHIP_CONE_HI_TILE", 32, 4);
    s.rz_bands = env("ORBHIP_RZ_BANDS", 0, 0);
    s.clist_cap = env("ORBHIP_FAST_CLIST_CAP", -1, 0);
    s.fast_nt = env("ORBHIP_FAST_NT", -1, 0);
    return s;
}

// k_pyr_cone tables from source level s0 (0: the frame): tiles of ts x ts pixels of the last
// level, every level l > s0 cut into the same tile grid (an even partition, the tile's owned
// pixels) plus the halo its level l+1 need reads (the need), the source level's need staged.
// Returns the tile count; rects (kMaxLevels per tile), the per-tile resize tables in the kernel's
// LDS layout (row indices clamped to the source), their stride, and the LDS bytes of the largest.
static int cone_tables(const ExtractPlan& P, const HostPlan& pl, int s0, int ts, std::vector<ConeRect>& rects,
                       std::vector<int>& ctab, size_t& tab_stride, size_t& lds_max) {
    const int L = P.n_levels;
    const LevelGeom& T = P.lv[L - 1];
    const int ntx = (T.w + ts - 1) / ts, nty = (T.h + ts - 1) / ts;
    lds_max = 0;
    rects.assign((size_t)ntx * nty * kMaxLevels, ConeRect{});
    // the source rectangle of level l's need [nx0, nx1) x [ny0, ny1) on level l - 1
    auto source_of = [&](int l, int nx0, int nx1, int ny0, int ny1, int* a0, int* a1, int* b0, int* b1) {
        const LevelGeom& U = P.lv[l];
        const LevelGeom& G = P.lv[l - 1];
        *a0 = pl.xofs[U.xtab_off + nx0];
        *a1 = pl.xofs[U.xtab_off + nx1 - 1] + ((nx1 - 1) < U.xmax ? 1 : 0) + 1;
        auto clampr = [&](int r) { return r < 0 ? 0 : (r < G.h ? r : G.h - 1); };
        *b0 = clampr(pl.yofs[U.ytab_off + ny0]);
        *b1 = clampr(pl.yofs[U.ytab_off + ny1 - 1] + 1) + 1;
    };
    for (int ti = 0; ti < nty; ti++)
        for (int tj = 0; tj < ntx; tj++) {
            ConeRect* R = &rects[((size_t)ti * ntx + tj) * kMaxLevels];
            int nx0 = 0, nx1 = 0, ny0 = 0, ny1 = 0;   // need of the level above (l + 1)
            for (int l = L - 1; l > s0; l--) {
                const LevelGeom& G = P.lv[l];
                const int ox0 = (int)((int64_t)tj * G.w / ntx), ox1 = (int)((int64_t)(tj + 1) * G.w / ntx);
                const int oy0 = (int)((int64_t)ti * G.h / nty), oy1 = (int)((int64_t)(ti + 1) * G.h / nty);
                int a0 = ox0, a1 = ox1, b0 = oy0, b1 = oy1;
                if (l < L - 1 && nx1 > nx0 && ny1 > ny0) {   // inputs of the level-(l+1) need
                    int lo, hi, r0, r1;
                    source_of(l + 1, nx0, nx1, ny0, ny1, &lo, &hi, &r0, &r1);
                    a0 = std::min(a0, lo); a1 = std::max(a1, hi);
                    b0 = std::min(b0, r0); b1 = std::max(b1, r1);
                    if (ox1 <= ox0 || oy1 <= oy0) { a0 = lo; a1 = hi; b0 = r0; b1 = r1; }
                }
                R[l] = ConeRect{(int16_t)a0, (int16_t)a1, (int16_t)b0, (int16_t)b1,
                                (int16_t)ox0, (int16_t)ox1, (int16_t)oy0, (int16_t)oy1};
                nx0 = a0; nx1 = a1; ny0 = b0; ny1 = b1;
            }
            {   // source-level inputs of the level-(s0+1) need (staged in LDS)
                int lo, hi, r0, r1;
                source_of(s0 + 1, nx0, nx1, ny0, ny1, &lo, &hi, &r0, &r1);
                R[s0] = ConeRect{(int16_t)lo, (int16_t)hi, (int16_t)r0, (int16_t)r1, 0, 0, 0, 0};
            }
            size_t tot = 0, ttot = 0;
            for (int l = s0; l < L; l++) {   // source: rows of round_up(width + 3, 4) (dword staging)
                const size_t wl = l == s0 ? (size_t)((R[s0].nx1 - R[s0].nx0 + 6) & ~3) : (size_t)(R[l].nx1 - R[l].nx0);
                tot += (wl * (R[l].ny1 - R[l].ny0) + 15) & ~size_t(15);
            }
            for (int l = s0 + 1; l < L; l++)
                ttot += 4 * (2 * (size_t)(R[l].nx1 - R[l].nx0) + 3 * (size_t)(R[l].ny1 - R[l].ny0));
            lds_max = std::max(lds_max, tot + ttot);
        }
    tab_stride = 0;
    for (int t = 0; t < ntx * nty; t++) {
        size_t tt = 0;
        for (int l = s0 + 1; l < L; l++) {
            const ConeRect& r = rects[(size_t)t * kMaxLevels + l];
            tt += 2 * (size_t)(r.nx1 - r.nx0) + 3 * (size_t)(r.ny1 - r.ny0);
        }
        tab_stride = std::max(tab_stride, tt);
    }
    ctab.assign((size_t)ntx * nty * tab_stride, 0);
    for (int t = 0; t < ntx * nty; t++) {
        int* o = ctab.data() + (size_t)t * tab_stride;
        for (int l = s0 + 1; l < L; l++) {
            const LevelGeom& D = P.lv[l];
            const LevelGeom& S = P.lv[l - 1];
            const ConeRect r = rects[(size_t)t * kMaxLevels + l];
            const int nw = r.nx1 - r.nx0, nh = r.ny1 - r.ny0;
            for (int i = 0; i < nw; i++) {
                o[i] = pl.xofs[D.xtab_off + r.nx0 + i];
                o[nw + i] = pl.xalpha[D.xtab_off + r.nx0 + i];
            }
            auto clampr = [&](int v) { return v < 0 ? 0 : (v < S.h ? v : S.h - 1); };
            for (int j = 0; j < nh; j++) {
                const int sy = pl.yofs[D.ytab_off + r.ny0 + j];
                o[2 * nw + 3 * j] = clampr(sy);
                o[2 * nw + 3 * j + 1] = clampr(sy + 1);
                o[2 * nw + 3 * j + 2] = pl.ybeta[D.ytab_off + r.ny0 + j];
            }
            o += 2 * nw + 3 * nh;
        }
    }
    return ntx * nty;
}
int plan_build_host(const orbhip_orb_params& prm, const OrbTables& tab, int w, int h, const PlanSwitches& sw,
                    HostPlan& out) {
    out = HostPlan();
    ExtractPlan& P = out.h;
    const int L = prm.n_levels;
    P.w = w; P.h = h; P.n_levels = L;
    P.ini_th = std::min(std::max(prm.ini_th_fast, 0), 255);
    P.min_th = std::min(std::max(prm.min_th_fast, 0), 255);
    P.clist_cap = sw.clist_cap < 0 ? kClistCap : std::min(sw.clist_cap, kClistCap);
    P.fast_nt = 0;
    if (sw.fast_nt >= 0) {
        const int v = sw.fast_nt;
        if (v == 128 || v == 256 || v == 512 || v == 1024) P.fast_nt = v;
        else std::fprintf(stderr, "orbhip: ORBHIP_FAST_NT=%d ignored (128, 256, 512 or 1024)\n", v);
    }
    for (int i = 0; i < 7; i++) P.blurk[i] = tab.blurk[i];
    // k_desc hard-codes these taps (GaussianBlur 7x7 sigma 2 is fixed in ORBextractor)
    static const int kTaps[7] = {18, 34, 48, 56, 48, 34, 18};
    for (int i = 0; i < 7; i++)
        if (P.blurk[i] != kTaps[i]) return ORBHIP_ERR_UNSUPPORTED;
    int64_t pyr_off = 0;
    int cell_base = 0, slot_base = 0, kp_base = 0, max_cells = 0, hc_max = 7, wc_max = 7;
    for (int l = 0; l < L; l++) {
        LevelGeom& G = P.lv[l];
        G.w = round_even_f((float)w * tab.inv_scale[l]);
        G.h = round_even_f((float)h * tab.inv_scale[l]);
        if (G.w < 64 || G.h < 64) return ORBHIP_ERR_UNSUPPORTED;   // every level must host 43x43 patches
        G.pitch = l == 0 ? 0 : ((G.w + 63) / 64) * 64;
        G.pyr_off = l == 0 ? 0 : pyr_off;
        if (l > 0) pyr_off += (int64_t)G.pitch * G.h;
        G.scale = tab.scale[l];
        G.n_feat = tab.feat[l];
        G.patch_size = (int)(31 * tab.scale[l]);
        // resize tables (level l from l-1); each level's column table starts 16-byte aligned and
        // is padded, so k_resize reads 4 consecutive entries as one int4
        while (out.xofs.size() % 4) { out.xofs.push_back(0); out.xalpha.push_back(0); }
        G.xtab_off = (int)out.xofs.size();
        G.ytab_off = (int)out.yofs.size();
        G.xmax = G.w;
        G.vend = 0;
        G.rz_noclamp = 1;
        // |p| <= 255 and taps a0, a1, b0, b1 >= 0 with a0 + a1, b0 + b1 <= 2049 keep every
        // intermediate of the vertical pass in range: (255 * 2049) >> 4 < 32768, and the rounded
        // sum (t + 2) >> 2 <= 255
        auto taps_ok = [](int packed) {
            const int t0 = (int)(short)(packed & 0xFFFF), t1 = (int)(short)(packed >> 16);
            return t0 >= 0 && t1 >= 0 && t0 + t1 <= 2049;
        };
        if (l > 0) {
            const int sw = P.lv[l - 1].w, sh = P.lv[l - 1].h, dw = G.w, dh = G.h;
            double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
            double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
            int isx = round_even_d(scale_x), isy = round_even_d(scale_y);
            if (std::abs(scale_x - isx) < DBL_EPSILON && std::abs(scale_y - isy) < DBL_EPSILON && isx == 2 && isy == 2)
                return ORBHIP_ERR_UNSUPPORTED;   // OpenCV switches to INTER_AREA for exact 2x
            int xmax = dw;
            for (int dx = 0; dx < dw; dx++) {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = floor_f(fx);
                fx -= sx;
                if (sx < 0) { fx = 0; sx = 0; }
                if (sx + 1 >= sw) {
                    xmax = std::min(xmax, dx);
                    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
                }
                out.xofs.push_back(sx);
                const short a0 = sat_s16(round_even_f((1.f - fx) * 2048)), a1 = sat_s16(round_even_f(fx * 2048));
                out.xalpha.push_back((int)(uint16_t)a0 | ((int)(uint16_t)a1 << 16));
                if (!taps_ok(out.xalpha.back())) G.rz_noclamp = 0;
            }
            for (int dy = 0; dy < dh; dy++) {
                float fy = (float)((dy + 0.5) * scale_y - 0.5);
                int sy = floor_f(fy);
                fy -= sy;
                out.yofs.push_back(sy);
                const short b0 = sat_s16(round_even_f((1.f - fy) * 2048)), b1 = sat_s16(round_even_f(fy * 2048));
                out.ybeta.push_back((int)(uint16_t)b0 | ((int)(uint16_t)b1 << 16));
                if (!taps_ok(out.ybeta.back())) G.rz_noclamp = 0;
            }
            G.xmax = xmax;
            int x = 0;
            for (; x <= dw - 16; x += 16) {}
            for (; x < dw - 8; x += 8) {}
            G.vend = x;
        }
        // cells (ComputeKeyPointsOctTree)
        const int EDGE = 19;
        G.min_bx = EDGE - 3; G.min_by = EDGE - 3;
        G.max_bx = G.w - EDGE + 3; G.max_by = G.h - EDGE + 3;
        const float width = (float)(G.max_bx - G.min_bx), height = (float)(G.max_by - G.min_by);
        G.n_cols = (int)(width / 35.f);
        G.n_rows = (int)(height / 35.f);
        if (G.n_cols <= 0 || G.n_rows <= 0) return ORBHIP_ERR_UNSUPPORTED;
        G.w_cell = (int)std::ceil(width / G.n_cols);
        G.h_cell = (int)std::ceil(height / G.n_rows);
        G.cell_base = cell_base;
        G.slot_base = slot_base;
        int ncell = 0;
        for (int i = 0; i < G.n_rows; i++) {
            const float iniY = (float)(G.min_by + i * G.h_cell);
            float maxY = iniY + G.h_cell + 6;
            const bool skipY = iniY >= G.max_by - 3;
            if (maxY > G.max_by) maxY = (float)G.max_by;
            for (int j = 0; j < G.n_cols; j++) {
                const float iniX = (float)(G.min_bx + j * G.w_cell);
                float maxX = iniX + G.w_cell + 6;
                const bool skipX = iniX >= G.max_bx - 6;
                if (maxX > G.max_bx) maxX = (float)G.max_bx;
                CellGeom cg{};
                cg.level = (int16_t)l;
                cg.x0 = (int16_t)iniX; cg.y0 = (int16_t)iniY;
                cg.wc = (skipY || skipX) ? 0 : (int16_t)((int)maxX - (int)iniX);
                cg.hc = (skipY || skipX) ? 0 : (int16_t)((int)maxY - (int)iniY);
                if (cg.wc > 76 || cg.hc > 76) return ORBHIP_ERR_UNSUPPORTED;
                cg.slot_off = slot_base;
                const int dc = std::max(cg.wc - 6, 0), dr = std::max(cg.hc - 6, 0);
                slot_base += ((dc + 1) / 2) * ((dr + 1) / 2);   // max strict-NMS survivors
                if (cg.wc > 6 && cg.hc > 6) {   // cells k_fast_cells works on
                    hc_max = std::max(hc_max, (int)cg.hc);
                    wc_max = std::max(wc_max, (int)cg.wc);
                }
                out.cells.push_back(cg);
                ncell++;
            }
        }
        G.n_cells = ncell;
        G.n_slots = slot_base - G.slot_base;
        cell_base += ncell;
        max_cells = std::max(max_cells, ncell);
        // DistributeOctTree roots
        G.n_ini = (int)std::round((float)(G.max_bx - G.min_bx) / (G.max_by - G.min_by));
        if (G.n_ini <= 0 || G.n_ini > 64) return ORBHIP_ERR_UNSUPPORTED;
        G.hX = (float)(G.max_bx - G.min_bx) / G.n_ini;
        G.kp_cap = G.n_feat + 3 + 4 * G.n_ini;
        G.kp_base = kp_base;
        kp_base += G.kp_cap;
        if ((G.max_bx - G.min_bx) >= 4096 || (G.max_by - G.min_by) >= 4096) return ORBHIP_ERR_UNSUPPORTED;
        // k_octree interval tables: the first 6 quadrant splits of DistributeOctTree's root
        // rectangles (DivideNode: halfX = ceil((UR.x - UL.x) / 2.f)) are fixed by geometry, so a
        // column's root and x-side choices (and a row's y-side choices) are tabulated once
        {
            auto bits6 = [](int v, int a0, int a1) {
                int b = 0;
                for (int d = 0; d < 6; d++) {
                    const int sv = a0 + (int)std::ceil((float)(a1 - a0) / 2);
                    const bool hi = v >= sv;
                    (hi ? a0 : a1) = sv;
                    b = 2 * b + (hi ? 1 : 0);
                }
                return b;
            };
            const int Wl = G.max_bx - G.min_bx, Hl = G.max_by - G.min_by;
            G.oct_tab_off = (int)out.otab.size();
            for (int x = 0; x < Wl; x++) {
                int r = (int)((float)x / G.hX);
                r = r < 0 ? 0 : (r >= G.n_ini ? G.n_ini - 1 : r);
                out.otab.push_back((uint16_t)((r << 8) | bits6(x, (int)(G.hX * (float)r), (int)(G.hX * (float)(r + 1)))));
            }
            for (int y = 0; y < Hl; y++) out.otab.push_back((uint16_t)bits6(y, 0, Hl));
        }
    }
    P.n_cells_total = cell_base;
    P.n_slots_total = slot_base;
    P.kp_slots_total = kp_base;
    P.pyr_bytes = ((pyr_off + 255) / 256) * 256;
    P.max_cells_level = max_cells;
    out.kp_cap_frame = kp_base;
    P.fast_win_rows = hc_max;   // k_fast_cells' LDS variant
    P.fast_win_cols = wc_max;
    // cone pyramid tables: tiles of ~10x10 on the last level (252 at 640x480: the per-tile cascade
    // is latency bound, so smaller cones finish sooner), an even partition of every level; for
    // batches a second set from level kConeHiStart with bigger tiles (the small levels' launches
    // are latency bound there, the big levels' k_resize launches stream)
    if (L > 1) {
        std::vector<ConeRect> rects;
        std::vector<int> ctab;
        size_t stride = 0, lds = 0;
        const int ts = sw.cone_tile;
        int tiles = cone_tables(P, out, 0, ts, rects, ctab, stride, lds);
        if (lds <= 60 * 1024) {
            out.cone_tab.swap(ctab);
            out.cone_tab_stride = (int)stride;
            out.cone.swap(rects);
            out.cone_tiles = tiles;
            out.cone_lds = lds;
        }
        if (L > kConeHiStart + 1) {
            tiles = cone_tables(P, out, kConeHiStart, sw.cone_hi_tile, rects, ctab, stride, lds);
            if (lds <= 60 * 1024) {
                out.cone_hi_tab.swap(ctab);
                out.cone_hi_tab_stride = (int)stride;
                out.cone_hi.swap(rects);
                out.cone_hi_tiles = tiles;
                out.cone_hi_lds = lds;
            }
        }
    }
    // k_resize_bands rows: per band, from the last level down, its own rows of the level plus the
    // rows the next level's band rows read (the source rows of k_resize's row tables, clamped)
    {
        const int nb = std::min(sw.rz_bands, L > 0 ? P.lv[L - 1].h : 0);
        if (L > kBandStart + 1 && nb > 0) {
            out.bands.assign((size_t)nb * kMaxLevels * 2, 0);
            for (int b = 0; b < nb; b++) {
                int n0 = 0, n1 = 0;   // the rows of level l + 1 this band computes
                for (int l = L - 1; l > kBandStart; l--) {
                    const LevelGeom& G = P.lv[l];
                    int r0 = (int)((int64_t)b * G.h / nb), r1 = (int)((int64_t)(b + 1) * G.h / nb);
                    if (l < L - 1 && n1 > n0) {
                        const LevelGeom& U = P.lv[l + 1];
                        auto clampr = [&](int r) { return r < 0 ? 0 : (r < G.h ? r : G.h - 1); };
                        const int s0r = clampr(out.yofs[U.ytab_off + n0]);
                        const int s1r = clampr(out.yofs[U.ytab_off + n1 - 1] + 1) + 1;
                        if (r1 > r0) { r0 = std::min(r0, s0r); r1 = std::max(r1, s1r); }
                        else { r0 = s0r; r1 = s1r; }
                    }
                    out.bands[((size_t)b * kMaxLevels + l) * 2] = r0;
                    out.bands[((size_t)b * kMaxLevels + l) * 2 + 1] = r1;
                    n0 = r0; n1 = r1;
                }
            }
            out.nbands = nb;
        }
    }
    // k_pyr_flow bands: task (l, b) = output rows [16 b, 16 b + 16) of level l; its source rows are
    // what resize_tile reads for each 4-row group (the interior path loads kRzSrc = 6 rows from the
    // group's first clamped source row, the per-row path rows sy and sy + 1), clamped
    if (L > 1) {
        constexpr int kFR = 16, kGroup = 4, kSrcRows = 6;
        int nbt = 0;
        for (int l = 1; l < L; l++) {
            out.flow_boff[l] = nbt;
            nbt += (P.lv[l].h + kFR - 1) / kFR;
        }
        for (int l = L; l <= kMaxLevels; l++) out.flow_boff[l] = nbt;
        out.flow_nbt = nbt;
        out.flow_dep.assign((size_t)nbt * 2, 0);
        for (int l = 2; l < L; l++) {
            const LevelGeom& G = P.lv[l];
            const int Sh = P.lv[l - 1].h;
            auto clampr = [&](int r) { return r < 0 ? 0 : (r < Sh ? r : Sh - 1); };
            for (int b = 0; b * kFR < G.h; b++) {
                const int r0 = b * kFR, r1 = std::min(r0 + kFR, G.h);
                int lo = Sh, hi = 0;
                for (int g = r0; g < r1; g += kGroup) {
                    const int rb = clampr(out.yofs[G.ytab_off + g]);
                    lo = std::min(lo, rb);
                    hi = std::max(hi, std::min(rb + kSrcRows - 1, Sh - 1));
                    for (int dy = g; dy < std::min(g + kGroup, r1); dy++) {
                        lo = std::min(lo, clampr(out.yofs[G.ytab_off + dy]));
                        hi = std::max(hi, clampr(out.yofs[G.ytab_off + dy] + 1));
                    }
                }
                out.flow_dep[(size_t)(out.flow_boff[l] + b) * 2] = lo / kFR;
                out.flow_dep[(size_t)(out.flow_boff[l] + b) * 2 + 1] = hi / kFR;
            }
        }
    }
    // IC_Angle disc offsets (u, v) packed as int16 pairs
    for (int v = -15; v <= 15; v++) {
        const int d = tab.umax[std::abs(v)];
        for (int u = -d; u <= d; u++) out.disc.push_back((int)((uint32_t)(uint16_t)u | ((uint32_t)(uint16_t)v << 16)));
    }
    P.n_disc = (int)out.disc.size();   // <= 31 x 31 (k_desc_kp holds 4 entries per thread)
    if (P.n_disc > 1024) return ORBHIP_ERR_UNSUPPORTED;
    out.disc.resize(1024, 0);   // zero-padded: k_desc_kp loads 4 x 256 entries without a bound (a (0, 0) entry adds nothing)
    // octree LDS configuration
    int max_kp_cap = 0;
    for (int l = 0; l < L; l++) max_kp_cap = std::max(max_kp_cap, P.lv[l].kp_cap);
    OctreeCfg& oc = out.oct;
    oc.node_cap = ((max_kp_cap + 63) / 64) * 64;
    oc.sort_cap = 1;
    while (oc.sort_cap < oc.node_cap) oc.sort_cap <<= 1;
    oc.key_cap = 0;
    const size_t budget = 160 * 1024;
    const size_t base = octree_lds_bytes(P, oc);
    if (base + 1024 > budget) return ORBHIP_ERR_UNSUPPORTED;
    oc.key_cap = (int)std::min<size_t>(16384, ((budget - base - 64) / 6) & ~size_t(15));
    while (octree_lds_bytes(P, oc) > budget) oc.key_cap -= 16;
    for (int i = 0; i < 4; i++) { out.xofs.push_back(0); out.xalpha.push_back(0); }   // int4 tail reads
    return ORBHIP_OK;
}

}  // namespace orbhip
