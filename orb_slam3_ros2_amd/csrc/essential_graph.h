// Optimizer::OptimizeEssentialGraph on the device (essential_graph.hip): the 7-dof pose graph of
// CorrectLoop / MergeLocal. The records the kernels read, the argument check, the block structure of
// H (the gather lists of the deterministic assembly and the solvers' row_first) and the packing of
// a call into the staging block's host image: plain C++, so that a host-only program can include
// this file and run all of it without the HIP runtime.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbhip.h"
#include "stage.h"

namespace orbhip {

constexpr int kEgMaxN = 4096;            // == kDagMaxN: 7 x free vertices at most (585 free vertices)
constexpr int kEgMaxVertices = 65535;
constexpr int kEgMaxEdges = 65536;
constexpr int kEgMaxPoints = 1 << 22;
// the smallest system the persistent DAG solver's own tests cover; smaller ones take the blocked solver
constexpr int kEgDagMinN = 70;

// one linearised edge: J[c][r] = d e_r / d component c (c < 7: vertex i, else vertex j), the error
struct EgEdgeLin {
    double J[14][7];
    double e[7];
    double chi2;
};

// the Levenberg state of a call, on the device (the phase word gates every kernel and the solvers)
struct EgCtl {
    int32_t phase;               // kPhBuild / kPhTrial / kPhDone (ba_args.h)
    int32_t it, iterations, trials, rejected, qmax, fix_scale, pad;
    double lambda, ni, currentChi, initChi, lambda_init;
};

// a 7x7 block of H's lower triangle (br >= bc); its contributions are ent[first .. first + count):
// edge << 3 | form, in edge order; form 0: Ji^T Ji, 1: Jj^T Jj, 2: Ji^T Jj, 3: Jj^T Ji. The rows of b
// of block k gather ent[bfirst[k] .. bfirst[k + 1]): form 0: -Ji^T e, 1: -Jj^T e
struct EgBlock {
    int32_t br, bc, first, count;
};

struct EgStructure {
    int nf = 0, n = 0;                   // free vertices, 7 nf
    std::vector<int32_t> vidx;           // vertex -> block (-1: fixed)
    std::vector<int32_t> free_v;         // block -> vertex
    std::vector<EgBlock> blocks;         // the nf diagonal blocks first, then the connected pairs
    std::vector<int32_t> ent;            // H entries, then b's (block k of b: bfirst[k] .. bfirst[k + 1])
    std::vector<int32_t> bfirst;         // nf + 1, offsets into ent
    std::vector<int32_t> row_first;      // ceil(n / 32): first 32-column tile with a block, per 32-row tile
};

struct EgLayout {
    size_t o_ctl, o_S, o_vidx, o_freev, o_eij, o_eS, o_blocks, o_ent, o_bfirst, o_rf, o_pts, o_ref, up_bytes;
    size_t o_out_ctl, o_out_S, o_out_pts, back_end;   // read back: EgCtl, the estimates, the points
    size_t o_St, o_lin, o_chi2, o_hdiag, o_b, o_x, o_flag, total;
};

inline bool eg_finite8(const double* p) {
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(p[k])) return false;
    return p[7] > 0.0;
}

// ORBHIP_OK, ORBHIP_ERR_ARG or ORBHIP_ERR_UNSUPPORTED; nothing is written
inline int eg_check(const orbhip_essential_graph_problem* p, const orbhip_essential_graph_result* r) {
    if (!p || !r) return ORBHIP_ERR_ARG;
    if (p->n_vertices < 0 || p->n_edges < 0 || p->n_points < 0 || p->iterations < 0) return ORBHIP_ERR_ARG;
    if (!(p->lambda_init > 0.0) || !std::isfinite(p->lambda_init)) return ORBHIP_ERR_ARG;
    if (p->n_vertices > 0 && (!p->S || !p->fixed || !r->S)) return ORBHIP_ERR_ARG;
    if (p->n_edges > 0 && (!p->edge_ij || !p->edge_S)) return ORBHIP_ERR_ARG;
    if (p->n_points > 0 && (!p->points || !p->point_ref || !r->points)) return ORBHIP_ERR_ARG;
    if (p->n_vertices > kEgMaxVertices || p->n_edges > kEgMaxEdges || p->n_points > kEgMaxPoints)
        return ORBHIP_ERR_UNSUPPORTED;
    for (int v = 0; v < p->n_vertices; v++)
        if (!eg_finite8(p->S + 8 * (size_t)v)) return ORBHIP_ERR_ARG;
    for (int e = 0; e < p->n_edges; e++) {
        const int i = p->edge_ij[2 * e], j = p->edge_ij[2 * e + 1];
        if (i < 0 || j < 0 || i >= p->n_vertices || j >= p->n_vertices || i == j) return ORBHIP_ERR_ARG;
        if (!eg_finite8(p->edge_S + 8 * (size_t)e)) return ORBHIP_ERR_ARG;
    }
    for (int m = 0; m < p->n_points; m++)
        if (p->point_ref[m] < 0 || p->point_ref[m] >= p->n_vertices) return ORBHIP_ERR_ARG;
    int nf = 0;
    for (int v = 0; v < p->n_vertices; v++) nf += p->fixed[v] == 0;
    if (7 * nf > kEgMaxN) return ORBHIP_ERR_UNSUPPORTED;
    return ORBHIP_OK;
}

// the block structure of a checked problem, in the caller's vertex order (the library does not
// reorder: keyframe-id order keeps spanning-tree and covisibility blocks near the diagonal and puts
// the loop edges' rows last, where their fill is cheap)
inline void eg_structure(const orbhip_essential_graph_problem* p, EgStructure& s) {
    const int nv = p->n_vertices, E = p->n_edges;
    s.vidx.assign((size_t)nv, -1);
    s.free_v.clear();
    for (int v = 0; v < nv; v++)
        if (!p->fixed[v]) { s.vidx[v] = (int32_t)s.free_v.size(); s.free_v.push_back(v); }
    s.nf = (int)s.free_v.size();
    s.n = 7 * s.nf;
    // (block key, edge << 3 | form), sorted by key then edge: every block's entries in edge order
    struct Item { int64_t key; int32_t ent; };
    std::vector<Item> hs, bs;
    hs.reserve(3 * (size_t)E);
    bs.reserve(2 * (size_t)E);
    const int64_t nf = s.nf;
    auto key = [&](int br, int bc) { return br == bc ? (int64_t)br : nf + (int64_t)br * nf + bc; };
    for (int e = 0; e < E; e++) {
        const int bi = s.vidx[p->edge_ij[2 * e]], bj = s.vidx[p->edge_ij[2 * e + 1]];
        if (bi >= 0) { hs.push_back({key(bi, bi), e << 3 | 0}); bs.push_back({bi, e << 3 | 0}); }
        if (bj >= 0) { hs.push_back({key(bj, bj), e << 3 | 1}); bs.push_back({bj, e << 3 | 1}); }
        if (bi >= 0 && bj >= 0) {
            if (bi > bj) hs.push_back({key(bi, bj), e << 3 | 2});    // (row i, col j) = Ji^T Jj
            else hs.push_back({key(bj, bi), e << 3 | 3});            // (row j, col i) = Jj^T Ji
        }
    }
    auto by_key = [](const Item& a, const Item& b) { return a.key != b.key ? a.key < b.key : a.ent < b.ent; };
    std::sort(hs.begin(), hs.end(), by_key);
    std::sort(bs.begin(), bs.end(), by_key);
    s.blocks.clear();
    s.ent.clear();
    for (int k = 0; k < s.nf; k++) s.blocks.push_back({k, k, 0, 0});   // a free vertex without an edge: a zero block
    size_t at = 0;
    for (int k = 0; k < s.nf; k++) {
        s.blocks[k].first = (int32_t)s.ent.size();
        while (at < hs.size() && hs[at].key == k) s.ent.push_back(hs[at++].ent);
        s.blocks[k].count = (int32_t)s.ent.size() - s.blocks[k].first;
    }
    while (at < hs.size()) {
        const int64_t kk = hs[at].key - nf;
        EgBlock b{(int32_t)(kk / nf), (int32_t)(kk % nf), (int32_t)s.ent.size(), 0};
        while (at < hs.size() && hs[at].key - nf == kk) s.ent.push_back(hs[at++].ent);
        b.count = (int32_t)s.ent.size() - b.first;
        s.blocks.push_back(b);
    }
    s.bfirst.assign((size_t)s.nf + 1, 0);
    at = 0;
    for (int k = 0; k < s.nf; k++) {
        s.bfirst[k] = (int32_t)s.ent.size();
        while (at < bs.size() && bs[at].key == k) s.ent.push_back(bs[at++].ent);
    }
    s.bfirst[s.nf] = (int32_t)s.ent.size();
    const int nt = (s.n + 31) / 32;
    s.row_first.resize((size_t)nt);
    for (int R = 0; R < nt; R++) s.row_first[R] = R;
    for (const EgBlock& b : s.blocks) {
        const int c0 = 7 * b.bc / 32;   // the block's first column tile; its rows span at most two row tiles
        for (int R = 7 * b.br / 32; R <= (7 * b.br + 6) / 32; R++) s.row_first[R] = std::min(s.row_first[R], c0);
    }
}

inline EgLayout eg_layout(const orbhip_essential_graph_problem* p, const EgStructure& s) {
    const size_t nv = (size_t)p->n_vertices, E = (size_t)p->n_edges, M = (size_t)p->n_points, n = (size_t)s.n;
    EgLayout L{};
    StageLayout lay(256);
    L.o_ctl = lay.take(sizeof(EgCtl));
    L.o_S = lay.take(64 * nv);
    L.o_vidx = lay.take(4 * nv);
    L.o_freev = lay.take(4 * (size_t)s.nf);
    L.o_eij = lay.take(8 * E);
    L.o_eS = lay.take(64 * E);
    L.o_blocks = lay.take(sizeof(EgBlock) * s.blocks.size());
    L.o_ent = lay.take(4 * s.ent.size());
    L.o_bfirst = lay.take(4 * s.bfirst.size());
    L.o_rf = lay.take(4 * s.row_first.size());
    L.o_pts = lay.take(12 * M);
    L.o_ref = lay.take(4 * M);
    L.up_bytes = lay.total();
    L.o_out_ctl = lay.take(sizeof(EgCtl));
    L.o_out_S = lay.take(64 * nv);
    L.o_out_pts = lay.take(12 * M);
    L.back_end = lay.total();
    L.o_St = lay.take(64 * nv);
    L.o_lin = lay.take(sizeof(EgEdgeLin) * E);
    L.o_chi2 = lay.take(8 * E);
    L.o_hdiag = lay.take(8 * n);
    L.o_b = lay.take(8 * n);
    L.o_x = lay.take(8 * n);
    L.o_flag = lay.take(16 * sizeof(int32_t));
    L.total = lay.total();
    return L;
}

// the upload part of a checked call into the host image h (L.up_bytes bytes)
inline void eg_pack(const orbhip_essential_graph_problem* p, const EgStructure& s, const EgLayout& L, uint8_t* h) {
    const size_t nv = (size_t)p->n_vertices, E = (size_t)p->n_edges, M = (size_t)p->n_points;
    EgCtl c{};
    const bool run = p->iterations > 0 && s.nf > 0 && E > 0;
    c.phase = run ? 0 : 2;
    c.iterations = p->iterations;
    c.fix_scale = p->fix_scale != 0;
    c.ni = 2.0;
    c.lambda_init = p->lambda_init;
    std::memcpy(h + L.o_ctl, &c, sizeof(c));
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::memcpy(h + o, src, bytes); };
    put(L.o_S, p->S, 64 * nv);
    put(L.o_vidx, s.vidx.data(), 4 * nv);
    put(L.o_freev, s.free_v.data(), 4 * s.free_v.size());
    put(L.o_eij, p->edge_ij, 8 * E);
    put(L.o_eS, p->edge_S, 64 * E);
    put(L.o_blocks, s.blocks.data(), sizeof(EgBlock) * s.blocks.size());
    put(L.o_ent, s.ent.data(), 4 * s.ent.size());
    put(L.o_bfirst, s.bfirst.data(), 4 * s.bfirst.size());
    put(L.o_rf, s.row_first.data(), 4 * s.row_first.size());
    put(L.o_pts, p->points, 12 * M);
    put(L.o_ref, p->point_ref, 4 * M);
}

#ifdef __HIPCC__
struct StageBlock;
struct StageTimer;
struct EgWorkspace;   // the dense S, the solvers' buffers: grown on demand, one per context
EgWorkspace* eg_ws_create();
void eg_ws_destroy(EgWorkspace* ws);
// profile stage 14 brackets the call's launches; returns ORBHIP_OK or an error
int eg_optimize(EgWorkspace* ws, StageBlock& S, StageTimer& timer, hipStream_t st,
                const orbhip_essential_graph_problem* prob, orbhip_essential_graph_result* res);
#endif

}  // namespace orbhip
