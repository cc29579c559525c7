// OptimizeEssentialGraph's host side without a device: the argument check, the block structure (gather
// lists, row_first), the staging layout and the packing of a call (csrc/essential_graph.h), as a
// program of its own so that it can run under AddressSanitizer and UBSan on the CPU:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -Iorb_slam3_ros2_amd/csrc tools/essential_graph_args_check.cpp -o /tmp/eg_args_check && /tmp/eg_args_check
// The image is allocated with exactly the bytes the layout asks for, so a write past it is reported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "essential_graph.h"

using namespace orbhip;

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

// a chain of nv vertices with k more edges back per vertex and a few loop edges; `fixed_every`
// fixes vertex 0 and every such vertex
struct Scene {
    std::vector<double> S, eS, outS;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> ij, ref;
    std::vector<float> pts, outP;
    orbhip_essential_graph_problem p{};
    orbhip_essential_graph_result r{};
    Scene(int nv, int k, int fixed_every, int M) : S(8 * nv), outS(8 * nv), fixed(nv), ref(M), pts(3 * M), outP(3 * M) {
        for (int v = 0; v < nv; v++) {
            S[8 * v + 3] = 1.0; S[8 * v + 4] = v; S[8 * v + 7] = 1.0 + 0.01 * (v % 3);
            fixed[v] = v == 0 || (fixed_every && v % fixed_every == 0);
        }
        for (int i = 1; i < nv; i++)
            for (int j = i - 1; j >= 0 && j >= i - 1 - k; j--) {
                if ((i + j) % 3 == 0) { ij.push_back(j); ij.push_back(i); }   // some with i < j
                else { ij.push_back(i); ij.push_back(j); }
            }
        for (int a = 0; a < 3 && nv > 8; a++) { ij.push_back(nv - 1 - a); ij.push_back(a); }
        if (nv > 2) { ij.push_back(2); ij.push_back(1); }                      // a doubled pair
        const int E = (int)ij.size() / 2;
        eS.assign(8 * (size_t)E, 0.0);
        for (int e = 0; e < E; e++) { eS[8 * e + 3] = 1.0; eS[8 * e + 7] = 1.0; }
        for (int m = 0; m < M; m++) { ref[m] = m % nv; pts[3 * m] = (float)m; }
        p.n_vertices = nv; p.S = S.data(); p.fixed = fixed.data();
        p.n_edges = E; p.edge_ij = ij.data(); p.edge_S = eS.data();
        p.fix_scale = nv % 2; p.iterations = 20; p.lambda_init = 1e-16;
        p.n_points = M; p.points = M ? pts.data() : nullptr; p.point_ref = M ? ref.data() : nullptr;
        r.S = outS.data(); r.points = M ? outP.data() : nullptr;
    }
};

static void structure_is_sound(const Scene& sc) {
    EXPECT(eg_check(&sc.p, &sc.r) == ORBHIP_OK);
    EgStructure s;
    eg_structure(&sc.p, s);
    int nf = 0;
    for (int v = 0; v < sc.p.n_vertices; v++) nf += !sc.fixed[v];
    EXPECT(s.nf == nf && s.n == 7 * nf && (int)s.free_v.size() == nf);
    // every block once, in the lower triangle; every contribution of every edge exactly once
    std::set<std::pair<int, int>> seen;
    size_t hent = 0;
    for (const EgBlock& b : s.blocks) {
        EXPECT(b.br >= b.bc && b.br < nf && b.bc >= 0);
        EXPECT(seen.insert({b.br, b.bc}).second);
        EXPECT(b.first >= 0 && b.first + b.count <= (int)s.ent.size());
        for (int k = b.first; k < b.first + b.count; k++) {
            const int e = s.ent[k] >> 3, form = s.ent[k] & 7;
            EXPECT(e >= 0 && e < sc.p.n_edges && form < 4);
            if (k > b.first) EXPECT(s.ent[k] >> 3 >= s.ent[k - 1] >> 3);      // edge order
            const int bi = s.vidx[sc.ij[2 * e]], bj = s.vidx[sc.ij[2 * e + 1]];
            if (form == 0) EXPECT(b.br == bi && b.bc == bi);
            if (form == 1) EXPECT(b.br == bj && b.bc == bj);
            if (form == 2) EXPECT(b.br == bi && b.bc == bj);
            if (form == 3) EXPECT(b.br == bj && b.bc == bi);
            // inside the envelope the solvers are told
            EXPECT(s.row_first[7 * b.br / 32] <= 7 * b.bc / 32);
            EXPECT(s.row_first[(7 * b.br + 6) / 32] <= 7 * b.bc / 32);
        }
        hent += (size_t)b.count;
    }
    size_t want = 0, wantb = 0;
    for (int e = 0; e < sc.p.n_edges; e++) {
        const bool fi = s.vidx[sc.ij[2 * e]] >= 0, fj = s.vidx[sc.ij[2 * e + 1]] >= 0;
        want += fi + fj + (fi && fj);
        wantb += fi + fj;
    }
    EXPECT(hent == want && s.ent.size() == want + wantb);
    EXPECT((int)s.bfirst.size() == nf + 1 && (nf == 0 || s.bfirst[0] == (int)want) && s.bfirst[nf] == (int)s.ent.size());
    for (size_t R = 0; R < s.row_first.size(); R++) EXPECT(s.row_first[R] >= 0 && s.row_first[R] <= (int)R);
    const EgLayout L = eg_layout(&sc.p, s);
    EXPECT(L.up_bytes <= L.o_out_ctl && L.back_end <= L.o_St && L.o_flag + 64 <= L.total);
    std::unique_ptr<uint8_t[]> img(new uint8_t[L.up_bytes]);
    eg_pack(&sc.p, s, L, img.get());
    EgCtl c;
    std::memcpy(&c, img.get() + L.o_ctl, sizeof c);
    const bool run = sc.p.iterations > 0 && nf > 0 && sc.p.n_edges > 0;
    EXPECT(c.phase == (run ? 0 : 2) && c.iterations == sc.p.iterations && c.lambda_init == sc.p.lambda_init);
    EXPECT(std::memcmp(img.get() + L.o_S, sc.S.data(), 64 * (size_t)sc.p.n_vertices) == 0);
}

int main() {
    for (int nv : {1, 2, 3, 5, 6, 10, 11, 65, 151, 586}) {
        for (int k : {0, 1, 3})
            for (int fe : {0, 4}) structure_is_sound(Scene(nv, k, fe, nv % 4 ? 70 : 0));
    }
    {   // the envelope's last size and the first one beyond it
        Scene a(586, 1, 0, 0), b(587, 1, 0, 0);
        EXPECT(eg_check(&a.p, &a.r) == ORBHIP_OK);
        EXPECT(eg_check(&b.p, &b.r) == ORBHIP_ERR_UNSUPPORTED);
    }
    {   // every argument error, the outputs untouched (eg_check takes them const)
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        auto bad = [&](auto&& f) { Scene s(10, 2, 0, 9); f(s); return eg_check(&s.p, &s.r); };
        EXPECT(eg_check(nullptr, nullptr) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.S = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.fixed = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.edge_ij = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.edge_S = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.points = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.point_ref = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.r.S = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.r.points = nullptr; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.n_vertices = -1; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.n_edges = -1; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.n_points = -1; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.iterations = -1; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.lambda_init = 0.0; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([&](Scene& s) { s.p.lambda_init = nan; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.ij[4] = 10; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.ij[5] = -1; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.ij[6] = s.ij[7]; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.ref[3] = 10; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([&](Scene& s) { s.S[13] = nan; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([&](Scene& s) { s.eS[4] = inf; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.S[15] = 0.0; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.eS[7] = -1.0; }) == ORBHIP_ERR_ARG);
        EXPECT(bad([](Scene& s) { s.p.n_edges = kEgMaxEdges + 1; }) == ORBHIP_ERR_UNSUPPORTED);
        EXPECT(bad([](Scene& s) { s.p.n_points = kEgMaxPoints + 1; }) == ORBHIP_ERR_UNSUPPORTED);
        EXPECT(bad([](Scene& s) { s.p.n_vertices = kEgMaxVertices + 1; }) == ORBHIP_ERR_UNSUPPORTED);
    }
    std::printf(fails ? "essential_graph_args_check: %d FAILED\n" : "essential_graph_args_check: ok\n", fails);
    return fails ? 1 : 0;
}
