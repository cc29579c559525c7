// Stand-alone check of the BA host preparation (csrc/ba_prep.cpp), for running under sanitizers
// on the CPU: prepares a few seeded problems serially, into a reused Prep, and on host threads
// (a problem large enough for the threaded pair lists), and an invalid one. No GPU, no HIP call.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//     -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iorb_slam3_ros2_amd/csrc \
//     tools/ba_prep_check.cpp orb_slam3_ros2_amd/csrc/ba_prep.cpp -o ba_prep_check && ./ba_prep_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "orbhip_ba.h"

namespace {

struct Problem {
    std::vector<float> q, t, pts, uv, sig;
    std::vector<unsigned char> fixed;
    std::vector<int> ep, em, oct;
    orbhip_ba_problem c{};
};

// P keyframes (the first nfix fixed), M landmarks, each seen by `obs` distinct keyframes of a window
void make(Problem& p, int P, int M, int obs, int window, int nfix, uint64_t seed) {
    auto rnd = [&seed] {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(seed >> 33);
    };
    p.q.assign(4 * (size_t)P, 0.f);
    for (int i = 0; i < P; i++) p.q[4 * i + 3] = 1.f;
    p.t.assign(3 * (size_t)P, 0.f);
    p.pts.assign(3 * (size_t)M, 1.f);
    p.fixed.assign(P, 0);
    for (int i = 0; i < nfix; i++) p.fixed[i] = 1;
    p.sig.assign(8, 1.f);
    for (int m = 0; m < M; m++) {
        const int start = rnd() % P;
        std::vector<int> seen;
        while ((int)seen.size() < obs) {
            const int k = (start + rnd() % window) % P;
            bool dup = false;
            for (int s : seen) dup = dup || s == k;
            if (!dup) seen.push_back(k);
        }
        for (int k : seen) {
            p.ep.push_back(k);
            p.em.push_back(m);
            p.oct.push_back(rnd() % 8);
            p.uv.push_back(0.f);
            p.uv.push_back(0.f);
        }
    }
    orbhip_ba_problem& c = p.c;
    c.n_poses = P; c.n_points = M; c.n_edges = (int)p.ep.size(); c.n_octaves = 8;
    c.pose_q = p.q.data(); c.pose_t = p.t.data(); c.pose_fixed = p.fixed.data(); c.points = p.pts.data();
    c.edge_pose = p.ep.data(); c.edge_point = p.em.data(); c.edge_uv = p.uv.data(); c.edge_octave = p.oct.data();
    c.inv_sigma2 = p.sig.data();
}

}  // namespace

int main() {
    struct { int P, M, obs, window, nfix, threads; } cases[] = {
        {7, 60, 4, 7, 1, 1},          // a small LBA: serial, then into the reused Prep
        {23, 300, 4, 23, 2, 1},
        {1, 5, 1, 1, 1, 1},           // every keyframe fixed: n = 0
        {100, 3000, 4, 20, 1, 4},     // below the threaded size: the serial lists either way
        {200, 6000, 4, 30, 1, 4},     // 24000 edges: the pair lists on 4 host threads
        {200, 6000, 5, 30, 1, 16},
    };
    int bad = 0;
    for (const auto& k : cases) {
        Problem p;
        make(p, k.P, k.M, k.obs, k.window, k.nfix, 1000 + k.P);
        double out4[4] = {0, 0, 0, 0};
        const int rc = orbhip::ba_test_prepare(&p.c, k.threads, out4);
        std::printf("P=%d M=%d E=%d threads=%d: rc %d, %.0f blocks, %.0f pairs\n", k.P, k.M, p.c.n_edges, k.threads, rc,
                    out4[0], out4[1]);
        bad += rc != 0;
    }
    Problem p;
    make(p, 7, 60, 4, 7, 1, 5);
    p.ep[3] = 7;   // out of range
    const int rc = orbhip::ba_test_prepare(&p.c, 1, nullptr);
    std::printf("invalid edge: rc %d\n", rc);
    bad += rc != ORBHIP_ERR_ARG;
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
