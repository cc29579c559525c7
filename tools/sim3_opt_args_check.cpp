// OptimizeSim3's host side without a device: the argument check, the staging layout and the packing
// of a batch (csrc/sim3_opt.h), as a program of its own so that it can run under AddressSanitizer and
// UBSan on the CPU:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -Iorb_slam3_ros2_amd/csrc tools/sim3_opt_args_check.cpp -o /tmp/sim3_opt_args_check && /tmp/sim3_opt_args_check
// The image is allocated with exactly the bytes the layout asks for, so a write past it is reported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "sim3_opt.h"

using namespace orbhip;

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

struct Scene {
    std::vector<float> X1, X2, o1, o2, i1, i2;
    orbhip_sim3_opt_problem p{};
    explicit Scene(int n) : X1(3 * n), X2(3 * n), o1(2 * n), o2(2 * n), i1(n), i2(n) {
        for (int e = 0; e < n; e++) {
            for (int k = 0; k < 3; k++) { X1[3 * e + k] = 1.0f + e + 0.1f * k; X2[3 * e + k] = 2.0f + e + 0.1f * k; }
            for (int k = 0; k < 2; k++) { o1[2 * e + k] = 300.0f + e + k; o2[2 * e + k] = 200.0f + e + k; }
            i1[e] = 1.0f / (1 + e % 3); i2[e] = 0.5f / (1 + e % 5);
        }
        p.n = n;
        p.X1c = n ? X1.data() : nullptr; p.X2c = n ? X2.data() : nullptr;
        p.obs1 = n ? o1.data() : nullptr; p.obs2 = n ? o2.data() : nullptr;
        p.inv_sigma2_1 = n ? i1.data() : nullptr; p.inv_sigma2_2 = n ? i2.data() : nullptr;
        const float cam[4] = {600.f, 601.f, 320.f, 240.f};
        std::memcpy(p.cam1, cam, sizeof cam);
        std::memcpy(p.cam2, cam, sizeof cam);
        p.q[3] = 1.0; p.t[0] = 0.1; p.t[1] = -0.2; p.t[2] = 0.3; p.s = 1.1; p.th2 = 10.0; p.fix_scale = n % 2;
    }
};

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- the check ----
    Scene a(65);
    orbhip_sim3_opt_result r{};
    EXPECT(sim3_opt_check(&a.p, 1, &r) == ORBHIP_OK);
    EXPECT(sim3_opt_check(nullptr, 0, nullptr) == ORBHIP_OK);
    EXPECT(sim3_opt_check(nullptr, 1, &r) == ORBHIP_ERR_ARG);
    EXPECT(sim3_opt_check(&a.p, 1, nullptr) == ORBHIP_ERR_ARG);
    EXPECT(sim3_opt_check(&a.p, -1, &r) == ORBHIP_ERR_ARG);
    EXPECT(sim3_opt_check(&a.p, kSim3OptMaxBatch + 1, &r) == ORBHIP_ERR_UNSUPPORTED);   // refused before probs[1] is read
    auto bad = [&](auto&& change, int want) {
        orbhip_sim3_opt_problem p = a.p;
        change(p);
        EXPECT(sim3_opt_check(&p, 1, &r) == want);
        orbhip_sim3_opt_problem two[2] = {a.p, p};
        orbhip_sim3_opt_result rr[2] = {};
        EXPECT(sim3_opt_check(two, 2, rr) == want);
    };
    bad([](auto& p) { p.n = -1; }, ORBHIP_ERR_ARG);
    bad([](auto& p) { p.X1c = nullptr; }, ORBHIP_ERR_ARG);
    bad([](auto& p) { p.X2c = nullptr; }, ORBHIP_ERR_ARG);
    bad([](auto& p) { p.obs1 = nullptr; }, ORBHIP_ERR_ARG);
    bad([](auto& p) { p.obs2 = nullptr; }, ORBHIP_ERR_ARG);
    bad([](auto& p) { p.inv_sigma2_1 = nullptr; }, ORBHIP_ERR_ARG);
    bad([](auto& p) { p.inv_sigma2_2 = nullptr; }, ORBHIP_ERR_ARG);
    for (double v : {0.0, -500.0, nan, inf}) {
        bad([v](auto& p) { p.cam1[0] = (float)v; }, ORBHIP_ERR_ARG);
        bad([v](auto& p) { p.cam1[1] = (float)v; }, ORBHIP_ERR_ARG);
        bad([v](auto& p) { p.cam2[0] = (float)v; }, ORBHIP_ERR_ARG);
        bad([v](auto& p) { p.cam2[1] = (float)v; }, ORBHIP_ERR_ARG);
        bad([v](auto& p) { p.th2 = v; }, ORBHIP_ERR_ARG);
        bad([v](auto& p) { p.s = v; }, ORBHIP_ERR_ARG);
    }
    for (double v : {nan, inf, -inf}) {
        for (int k = 0; k < 4; k++) bad([v, k](auto& p) { p.q[k] = v; }, ORBHIP_ERR_ARG);
        for (int k = 0; k < 3; k++) bad([v, k](auto& p) { p.t[k] = v; }, ORBHIP_ERR_ARG);
    }
    bad([](auto& p) { p.n = kSim3OptMaxN + 1; }, ORBHIP_ERR_UNSUPPORTED);
    bad([](auto& p) { p.n = 0; p.X1c = p.X2c = p.obs1 = p.obs2 = p.inv_sigma2_1 = p.inv_sigma2_2 = nullptr; }, ORBHIP_OK);

    // ---- layout and packing: 1, 3 and 64 problems of mixed sizes (0 among them), the largest size ----
    for (int B : {1, 3, kSim3OptMaxBatch}) {
        std::vector<std::unique_ptr<Scene>> sc;
        std::vector<orbhip_sim3_opt_problem> probs;
        for (int b = 0; b < B; b++) {
            const int n = B == 1 ? kSim3OptMaxN : (b % 4 == 2 ? 0 : 1 + 37 * b % 300);
            sc.emplace_back(new Scene(n));
            probs.push_back(sc.back()->p);
        }
        std::vector<orbhip_sim3_opt_result> res(B);
        EXPECT(sim3_opt_check(probs.data(), B, res.data()) == ORBHIP_OK);
        const Sim3OptLayout L = sim3_opt_layout(probs.data(), B);
        EXPECT(L.o_hdr == 0 && L.o_edge >= sizeof(Sim3OptHdr) * B && L.up_bytes >= L.o_edge + sizeof(Sim3OptEdge) * L.E);
        EXPECT(L.o_out >= L.up_bytes && L.o_keep >= L.o_out + sizeof(Sim3OptOut) * B && L.back_end >= L.o_keep + L.E);
        EXPECT(L.o_c2 >= L.back_end && L.o_rm >= L.o_c2 + 16 * L.E && L.total >= L.o_rm + L.E);
        EXPECT(L.o_edge % 256 == 0 && L.o_out % 256 == 0 && L.o_c2 % 256 == 0);
        std::unique_ptr<uint8_t[]> img(new uint8_t[L.up_bytes]);
        std::memset(img.get(), 0xEE, L.up_bytes);
        sim3_opt_pack(probs.data(), B, L, img.get());
        const Sim3OptHdr* hh = (const Sim3OptHdr*)(img.get() + L.o_hdr);
        const Sim3OptEdge* he = (const Sim3OptEdge*)(img.get() + L.o_edge);
        size_t off = 0;
        for (int b = 0; b < B; b++) {
            const Scene& s = *sc[b];
            EXPECT(hh[b].n == s.p.n && (size_t)hh[b].off == off && hh[b].fix_scale == (s.p.n % 2));
            EXPECT(hh[b].S0[3] == 1.0 && hh[b].S0[4] == 0.1 && hh[b].S0[7] == 1.1 && hh[b].cam2[1] == 601.0);
            EXPECT(hh[b].delta == (double)(float)std::sqrt(10.0) && hh[b].th2 == 10.0);
            for (int e = 0; e < s.p.n; e += (s.p.n > 64 ? 61 : 1)) {
                const Sim3OptEdge& E = he[off + e];
                EXPECT(E.f[0] == s.X1[3 * e] && E.f[5] == s.X2[3 * e + 2] && E.f[7] == s.o1[2 * e + 1] &&
                       E.f[8] == s.o2[2 * e] && E.f[10] == s.i1[e] && E.f[11] == s.i2[e]);
            }
            off += (size_t)s.p.n;
        }
        EXPECT(off == L.E);
    }
    if (fails) return 1;
    std::printf("sim3 opt args OK\n");
    return 0;
}
