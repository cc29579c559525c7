// Host preparation of the bundle-adjustment problems (ba_prep.h): plain host C++, no HIP call.
#include "ba_prep.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "ba_chol_blocked.h"
#include "orbhip_ba.h"

namespace orbhip {

int host_threads() {
    static const int n = [] {
        const char* s = std::getenv("ORBHIP_BA_THREADS");
        if (s && std::atoi(s) > 0) return std::atoi(s);
        const unsigned hw = std::thread::hardware_concurrency();
        return (int)std::min<unsigned>(16, hw ? hw : 1);
    }();
    return n;
}

// r06 (late): one large problem (E >= kPrepParallelE, a GBA) writes its outputs on the pool (C5
// 0.146 -> 0.05 ms; its pair lists and packing measured slower there, tools/r06/gpu_hostpool_ab.sh);
// ORBHIP_HOST_POOL=0 keeps every host loop on the calling thread
bool host_pool_on() {
    static const bool on = [] {
        const char* s = std::getenv("ORBHIP_HOST_POOL");
        return !(s && s[0] == '0') && host_threads() > 1;
    }();
    return on;
}

// The Schur pair lists of prepare() on host threads, identical to the serial build:
//   1. landmark chunk t (contiguous): its pairs counted per pose row ia;
//   2. the same chunk writes its pairs (ib, ea, eb) at its per-row cursors (rows in order, chunks
//      in order within a row: landmark order within a row);
//   3. rows in parallel: a stable counting sort by ib gives the row's blocks (j = i always, others
//      with pairs) and their pairs at the row's offset; then the blocks are listed row by row.
static void schur_pairs_parallel(Prep& o, const int* eopt, int threads) {
    const int M = o.M, np = o.np;
    const int T = std::max(1, std::min(threads, M / 512 + 1));
    // scratch kept per calling thread across calls; the lambdas below run on the pool's threads, so
    // they must reach it through these references (a thread_local named inside them would be the
    // worker's own, empty instance)
    static thread_local std::vector<size_t> rc_s, roff_s;
    static thread_local std::vector<int> tj_s, tab_s;
    static thread_local std::vector<std::vector<int>> rb_s;
    std::vector<size_t>& rc = rc_s;
    std::vector<size_t>& roff = roff_s;
    std::vector<int>& tj = tj_s;
    std::vector<int>& tab = tab_s;
    std::vector<std::vector<int>>& rb = rb_s;
    std::vector<int> m0(T + 1);
    for (int t = 0; t <= T; t++) m0[t] = (int)((long long)M * t / T);
    rc.assign((size_t)T * np, 0);
    roff.assign(np + 1, 0);
    rb.resize(np);
    for (auto& v : rb) v.clear();
    HostPool& pool = HostPool::get(host_threads() - 1);
    pool.run(T, [&](int t) {
        size_t* c = rc.data() + (size_t)t * np;
        for (int m = m0[t]; m < m0[t + 1]; m++) {
            const int k0 = o.pt_ptr[m], k1 = o.pt_ptr[m + 1];
            for (int ka = k0; ka < k1; ka++) {
                const int ia = eopt[ka];
                if (ia < 0) continue;
                for (int kb = k0; kb < k1; kb++) c[ia] += eopt[kb] >= ia;
            }
        }
    });
    size_t total = 0;
    for (int i = 0; i < np; i++) {
        roff[i] = total;
        for (int t = 0; t < T; t++) {
            const size_t v = rc[(size_t)t * np + i];
            rc[(size_t)t * np + i] = total;
            total += v;
        }
    }
    roff[np] = total;
    tj.resize(total);
    tab.resize(2 * total);
    o.blk_pairs.resize(2 * total);
    pool.run(T, [&](int t) {
        size_t* c = rc.data() + (size_t)t * np;
        for (int m = m0[t]; m < m0[t + 1]; m++) {
            const int k0 = o.pt_ptr[m], k1 = o.pt_ptr[m + 1];
            for (int ka = k0; ka < k1; ka++) {
                const int ia = eopt[ka];
                if (ia < 0) continue;
                const int ea = o.pt_edges[ka];
                for (int kb = k0; kb < k1; kb++) {
                    const int ib = eopt[kb];
                    if (ib < ia) continue;
                    const size_t slot = c[ia]++;
                    tj[slot] = ib;
                    tab[2 * slot] = ea;
                    tab[2 * slot + 1] = o.pt_edges[kb];
                }
            }
        }
    });
    const int RB = 8;   // rows per task
    pool.run((np + RB - 1) / RB, [&](int task) {
        static thread_local std::vector<int> cj;
        cj.assign(np, 0);
        for (int i = task * RB; i < std::min(np, task * RB + RB); i++) {
            const size_t a = roff[i], b = roff[i + 1];
            for (size_t k = a; k < b; k++) cj[tj[k]]++;
            int s = 0;
            for (int j = i; j < np; j++) {
                const int cnt = cj[j];
                if (j == i || cnt > 0) { rb[i].push_back(j); rb[i].push_back(cnt); }
                cj[j] = s;   // from here on: the block's cursor within the row
                s += cnt;
            }
            for (size_t k = a; k < b; k++) {
                const size_t slot = a + (size_t)cj[tj[k]]++;
                o.blk_pairs[2 * slot] = tab[2 * k];
                o.blk_pairs[2 * slot + 1] = tab[2 * k + 1];
            }
            for (int j = i; j < np; j++) cj[j] = 0;
        }
    });
    o.blk_ptr.assign(1, 0);
    size_t s = 0;
    for (int i = 0; i < np; i++)
        for (size_t q = 0; q < rb[i].size(); q += 2) {
            o.blk_i.push_back(i);
            o.blk_j.push_back(rb[i][q]);
            s += (size_t)rb[i][q + 1];
            o.blk_ptr.push_back((int)s);
        }
}

// a Prep for the next call with its vectors' capacity kept (no allocation / first-touch page
// faults on the hot path: the C5 lists are a few MB)
void prep_reset(Prep& o) {
    o.rc = 0;
    o.P = o.M = o.E = o.np = o.n = o.nblk = 0;
    for (auto* v : {&o.opt, &o.pt_ptr, &o.pt_edges, &o.ps_ptr, &o.ps_edges, &o.blk_i, &o.blk_j, &o.blk_ptr,
                    &o.blk_pairs, &o.row_first, &o.cb_tiles, &o.cb_off, &o.items, &o.fin, &o.ifin})
        v->clear();
    o.own.clear();
    o.nslot = 0;
    o.use_dag = o.use_nd = o.use_nd_sh = false;
    o.dag = DagPlan{};
    o.nd = NdPlan{};
    o.dag_task_cap = 0;
    o.o_chi2 = o.o_state = o.o_obs = o.o_scr = o.o_int = 0;
}

int prepare(const orbhip_ba_problem* pr, Prep& o, int chunk, int threads) {
    const int P = pr->n_poses, M = pr->n_points, E = pr->n_edges;
    if (P < 0 || M < 0 || E < 0 || (P && (!pr->pose_q || !pr->pose_t || !pr->pose_fixed)) || (M && !pr->points) ||
        (E && (!pr->edge_pose || !pr->edge_point || !pr->edge_uv || !pr->edge_octave || !pr->inv_sigma2)))
        return ORBHIP_ERR_ARG;
    for (int e = 0; e < E; e++)
        if (pr->edge_pose[e] < 0 || pr->edge_pose[e] >= P || pr->edge_point[e] < 0 || pr->edge_point[e] >= M ||
            pr->edge_octave[e] < 0 || pr->edge_octave[e] >= pr->n_octaves)
            return ORBHIP_ERR_ARG;
    static const bool pdbg = std::getenv("ORBHIP_PREP_DBG") != nullptr;
    auto tus = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tp[8] = {tus()};
    o.P = P; o.M = M; o.E = E;
    o.opt.assign(P, -1);
    int np = 0;
    for (int i = 0; i < P; i++)
        if (!pr->pose_fixed[i]) o.opt[i] = np++;
    o.np = np;
    o.n = 6 * np;
    // n <= kCholSmallN: single-workgroup Cholesky (LDS-resident panel); larger: blocked solver
    if (o.n > kCbMaxN) return ORBHIP_ERR_UNSUPPORTED;
    const int* e_pose = pr->edge_pose;
    const int* e_pt = pr->edge_point;
    o.pt_ptr.assign(M + 1, 0);
    o.ps_ptr.assign(np + 1, 0);
    for (int e = 0; e < E; e++) {
        o.pt_ptr[e_pt[e] + 1]++;
        if (o.opt[e_pose[e]] >= 0) o.ps_ptr[o.opt[e_pose[e]] + 1]++;
    }
    for (int m = 0; m < M; m++) o.pt_ptr[m + 1] += o.pt_ptr[m];
    for (int i = 0; i < np; i++) o.ps_ptr[i + 1] += o.ps_ptr[i];
    o.pt_edges.resize(E);
    o.ps_edges.resize(o.ps_ptr[np]);
    // scratch kept per host thread across calls (no page faults on the hot path): eopt[k] = the opt
    // index of the pose of landmark-CSR slot k (one load per pair endpoint below), cnt = the dense
    // (i, j) pair counts, then the blocks' fill cursors
    static thread_local std::vector<int> eopt, cnt, fp, fq;   // (fp / fq: the fill cursors, no allocation per call)
    eopt.resize(E);
    {
        fp.assign(o.pt_ptr.begin(), o.pt_ptr.end() - 1);
        fq.assign(o.ps_ptr.begin(), o.ps_ptr.end() - 1);
        for (int e = 0; e < E; e++) {
            const int oi = o.opt[e_pose[e]];
            const int k = fp[e_pt[e]]++;
            o.pt_edges[k] = e;
            eopt[k] = oi;
            if (oi >= 0) o.ps_edges[fq[oi]++] = e;
        }
    }
    tp[1] = tus();
    // Schur pairs (a, b) of one landmark with opt(a) <= opt(b), grouped by block (i, j) (row-major
    // over i <= j, every diagonal block listed); within a block: landmark order (deterministic).
    // Large problems: schur_pairs_parallel (the same lists, built on host threads)
    if (threads > 1 && E >= kPrepParallelE) {
        schur_pairs_parallel(o, eopt.data(), threads);
    } else {
        // a counting sort on the dense block id i*np + j
        cnt.assign((size_t)np * np, 0);
        size_t npairs = 0;
        for (int m = 0; m < M; m++) {
            const int k0 = o.pt_ptr[m], k1 = o.pt_ptr[m + 1];
            for (int ka = k0; ka < k1; ka++) {
                const int ia = eopt[ka];
                if (ia < 0) continue;
                int* row = cnt.data() + (size_t)ia * np;
                for (int kb = k0; kb < k1; kb++) {
                    const int ib = eopt[kb];
                    if (ib < ia) continue;   // also drops the fixed poses (-1)
                    row[ib]++;
                    npairs++;
                }
            }
        }
        o.blk_ptr.assign(1, 0);
        {
            int s = 0;
            for (int i = 0; i < np; i++) {
                int* row = cnt.data() + (size_t)i * np;
                for (int j = i; j < np; j++) {
                    const int c = row[j];
                    if (i == j || c > 0) {
                        o.blk_i.push_back(i);
                        o.blk_j.push_back(j);
                        row[j] = s;   // from here on: the block's fill cursor
                        s += c;
                        o.blk_ptr.push_back(s);
                    }
                }
            }
        }
        o.blk_pairs.resize(2 * npairs);
        int* bp = o.blk_pairs.data();
        for (int m = 0; m < M; m++) {
            const int k0 = o.pt_ptr[m], k1 = o.pt_ptr[m + 1];
            for (int ka = k0; ka < k1; ka++) {
                const int ia = eopt[ka];
                if (ia < 0) continue;
                const int ea = o.pt_edges[ka];
                int* row = cnt.data() + (size_t)ia * np;
                for (int kb = k0; kb < k1; kb++) {
                    const int ib = eopt[kb];
                    if (ib < ia) continue;
                    const int slot = row[ib]++;
                    bp[2 * (size_t)slot] = ea;
                    bp[2 * (size_t)slot + 1] = o.pt_edges[kb];
                }
            }
        }
    }
    tp[2] = tus();
    o.nblk = (int)o.blk_i.size();
    {   // envelope of S: first pose column coupled to each pose row (blocks are stored i <= j)
        std::vector<int> fp(np);
        for (int i = 0; i < np; i++) fp[i] = i;
        for (int b = 0; b < o.nblk; b++) fp[o.blk_j[b]] = std::min(fp[o.blk_j[b]], o.blk_i[b]);
        const int nt = (o.n + 31) / 32;
        o.row_first.assign(nt, 0);
        for (int R = 0; R < nt; R++) {
            int f = R;
            for (int r = 32 * R; r < std::min(o.n, 32 * R + 32); r++) f = std::min(f, (6 * fp[r / 6]) / 32);
            o.row_first[R] = f;
        }
    }
    // Schur work items: chunks of at most `chunk` pairs; a block with one off-diagonal chunk is
    // written by its item, the others (and every diagonal block) are summed inside one work-group
    // of k_ba_schur_items (r06): at most kItemsWg chunks per block (a longer block takes longer
    // chunks), and a block that would straddle a work-group boundary starts the next work-group
    // (empty items, blk -1, pad the one before)
    // (two passes: the count, then direct stores into the sized arrays; per-item vector inserts
    // cost ~6 ns each, 0.3 ms at C5)
    size_t nit = 0, nfin = 0;
    for (int b = 0; b < o.nblk; b++) {
        const int k0 = o.blk_ptr[b], k1 = o.blk_ptr[b + 1];
        if (o.blk_i[b] != o.blk_j[b] && k1 - k0 <= chunk) { nit++; continue; }
        const int cb = std::max(chunk, (k1 - k0 + kItemsWg - 1) / kItemsWg);
        const int nch = std::max(1, (k1 - k0 + cb - 1) / cb);
        const int at = (int)(nit % kItemsWg);
        if (at + nch > kItemsWg) nit += kItemsWg - at;
        nit += nch;
        nfin++;
    }
    o.items.resize(4 * nit);
    o.ifin.resize(nit);
    o.fin.resize(3 * nfin);
    int* itp = o.items.data();
    int* ifp = o.ifin.data();
    int* fnp = o.fin.data();
    size_t it = 0;
    int f = 0;
    for (int b = 0; b < o.nblk; b++) {
        const int k0 = o.blk_ptr[b], k1 = o.blk_ptr[b + 1];
        const bool diag = o.blk_i[b] == o.blk_j[b];
        if (!diag && k1 - k0 <= chunk) {
            int* q = itp + 4 * it;
            q[0] = k0; q[1] = k1; q[2] = b; q[3] = -1;
            ifp[it++] = -1;
            continue;
        }
        const int cb = std::max(chunk, (k1 - k0 + kItemsWg - 1) / kItemsWg);
        const int nch = std::max(1, (k1 - k0 + cb - 1) / cb);
        const int at = (int)(it % kItemsWg);
        if (at + nch > kItemsWg)
            for (int q = at; q < kItemsWg; q++) {
                int* r = itp + 4 * it;
                r[0] = 0; r[1] = 0; r[2] = -1; r[3] = -1;
                ifp[it++] = -1;
            }
        fnp[3 * f] = b; fnp[3 * f + 1] = o.nslot; fnp[3 * f + 2] = nch;
        for (int c = 0; c < nch; c++) {
            int* r = itp + 4 * it;
            r[0] = k0 + c * cb; r[1] = std::min(k1, k0 + (c + 1) * cb); r[2] = b; r[3] = o.nslot + c;
            ifp[it++] = f;
        }
        o.nslot += nch;
        f++;
    }
    tp[3] = tus();
    if (pdbg) std::fprintf(stderr, "prepare E=%d: csr %.0f us, pairs %.0f us, envelope+items %.0f us\n", E, tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2]);
    return ORBHIP_OK;
}

int ba_test_prepare(const orbhip_ba_problem* pr, int threads, double* out4) {
    Prep a, b;
    int rc = prepare(pr, a, kSchurChunk, 1);
    if (rc) return rc;
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    // out4[3]: the threaded build (threads > 1) or the serial build into a reused Prep (threads = 1)
    if (threads == 1) {
        prep_reset(a);
        const auto t1 = std::chrono::steady_clock::now();
        rc = prepare(pr, a, kSchurChunk, 1);
        const double ms1 = ms_since(t1);
        if (rc) return rc;
        if (out4) out4[3] = ms1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    rc = prepare(pr, b, kSchurChunk, threads);
    const double ms = ms_since(t0);
    if (rc) return rc;
    if (threads == 1) {
        if (out4) { out4[0] = b.nblk; out4[1] = (double)(b.blk_pairs.size() / 2); out4[2] = ms; }
        return a.blk_pairs == b.blk_pairs ? ORBHIP_OK : -1;
    }
    const bool same = a.opt == b.opt && a.pt_ptr == b.pt_ptr && a.pt_edges == b.pt_edges && a.ps_ptr == b.ps_ptr &&
                      a.ps_edges == b.ps_edges && a.blk_i == b.blk_i && a.blk_j == b.blk_j && a.blk_ptr == b.blk_ptr &&
                      a.blk_pairs == b.blk_pairs && a.row_first == b.row_first && a.items == b.items && a.fin == b.fin &&
                      a.nslot == b.nslot && a.nblk == b.nblk;
    if (out4) {
        out4[0] = b.nblk;
        out4[1] = (double)(b.blk_pairs.size() / 2);
        out4[2] = (double)(b.items.size() / 4);
        out4[3] = ms;
    }
    return same ? ORBHIP_OK : -1;
}

}  // namespace orbhip
