// Host-only preparation of one bundle-adjustment problem (ba_prep.cpp): index mapping, the landmark
// and pose CSRs, the Schur pair lists, S's envelope and the Schur work items. No HIP call; the
// solver (ba_solver.hip) packs these lists into its device buffers.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/orbhip.h"
#include "ba_chol_dag.h"
#include "ba_nd.h"

namespace orbhip {

constexpr int kItemsWg = 128;      // Schur work items per k_ba_schur_items work-group (two lanes each)
constexpr int kSchurChunk = 16;    // pairs per Schur work item (one lane)
constexpr int kPrepParallelE = 20000;   // edges from which one problem's pair lists use host threads

// per-problem host preparation (O(E)): index mapping, CSRs, Schur pair lists by counting sort
struct Prep {
    int rc = 0;
    int P = 0, M = 0, E = 0, np = 0, n = 0, nblk = 0;
    std::vector<int> opt, pt_ptr, pt_edges, ps_ptr, ps_edges, blk_i, blk_j, blk_ptr, blk_pairs;
    std::vector<int> row_first;   // blocked Cholesky structure: first 32-col tile per 32-row tile
    std::vector<int> cb_tiles, cb_off;   // blocked Cholesky: envelope tiles per panel (cb_envelope_tiles)
    std::vector<int> items, fin;  // Schur work items {k0, k1, blk, slot} and finisher blocks {blk, slot0, n}
    std::vector<int> ifin;        // each item's finisher entry (-1: the block's only item)
    int nslot = 0;
    bool use_dag = false;         // the persistent tiled-DAG Cholesky (ba_chol_dag.hip)
    DagPlan dag;                  // its helper task lists
    bool use_nd = false;          // nested dissection over the DAG solver (ba_nd.hip): a lone banded GBA
    NdPlan nd;
    bool use_nd_sh = false;       // a shard of a sharded solve by keyframe segments (segment = shard)
    std::vector<unsigned char> own;   // ... the poses whose pose-side terms it adds
    size_t dag_task_cap = 0;      // ints reserved for the lists (RCCL shards: planned after the union envelope)
    // where this problem starts (elements) in the C / A / U / R segments and the int segment of the
    // packed buffers; the arrays inside: place_problem in ba_solver.hip
    size_t o_chi2 = 0, o_state = 0, o_obs = 0, o_scr = 0, o_int = 0;
};

// fills o from pr (chunk: pairs per Schur work item; threads > 1: a large problem's pair lists on the
// host pool); ORBHIP_OK, ORBHIP_ERR_ARG or ORBHIP_ERR_UNSUPPORTED
int prepare(const orbhip_ba_problem* pr, Prep& o, int chunk, int threads);
// a Prep for the next call with its vectors' capacity kept (no allocation / first-touch page
// faults on the hot path: the C5 lists are a few MB)
void prep_reset(Prep& o);
int host_threads();     // ORBHIP_BA_THREADS, else min(16, the hardware's)
bool host_pool_on();    // ORBHIP_HOST_POOL=0 keeps every host loop on the calling thread

// fn(i) for i in [0, n) on up to `threads` host threads (problems are independent)
template <typename F>
void parallel_for(int n, int threads, F fn) {
    threads = std::max(1, std::min(threads, n));
    if (threads == 1) {
        for (int i = 0; i < n; i++) fn(i);
        return;
    }
    std::atomic<int> next{0};
    auto work = [&] {
        for (int i; (i = next.fetch_add(1)) < n;) fn(i);
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}

// A persistent host worker pool for the preparation of one large problem: run(n, fn) calls fn(i)
// for i in [0, n) on the caller and the idle workers (indices claimed dynamically, so it completes
// on the caller alone if no worker is free), and returns when every call has returned. One run at a
// time: a concurrent caller (another context's thread) runs its loop alone.
// Created lazily, on the first large problem prepared with ORBHIP_PREP_THREADS > 1 (never
// otherwise), and deliberately leaked with detached workers: no destructor runs at process exit
// or library unload, so no join can meet a worker inside run() or a destroyed mutex.
class HostPool {
  public:
    static HostPool& get(int workers) {
        static HostPool* pool = new HostPool(workers);
        return *pool;
    }
    template <typename F>
    void run(int n, F&& fn) {
        std::unique_lock<std::mutex> busy(run_m_, std::try_to_lock);
        if (!busy.owns_lock() || workers_.empty()) {
            for (int i = 0; i < n; i++) fn(i);
            return;
        }
        std::function<void(int)> job(fn);
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &job;
            n_ = n;
            next_.store(0, std::memory_order_relaxed);
            active_ = (int)workers_.size();
            gen_++;
        }
        cv_.notify_all();
        for (int i; (i = next_.fetch_add(1)) < n;) job(i);
        std::unique_lock<std::mutex> g(m_);
        done_cv_.wait(g, [&] { return active_ == 0; });   // every worker has left this job
        job_ = nullptr;
    }

  private:
    explicit HostPool(int workers) {
        for (int w = 0; w < workers; w++) {
            std::thread t([this] { loop(); });
            t.detach();
            workers_.push_back(w);
        }
    }
    ~HostPool() = delete;   // leaked (see above)
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            std::function<void(int)>* job;
            int n;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return gen_ != seen; });
                seen = gen_;
                job = job_;
                n = n_;
            }
            if (job)
                for (int i; (i = next_.fetch_add(1)) < n;) (*job)(i);
            std::lock_guard<std::mutex> g(m_);
            if (--active_ == 0) done_cv_.notify_one();
        }
    }
    std::vector<int> workers_;   // the detached workers' indices (their count is what run() uses)
    std::mutex run_m_, m_;
    std::condition_variable cv_, done_cv_;
    std::function<void(int)>* job_ = nullptr;
    int n_ = 0, active_ = 0;
    std::atomic<int> next_{0};
    unsigned long long gen_ = 0;
};

}  // namespace orbhip
