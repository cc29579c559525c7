// Bundle-adjustment back-end (Optimizer::LocalBundleAdjustment / BundleAdjustment) host driver.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbhip.h"

namespace orbhip {
struct BaWorkspace;
BaWorkspace* ba_create();
void ba_destroy(BaWorkspace* ws);
int ba_solve(BaWorkspace* ws, const orbhip_ba_problem* prob, orbhip_ba_result* res, const volatile int* stop,
             hipStream_t st);
// shard_mode: kShardNone = B independent problems; kShardLocal = B shards of ONE problem in this
// process (device-side sum across the batch); kShardRccl = this rank's B consecutive shards
// (rank * B .. rank * B + B - 1 of nranks * B, the same B on every rank) of ONE problem: they are
// summed on the device, then over the ranks by RCCL all-reduces on the communicator of ba_comm_init.
constexpr int kShardNone = 0, kShardLocal = 1, kShardRccl = 2;
// no_dag: never the persistent DAG Cholesky (set by the re-run after a DAG hand-off timeout);
// no_nd: no nested dissection (set by the re-run when the device setup refuses a plan)
// sx: null, or per problem the stereo part of an orbhip_ba_stereo_problem (kShardNone only): the
// call runs the stereo-edge kernels when some edge_ur of it is >= 0, else the monocular ones
struct BaStereoExt {
    const float* edge_ur;
    float bf, delta_s;
};
int ba_solve_batch(BaWorkspace* ws, const orbhip_ba_problem* const* probs, int B, orbhip_ba_result* const* res,
                   const volatile int* stop, hipStream_t st, int shard_mode, bool no_dag = false,
                   bool no_nd = false, const BaStereoExt* sx = nullptr);
// DAG hand-off timeouts this workspace saw, and the solves it re-ran on the other solvers
void ba_stats(BaWorkspace* ws, long long* timeouts, long long* reruns);
int ba_comm_init(BaWorkspace* ws, int nranks, int rank, const void* id);
int ba_comm_unique_id(void* id);
int ba_test_cholesky_reg(const double* A, const double* b, double* x, int n, int reps, float* ms,
                         unsigned long long* phases5);
int ba_test_cholesky(const double* A, const double* b, double* x, int n, unsigned long long* phases5, float* ms);
// host only (ba_prep.cpp): the problem preparation serial and on `threads` host threads; 0 when
// every list is identical (out4: blocks, pairs, Schur items, host ms of the threaded build), -1
// otherwise; threads == 1: a serial build into a reused Prep against a fresh one (out4: blocks,
// pairs, host ms of the fresh build, host ms of the reused one)
int ba_test_prepare(const orbhip_ba_problem* pr, int threads, double* out4);
}  // namespace orbhip
