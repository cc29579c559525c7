// The workspace the context keeps for the projection searches (proj_kernels.hip) and
// SearchForInitialization (init_kernels.hip): one staging block and one pinned image for both, so
// a context's footprint is that of its largest call. Private to those two files; proj.h forward
// declares the struct for everyone else.
#pragma once
#include <hip/hip_runtime.h>

#include "proj.h"
#include "stage.h"

namespace orbhip {

struct ProjWorkspace {
    StageBlock s{true};      // the two-launch form writes its results straight into the pinned image
    int* arrive = nullptr;   // the one-launch search's arrival counter (0 between launches)
    int ahead = 4;   // rounds launched per host sync (adapts to the last search)
    int init_ahead = 6;   // the same for SearchForInitialization's rounds
    // the last projection search (orbhip_test_proj_stats): the form that produced the result (0 lists
    // + resolve, 1 a list overflowed and the rounds produced it, 2 rounds only, -1 none yet or no
    // queries), its rounds, the list entries the resolve saw (form 0) and the call's ent_cap
    int st_form = -1, st_rounds = 0, st_entries = 0, st_ent_cap = 0;
    // the last SearchForInitialization (orbhip_test_init_stats): the form that produced the result (0
    // the rounds converged, 1 the chain after a claim-slot overflow, 2 the chain after the round cap,
    // 3 the chain by ORBHIP_INIT_CHAIN, -1 none yet, no queries, or an error), the round that
    // changed nothing (else the rounds run), the octave-0 counts, and where the call's need[] lies
    // in the block (need_live: no later call has laid the block out again)
    int in_form = -1, in_round = 0, in_nq0 = 0, in_nr0 = 0;
    size_t in_need_off = 0;
    bool in_need_live = false;
    ~ProjWorkspace() {
        if (arrive) (void)hipFree(arrive);
    }
};

// the block of `total` bytes on both sides, and the arrival counter
inline int proj_ws_ensure(ProjWorkspace* ws, size_t total) {
    if (!ws->arrive) {
        ORBHIP_HIPOK(" proj", hipMalloc((void**)&ws->arrive, sizeof(int)));
        ORBHIP_HIPOK(" proj", hipMemset(ws->arrive, 0, sizeof(int)));
    }
    ws->in_need_live = false;   // the block is laid out anew
    ORBHIP_HIPOK(" proj", ws->s.ensure(total, total));
    return ORBHIP_OK;
}

}  // namespace orbhip
