// What the camera front-end (frontend.cpp) needs of a context beyond the C-ABI (orbhip_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbhip.h"

hipStream_t ctx_stream(const orbhip_ctx* c);
void ctx_set_extract_hints(orbhip_ctx* c, int cone_tile, int fast_nt);   // extract.h, extract_set_hints
