// Host-only check of StageLayout (orb_slam3_ros2_amd/csrc/stage.h), the offset allocator every
// host call lays its staging block out with. No HIP, no library: plain C++.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stage.h"

using orbhip::StageLayout;

static int failures = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                           \
        }                                                                         \
    } while (0)

// every offset is aligned and not below the end of the segment before it; the total is the aligned end
static void check_properties(size_t align, const std::vector<size_t>& sizes) {
    StageLayout lay(align);
    size_t end = 0;
    for (size_t bytes : sizes) {
        const size_t o = lay.take(bytes);
        CHECK(o % align == 0);
        CHECK(o >= end);
        CHECK(o < end + align);   // no more padding than the alignment needs
        end = o + bytes;
    }
    const size_t total = lay.total();
    CHECK(total % align == 0);
    CHECK(total >= end && total < end + align);
    CHECK(lay.total() == total);   // asking again takes nothing
}

int main() {
    const std::vector<size_t> mixed = {0, 1, 15, 16, 17, 0, 0, 255, 256, 257, 4096, 3, 0, 12345, 1};
    for (size_t align : {size_t(16), size_t(256)}) check_properties(align, mixed);

    // a zero-byte segment takes no space but still returns an aligned offset
    {
        StageLayout lay(16);
        CHECK(lay.take(0) == 0);
        CHECK(lay.take(5) == 0);
        CHECK(lay.take(0) == 16);
        CHECK(lay.take(0) == 16);
        CHECK(lay.take(7) == 16);
        CHECK(lay.total() == 32);
    }

    // triangulation-style, 16-byte segments: 2 sides of 48 bytes, 1 geometry of 48, 8 scale factors,
    // 8 sigma2, then a keyframe of 3 features (20-byte keypoints, 32-byte descriptors, 4-byte nodes,
    // 8-byte weights, 1-byte flags), the end of the upload, and a 5-byte tail. Offsets by hand.
    {
        StageLayout lay(16);
        CHECK(lay.take(96) == 0);
        CHECK(lay.take(48) == 96);
        CHECK(lay.take(32) == 144);
        CHECK(lay.take(32) == 176);
        CHECK(lay.take(60) == 208);    // ends at 268
        CHECK(lay.take(96) == 272);
        CHECK(lay.take(12) == 368);    // ends at 380
        CHECK(lay.take(24) == 384);
        CHECK(lay.take(3) == 416);     // 408 -> 416, ends at 419
        CHECK(lay.total() == 432);     // the upload's end
        CHECK(lay.take(5) == 432);
        CHECK(lay.total() == 448);
    }

    // projection-style, 256-byte segments: 8 keypoints of 20 bytes, their descriptors, 8 claimed bytes,
    // 8 scale factors, an absent (zero-byte) segment, 300 bytes of outputs. Offsets by hand.
    {
        StageLayout lay(256);
        CHECK(lay.take(160) == 0);
        CHECK(lay.take(256) == 256);   // exactly one segment: the next starts at 512, not 768
        CHECK(lay.take(8) == 512);
        CHECK(lay.take(32) == 768);
        CHECK(lay.take(0) == 1024);
        CHECK(lay.take(300) == 1024);
        CHECK(lay.total() == 1536);
    }

    if (failures) return 1;
    std::printf("stage layout OK\n");
    return 0;
}
