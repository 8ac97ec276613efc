// Host build of the clean-buffer-set rule (fidget_amd/csrc/frame_plan.hpp: set_is_clean, leaves_set_clean, set_left_by - no HIP, no
// device) for tests/test_clean_sets.py.  Arguments: cases of eight numbers each -
//   left.valid left.pixels left.mind_words  want.pixels want.mind_words  out_is_device profiling queued_whole
// - and per case one line: skip=<the frame skips its clears> cleans=<its k_finish3d cleans behind itself> then the record the frame leaves.
#include <stdio.h>
#include <stdlib.h>

#include "frame_plan.hpp"

int main(int argc, char** argv) {
    if ((argc - 1) % 8) { fprintf(stderr, "eight numbers per case\n"); return 2; }
    for (int i = 1; i + 8 <= argc; i += 8) {
        auto num = [&](int k) { return strtoull(argv[i + k], nullptr, 10); };
        CleanSig left, want;
        left.valid = num(0) != 0; left.pixels = num(1); left.mind_words = num(2);
        want.valid = true; want.pixels = num(3); want.mind_words = num(4);
        CleanFrame f;
        f.out_is_device = num(5) != 0; f.profiling = num(6) != 0;
        const CleanSig rec = set_left_by(f, want, num(7) != 0);
        printf("skip=%d cleans=%d valid=%d pixels=%llu mind_words=%llu\n", set_is_clean(left, want) ? 1 : 0, leaves_set_clean(f) ? 1 : 0, rec.valid ? 1 : 0,
               (unsigned long long)rec.pixels, (unsigned long long)rec.mind_words);
    }
    return 0;
}
