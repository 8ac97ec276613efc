// Host build of the voxel bitmap's index arithmetic (fidget_amd/csrc/mesh_vox.hpp: no HIP, no device) for tests/test_voxels.py: prints what
// the header gives, one line per case; the test works the same things out in Python and compares.
//   words_D: n=...                                   fhvox::n_words
//   bits: b=... (64 values, lx fastest)              fhvox::voxel_bit
//   full_D_L_A_ox_oy_oz: r= vec= rows= slots= w=...  every word index k_vox_full's loop stores for the Full cell of level L at that origin
//                                                    (depth D, A: bitmap 16-byte aligned), in slot and store order, vec words per store
#include <stdio.h>

#include <string>
#include <vector>

#include "mesh_vox.hpp"

using namespace fhvox;

static uint64_t path_of(uint32_t level, const uint32_t o[3]) {       // 3 bits per level below a leading 1, the last level lowest
    uint64_t p = 1;
    for (uint32_t l = level; l-- > 0;) p = (p << 3) | ((o[0] >> l) & 1u) | (((o[1] >> l) & 1u) << 1) | (((o[2] >> l) & 1u) << 2);
    return p;
}

int main() {
    for (uint32_t d = 0; d <= 12; d++) printf("words_%u: n=%llu\n", d, (unsigned long long)n_words(d));
    std::string bits;
    for (uint32_t lz = 0; lz < 4; lz++) for (uint32_t ly = 0; ly < 4; ly++) for (uint32_t lx = 0; lx < 4; lx++) bits += (bits.empty() ? "" : ",") + std::to_string(voxel_bit(lx, ly, lz));
    printf("bits: b=%s\n", bits.c_str());
    for (uint32_t depth = 0; depth <= 4; depth++)
        for (uint32_t level = 0; level <= depth; level++)
            for (int aligned = 0; aligned < 2; aligned++) {
                const uint32_t m = (1u << level) - 1;
                const uint32_t origins[4][3] = {{0, 0, 0}, {m, m, m}, {m / 2, 0, m}, {1 & m, m, m / 2}};
                for (int oi = 0; oi < (level == 0 ? 1 : 4); oi++) {
                    const uint32_t* o = origins[oi];
                    const uint64_t path = path_of(level, o);
                    uint32_t back[3];
                    cell_origin(path, level, back);
                    if (back[0] != o[0] || back[1] != o[1] || back[2] != o[2]) { printf("origin mismatch\n"); return 1; }
                    const FullSlots S = full_slots(depth, level, aligned != 0);
                    const uint64_t cell = cell_word(path, level, depth);
                    std::string w;
                    for (uint32_t k = 0; k < (1u << S.lg_per_cell); k++)             // the loop of k_vox_full over one cell's slots
                        for (uint32_t q = 0; q < S.rows; q++) {
                            const uint64_t first = slot_word(S, depth, cell, k, q);
                            for (uint32_t v = 0; v < S.vec; v++) w += (w.empty() ? "" : ",") + std::to_string(first + v);
                        }
                    printf("full_%u_%u_%d_%u_%u_%u: r=%u vec=%u rows=%u slots=%u w=%s\n", depth, level, aligned, o[0], o[1], o[2], S.r, S.vec, S.rows, 1u << S.lg_per_cell, w.c_str());
                }
            }
    return 0;
}
