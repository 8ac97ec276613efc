// Host build of the bit arithmetic of a voxel bitmap along a direction (fidget_amd/csrc/mesh_flow.hpp: no HIP, no device) for
// tests/test_directional.py.  Reads one query per line of stdin,
//   G depth s0 s1 ... k0 k1 ...     B^3 hexadecimal words of seeds, then B^3 of blockers; B = 1 << depth, word (bz B + by) B + bx
// walks the bitmaps the way the kernels of flow.hip do - a column of bricks with the carry, a row of bricks by its pairs (G, P), a brick
// with the nine words around it and the nine below, zeros beyond the grid - and prints, every number hexadecimal, a bitmap a line:
//   F    6 lines        the flow towards d = 0 .. 5, marched brick by brick with the carry in the word's entry plane
//   X    4 lines        the flow towards d = 0, 1 from the pairs (G, P) of the words, the carries folded along every row from its first
//                       brick on, then by halves (the association a scan across lanes makes)
//   M    24 lines       the seeds moved by s along axis a, for a = 0, 1, 2 and s = -4 .. -1, 1 .. 4
//   O    204 lines      the overhangs of the seeds as a solid for up = 0 .. 5, bed = 0, 1, reach2 = 0 .. 16
//   H    3 lines        the heights of the seeds along axis 0, 1, 2: 3 N^2 numbers each, as 32-bit patterns
// The test works the same out with tests/directional_ref.py and compares.  The arrays are sized exactly, so that a step past them is
// the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_flow.hpp"

struct Grid {
    uint32_t depth, B;
    std::vector<uint64_t> words;
    uint64_t at(int64_t bx, int64_t by, int64_t bz) const {          // 0 beyond the grid (coordinates may be -1 or B)
        if (bx < 0 || by < 0 || bz < 0 || bx >= (int64_t)B || by >= (int64_t)B || bz >= (int64_t)B) return 0;
        return words[fhvox::word_index(depth, (uint32_t)bx, (uint32_t)by, (uint32_t)bz)];
    }
};

static void print_line(char tag, const std::vector<uint64_t>& v) {
    printf("%c", tag);
    for (uint64_t x : v) printf(" %" PRIx64, x);
    printf("\n");
}
// the word of the i-th brick that a flow towards d meets in column (p, q) of the two other axes
static size_t column_word(const Grid& G, uint32_t d, uint32_t p, uint32_t q, uint32_t i) {
    const uint32_t along = (d & 1) ? i : G.B - 1 - i, axis = d >> 1;
    const uint32_t c[3] = {axis == 0 ? along : p, axis == 1 ? along : (axis == 0 ? p : q), axis == 2 ? along : q};
    return (size_t)fhvox::word_index(G.depth, c[0], c[1], c[2]);
}
// the carries of the row's bricks i in [lo, hi) composed by halves
static fhfl::GP fold_halves(const std::vector<fhfl::GP>& gp, uint32_t lo, uint32_t hi) {
    if (hi - lo == 1) return gp[lo];
    const uint32_t mid = lo + (hi - lo) / 2;
    return fhfl::gp_then(fold_halves(gp, lo, mid), fold_halves(gp, mid, hi));
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        Grid S, K;
        in >> what >> S.depth;
        if (!in || what != 'G' || S.depth > 2) { printf("bad query\n"); return 1; }
        K.depth = S.depth;
        S.B = K.B = 1u << S.depth;
        S.words.resize((size_t)fhvox::n_words(S.depth));
        K.words.resize(S.words.size());
        for (auto& w : S.words) in >> std::hex >> w;
        for (auto& w : K.words) in >> std::hex >> w;
        if (!in) { printf("bad query\n"); return 1; }
        const uint32_t B = S.B, N = 4 * B;
        const size_t n = S.words.size();

        for (uint32_t d = 0; d < 6; d++) {          // F: the march of k_flow_yz, here along x as well
            std::vector<uint64_t> out(n);
            for (uint32_t q = 0; q < B; q++)
                for (uint32_t p = 0; p < B; p++) {
                    uint64_t carry = 0;
                    for (uint32_t i = 0; i < B; i++) {
                        const size_t w = column_word(S, d, p, q, i);
                        const uint64_t r = fhfl::flow_word(S.words[w], ~K.words[w], carry, d);
                        carry = fhfl::carry_out(r | S.words[w], d);
                        out[w] = r;
                    }
                }
            print_line('F', out);
        }
        for (uint32_t d = 0; d < 2; d++)          // X: the pairs of k_flow_x
            for (uint32_t order = 0; order < 2; order++) {
                std::vector<uint64_t> out(n);
                for (uint32_t q = 0; q < B; q++)
                    for (uint32_t p = 0; p < B; p++) {
                        std::vector<fhfl::GP> gp(B);
                        for (uint32_t i = 0; i < B; i++) {
                            const size_t w = column_word(S, d, p, q, i);
                            gp[i] = fhfl::gp_of(S.words[w], ~K.words[w], d);
                            if ((gp[i].g | gp[i].p) & ~fhvm::X0) { printf("a pair beyond the X0 positions\n"); return 1; }
                        }
                        fhfl::GP before = fhfl::gp_identity();
                        for (uint32_t i = 0; i < B; i++) {
                            if (i > 0) before = order == 0 ? fhfl::gp_then(before, gp[i - 1]) : fold_halves(gp, 0, i);
                            const size_t w = column_word(S, d, p, q, i);
                            out[w] = fhfl::flow_word(S.words[w], ~K.words[w], fhfl::carry_from_x0(before.g, d), d);          // (nothing enters a row)
                        }
                    }
                print_line('X', out);
            }
        for (uint32_t axis = 0; axis < 3; axis++)          // M
            for (int32_t s = -4; s <= 4; s++) {
                if (s == 0) continue;
                std::vector<uint64_t> out(n);
                for (uint32_t bz = 0; bz < B; bz++)
                    for (uint32_t by = 0; by < B; by++)
                        for (uint32_t bx = 0; bx < B; bx++) {
                            const int64_t e[3] = {axis == 0, axis == 1, axis == 2};
                            out[(size_t)fhvox::word_index(S.depth, bx, by, bz)] = fhfl::moved(axis, S.at(bx, by, bz), S.at(bx - e[0], by - e[1], bz - e[2]),
                                                                                              S.at(bx + e[0], by + e[1], bz + e[2]), s);
                        }
                print_line('M', out);
            }
        for (uint32_t up = 0; up < 6; up++)          // O: k_overhangs
            for (uint32_t bed = 0; bed < 2; bed++)
                for (uint32_t reach2 = 0; reach2 <= fhfl::MAX_REACH2; reach2++) {
                    std::vector<uint64_t> out(n);
                    const uint32_t axis = up >> 1, U = fhfl::perp_u(axis), V = fhfl::perp_v(axis);
                    for (uint32_t bz = 0; bz < B; bz++)
                        for (uint32_t by = 0; by < B; by++)
                            for (uint32_t bx = 0; bx < B; bx++) {
                                uint64_t dil[2];          // at the brick, and at the one at -e(up)
                                int64_t under = 0;
                                for (uint32_t level = 0; level < 2; level++) {
                                    int64_t at[3] = {bx, by, bz};
                                    if (level == 1) at[axis] += (up & 1) ? -1 : 1;
                                    under = at[axis];
                                    uint64_t W[9];
                                    for (uint32_t t = 0; t < 9; t++) {
                                        int64_t c[3] = {at[0], at[1], at[2]};
                                        c[U] += (int64_t)(t % 3) - 1;
                                        c[V] += (int64_t)(t / 3) - 1;
                                        W[t] = S.at(c[0], c[1], c[2]);
                                    }
                                    dil[level] = fhfl::dilate_disc(W, U, V, reach2);
                                }
                                if (under < 0 || under >= (int64_t)B) dil[1] = bed ? ~(uint64_t)0 : 0;
                                out[(size_t)fhvox::word_index(S.depth, bx, by, bz)] = fhfl::unsupported(S.at(bx, by, bz), dil[0], dil[1], up);
                            }
                    print_line('O', out);
                }
        for (uint32_t axis = 0; axis < 3; axis++) {          // H: k_heights
            std::vector<uint64_t> out((size_t)3 * N * N);
            const uint32_t U = fhfl::perp_u(axis), V = fhfl::perp_v(axis);
            for (uint32_t q = 0; q < N; q++)
                for (uint32_t p = 0; p < N; p++) {
                    int32_t lo = -1, hi = -1, count = 0;
                    for (uint32_t b = 0; b < B; b++) {
                        int64_t at[3] = {0, 0, 0};
                        at[axis] = b; at[U] = p >> 2; at[V] = q >> 2;
                        const uint64_t col = fhfl::column(S.at(at[0], at[1], at[2]), axis, (p & 3) + 4 * (q & 3));
                        if (!col) continue;
                        if (lo < 0) lo = (int32_t)(4 * b + fhfl::column_lowest(col, axis));
                        hi = (int32_t)(4 * b + fhfl::column_highest(col, axis));
                        count += (int32_t)fhfl::column_count(col);
                    }
                    const size_t t = (size_t)q * N + p;
                    out[t] = (uint32_t)lo; out[(size_t)N * N + t] = (uint32_t)hi; out[(size_t)2 * N * N + t] = (uint32_t)count;
                }
            print_line('H', out);
        }
    }
    return 0;
}
