// Host build of the bit arithmetic of the outlines of a voxel bitmap's layers (fidget_amd/csrc/mesh_outline.hpp: no HIP, no device) for
// tests/test_outlines.py.  Reads one query per line of stdin,
//   G depth connectivity w0 w1 ...     B^3 hexadecimal words; B = 1 << depth, word (bz B + by) B + bx
// runs the passes the kernels of outline.hip run, serially over all N layers - the counts of every chunk of every lattice row from the
// row masks, their prefix sums, then per chunk the vertices' ranks, corners and successors - and prints, every number hexadecimal,
//   S    1 line        vertex_start: N + 1 numbers
//   X    1 line        xy: a | b << 16 per vertex
//   N    1 line        next per vertex
// The test works the same out with tests/outlines_ref.py and compares.  The arrays are sized exactly, so that a step past them is the
// sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_outline.hpp"

static void print_line(char tag, const std::vector<uint64_t>& v) {
    printf("%c", tag);
    for (uint64_t x : v) printf(" %" PRIx64, x);
    printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        uint32_t depth = 0, conn = 0;
        in >> what >> depth >> conn;
        if (!in || what != 'G' || depth > 4 || !fhol::conn_ok(conn)) { printf("bad query\n"); return 1; }
        std::vector<uint64_t> words((size_t)fhvox::n_words(depth));
        for (auto& w : words) in >> std::hex >> w;
        if (!in) { printf("bad query\n"); return 1; }
        const uint32_t N = 4u << depth, C = fhol::n_chunks(depth);
        const size_t n_entries = (size_t)N * (N + 1) * C;
        std::vector<uint32_t> base(n_entries + 1);
        std::vector<uint64_t> start(N + 1);
        uint32_t run = 0;
        for (uint32_t k = 0; k < N; k++) {
            start[k] = run;
            for (uint32_t b = 0; b <= N; b++)
                for (uint32_t c = 0; c < C; c++) {
                    const size_t e = (size_t)fhol::entry(depth, k, b, c);
                    if (e >= n_entries) { printf("an entry beyond the arrays\n"); return 1; }
                    base[e] = run;
                    run += fhol::count(fhol::row_masks(words.data(), depth, k, b, c));
                }
        }
        base[n_entries] = run;
        start[N] = run;
        std::vector<uint64_t> xy(run, ~(uint64_t)0), next(run, ~(uint64_t)0);
        for (uint32_t k = 0; k < N; k++)
            for (uint32_t b = 0; b <= N; b++)
                for (uint32_t c = 0; c < C; c++) {
                    const fhol::Masks M = fhol::row_masks(words.data(), depth, k, b, c);
                    const uint32_t first = base[(size_t)fhol::entry(depth, k, b, c)];
                    for (uint32_t d = 0; d < 4; d++)
                        for (uint32_t rest = M.leave[d]; rest != 0; rest &= rest - 1) {
                            const uint32_t s = (uint32_t)__builtin_ctz(rest), v = first + fhol::rank_leaving(M, s, d);
                            if (xy.at(v) != ~(uint64_t)0) { printf("a vertex written twice\n"); return 1; }
                            xy.at(v) = (fhol::CHUNK * c + s) | (b << 16);
                            next.at(v) = fhol::successor(words.data(), depth, k, k, conn, base.data(), M, b, c, s, d);
                        }
                }
        print_line('S', start);
        print_line('X', xy);
        print_line('N', next);
    }
    return 0;
}
