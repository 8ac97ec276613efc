// Host build of the arithmetic of the nesting of a voxel bitmap's outlines (fidget_amd/csrc/mesh_nest.hpp: no HIP, no device) for
// tests/test_nesting.py.  Reads one query per line of stdin,
//   G depth connectivity w0 w1 ...     B^3 hexadecimal words; B = 1 << depth, word (bz B + by) B + bx
// makes the outlines of all N layers with mesh_outline.hpp - counts, prefix sums, corners and successors - and the loops by walking
// `next` from every vertex not yet seen, in ascending order, so that loops are numbered by ascending leader; then runs what the
// kernels of nest.hip run, serially: per loop the row scan, the column walk and the vertex search (left_of), then the rounds of
// pointer doubling for the parents and for the depths, from one buffer into the other.  Prints, every number hexadecimal,
//   S    1 line        loop_start: N + 1 numbers
//   L    1 line        left per loop
//   P    1 line        parent per loop
//   D    1 line        depth per loop
// The test works the same out with tests/nesting_ref.py and compares.  The arrays are sized exactly, so that a step past them is the
// sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>

#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_nest.hpp"

static void print_line(char tag, const std::vector<uint32_t>& v) {
    printf("%c", tag);
    for (uint32_t x : v) printf(" %" PRIx32, x);
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
        // ---- the outlines: xy, next, vertex_start
        const size_t n_entries = (size_t)N * (N + 1) * C;
        std::vector<uint32_t> base(n_entries + 1), vertex_start(N + 1);
        uint32_t run = 0;
        for (uint32_t k = 0; k < N; k++) {
            vertex_start[k] = run;
            for (uint32_t b = 0; b <= N; b++)
                for (uint32_t c = 0; c < C; c++) {
                    base[(size_t)fhol::entry(depth, k, b, c)] = run;
                    run += fhol::count(fhol::row_masks(words.data(), depth, k, b, c));
                }
        }
        base[n_entries] = vertex_start[N] = run;
        std::vector<uint32_t> xy(run), next(run);
        for (uint32_t k = 0; k < N; k++)
            for (uint32_t b = 0; b <= N; b++)
                for (uint32_t c = 0; c < C; c++) {
                    const fhol::Masks M = fhol::row_masks(words.data(), depth, k, b, c);
                    const uint32_t first = base[(size_t)fhol::entry(depth, k, b, c)];
                    for (uint32_t d = 0; d < 4; d++)
                        for (uint32_t rest = M.leave[d]; rest != 0; rest &= rest - 1) {
                            const uint32_t s = (uint32_t)__builtin_ctz(rest), v = first + fhol::rank_leaving(M, s, d);
                            xy.at(v) = (fhol::CHUNK * c + s) | (b << 16);
                            next.at(v) = fhol::successor(words.data(), depth, k, k, conn, base.data(), M, b, c, s, d);
                        }
                }
        // ---- the loops: loop_of, leader, area2, loop_start
        std::vector<uint32_t> loop_of(run, fhnest::NONE), leader, loop_start(N + 1);
        std::vector<int64_t> area2;
        for (uint32_t k = 0, v = 0; k < N; k++) {
            loop_start[k] = (uint32_t)leader.size();
            for (; v < vertex_start[k + 1]; v++) {
                if (loop_of[v] != fhnest::NONE) continue;
                int64_t sum = 0;
                uint32_t w = v;
                do {
                    loop_of.at(w) = (uint32_t)leader.size();
                    const uint32_t p = xy[w], q = xy.at(next[w]);
                    sum += (int64_t)(p & 0xFFFFu) * (q >> 16) - (int64_t)(q & 0xFFFFu) * (p >> 16);
                    w = next[w];
                } while (w != v);
                leader.push_back(v);
                area2.push_back(sum);
            }
        }
        const uint32_t n = (uint32_t)leader.size();
        loop_start[N] = n;
        // ---- the nesting, as nest.hip runs it
        std::vector<uint32_t> left(n), link[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
        uint64_t largest = 0;
        for (uint32_t k = 0; k < N; k++) largest = std::max<uint64_t>(largest, loop_start[k + 1] - loop_start[k]);
        const uint32_t rounds = fhnest::rounds(largest);
        for (uint32_t l = 0; l < n; l++) {
            const uint32_t k = fhnest::layer_of(loop_start.data(), N, l);
            if (l < loop_start[k] || l >= loop_start[k + 1]) { printf("a loop outside its layer\n"); return 1; }
            left[l] = link[0][l] = fhnest::left_of(words.data(), depth, k, xy.data(), loop_of.data(), vertex_start[k], vertex_start[k + 1], loop_start[k], l, leader[l]);
        }
        for (uint32_t r = 0; r < rounds; r++)
            for (uint32_t l = 0; l < n; l++) link[(r + 1) & 1u][l] = fhnest::resolve_step(link[r & 1u].data(), area2.data(), l);
        const std::vector<uint32_t>& parent = link[rounds & 1u];
        std::vector<uint32_t> anc[2] = {parent, std::vector<uint32_t>(n)}, hops[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
        for (uint32_t l = 0; l < n; l++) hops[0][l] = parent[l] != fhnest::NONE;
        for (uint32_t r = 0; r < rounds; r++)
            for (uint32_t l = 0; l < n; l++) fhnest::depth_step(anc[r & 1u].data(), hops[r & 1u].data(), l, anc[(r + 1) & 1u][l], hops[(r + 1) & 1u][l]);
        for (uint32_t l = 0; l < n; l++)
            if (rounds > 0 && anc[rounds & 1u][l] != fhnest::NONE) { printf("a chain that has not ended\n"); return 1; }
        print_line('S', loop_start);
        print_line('L', left);
        print_line('P', parent);
        print_line('D', hops[rounds & 1u]);
    }
    return 0;
}
