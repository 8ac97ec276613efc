// Host build of the check of a triangle mesh (fidget_amd/csrc/mesh_topo.hpp: no HIP, no device) for tests/test_mesh_topology.py.  Reads
// one query per line of stdin, every number hexadecimal (floats as their bit patterns),
//   Q weld table_log2 nv [3 nv floats] indexed nt [3 nt indices, if indexed]
// table_log2 = 0: the library's choice.  Walks the mesh the way the kernels of topo.hip do, one corner or triangle after the other - the
// check, the weld through fhtopo::vertex_insert, the flags and ranks of the first corners, the edges through fhtopo::edge_insert, the
// classes at the first uses, a union-find towards the smaller root, the shells' table - with the plain memory operations of
// fhtopo::Serial, and prints, every number hexadecimal:
//   C  the twelve counts;  with a triangle rejected nothing else
//   O  instead of all of it when a table had no room; the program then ends
//   V  the vertices' bits;  T  the triangles;  S  a shell per triangle;  E kind  the edges of one class, a b a b ..
//   H  per shell: triangles first unbalanced lo[3] hi[3] volume6 area2 (floats and doubles as bits; the sums in triangle order)
//   F  the triangles' volume6 terms;  A  their area2 terms
// The test works the same out with tests/mesh_topology_ref.py and compares.  The arrays are sized exactly, so that a step past them is
// the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_topo.hpp"

using fhtopo::Serial;

static uint64_t bits64(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static void row(const char* tag, const std::vector<uint64_t>& v) {
    printf("%s", tag);
    for (uint64_t x : v) printf(" %" PRIx64, x);
    printf("\n");
}
static uint32_t find(std::vector<uint32_t>& parent, uint32_t x) {
    while (parent[x] != x) x = parent[x];
    return x;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> std::hex;
        char what = 0;
        uint32_t weld = 0, table_log2 = 0, indexed = 0;
        uint64_t nv = 0, nt = 0;
        in >> what >> weld >> table_log2 >> nv;
        if (!in || what != 'Q' || weld > 1 || table_log2 > 24 || nv > (1u << 20)) { printf("bad query\n"); return 1; }
        std::vector<float> vertices((size_t)3 * nv);
        for (float& x : vertices) { uint32_t b = 0; in >> b; x = fhtopo::bits_float(b); }
        in >> indexed >> nt;
        if (!in || indexed > 1 || nt > (1u << 20) || (!indexed && !weld)) { printf("bad query\n"); return 1; }
        std::vector<uint64_t> triangles(indexed ? (size_t)3 * nt : 0);
        for (uint64_t& x : triangles) in >> x;
        if (!in) { printf("bad query\n"); return 1; }
        const uint32_t T = (uint32_t)nt, C = 3 * T;
        if (!indexed && nv > C) nv = C;
        std::vector<uint64_t> counts(12);
        counts[0] = T;
        // k_mt_check
        for (uint32_t t = 0; t < T; t++) {
            bool rejected = false;
            for (uint32_t k = 0; k < 3; k++) {
                const uint64_t at = indexed ? triangles[(size_t)3 * t + k] : (uint64_t)3 * t + k;
                if (at >= nv || !fhtopo::finite3(&vertices[(size_t)(3 * at)])) rejected = true;
            }
            counts[1] += rejected;
        }
        if (counts[1] || !T) { row("C", counts); continue; }
        const uint32_t log2_v = weld ? (table_log2 ? table_log2 : fhtopo::default_log2(T)) : 0, log2_e = table_log2 ? table_log2 : fhtopo::default_log2(T);
        const size_t slots_v = weld ? (size_t)fhtopo::n_slots(log2_v) : 0, slots_e = (size_t)fhtopo::n_slots(log2_e);
        counts[10] = slots_v; counts[11] = slots_e;
        const fhtopo::Corners corners{vertices.data(), indexed ? triangles.data() : nullptr};
        std::vector<uint32_t> vid(C), corner_slot(C);
        std::vector<float> out_vertices;
        bool full = false;
        if (weld) {
            // k_mt_weld
            std::vector<uint32_t> table(fhtopo::VERTEX_SLOT_WORDS * slots_v, fhtopo::EMPTY);
            for (uint32_t c = 0; c < C && !full; c++) {
                uint64_t slot = 0;
                full = !fhtopo::vertex_insert<Serial>(corners, table.data(), log2_v, c, slot);
                corner_slot[c] = (uint32_t)slot;
            }
            if (full) { printf("O vertex\n"); return 0; }
            // k_mt_vflag, the prefix sums, k_mt_vemit
            std::vector<uint32_t> rank((size_t)C + 1);
            for (uint32_t c = 0; c < C; c++) rank[(size_t)c + 1] = rank[c] + (fhtopo::vertex_first(table.data(), corner_slot[c]) == c ? 1u : 0u);
            counts[3] = rank[C];
            out_vertices.resize((size_t)3 * rank[C]);
            for (uint32_t c = 0; c < C; c++) {
                const uint32_t f = fhtopo::vertex_first(table.data(), corner_slot[c]);
                vid[c] = rank[f];
                if (f == c) memcpy(&out_vertices[(size_t)3 * rank[f]], fhtopo::position(corners, c), 12);
            }
        } else {
            // k_mt_ids, k_mt_used
            std::vector<uint8_t> used((size_t)nv);
            for (uint32_t c = 0; c < C; c++) {
                vid[c] = (uint32_t)triangles[c];
                used[vid[c]] = 1;
            }
            for (uint8_t u : used) counts[3] += u;
            out_vertices.assign(vertices.begin(), vertices.begin() + (size_t)3 * nv);
        }
        // k_mt_edges
        std::vector<uint64_t> edges(fhtopo::EDGE_SLOT_WORDS * slots_e, 0), out_triangles(C);
        std::vector<uint32_t> parent(T);
        std::vector<uint8_t> flat(T);
        for (uint32_t t = 0; t < T && !full; t++) {
            const uint32_t v[3] = {vid[3 * t], vid[3 * t + 1], vid[3 * t + 2]};
            for (uint32_t k = 0; k < 3; k++) out_triangles[(size_t)3 * t + k] = v[k];
            parent[t] = t;
            flat[t] = fhtopo::degenerate(v[0], v[1], v[2]);
            counts[2] += flat[t];
            for (uint32_t k = 0; k < 3 && !flat[t] && !full; k++) {
                uint64_t slot = 0;
                full = !fhtopo::edge_insert<Serial>(edges.data(), log2_e, v[k], v[(k + 1) % 3], 3 * t + k, slot);
                corner_slot[3 * t + k] = (uint32_t)slot;
            }
        }
        if (full) { printf("O edge\n"); return 0; }
        // k_mt_link
        std::vector<uint8_t> corner_class(C);
        for (uint32_t t = 0; t < T; t++) {
            for (uint32_t k = 0; k < 3 && !flat[t]; k++) {
                const uint32_t c = 3 * t + k, s = corner_slot[c], f = fhtopo::edge_first(edges.data(), s);
                if (f == c) {
                    const uint32_t cls = fhtopo::edge_class(fhtopo::edge_counts(edges.data(), s));
                    corner_class[c] = (uint8_t)(fhtopo::FIRST_USE | cls);
                    counts[4]++;
                    for (uint32_t kind = 0; kind < fhtopo::N_KINDS; kind++) counts[5 + kind] += (cls >> kind) & 1u;
                } else {
                    const uint32_t a = find(parent, t), b = find(parent, f / 3);
                    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
                }
            }
        }
        // k_cc_flatten, k_mt_roots, the prefix sums, k_mt_number
        std::vector<uint32_t> rank((size_t)T + 1), shell(T);
        for (uint32_t t = 0; t < T; t++) rank[(size_t)t + 1] = rank[t] + (parent[t] == t && !flat[t] ? 1u : 0u);
        const uint32_t S = rank[T];
        counts[9] = S;
        std::vector<uint32_t> shell_first(S);
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t root = find(parent, t);
            shell[t] = flat[t] ? fhtopo::EMPTY : rank[root];
            if (!flat[t] && root == t) shell_first[rank[root]] = t;
        }
        // k_mt_table
        std::vector<uint64_t> shell_triangles(S), shell_unbalanced(S), vol_terms(T), area_terms(T);
        std::vector<uint32_t> lo((size_t)3 * S, 0xFFFFFFFFu), hi((size_t)3 * S, 0);
        std::vector<double> volume6(S), area2(S);
        for (uint32_t t = 0; t < T; t++) {
            const float* p[3];
            for (uint32_t k = 0; k < 3; k++) p[k] = &out_vertices[(size_t)(3 * out_triangles[(size_t)3 * t + k])];
            const double v6 = fhtopo::volume6_term(p[0], p[1], p[2]), a2 = fhtopo::area2_term(p[0], p[1], p[2]);
            vol_terms[t] = bits64(v6); area_terms[t] = bits64(a2);
            const uint32_t s = shell[t];
            if (s == fhtopo::EMPTY) continue;
            shell_triangles[s]++;
            volume6[s] += v6; area2[s] += a2;
            for (uint32_t k = 0; k < 3; k++) {
                shell_unbalanced[s] += (corner_class[3 * t + k] & fhtopo::UNBALANCED) ? 1 : 0;
                for (uint32_t a = 0; a < 3; a++) {
                    const uint32_t o = fhtopo::ordered(fhtopo::canon(p[k][a]));
                    if (o < lo[(size_t)3 * s + a]) lo[(size_t)3 * s + a] = o;
                    if (o > hi[(size_t)3 * s + a]) hi[(size_t)3 * s + a] = o;
                }
            }
        }
        row("C", counts);
        std::vector<uint64_t> out;
        for (float x : out_vertices) out.push_back(fhtopo::float_bits(x));
        row("V", out);
        row("T", out_triangles);
        out.assign(shell.begin(), shell.end());
        row("S", out);
        // k_mt_eflag, the prefix sums, k_mt_eemit
        for (uint32_t kind = 0; kind < fhtopo::N_KINDS; kind++) {
            out.clear();
            for (uint32_t c = 0; c < C; c++) {
                if (!(corner_class[c] & fhtopo::FIRST_USE) || !(corner_class[c] & (1u << kind))) continue;
                const uint64_t key = fhtopo::edge_key((uint32_t)out_triangles[c], (uint32_t)out_triangles[fhtopo::next_corner(c)]);
                out.push_back(key >> 32);
                out.push_back(key & 0xFFFFFFFFull);
            }
            if (out.size() != 2 * counts[5 + kind]) { printf("an edge list of another length than its count\n"); return 1; }
            printf("E %x", kind);
            row("", out);
        }
        out.clear();
        for (uint32_t s = 0; s < S; s++) {
            out.push_back(shell_triangles[s]); out.push_back(shell_first[s]); out.push_back(shell_unbalanced[s]);
            for (uint32_t a = 0; a < 3; a++) out.push_back(fhtopo::unordered(lo[(size_t)3 * s + a]));
            for (uint32_t a = 0; a < 3; a++) out.push_back(fhtopo::unordered(hi[(size_t)3 * s + a]));
            out.push_back(bits64(volume6[s])); out.push_back(bits64(area2[s]));
        }
        row("H", out);
        row("F", vol_terms);
        row("A", area_terms);
    }
    return 0;
}
