// Host build of the slicing of a triangle mesh (fidget_amd/csrc/mesh_slice.hpp: no HIP, no device) for tests/test_mesh_slices.py.  Reads
// one query per line of stdin, every number hexadecimal (floats as their bit patterns),
//   Q table_log2 nv [3 nv floats] nt [3 nt indices] np [np floats]
// table_log2 = 0: the library's choice.  Walks the mesh the way the kernels of slice.hip do, one item after the other - the levels, the
// counts, the crossing edges through fhtopo::edge_insert, the counts at the first corners and their prefix sums, the crossings by
// fhslice::owner over those sums, the segments likewise, a union-find towards the smaller root, the loops' table - with the plain memory
// operations of fhtopo::Serial, and prints, every number hexadecimal:
//   U  instead of everything when the planes are not finite and strictly ascending
//   O  instead of everything when the table had no room
//   C  planes crossings segments loops irregular edge-slots
//   X  the positions' bits, x y x y ..;  P  a plane per crossing;  E  an edge per crossing, u v u v ..;  N  next;  L  loop_of;  D  degree
//   G  the segments, from to from to ..
//   H  per loop: leader plane crossings segments irregular area2 lo[2] hi[2] (floats and the double as bits; area2 summed in segment order)
//   K  per plane: crossings segments loops
// The test works the same out with tests/mesh_slices_ref.py and compares.  The arrays are sized exactly, so that a step past them is the
// sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_slice.hpp"

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
        uint32_t table_log2 = 0;
        uint64_t nv = 0, nt = 0, np = 0;
        in >> what >> table_log2 >> nv;
        if (!in || what != 'Q' || table_log2 > 24 || nv > (1u << 20)) { printf("bad query\n"); return 1; }
        std::vector<float> vertices((size_t)3 * nv);
        for (float& x : vertices) { uint32_t b = 0; in >> b; x = fhtopo::bits_float(b); }
        in >> nt;
        if (!in || nt > (1u << 20)) { printf("bad query\n"); return 1; }
        std::vector<uint64_t> triangles((size_t)3 * nt);
        for (uint64_t& x : triangles) { in >> x; if (x >= nv) { printf("bad query\n"); return 1; } }
        in >> np;
        if (!in || np > (1u << 20)) { printf("bad query\n"); return 1; }
        std::vector<float> zs((size_t)np);
        for (float& x : zs) { uint32_t b = 0; in >> b; x = fhtopo::bits_float(b); }
        if (!in) { printf("bad query\n"); return 1; }
        const uint32_t T = (uint32_t)nt, C = 3 * T, P = (uint32_t)np;
        if (!fhslice::planes_ok(zs.data(), P)) { printf("U\n"); continue; }
        // k_ms_levels
        std::vector<uint32_t> level((size_t)nv);
        for (size_t v = 0; v < nv; v++) level[v] = fhslice::level(zs.data(), P, vertices[3 * v + 2]);
        // k_ms_count
        std::vector<uint32_t> seg_count((size_t)T + 1), seg_base((size_t)T + 1);
        uint64_t crossing_corners = 0, n_segments = 0;
        const auto corners_of = [&](uint32_t t, uint32_t v[3], uint32_t a[3]) {
            for (uint32_t k = 0; k < 3; k++) { v[k] = (uint32_t)triangles[(size_t)3 * t + k]; a[k] = level[v[k]]; }
            return !fhtopo::degenerate(v[0], v[1], v[2]);
        };
        for (uint32_t t = 0; t < T; t++) {
            uint32_t v[3], a[3];
            if (!corners_of(t, v, a)) continue;
            for (uint32_t k = 0; k < 3; k++) crossing_corners += a[k] != a[(k + 1) % 3];
            seg_count[t] = fhslice::n_planes(fhslice::triangle_range(a));
            n_segments += seg_count[t];
        }
        // k_ms_insert
        const uint32_t log2 = table_log2 ? table_log2 : fhslice::default_log2(crossing_corners);
        const size_t slots = (size_t)fhtopo::n_slots(log2);
        std::vector<uint64_t> table(fhtopo::EDGE_SLOT_WORDS * slots, 0);
        std::vector<uint32_t> corner_slot((size_t)C, fhslice::NONE);
        bool full = false;
        for (uint32_t t = 0; t < T && !full; t++) {
            uint32_t v[3], a[3];
            if (!corners_of(t, v, a)) continue;
            for (uint32_t k = 0; k < 3 && !full; k++)
                full = !fhslice::corner_insert<Serial>(table.data(), log2, v[k], v[(k + 1) % 3], a[k], a[(k + 1) % 3], 3 * t + k, corner_slot[(size_t)3 * t + k]);
        }
        if (full) { printf("O\n"); continue; }
        // k_ms_first, the prefix sums, k_ms_ids
        std::vector<uint32_t> count((size_t)C + 1), base((size_t)C + 1);
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t s = corner_slot[c];
            if (s == fhslice::NONE || fhtopo::edge_first(table.data(), s) != c) continue;
            const uint64_t key = fhslice::edge_key_at(table.data(), s);
            count[c] = fhslice::n_planes(fhslice::edge_range(level[(size_t)(key >> 32)], level[(size_t)(key & 0xFFFFFFFFu)]));
        }
        for (uint32_t c = 0; c < C; c++) base[(size_t)c + 1] = base[c] + count[c];
        for (uint32_t t = 0; t < T; t++) seg_base[(size_t)t + 1] = seg_base[t] + seg_count[t];
        const uint32_t n = base[C], m = seg_base[T];
        if (m != n_segments) { printf("the segments' sum is not their count\n"); return 1; }
        std::vector<uint32_t> corner_base((size_t)C, fhslice::NONE);
        for (uint32_t c = 0; c < C; c++)
            if (corner_slot[c] != fhslice::NONE) corner_base[c] = base[fhtopo::edge_first(table.data(), corner_slot[c])];
        // k_ms_emit
        std::vector<float> xy((size_t)2 * n);
        std::vector<uint32_t> plane(n), edge((size_t)2 * n);
        for (uint32_t x = 0; x < n; x++) {
            const uint32_t c = (uint32_t)fhslice::owner(base.data(), C, x);
            const uint64_t key = fhtopo::edge_key((uint32_t)triangles[c], (uint32_t)triangles[fhtopo::next_corner(c)]);
            const uint32_t u = (uint32_t)(key >> 32), v = (uint32_t)key;
            const fhslice::Range r = fhslice::edge_range(level[u], level[v]);
            const uint32_t p = r.lo + (x - base[c]);
            if (p >= r.hi) { printf("a crossing beyond its edge's planes\n"); return 1; }
            plane[x] = p; edge[(size_t)2 * x] = u; edge[(size_t)2 * x + 1] = v;
            fhslice::position(&vertices[(size_t)3 * u], &vertices[(size_t)3 * v], zs[p], &xy[(size_t)2 * x]);
        }
        // k_ms_segments
        std::vector<uint32_t> seg((size_t)2 * m), parent(n);
        std::vector<uint64_t> next_words(n, 0), degree(n, 0);
        for (uint32_t x = 0; x < n; x++) parent[x] = x;
        for (uint32_t s = 0; s < m; s++) {
            const uint32_t t = (uint32_t)fhslice::owner(seg_base.data(), T, s);
            uint32_t v[3], a[3], id[2];
            corners_of(t, v, a);
            const uint32_t p = fhslice::triangle_range(a).lo + (s - seg_base[t]);
            const fhslice::SegmentEdges e = fhslice::segment_edges(a, p);
            const uint32_t k[2] = {e.from, e.to};
            for (uint32_t q = 0; q < 2; q++) {
                const fhslice::Range r = fhslice::edge_range(a[k[q]], a[(k[q] + 1) % 3]);
                if (p < r.lo || p >= r.hi || corner_base[(size_t)3 * t + k[q]] == fhslice::NONE) { printf("a segment on an edge that does not cross its plane\n"); return 1; }
                id[q] = fhslice::crossing_id(corner_base[(size_t)3 * t + k[q]], r, p);
            }
            seg[(size_t)2 * s] = id[0]; seg[(size_t)2 * s + 1] = id[1];
            Serial::add64(&degree[id[0]], 1);
            Serial::add64(&degree[id[1]], (uint64_t)1 << 32);
            Serial::max64(&next_words[id[0]], fhslice::next_word(t, id[1]));
            const uint32_t ra = find(parent, id[0]), rb = find(parent, id[1]);
            if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;
        }
        // k_cc_flatten, k_cc_roots, the prefix sums, k_cc_number
        std::vector<uint32_t> rank((size_t)n + 1), loop_of(n);
        for (uint32_t x = 0; x < n; x++) rank[(size_t)x + 1] = rank[x] + (parent[x] == x ? 1u : 0u);
        const uint32_t L = rank[n];
        for (uint32_t x = 0; x < n; x++) loop_of[x] = rank[find(parent, x)];
        // k_ms_measure_x, k_ms_measure_s
        std::vector<uint32_t> leader(L), loop_plane(L), loop_n(L), loop_m(L), loop_irregular(L), lo((size_t)2 * L, 0xFFFFFFFFu), hi((size_t)2 * L, 0), next(n);
        std::vector<uint8_t> degree_byte(n);
        std::vector<double> area2(L);
        uint64_t n_irregular = 0;
        for (uint32_t x = 0; x < n; x++) {
            const uint32_t l = loop_of[x];
            next[x] = fhslice::next_of(next_words[x]);
            degree_byte[x] = fhslice::degree_byte(degree[x]);
            loop_n[l]++;
            if (fhslice::irregular(degree[x])) { loop_irregular[l]++; n_irregular++; }
            if (parent[x] == x) { leader[l] = x; loop_plane[l] = plane[x]; }
            for (uint32_t q = 0; q < 2; q++) {
                const uint32_t o = fhtopo::ordered(fhtopo::canon(xy[(size_t)2 * x + q]));
                if (o < lo[(size_t)2 * l + q]) lo[(size_t)2 * l + q] = o;
                if (o > hi[(size_t)2 * l + q]) hi[(size_t)2 * l + q] = o;
            }
        }
        for (uint32_t s = 0; s < m; s++) {
            const uint32_t l = loop_of[seg[(size_t)2 * s]];
            loop_m[l]++;
            area2[l] += fhslice::area2_term(&xy[(size_t)2 * seg[(size_t)2 * s]], &xy[(size_t)2 * seg[(size_t)2 * s + 1]]);
        }
        std::vector<uint64_t> per_plane((size_t)3 * P);
        for (uint32_t l = 0; l < L; l++) {
            per_plane[(size_t)3 * loop_plane[l]] += loop_n[l]; per_plane[(size_t)3 * loop_plane[l] + 1] += loop_m[l]; per_plane[(size_t)3 * loop_plane[l] + 2]++;
        }
        row("C", {P, n, m, L, n_irregular, slots});
        std::vector<uint64_t> out;
        for (float x : xy) out.push_back(fhtopo::float_bits(x));
        row("X", out);
        out.assign(plane.begin(), plane.end()); row("P", out);
        out.assign(edge.begin(), edge.end()); row("E", out);
        out.assign(next.begin(), next.end()); row("N", out);
        out.assign(loop_of.begin(), loop_of.end()); row("L", out);
        out.assign(degree_byte.begin(), degree_byte.end()); row("D", out);
        out.assign(seg.begin(), seg.end()); row("G", out);
        out.clear();
        for (uint32_t l = 0; l < L; l++) {
            out.push_back(leader[l]); out.push_back(loop_plane[l]); out.push_back(loop_n[l]); out.push_back(loop_m[l]); out.push_back(loop_irregular[l]);
            out.push_back(bits64(area2[l]));
            for (uint32_t q = 0; q < 2; q++) out.push_back(fhtopo::unordered(lo[(size_t)2 * l + q]));
            for (uint32_t q = 0; q < 2; q++) out.push_back(fhtopo::unordered(hi[(size_t)2 * l + q]));
        }
        row("H", out);
        row("K", per_plane);
    }
    return 0;
}
