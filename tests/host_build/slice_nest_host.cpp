// Host build of the nesting of a mesh's slices (fidget_amd/csrc/mesh_slice_nest.hpp: no HIP, no device) for tests/test_slice_nesting.py.
// Reads the file named by its argument, one case per line, every number hexadecimal (floats and doubles as their bit patterns):
//   Q bands n [2 n xy] [n plane] [n next] [n loop_of] L [L leader] [L plane] [L crossings] [L irregular] [L area2] [2 L lo] [2 L hi] P
// - the arrays of a slices result and its loops' table.  bands = 0: the host's rule.  Runs the passes of slice_nest.hip one item after
// the other, as capi_slice_nest.hpp orders them - the planes' bands from the regular loops' extents and segment counts, the count pass
// with the halving rule, the prefix sums, the fill, the hits counted and written per leader, the parity reduction into a second array,
// the parents and the sums - and prints, every number hexadecimal:
//   O  instead of everything where bands, entries or hits reach 2^32 - 1
//   C  loops regular outer top max_depth improper misoriented planes bands entries hits
//   A  parent per loop;  D  depth;  N  n_children;  R  region_area2 (bits)
//   K  per plane: regular outer top max_depth improper misoriented bands
// The test works the same out with tests/slice_nesting_ref.py and compares.  The arrays are sized exactly, so that a step past them is
// the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_slice_nest.hpp"

static uint64_t bits64(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static double bits_double(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
static void row(const char* tag, const std::vector<uint64_t>& v) {
    printf("%s", tag);
    for (uint64_t x : v) printf(" %" PRIx64, x);
    printf("\n");
}
template <class T> static bool read(std::istream& in, std::vector<T>& v, size_t n) {
    v.resize(n);
    for (T& x : v) { uint64_t b = 0; in >> b; x = (T)b; }
    return (bool)in;
}
static bool read_floats(std::istream& in, std::vector<float>& v, size_t n) {
    v.resize(n);
    for (float& x : v) { uint32_t b = 0; in >> b; x = fhtopo::bits_float(b); }
    return (bool)in;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: slice_nest_host <file of cases>\n"); return 1; }
    std::ifstream file(argv[1]);
    if (!file) { printf("no such file\n"); return 1; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        in >> std::hex;
        char what = 0;
        uint32_t bands = 0;
        uint64_t n64 = 0, L64 = 0, P64 = 0;
        in >> what >> bands >> n64;
        if (!in || what != 'Q' || n64 > (1u << 22)) { printf("bad query\n"); return 1; }
        const uint32_t n = (uint32_t)n64;
        std::vector<float> xy, lo, hi;
        std::vector<uint32_t> plane, next, loop_of, leader, loop_plane, crossings, irregular;
        std::vector<uint64_t> area2_bits;
        if (!read_floats(in, xy, (size_t)2 * n) || !read(in, plane, n) || !read(in, next, n) || !read(in, loop_of, n)) { printf("bad query\n"); return 1; }
        in >> L64;
        if (!in || L64 > (1u << 22)) { printf("bad query\n"); return 1; }
        const uint32_t L = (uint32_t)L64;
        if (!read(in, leader, L) || !read(in, loop_plane, L) || !read(in, crossings, L) || !read(in, irregular, L) || !read(in, area2_bits, L) ||
            !read_floats(in, lo, (size_t)2 * L) || !read_floats(in, hi, (size_t)2 * L)) { printf("bad query\n"); return 1; }
        in >> P64;
        if (!in || P64 > (1u << 22)) { printf("bad query\n"); return 1; }
        const uint32_t P = (uint32_t)P64;
        // ---- the host's part, as capi_slice_nest.hpp has it
        std::vector<uint32_t> flags(L), plane_bands(P, 0);
        std::vector<uint64_t> plane_regular(P, 0);
        std::vector<float> y0(P, 0.0f), y1(P, 0.0f);
        uint64_t n_regular = 0, regular_segments = 0;
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t p = loop_plane[l];
            const bool regular = irregular[l] == 0 && p < P;
            flags[l] = (regular ? 0u : fhsn::IRREGULAR) | (bits_double(area2_bits[l]) > 0 ? fhsn::POSITIVE : 0u);
            if (!regular) continue;
            if (!plane_regular[p] || lo[(size_t)2 * l + 1] < y0[p]) y0[p] = lo[(size_t)2 * l + 1];
            if (!plane_regular[p] || hi[(size_t)2 * l + 1] > y1[p]) y1[p] = hi[(size_t)2 * l + 1];
            plane_regular[p] += crossings[l];
            regular_segments += crossings[l];
            n_regular++;
        }
        std::vector<uint32_t> parent(L, fhsn::NONE), depth(L, fhsn::NONE), n_children(L, 0);
        std::vector<double> region(L, 0.0);
        std::vector<uint64_t> counts((size_t)6 * P, 0);
        uint64_t n_bands = 0, n_entries = 0, n_hits = 0;
        bool overflow = false;
        if (P && n_regular && n) {
            for (uint32_t p = 0; p < P; p++) plane_bands[p] = bands ? bands : fhsn::default_bands(plane_regular[p]);
            std::vector<fhsn::Band> table(P);
            // the regular segment that leaves crossing v, as sn_segment of slice_nest.hip
            const auto segment = [&](uint32_t v, fhsn::Band& B, fhsn::BandRange& r) {
                const uint32_t l = loop_of[v], p = plane[v], w = next[v];
                if (l >= L || p >= P || w >= n || (flags[l] & fhsn::IRREGULAR)) return false;
                B = table[p];
                r = fhsn::segment_bands(xy[(size_t)2 * v + 1], xy[(size_t)2 * w + 1], B);
                return r.hi < B.nb && (uint64_t)B.base + B.nb <= n_bands;
            };
            std::vector<uint32_t> band_count;
            for (;;) {
                n_bands = 0;
                for (uint32_t p = 0; p < P; p++) {
                    table[p] = fhsn::Band{y0[p], fhsn::band_scale(y0[p], y1[p], plane_bands[p]), plane_bands[p], (uint32_t)n_bands};
                    n_bands += plane_bands[p];
                    if (n_bands > fhsn::MAX_ENTRIES) { overflow = true; break; }
                }
                if (overflow) break;
                // k_sn_count
                band_count.assign((size_t)n_bands, 0);
                n_entries = 0;
                for (uint32_t v = 0; v < n; v++) {
                    fhsn::Band B;
                    fhsn::BandRange r;
                    if (!segment(v, B, r)) continue;
                    for (uint32_t b = r.lo; b <= r.hi; b++) band_count[(size_t)B.base + b]++;
                    n_entries += (uint64_t)(r.hi - r.lo) + 1;
                }
                bool halved = false;
                if (!bands && n_entries > (uint64_t)fhsn::ENTRY_MULTIPLE * regular_segments)
                    for (uint32_t& nb : plane_bands)
                        if (nb > 1) { nb /= 2; halved = true; }
                if (!halved) break;
            }
            if (n_entries > fhsn::MAX_ENTRIES) overflow = true;
            if (!overflow) {
                // the prefix sums, k_sn_fill
                std::vector<uint32_t> band_start((size_t)n_bands + 1, 0), cursor, entries((size_t)n_entries);
                for (size_t b = 0; b < n_bands; b++) band_start[b + 1] = band_start[b] + band_count[b];
                cursor.assign(band_start.begin(), band_start.end() - 1);
                for (uint32_t v = 0; v < n; v++) {
                    fhsn::Band B;
                    fhsn::BandRange r;
                    if (!segment(v, B, r)) continue;
                    for (uint32_t b = r.lo; b <= r.hi; b++) entries[cursor[(size_t)B.base + b]++] = v;
                }
                // k_sn_hits, counting and then writing; `visit` hands every hit of leader l to `f`
                const auto visit = [&](uint32_t l, auto&& f) {
                    const uint32_t v0 = leader[l], p = loop_plane[l];
                    if ((flags[l] & fhsn::IRREGULAR) || v0 >= n || p >= P) return;
                    const fhsn::Band B = table[p];
                    const float* const q = &xy[(size_t)2 * v0];
                    const uint64_t b = (uint64_t)B.base + fhsn::band(q[1], B);
                    if (b >= n_bands) return;
                    for (uint32_t e = band_start[(size_t)b]; e < band_start[(size_t)b + 1]; e++) {
                        const uint32_t v = entries[e], w = next[v], m = loop_of[v];
                        if (w >= n || m == l || plane[v] != p) continue;
                        if (fhsn::hit(&xy[(size_t)2 * v], &xy[(size_t)2 * w], q)) f(m);
                    }
                };
                std::vector<uint32_t> hit_base((size_t)L + 1, 0);
                for (uint32_t l = 0; l < L; l++) {
                    uint32_t found = 0;
                    visit(l, [&](uint32_t) { found++; });
                    n_hits += found;
                    hit_base[(size_t)l + 1] = hit_base[l] + found;
                }
                if (n_hits > fhsn::MAX_ENTRIES) overflow = true;
                if (!overflow) {
                    std::vector<uint32_t> hits((size_t)n_hits), contain((size_t)n_hits);
                    for (uint32_t l = 0; l < L; l++) {
                        uint32_t k = hit_base[l];
                        visit(l, [&](uint32_t m) { hits[k++] = m; });
                    }
                    // k_sn_contain
                    for (uint32_t l = 0; l < L; l++) {
                        if (flags[l] & fhsn::IRREGULAR) continue;
                        const uint32_t at = hit_base[l], h = hit_base[(size_t)l + 1] - at;
                        uint32_t kept = 0;
                        for (uint32_t i = 0; i < h; i++)
                            if (fhsn::odd_first(hits.data() + at, h, i)) contain[(size_t)at + kept++] = hits[(size_t)at + i];
                        depth[l] = kept;
                    }
                    // k_sn_parent
                    for (uint32_t l = 0; l < L; l++) {
                        const uint32_t d = depth[l], p = loop_plane[l];
                        if ((flags[l] & fhsn::IRREGULAR) || d == fhsn::NONE || p >= P) continue;
                        const uint32_t up = fhsn::parent_of(contain.data() + hit_base[l], d, depth.data(), L);
                        parent[l] = up;
                        if (up != fhsn::NONE) n_children[up]++;
                        uint64_t* const c = &counts[(size_t)6 * p];
                        c[0]++;
                        if ((d & 1u) == 0) c[1]++;
                        if (up == fhsn::NONE) c[2]++;
                        if (d > c[3]) c[3] = d;
                        if (fhsn::improper(d, up, depth.data())) c[4]++;
                        if (fhsn::misoriented(d, flags[l])) c[5]++;
                    }
                    for (uint32_t l = 0; l < L; l++) region[l] = (flags[l] & fhsn::IRREGULAR) ? 0.0 : bits_double(area2_bits[l]);
                    for (uint32_t l = 0; l < L; l++)
                        if (parent[l] != fhsn::NONE) region[parent[l]] += bits_double(area2_bits[l]);
                }
            }
        } else {
            n_bands = 0;
        }
        if (overflow) { printf("O\n"); continue; }
        uint64_t total[6] = {0, 0, 0, 0, 0, 0};
        std::vector<uint64_t> per_plane;
        for (uint32_t p = 0; p < P; p++) {
            for (uint32_t k = 0; k < 6; k++) {
                const uint64_t c = counts[(size_t)6 * p + k];
                if (k == 3) { if (c > total[3]) total[3] = c; } else total[k] += c;
                per_plane.push_back(c);
            }
            per_plane.push_back(plane_bands[p]);
        }
        row("C", {L, total[0], total[1], total[2], total[3], total[4], total[5], P, n_bands, n_entries, n_hits});
        std::vector<uint64_t> out;
        out.assign(parent.begin(), parent.end()); row("A", out);
        out.assign(depth.begin(), depth.end()); row("D", out);
        out.assign(n_children.begin(), n_children.end()); row("N", out);
        out.clear();
        for (double x : region) out.push_back(bits64(x));
        row("R", out);
        row("K", per_plane);
    }
    return 0;
}
