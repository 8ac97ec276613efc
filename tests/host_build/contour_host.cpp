// Host build of the contouring arithmetic (fidget_amd/csrc/contour/contour.hpp: no HIP, no device) for tests/test_contours.py.  It runs
// the passes of the k_ctr_* kernels of mesh.hip as plain loops over the same header functions - the ballot words and block counts of the
// edge pass, their prefix sums, the vertices, the cells' counts and prefix sums, the segments with next[from] = to, the loops - and writes
// what they give to a file; the test compares it with the numpy model.
//   contour_host IMAGE OUT      IMAGE: u32 W, u32 H, W * H f32.
//                               OUT: u64 n_vertices, u64 n_segments, u64 n_loops, 2 n_v f32, 2 n_s u32, n_v u32 (next), n_v u32 (order),
//                               (n_loops + 1) u64 (loop_start), n_loops u8 (closed)
//   contour_host --loops NEXT OUT   NEXT: u64 n, n u32.  OUT: u64 ok, u64 n_loops, n u32 (order), (n_loops + 1) u64, n_loops u8
#include <stdio.h>
#include <string.h>

#include <vector>

#include "contour/contour.hpp"

using namespace fhctr;

template <class T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }
static bool put64(FILE* f, uint64_t v) { return fwrite(&v, 8, 1, f) == 1; }

static int run_loops(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1) { fclose(f); return 2; }
    std::vector<uint32_t> next(n);
    if (n && fread(next.data(), 4, n, f) != n) { fclose(f); return 2; }
    fclose(f);
    std::vector<uint32_t> order(n);
    std::vector<uint64_t> start(n + 1);
    std::vector<uint8_t> closed(n);
    uint64_t n_loops = 0;
    const bool ok = follow_loops(next.data(), n, order.data(), start.data(), closed.data(), &n_loops);
    if (!ok) n_loops = 0;
    start.resize(n_loops + 1);
    closed.resize(n_loops);
    FILE* o = fopen(out, "wb");
    if (!o) return 3;
    const bool w = put64(o, ok ? 1 : 0) && put64(o, n_loops) && put(o, order) && put(o, start) && put(o, closed);
    return fclose(o) == 0 && w ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--loops")) return run_loops(argv[2], argv[3]);
    if (argc != 3) { fprintf(stderr, "usage: contour_host IMAGE OUT | --loops NEXT OUT\n"); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t wh[2] = {0, 0};
    if (fread(wh, 4, 2, f) != 2) { fclose(f); return 2; }
    const uint32_t W = wh[0], H = wh[1];
    if (!size_ok(W, H)) { fclose(f); return 4; }
    std::vector<float> img((size_t)W * H);
    if (!img.empty() && fread(img.data(), 4, img.size(), f) != img.size()) { fclose(f); return 2; }
    fclose(f);

    // k_ctr_edges: one bit per edge, one count per block
    const uint64_t E = n_edges(W, H), NC = n_cells(W, H);
    const uint32_t eb = (uint32_t)((E + EDGE_BLOCK - 1) / EDGE_BLOCK), cb = (uint32_t)((NC + EDGE_BLOCK - 1) / EDGE_BLOCK);
    std::vector<uint64_t> bits((size_t)eb * 4, 0);
    std::vector<uint32_t> e_off(eb + 1, 0), c_off(cb + 1, 0);
    for (uint64_t e = 0; e < E; e++) {
        const Edge ed = edge_at((uint32_t)e, W, H);
        if (inside(img[edge_pixel0(ed, W)]) != inside(img[edge_pixel1(ed, W)])) { bits[e >> 6] |= (uint64_t)1 << (e & 63); e_off[e / EDGE_BLOCK + 1]++; }
    }
    for (uint32_t b = 0; b < eb; b++) e_off[b + 1] += e_off[b];       // the scan
    const uint32_t nv = e_off[eb];
    // k_ctr_vertices
    std::vector<float> verts((size_t)nv * 2);
    std::vector<uint32_t> next(nv, 0);
    for (uint64_t e = 0; e < E; e++) {
        if (!edge_crosses(bits.data(), (uint32_t)e)) continue;
        const Edge ed = edge_at((uint32_t)e, W, H);
        const uint32_t id = vertex_id(bits.data(), e_off.data(), (uint32_t)e);
        if (id >= nv) return 5;
        edge_vertex(ed, img[edge_pixel0(ed, W)], img[edge_pixel1(ed, W)], &verts[(size_t)id * 2]);
        next[id] = NONE;
    }
    // k_ctr_cells, the scan, k_ctr_segments
    auto cell = [&](uint64_t c, uint32_t& i, uint32_t& j) {
        j = (uint32_t)c / (W - 1); i = (uint32_t)c - j * (W - 1);
        const float* p = &img[(size_t)j * W + i];
        return cell_case(cell_mask(p[0], p[1], p[W + 1], p[W]), saddle_centre_inside(p[0], p[1], p[W + 1], p[W]));
    };
    for (uint64_t c = 0; c < NC; c++) { uint32_t i, j; c_off[c / EDGE_BLOCK + 1] += case_count(cell(c, i, j)); }
    for (uint32_t b = 0; b < cb; b++) c_off[b + 1] += c_off[b];
    const uint32_t ns = c_off[cb];
    std::vector<uint32_t> segs((size_t)ns * 2);
    uint32_t at = 0;
    for (uint64_t c = 0; c < NC; c++) {
        if (c % EDGE_BLOCK == 0) { if (at != c_off[c / EDGE_BLOCK]) return 6; }
        uint32_t i, j;
        const uint32_t cs = cell(c, i, j);
        for (uint32_t s = 0; s < case_count(cs); s++, at++) {
            const uint32_t ef = cell_edge(case_from(cs, s), i, j, W, H), et = cell_edge(case_to(cs, s), i, j, W, H);
            if (!edge_crosses(bits.data(), ef) || !edge_crosses(bits.data(), et) || at >= ns) return 7;
            const uint32_t from = vertex_id(bits.data(), e_off.data(), ef), to = vertex_id(bits.data(), e_off.data(), et);
            if (next[from] != NONE) return 8;         // one writer per word
            segs[(size_t)at * 2] = from; segs[(size_t)at * 2 + 1] = to;
            next[from] = to;
        }
    }
    if (at != ns) return 6;
    std::vector<uint32_t> order(nv);
    std::vector<uint64_t> start((size_t)nv + 1);
    std::vector<uint8_t> closed(nv);
    uint64_t n_loops = 0;
    if (!follow_loops(next.data(), nv, order.data(), start.data(), closed.data(), &n_loops)) return 9;
    start.resize(n_loops + 1);
    closed.resize(n_loops);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 3;
    const bool w = put64(o, nv) && put64(o, ns) && put64(o, n_loops) && put(o, verts) && put(o, segs) && put(o, next) && put(o, order) && put(o, start) && put(o, closed);
    return fclose(o) == 0 && w ? 0 : 3;
}
