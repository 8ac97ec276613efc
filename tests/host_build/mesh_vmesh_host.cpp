// Host build of the bit arithmetic of the boundary mesh of a voxel bitmap (fidget_amd/csrc/mesh_vmesh.hpp: no HIP, no device) for
// tests/test_voxel_mesh.py.  Reads one bitmap per line of stdin,
//   G depth w0 w1 ...         B^3 hexadecimal words, B = 1 << depth, word (bz B + by) B + bx
// walks it the way the kernels of vmesh.hip do - a brick's word and six neighbours, a corner brick's eight words, zeros beyond the grid -
// and prints five lines, every number hexadecimal:
//   S f0 .. f5 V E F n        the surface summary
//   M ...                     per brick its six exposed-face masks
//   C ...                     per corner brick, (B + 1)^3 of them: used corners, used edges along x, y, z
//   V ...                     per vertex the bit patterns of its three f32 coordinates
//   T ...                     per triangle its three vertex ids
// The test works the same out with tests/voxel_mesh_ref.py and compares.  The arrays are sized exactly, so that a step past them is
// the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_vmesh.hpp"

struct Grid {
    uint32_t depth, B;
    std::vector<uint64_t> words;
    // the brick's word, 0 beyond the grid (coordinates may be -1 or B)
    uint64_t at(int64_t bx, int64_t by, int64_t bz) const {
        if (bx < 0 || by < 0 || bz < 0 || bx >= (int64_t)B || by >= (int64_t)B || bz >= (int64_t)B) return 0;
        return words[fhvox::word_index(depth, (uint32_t)bx, (uint32_t)by, (uint32_t)bz)];
    }
};

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
        Grid G;
        in >> what >> G.depth;
        if (!in || what != 'G' || G.depth > 3) { printf("bad query\n"); return 1; }
        G.B = 1u << G.depth;
        G.words.resize((size_t)fhvox::n_words(G.depth));
        for (auto& w : G.words) in >> std::hex >> w;
        if (!in) { printf("bad query\n"); return 1; }
        const uint32_t B = G.B, N = 4 * B, S = fhvm::corner_side(G.depth);
        const size_t n_corner_bricks = (size_t)fhvm::n_corner_bricks(G.depth);

        // the counting pass: masks, counts, the summary
        std::vector<uint64_t> masks(6 * G.words.size()), corners(4 * n_corner_bricks), sum(10, 0);
        std::vector<uint32_t> face_base(G.words.size() + 1, 0), vert_base(n_corner_bricks + 1, 0);
        for (uint32_t bz = 0; bz < B; bz++)
            for (uint32_t by = 0; by < B; by++)
                for (uint32_t bx = 0; bx < B; bx++) {
                    const size_t w = (size_t)fhvox::word_index(G.depth, bx, by, bz);
                    const uint64_t nb[6] = {G.at((int64_t)bx - 1, by, bz), G.at((int64_t)bx + 1, by, bz), G.at(bx, (int64_t)by - 1, bz),
                                            G.at(bx, (int64_t)by + 1, bz), G.at(bx, by, (int64_t)bz - 1), G.at(bx, by, (int64_t)bz + 1)};
                    uint64_t m[6] = {0, 0, 0, 0, 0, 0};
                    fhvm::face_masks(G.words[w], nb, m);
                    uint32_t n_faces = 0;
                    for (uint32_t d = 0; d < 6; d++) {
                        masks[6 * w + d] = m[d];
                        sum[d] += fhvm::popcount64(m[d]);
                        n_faces += fhvm::popcount64(m[d]);
                    }
                    if (fhvm::faces_none(G.words[w], nb) && n_faces != 0) { printf("faces_none is wrong\n"); return 1; }
                    face_base[w + 1] = n_faces;
                    sum[9] += fhvm::popcount64(G.words[w]);
                }
        for (uint32_t cz = 0; cz < S; cz++)
            for (uint32_t cy = 0; cy < S; cy++)
                for (uint32_t cx = 0; cx < S; cx++) {
                    const size_t t = ((size_t)cz * S + cy) * S + cx;
                    uint64_t W[8];
                    for (uint32_t q = 0; q < 8; q++) W[q] = G.at((int64_t)cx - (q & 1), (int64_t)cy - ((q >> 1) & 1), (int64_t)cz - (q >> 2));
                    uint64_t used = 0, edges[3] = {0, 0, 0};
                    fhvm::corner_masks(W, used, edges);
                    if (fhvm::corners_none(W) && (used | edges[0] | edges[1] | edges[2]) != 0) { printf("corners_none is wrong\n"); return 1; }
                    corners[4 * t] = used;
                    for (uint32_t a = 0; a < 3; a++) { corners[4 * t + 1 + a] = edges[a]; sum[7] += fhvm::popcount64(edges[a]); }
                    sum[6] += fhvm::popcount64(used);
                    vert_base[t + 1] = fhvm::popcount64(used);
                }
        for (size_t w = 0; w < G.words.size(); w++) face_base[w + 1] += face_base[w];
        for (size_t t = 0; t < n_corner_bricks; t++) vert_base[t + 1] += vert_base[t];
        sum[8] = sum[0] + sum[1] + sum[2] + sum[3] + sum[4] + sum[5];

        // the vertices: per corner brick, one per flagged bit
        std::vector<uint64_t> verts(3 * (size_t)sum[6]), tris(6 * (size_t)sum[8]);
        for (size_t t = 0; t < n_corner_bricks; t++) {
            const uint64_t used = corners[4 * t];
            const uint32_t cx = (uint32_t)(t % S), cy = (uint32_t)(t / S % S), cz = (uint32_t)(t / S / S);
            for (uint32_t r = 0; r < fhvm::popcount64(used); r++) {
                const uint32_t bit = fhvm::select_bit(used, r);
                const uint32_t c[3] = {4 * cx + (bit & 3), 4 * cy + ((bit >> 2) & 3), 4 * cz + (bit >> 4)};
                if (fhvm::corner_brick(G.depth, c[0], c[1], c[2]) != t || fhvm::corner_bit(c[0], c[1], c[2]) != bit || fhvm::rank_below(used, bit) != r) {
                    printf("the corner numbering is wrong\n");
                    return 1;
                }
                for (uint32_t a = 0; a < 3; a++) {
                    const float x = fhvm::corner_coord(c[a], N);
                    uint32_t bits;
                    memcpy(&bits, &x, 4);
                    verts[3 * ((size_t)vert_base[t] + r) + a] = bits;
                }
            }
        }
        // the faces: per brick, per direction, per exposed bit
        for (size_t w = 0; w < G.words.size(); w++) {
            const uint32_t bx = (uint32_t)(w % B), by = (uint32_t)(w / B % B), bz = (uint32_t)(w / B / B);
            size_t f = face_base[w];
            for (uint32_t d = 0; d < 6; d++) {
                const uint64_t m = masks[6 * w + d];
                for (uint32_t r = 0; r < fhvm::popcount64(m); r++, f++) {
                    const uint32_t bit = fhvm::select_bit(m, r);
                    uint32_t c[4][3];
                    fhvm::face_corners(4 * bx + (bit & 3), 4 * by + ((bit >> 2) & 3), 4 * bz + (bit >> 4), d, c);
                    uint64_t id[4];
                    for (uint32_t q = 0; q < 4; q++) {
                        const uint32_t t = fhvm::corner_brick(G.depth, c[q][0], c[q][1], c[q][2]);
                        id[q] = (uint64_t)vert_base[t] + fhvm::rank_below(corners[4 * (size_t)t], fhvm::corner_bit(c[q][0], c[q][1], c[q][2]));
                    }
                    const uint64_t six[6] = {id[0], id[1], id[2], id[0], id[2], id[3]};
                    for (uint32_t q = 0; q < 6; q++) tris[6 * f + q] = six[q];
                }
            }
        }
        print_line('S', sum);
        print_line('M', masks);
        print_line('C', corners);
        print_line('V', verts);
        print_line('T', tris);
    }
    return 0;
}
