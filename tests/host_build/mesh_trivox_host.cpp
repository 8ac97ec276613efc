// Host build of the arithmetic of the solid voxelization of a triangle mesh (fidget_amd/csrc/mesh_trivox.hpp: no HIP, no device) for
// tests/test_mesh_voxels.py.  Reads one query per line of stdin, every number hexadecimal (floats and doubles as their bit patterns),
//   Q depth m [12 doubles] nv [3 nv floats] indexed nt [3 nt indices, if indexed] G
//   Q depth m [12 doubles] nv [3 nv floats] indexed nt [3 nt indices, if indexed] C nc [j k] x nc
// m = 1: a mesh_to_world matrix follows.  Walks the mesh the way the kernels of trivox.hip do - a record per triangle from the snap and
// the set-up, the items of work numbered through the triangles' boxes, a toggle per covered column into the bricks' words or the exit
// plane, the fill along every row of bricks with the parity handed from word to word - and prints, every number hexadecimal:
//   G:  I  the eight numbers of `info`;  B  the B^3 words of the bitmap
//   C:  per triangle  T kind j0 k0 nj nk  and  C  one number per column asked for: 0 not covered, 1 the exit plane, i + 2 voxel i
// The test works the same out with tests/mesh_voxels_ref.py and compares.  The arrays are sized exactly, so that a step past them is
// the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_trivox.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> std::hex;
        char what = 0, mode = 0;
        uint32_t depth = 0, has_m = 0, indexed = 0;
        uint64_t nv = 0, nt = 0;
        double m[12];
        in >> what >> depth >> has_m;
        if (!in || what != 'Q' || depth > fhvox::MAX_DEPTH || has_m > 1) { printf("bad query\n"); return 1; }
        if (has_m)
            for (double& x : m) { uint64_t bits = 0; in >> bits; memcpy(&x, &bits, 8); }
        in >> nv;
        if (!in || nv > (1u << 20)) { printf("bad query\n"); return 1; }
        std::vector<float> vertices((size_t)3 * nv);
        for (float& x : vertices) { uint32_t bits = 0; in >> bits; memcpy(&x, &bits, 4); }
        in >> indexed >> nt;
        if (!in || nt > (1u << 20)) { printf("bad query\n"); return 1; }
        std::vector<uint64_t> triangles(indexed ? (size_t)3 * nt : 0);
        for (uint64_t& x : triangles) in >> x;
        in >> mode;
        if (!in || (mode != 'G' && mode != 'C') || (mode == 'G' && depth > 3)) { printf("bad query\n"); return 1; }
        const uint32_t N = 4u << depth, B = 1u << depth;

        // k_tv_setup
        std::vector<fhtv::Tri> records((size_t)nt);
        std::vector<uint32_t> kinds((size_t)nt);
        std::vector<uint64_t> prefix((size_t)nt + 1);
        uint64_t info[8] = {nt, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t t = 0; t < nt; t++) {
            int32_t q[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            bool ok = true;
            for (uint32_t c = 0; c < 3; c++) {
                const uint64_t at = indexed ? triangles[(size_t)(3 * t + c)] : 3 * t + c;
                if (at >= nv) { ok = false; continue; }
                ok = fhtv::snap_vertex(&vertices[(size_t)(3 * at)], has_m ? m : nullptr, depth, q[c]) && ok;
            }
            const int32_t zero[3] = {0, 0, 0};
            kinds[(size_t)t] = ok ? fhtv::setup(q[0], q[1], q[2], depth, records[(size_t)t]) : fhtv::TV_REJECTED;
            if (!ok) (void)fhtv::setup(zero, zero, zero, depth, records[(size_t)t]);
            info[1] += kinds[(size_t)t] == fhtv::TV_REJECTED;
            info[2] += kinds[(size_t)t] == fhtv::TV_FLAT;
            prefix[(size_t)t + 1] = prefix[(size_t)t] + fhtv::n_columns(records[(size_t)t]);
        }
        if (mode == 'C') {
            uint32_t nc = 0;
            in >> nc;
            std::vector<uint32_t> cols((size_t)2 * nc);
            for (uint32_t& x : cols) in >> x;
            if (!in) { printf("bad query\n"); return 1; }
            for (uint64_t t = 0; t < nt; t++) {
                const fhtv::Tri& T = records[(size_t)t];
                printf("T %x %x %x %x %x\n", kinds[(size_t)t], (unsigned)T.j0, (unsigned)T.k0, (unsigned)T.nj, (unsigned)T.nk);
                printf("C");
                for (uint32_t c = 0; c < nc; c++) {
                    int64_t i = 0;
                    // (the kernel asks only inside the box; the test may ask anywhere on the grid: the edge tests decide alone)
                    const bool covered = kinds[(size_t)t] == fhtv::TV_OK && cols[2 * c] < N && cols[2 * c + 1] < N && fhtv::cover_cross(T, depth, cols[2 * c], cols[2 * c + 1], i);
                    printf(" %" PRIx64, !covered ? (uint64_t)0 : (i == fhtv::TV_EXIT ? (uint64_t)1 : (uint64_t)i + 2));
                }
                printf("\n");
            }
            continue;
        }
        // k_tv_cross: item w of the W = prefix[nt] is column `local` of its triangle's box
        std::vector<uint64_t> bricks((size_t)fhvox::n_words(depth)), exit_plane((size_t)fhtv::exit_words(depth));
        info[7] = prefix[(size_t)nt];
        uint64_t t = 0;
        for (uint64_t w = 0; w < prefix[(size_t)nt]; w++) {
            while (w >= prefix[(size_t)t + 1]) t++;
            const fhtv::Tri& T = records[(size_t)t];
            const uint32_t local = (uint32_t)(w - prefix[(size_t)t]);
            const uint32_t j = T.j0 + local % T.nj, k = T.k0 + local / T.nj;
            int64_t i = 0;
            if (!fhtv::cover_cross(T, depth, j, k, i)) continue;
            info[3]++;
            if (i == fhtv::TV_EXIT) {
                info[4]++;
                const uint64_t at = fhtv::exit_index(depth, j, k);
                exit_plane[(size_t)(at >> 6)] ^= (uint64_t)1 << (at & 63);
            } else {
                if (i < 0 || i >= (int64_t)N) { printf("a crossing beyond the grid\n"); return 1; }
                bricks[(size_t)fhtv::voxel_word(depth, (uint32_t)i, j, k)] ^= fhtv::voxel_bit((uint32_t)i, j, k);
            }
        }
        // k_tv_fill: every row of bricks, the parity of the words before handed on
        for (uint32_t row = 0; row < B * B; row++) {
            uint64_t carry = 0, last = 0;
            for (uint32_t bx = 0; bx < B; bx++) {
                uint64_t& word = bricks[((size_t)row << depth) + bx];
                const uint64_t filled = fhtv::fill_word(word);
                if (fhtv::fill_carry(filled) & ~fhvm::X0) { printf("a parity beyond the X0 positions\n"); return 1; }
                word = last = fhtv::fill_apply(filled, carry);
                carry ^= fhtv::fill_carry(filled);
                info[6] += (uint64_t)__builtin_popcountll(word);
            }
            info[5] += (uint64_t)__builtin_popcountll(fhtv::open_ends(last, exit_plane.data(), depth, row & (B - 1), row >> depth));
        }
        printf("I");
        for (uint64_t x : info) printf(" %" PRIx64, x);
        printf("\nB");
        for (uint64_t x : bricks) printf(" %" PRIx64, x);
        printf("\n");
    }
    return 0;
}
