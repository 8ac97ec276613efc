// Host build of the arithmetic of the local thickness (fidget_amd/csrc/mesh_thick.hpp: no HIP, no device) for tests/test_thickness.py.
// One query per line of stdin, one line of answers each; the test works the same out with tests/thickness_ref.py and compares.
//   Q lo hi             ->  pairs "x w": fhlt::isqrt(x) = w at x = lo and at every x in (lo, hi] where it differs from isqrt(x - 1)
//   W f r               ->  (2 r + 1)^2 values, dz outermost then dy, both -r .. r: fhlt::row_half of the ball f at that row, -1 where absent
//   N v                 ->  need(v, class 1), need(v, class 2), need(v, class 3) from fhlt::need_tables_host(v)
//   T n prune f0 f1 ... ->  balls painted, then n^3 values: fhlt::thickness_host of the field [k][j][i], n^3 values, decimal
// The buffers are sized exactly, so that a step past them is the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_thick.hpp"

static int bad() { printf("bad query\n"); return 1; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        in >> what;
        if (what == 'Q') {
            uint32_t lo = 0, hi = 0;
            in >> lo >> hi;
            if (!in || lo > hi || hi > fhlt::MAX_F) return bad();
            uint32_t last = fhlt::isqrt(lo);
            printf("%" PRIu32 " %" PRIu32, lo, last);
            for (uint32_t x = lo + 1; x <= hi && x != 0; x++) {
                const uint32_t w = fhlt::isqrt(x);
                if (w != last) printf(" %" PRIu32 " %" PRIu32, x, w);
                last = w;
            }
        } else if (what == 'W') {
            uint32_t f = 0;
            int32_t r = 0;
            in >> f >> r;
            if (!in || f == 0 || f > fhlt::MAX_F || r < 0 || r > 64) return bad();
            for (int32_t dz = -r; dz <= r; dz++)
                for (int32_t dy = -r; dy <= r; dy++) {
                    const uint32_t dd = (uint32_t)(dy * dy + dz * dz);
                    printf("%s%" PRId64, dz == -r && dy == -r ? "" : " ", fhlt::row_present(f, dd) ? (int64_t)fhlt::row_half(f, dd) : (int64_t)-1);
                }
        } else if (what == 'N') {
            uint32_t v = 0;
            in >> v;
            if (!in || v == 0 || v > 1u << 16) return bad();
            const std::vector<uint32_t> t = fhlt::need_tables_host(v);
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32, t[v], t[(size_t)(v + 1) + v], t[2 * (size_t)(v + 1) + v]);
        } else if (what == 'T') {
            uint32_t n = 0, prune = 0;
            in >> n >> prune;
            if (!in || n == 0 || n > 64) return bad();
            std::vector<uint32_t> F((size_t)n * n * n), T((size_t)n * n * n);
            for (auto& v : F) in >> v;
            if (!in) return bad();
            uint64_t balls = 0;
            if (!fhlt::thickness_host(F.data(), n, T.data(), prune != 0, &balls)) { printf("refused\n"); continue; }
            printf("%" PRIu64, balls);
            for (const uint32_t v : T) printf(" %" PRIu32, v);
        } else {
            return bad();
        }
        printf("\n");
    }
    return 0;
}
