// Host build of the bit arithmetic of connected-component labelling (fidget_amd/csrc/mesh_cc.hpp: no HIP, no device) for
// tests/test_components.py.  Reads one query per line from stdin and prints one answer line for each; the test works the same things
// out with tests/components_ref.py and compares.  Words and masks are hexadecimal.
//   L word conn               ->  n m0 m1 ...       fhcc::local_components (and fhcc::local_count, which must agree: "count mismatch")
//   C mask dx dy dz conn      ->  image             fhcc::carry
//   D                         ->  dx,dy,dz ...      fhcc::direction for d = 0 .. 12
//   B mask bx by bz nb        ->  lo0 lo1 lo2 hi0 hi1 hi2 border      fhcc::local_bounds, fhcc::touches_border (nb bricks per axis)
//   K key depth               ->  i j k             fhcc::key_voxel
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "mesh_cc.hpp"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        uint64_t a = 0, key = 0;
        uint32_t conn = 0, bx = 0, by = 0, bz = 0, nb = 0, depth = 0;
        int dx = 0, dy = 0, dz = 0;
        if (sscanf(line, "L %" SCNx64 " %u", &a, &conn) == 2) {
            uint64_t masks[fhcc::MAX_LOCAL + 1];
            memset(masks, 0xEE, sizeof masks);       // (a 33rd entry that must stay as it is)
            const uint32_t n = fhcc::local_components(a, conn, masks);
            if (n != fhcc::local_count(a, conn) || n > fhcc::MAX_LOCAL || masks[fhcc::MAX_LOCAL] != 0xEEEEEEEEEEEEEEEEull) { printf("count mismatch\n"); return 1; }
            printf("%u", n);
            for (uint32_t k = 0; k < n; k++) printf(" %" PRIx64, masks[k]);
            printf("\n");
        } else if (sscanf(line, "C %" SCNx64 " %d %d %d %u", &a, &dx, &dy, &dz, &conn) == 5) {
            printf("%" PRIx64 "\n", fhcc::carry(a, dx, dy, dz, conn));
        } else if (line[0] == 'D') {
            for (uint32_t d = 0; d < fhcc::N_DIRS; d++) {
                fhcc::direction(d, dx, dy, dz);
                printf("%s%d,%d,%d", d ? " " : "", dx, dy, dz);
            }
            printf("\n");
        } else if (sscanf(line, "B %" SCNx64 " %u %u %u %u", &a, &bx, &by, &bz, &nb) == 5) {
            uint32_t lo[3], hi[3];
            fhcc::local_bounds(a, lo, hi);
            printf("%u %u %u %u %u %u %d\n", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], fhcc::touches_border(a, bx, by, bz, nb) ? 1 : 0);
        } else if (sscanf(line, "K %" SCNu64 " %u", &key, &depth) == 2) {
            uint32_t v[3];
            fhcc::key_voxel(key, depth, v);
            printf("%u %u %u\n", v[0], v[1], v[2]);
        } else {
            printf("bad query\n");
            return 1;
        }
    }
    return 0;
}
