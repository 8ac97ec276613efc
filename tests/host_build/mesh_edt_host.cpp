// Host build of the line arithmetic of the exact distance transform (fidget_amd/csrc/mesh_edt.hpp: no HIP, no device) for
// tests/test_distance.py.  Reads one line of the grid per line of stdin and prints its transform on one line; the test works the same
// out with tests/distance_ref.py and compares.  "No distance" is 4294967295.
//   R n w0 w1 ...       ->  n values      fhedt::row_line: a row of n voxels as (n + 63) / 64 hexadecimal mask words, bit b of word w voxel 64 w + b
//   C n f0 f1 ...       ->  n values      fhedt::column_line: a column of n squared distances, decimal
// The buffers are sized exactly - n values, n stack entries - so that a step past them is the sanitizers' to see.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_edt.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        uint32_t n = 0;
        in >> what >> n;
        if (!in || n == 0 || n > (4u << fhedt::MAX_DEPTH)) { printf("bad query\n"); return 1; }
        std::vector<uint32_t> out(n);
        if (what == 'R') {
            std::vector<uint64_t> mask((n + 63) / 64);
            for (auto& w : mask) in >> std::hex >> w;
            if (!in) { printf("bad query\n"); return 1; }
            fhedt::row_line(mask.data(), n, out.data());
        } else if (what == 'C') {
            for (auto& v : out) in >> v;
            if (!in) { printf("bad query\n"); return 1; }
            std::vector<fhedt::Entry> stack(n);
            fhedt::column_line(out.data(), n, stack.data());
        } else {
            printf("bad query\n");
            return 1;
        }
        for (uint32_t p = 0; p < n; p++) printf("%s%" PRIu32, p ? " " : "", out[p]);
        printf("\n");
    }
    return 0;
}
