// The integer arithmetic of the local thickness of a distance field (fhip_distance_thickness, include/fidget_hip.h).  F is a finished field
// of squared distances, 0 on the foreground; T(p) = max { F(c) : F(c) > |p - c|^2 }, the squared radius of the largest ball that fits and
// holds p (Hildebrand & Rueegsegger), 0 where there is none.  Here: the exact integer square root, the half-width of a ball's row, the
// shells behind the domination test that drops a centre whose ball lies inside a neighbour's, that test, and a serial thickness_host made
// of the same pieces.  No HIP and no memory of its own in the shared part: compiled for the device by thick.hip and for the host by
// tests/host_build/mesh_thick_host.cpp.  There is no counterpart in the reference: it has no voxel bitmap.
#pragma once
#include <stdint.h>

#include "mesh_vox.hpp"

namespace fhlt {
constexpr uint32_t MAX_F = 3u * 1023u * 1023u;       // the largest squared distance in a grid of 1024^3: 3 139 587 < 2^22
constexpr uint32_t SMALL_F = 16;                     // balls up to this squared radius span at most 7 voxels a row

// floor(sqrt(x)) for x <= MAX_F (a float holds every such x; whatever the root's rounding, the two loops end on w^2 <= x < (w + 1)^2)
FHV_HD uint32_t isqrt(uint32_t x) {
    uint32_t w = (uint32_t)__builtin_sqrtf((float)x);
    while (w * w > x) w--;
    while ((w + 1) * (w + 1) <= x) w++;
    return w;
}
// The ball of squared radius f > 0 around c is the voxels p with |p - c|^2 < f.  Its row at offset (dy, dz), dd = dy^2 + dz^2, is there
// iff dd < f, and then spans cx - w .. cx + w with w = row_half(f, dd); every row lies within `reach(f)` of c in each axis.
FHV_HD bool row_present(uint32_t f, uint32_t dd) { return dd < f; }
FHV_HD uint32_t row_half(uint32_t f, uint32_t dd) { return isqrt(f - 1 - dd); }
FHV_HD uint32_t reach(uint32_t f) { return isqrt(f - 1); }

// ---- domination: the ball of c lies inside the ball of c' = c + d, d one of the 26 offsets --------------------------------------------------
// iff F(c') >= need(F(c), class(d)), need(v, d) = 1 + max { |q - d|^2 : q integer, |q|^2 < v }.  |q - d|^2 = |q|^2 - 2 q.d + |d|^2 is
// largest with every component of q against d, so by symmetry only the number of non-zero components of d counts, its class 1, 2 or 3,
// and over the shell |q|^2 = n the maximum is taken at a lattice point a >= b >= c >= 0 of it: shell_value.  need is the running maximum
// over the shells below v, plus one (need_scan, in place over the table of shell maxima; k_lt_need does the same in parallel).
FHV_HD uint32_t offset_class(int32_t dx, int32_t dy, int32_t dz) { return (uint32_t)(dx != 0) + (uint32_t)(dy != 0) + (uint32_t)(dz != 0); }
FHV_HD uint32_t shell_value(uint32_t cls, uint32_t a, uint32_t b, uint32_t c) {          // (a >= b >= c)
    const uint32_t n = a * a + b * b + c * c;
    return cls == 1 ? n + 2 * a + 1 : cls == 2 ? n + 2 * (a + b) + 2 : n + 2 * (a + b + c) + 3;
}
// The tables: need[(cls - 1) * (vmax + 1) + v] for v = 0 .. vmax (entry 0 is never asked for: a centre has F > 0).
FHV_HD void need_scan(uint32_t* table, uint32_t vmax) {
    uint32_t run = 0;
    for (uint32_t v = 0; v <= vmax; v++) {
        const uint32_t s = table[v];
        table[v] = 1 + run;
        if (s > run) run = s;
    }
}
// Is the centre (i, j, k) with f = F > 0 kept, i.e. dominated by none of its neighbours in the grid?  Inclusion is strict - two balls
// around different centres are never equal - so chains of domination end, and dropping every dominated centre at once leaves T as it is.
FHV_HD bool keep_centre(const uint32_t* F, uint32_t N, uint32_t i, uint32_t j, uint32_t k, uint32_t f, const uint32_t* need, uint32_t vmax) {
    for (int32_t dz = -1; dz <= 1; dz++)
        for (int32_t dy = -1; dy <= 1; dy++)
            for (int32_t dx = -1; dx <= 1; dx++) {
                const uint32_t cls = offset_class(dx, dy, dz);
                const uint32_t x = i + (uint32_t)dx, y = j + (uint32_t)dy, z = k + (uint32_t)dz;          // (-1 wraps to above N)
                if (cls == 0 || x >= N || y >= N || z >= N) continue;          // outside the grid there is no centre
                if (F[((size_t)z * N + y) * N + x] >= need[(size_t)(cls - 1) * (vmax + 1) + f]) return false;
            }
    return true;
}
// the part of row (dy, dz) of the ball (f, cx) inside a grid of N: lo <= hi; the row is present
FHV_HD void row_span(uint32_t f, uint32_t cx, uint32_t dd, uint32_t N, uint32_t& lo, uint32_t& hi) {
    const uint32_t w = row_half(f, dd);
    lo = cx > w ? cx - w : 0;
    hi = cx + w < N ? cx + w : N - 1;
}
}  // namespace fhlt

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
namespace fhlt {
// the three tables for v <= vmax, serially: every lattice point a >= b >= c >= 0 below shell vmax, then the scan
inline std::vector<uint32_t> need_tables_host(uint32_t vmax) {
    std::vector<uint32_t> t(3 * ((size_t)vmax + 1), 0);
    for (uint32_t a = 0; a * a < vmax; a++)
        for (uint32_t b = 0; b <= a && a * a + b * b < vmax; b++)
            for (uint32_t c = 0; c <= b && a * a + b * b + c * c < vmax; c++) {
                const uint32_t n = a * a + b * b + c * c;
                for (uint32_t cls = 1; cls <= 3; cls++) {
                    uint32_t& s = t[(size_t)(cls - 1) * (vmax + 1) + n];
                    const uint32_t v = shell_value(cls, a, b, c);
                    if (v > s) s = v;
                }
            }
    for (uint32_t cls = 0; cls < 3; cls++) need_scan(t.data() + (size_t)cls * (vmax + 1), vmax);
    return t;
}
// T from F, both [N][N][N] = [k][j][i]: false for a field without foreground (a value above MAX_F), whose balls are unbounded.
// `balls`: how many centres were painted - with `prune` the kept ones, without it all of them.
inline bool thickness_host(const uint32_t* F, uint32_t N, uint32_t* T, bool prune, uint64_t* balls) {
    const size_t n = (size_t)N * N * N;
    uint32_t vmax = 1;
    for (size_t p = 0; p < n; p++) {
        if (F[p] > MAX_F) return false;
        if (F[p] > vmax) vmax = F[p];
        T[p] = 0;
    }
    const std::vector<uint32_t> need = need_tables_host(vmax);
    uint64_t painted = 0;
    for (uint32_t k = 0; k < N; k++)
        for (uint32_t j = 0; j < N; j++)
            for (uint32_t i = 0; i < N; i++) {
                const uint32_t f = F[((size_t)k * N + j) * N + i];
                if (f == 0 || (prune && !keep_centre(F, N, i, j, k, f, need.data(), vmax))) continue;
                painted++;
                const int32_t R = (int32_t)reach(f);
                for (int32_t dz = -R; dz <= R; dz++)
                    for (int32_t dy = -R; dy <= R; dy++) {
                        const uint32_t z = k + (uint32_t)dz, y = j + (uint32_t)dy, dd = (uint32_t)(dy * dy + dz * dz);
                        if (z >= N || y >= N || !row_present(f, dd)) continue;
                        uint32_t lo, hi;
                        row_span(f, i, dd, N, lo, hi);
                        uint32_t* const row = T + ((size_t)z * N + y) * N;
                        for (uint32_t x = lo; x <= hi; x++)
                            if (row[x] < f) row[x] = f;
                    }
            }
    if (balls) *balls = painted;
    return true;
}
}  // namespace fhlt
#endif
