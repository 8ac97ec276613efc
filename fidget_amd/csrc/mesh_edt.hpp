// The integer arithmetic of one line of the exact Euclidean distance transform of the voxel bitmap (fhip_voxels_distance,
// include/fidget_hip.h): the pass along i on a row's bit mask - the nearest set bit on either side by count-leading / count-trailing
// zeros on masked words - and the pass along j or k on a column of squared distances - the lower envelope of the parabolas
// f(q) + (p - q)^2 (Felzenszwalb & Huttenlocher; Meijster, Roerdink & Hesselink), integers throughout.  No HIP and no memory of its
// own: compiled for the device by edt.hip, where a lane runs a column with its stack in LDS or in a workspace, and for the host by
// tests/host_build/mesh_edt_host.cpp.  There is no counterpart in the reference: it has no voxel bitmap.
#pragma once
#include <stdint.h>

#include "mesh_vox.hpp"

namespace fhedt {
constexpr uint32_t MAX_DEPTH = 8;                // N = 1024: the field is 4 GiB
constexpr uint32_t NONE = 0xFFFFFFFFu;           // "no distance": no foreground voxel in the line (in the grid)
constexpr uint32_t MAX_WORDS = 16;               // 64-bit mask words of a row at MAX_DEPTH

// ---- along i: a row as a bit mask, bit b of word w is voxel i = 64 w + b --------------------------------------------------------------
FHV_HD int32_t highest_bit(uint64_t m) { return 63 - (int32_t)__builtin_clzll(m); }          // (m != 0)
FHV_HD int32_t lowest_bit(uint64_t m) { return (int32_t)__builtin_ctzll(m); }                // (m != 0)
// what word w of a row of n_words sees beyond itself: the nearest set bit in the words below it and in the words above it, as
// positions in the row, -1 where there is none
FHV_HD void row_links(const uint64_t* mask, uint32_t n_words, uint32_t w, int32_t& below, int32_t& above) {
    below = above = -1;
    for (uint32_t u = w; u-- > 0;)
        if (mask[u]) { below = (int32_t)(64 * u) + highest_bit(mask[u]); break; }
    for (uint32_t u = w + 1; u < n_words; u++)
        if (mask[u]) { above = (int32_t)(64 * u) + lowest_bit(mask[u]); break; }
}
// the squared distance from voxel 64 w + b to the nearest set bit of its row: m is word w, (below, above) its row_links
FHV_HD uint32_t row_d2(uint64_t m, uint32_t w, uint32_t b, int32_t below, int32_t above) {
    const int32_t pos = (int32_t)(64 * w + b);
    const uint64_t lo = m & (~(uint64_t)0 >> (63 - b)), hi = m & (~(uint64_t)0 << b);          // the bits at or below b; at or above b
    const int32_t L = lo ? (int32_t)(64 * w) + highest_bit(lo) : below, R = hi ? (int32_t)(64 * w) + lowest_bit(hi) : above;
    uint32_t d = NONE;
    if (L >= 0) d = (uint32_t)(pos - L);
    if (R >= 0 && (uint32_t)(R - pos) < d) d = (uint32_t)(R - pos);
    return d == NONE ? NONE : d * d;             // (d <= 1023)
}
// a whole row of N voxels (the host's line routine; k_edt_rows deals the same two calls out to its lanes)
FHV_HD void row_line(const uint64_t* mask, uint32_t N, uint32_t* out) {
    const uint32_t n_words = (N + 63) / 64;
    for (uint32_t w = 0; w < n_words; w++) {
        int32_t below, above;
        row_links(mask, n_words, w, below, above);
        for (uint32_t b = 0; b < 64 && 64 * w + b < N; b++) out[64 * w + b] = row_d2(mask[w], w, b, below, above);
    }
}

// ---- along j or k: out[p] = min over q with f[q] != NONE of f[q] + (p - q)^2 -----------------------------------------------------------
// Widths.  N <= 1024, so (p - q)^2 <= 1023^2 = 1 046 529.  The pass along j reads f <= 1023^2 and the pass along k reads
// f <= 2 * 1023^2 = 2 093 058; every sum formed below - a parabola's value f + (p - q)^2, or f + q^2 in the numerator of `sep` - is at
// most 3 * 1023^2 = 3 139 587 < 2^22.  The one difference formed, the numerator of `sep`, is not negative (see there).  So uint32 holds
// everything, with ten bits to spare.  NONE would not: an entry with f == NONE never comes in here - env_add's caller skips it - and a
// column without any finite entry is left as it is.
//
// The envelope is a stack of entries: parabola q of height f is the lowest one from p = z on, until the next entry's z.  q and z are
// below 1024 and share a word.
struct alignas(8) Entry {
    uint32_t qz, f;       // q | z << 16
};
FHV_HD Entry entry(uint32_t q, uint32_t z, uint32_t f) { return Entry{q | (z << 16), f}; }
FHV_HD uint32_t entry_q(const Entry& e) { return e.qz & 0xFFFFu; }
FHV_HD uint32_t entry_z(const Entry& e) { return e.qz >> 16; }
FHV_HD uint32_t sq_diff(uint32_t a, uint32_t b) { const uint32_t d = a > b ? a - b : b - a; return d * d; }
FHV_HD uint32_t value_at(const Entry& e, uint32_t p) { return e.f + sq_diff(p, entry_q(e)); }

// Add parabola q of height fq (finite) to the envelope of the parabolas before it; q ascends from call to call.  `top` is the index of
// the last entry, -1 for an empty stack, and `t` a copy of that entry; `stack` is anything with get(k) and set(k, entry) - entries
// 0 .. top are in it.  At most one entry per q: N entries do.
template <class Stack>
FHV_HD void env_add(Stack& stack, int32_t& top, Entry& t, uint32_t N, uint32_t q, uint32_t fq) {
    // an entry that q undercuts where it begins is hidden by q from there on: q lies to its right, so q gains on it as p grows
    while (top >= 0 && value_at(t, entry_z(t)) > fq + sq_diff(entry_z(t), q)) {
        top--;
        if (top >= 0) t = stack.get((uint32_t)top);
    }
    if (top < 0) {
        top = 0;
        t = entry(q, 0, fq);
        stack.set(0, t);
        return;
    }
    // u = the top entry's parabola is at most q's at p = z: (fq + q^2) - (f_u + u^2) - 2 p (q - u) >= 0 there, so with z >= 0 the
    // numerator is not negative, and sep = the last p at which u is still at most q is at least z.  q takes over at sep + 1 > z.
    const uint32_t u = entry_q(t);
    const uint32_t sep = ((fq + q * q) - (t.f + u * u)) / (2 * (q - u));
    if (sep + 1 < N) {
        top++;
        t = entry(q, sep + 1, fq);
        stack.set((uint32_t)top, t);
    }
}
// Read the envelope off: put(p, value) for p = 0 .. N - 1 in ascending order.  top >= 0.
template <class Stack, class Put>
FHV_HD void env_scan(const Stack& stack, int32_t top, uint32_t N, Put put) {
    Entry cur = stack.get(0), next = cur;
    uint32_t k = 0, next_z = N;
    if (top > 0) { next = stack.get(1); next_z = entry_z(next); }
    for (uint32_t p = 0; p < N; p++) {
        if (p == next_z) {          // (the entries' z ascend strictly: one step at most)
            cur = next;
            k++;
            next_z = N;
            if ((int32_t)k < top) { next = stack.get(k + 1); next_z = entry_z(next); }
        }
        put(p, value_at(cur, p));
    }
}

// a whole column of N values, in place, with N entries of stack (the host's line routine; k_edt_cols does the same per lane)
struct LineStack {
    Entry* e;
    FHV_HD Entry get(uint32_t k) const { return e[k]; }
    FHV_HD void set(uint32_t k, const Entry& v) { e[k] = v; }
};
FHV_HD void column_line(uint32_t* f, uint32_t N, Entry* entries) {
    LineStack stack{entries};
    int32_t top = -1;
    Entry t = entry(0, 0, 0);
    for (uint32_t q = 0; q < N; q++)
        if (f[q] != NONE) env_add(stack, top, t, N, q, f[q]);
    if (top < 0) return;          // nothing finite: the column stays NONE
    env_scan(stack, top, N, [&](uint32_t p, uint32_t v) { f[p] = v; });
}
}  // namespace fhedt
