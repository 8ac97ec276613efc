// The rules of tape simplification down the octree (capi_mesh.hpp split_tapes): where a build splits, which cells get a tape of their own,
// how the tapes are packed for the device and when a split is used at all.  Arithmetic on sizes and paths, no HIP and no device: built for
// the host by tests/host_build/mesh_split_host.cpp.  A cell's path holds 3 bits per level below the root under a leading 1, so the cells of
// level l have the paths 8^l .. 2 * 8^l - 1.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace fhsplit {
inline uint64_t level_base(uint32_t level) { return (uint64_t)1 << (3 * level); }      // 8^level: first path and number of cells of a level

// (option mesh_simplify_min_ops, default 256: shorter tapes are evaluated as they are - gyroid-sphere's 28 ops gain nothing and keep the
// assembly bulk interpreter for their leaf samples; 0 = never.  The level: 4 - 4 096 cells at most, a 16th of the region across, where
// prospero.vm's 6 363 ops are down to a few hundred - or two above the leaves of a shallower octree)
// ... and once more at depth - 2 (at most level 7: a table of 8^7 entries), from the first split's tapes, when the first one was taken:
// prospero.vm's level-4 tapes still hold ~600 ops, and the leaf samples of a depth-8 build walked them 16 M times.  0: no split.
struct SplitLevels { uint32_t l1, l2; };
inline SplitLevels split_levels(int min_ops_option, size_t n_ops, uint32_t n_choices, uint32_t depth) {
    SplitLevels s;
    s.l1 = (min_ops_option > 0 && n_ops >= (size_t)min_ops_option && n_choices > 0 && depth >= 3) ? std::min<uint32_t>(4, depth - 2) : 0;
    s.l2 = (s.l1 == 4 && depth >= 7) ? std::min<uint32_t>(7, depth - 2) : 0;
    return s;
}

// a cell keeps a simplified tape only where simplification worked and left fewer ops than the tape it came from (the root tape at the first
// split, its ancestor's at the second); otherwise it goes on with that one
inline bool split_accepts(bool ok, size_t n_ops, size_t parent_ops) { return ok && n_ops != 0 && n_ops < parent_ops; }
// second split: which of the first split's kept tapes a cell of level l2 inherited - sub_of is indexed like the first split's table and
// holds -1 where the ancestor kept the root tape (then so does the cell)
inline int32_t split_parent(const std::vector<int32_t>& sub_of, uint64_t path, uint32_t l1, uint32_t l2) {
    const uint64_t i1 = (path >> (3 * (l2 - l1))) - level_base(l1);
    return i1 < sub_of.size() ? sub_of[(size_t)i1] : -1;
}

// What the kernels read: per cell of the level (index: path - 8^level) where its tape starts in one array of ops and how long it is;
// {0, 0}: no tape of its own.  Offsets are 32 bits wide: OPS_LIMIT_32 for the second split (8^7 cells); the first one (at most 4 096
// cells) has never had a limit and keeps none.
struct TabEntry { uint32_t off, len; };
constexpr uint64_t OPS_LIMIT_32 = (uint64_t)1 << 32, NO_OPS_LIMIT = ~(uint64_t)0;
inline bool ops_fit(uint64_t have, uint64_t more, uint64_t limit) { return have + more < limit; }
struct SplitPack {
    std::vector<TabEntry> tab;
    std::vector<uint64_t> ops;
    std::vector<uint32_t> taken;        // the candidates that got an entry, in order
    uint64_t n_tapes = 0, n_ops = 0;
};
// candidate j: the cell's path, its simplified ops (null: not accepted) and how many
inline SplitPack pack_split(uint32_t level, size_t n, const uint64_t* path, const uint64_t* const* ops, const size_t* len, uint64_t ops_limit) {
    SplitPack S;
    const uint64_t n_tab = level_base(level);
    S.tab.assign((size_t)n_tab, TabEntry{0, 0});
    for (size_t j = 0; j < n; j++) {
        if (!ops[j]) continue;
        const uint64_t idx = path[j] - n_tab;
        if (idx >= n_tab || !ops_fit(S.n_ops, len[j], ops_limit)) continue;
        S.tab[(size_t)idx] = TabEntry{(uint32_t)S.n_ops, (uint32_t)len[j]};
        S.ops.insert(S.ops.end(), ops[j], ops[j] + len[j]);
        S.taken.push_back((uint32_t)j);
        S.n_tapes++; S.n_ops += len[j];
    }
    return S;
}

// ... where it pays: the lanes of a wave then walk tapes of their own through the generic interpreter, and a tape that fits the
// assembly bulk interpreter (<= 32 registers) gives that up for its leaf samples - bear.vm's smooth blend keeps 3/4 of its ops
// at this level and meshes twice as fast WITHOUT (measured, profiles/r04g); prospero.vm keeps 1/20 and gains 16x
inline bool split_worth_using(uint64_t sub_ops, uint64_t sub_tapes, size_t root_ops, bool bulk_capable) {
    const double kept = sub_tapes ? (double)sub_ops / ((double)sub_tapes * (double)root_ops) : 1.0;
    return !(kept >= (bulk_capable ? 0.25 : 0.75));
}
// (only where the first split left tapes worth pruning again: 128 ops on average - colonnade.vm's are ~50 and a second split cost it 20 % -
// and the choices of the level's cells fit 3 GiB)
inline bool second_split_wanted(bool first_in_use, size_t n_kept, uint64_t sub_ops, uint64_t sub_tapes, uint64_t n_cells, uint32_t n_choices) {
    return first_in_use && n_kept != 0 && sub_ops >= 128 * sub_tapes && n_cells * n_choices <= ((uint64_t)3 << 30);
}
}  // namespace fhsplit
