// Host build of the mesh driver's split rules (fidget_amd/csrc/mesh_split.hpp: no HIP, no device) for tests/test_mesh_split.py:
// prints what the rules give for small inputs, one line per case; the test restates the rules and compares.
#include <stdio.h>

#include <string>

#include "mesh_split.hpp"

using namespace fhsplit;

struct Cand { uint64_t path; bool ok; size_t len; };       // a candidate's ops: len copies of 1000 * (j + 1) + position

// `parent_len`: the tape every candidate was simplified from; the candidates' parents for the second split come from sub_of / kept_len
static void print_pack(const char* name, uint32_t level, const std::vector<Cand>& cands, const std::vector<size_t>& parent_len, uint64_t limit) {
    std::vector<std::vector<uint64_t>> store(cands.size());
    std::vector<uint64_t> path(cands.size());
    std::vector<const uint64_t*> ops(cands.size());
    std::vector<size_t> len(cands.size());
    for (size_t j = 0; j < cands.size(); j++) {
        for (size_t k = 0; k < cands[j].len; k++) store[j].push_back(1000 * (j + 1) + k);
        path[j] = cands[j].path; len[j] = cands[j].len;
        ops[j] = split_accepts(cands[j].ok, cands[j].len, parent_len[j]) ? store[j].data() : nullptr;
    }
    const SplitPack S = pack_split(level, cands.size(), path.data(), ops.data(), len.data(), limit);
    std::string tab, o, taken;
    for (size_t i = 0; i < S.tab.size(); i++) if (S.tab[i].len) tab += (tab.empty() ? "" : ",") + std::to_string(i) + ":" + std::to_string(S.tab[i].off) + "+" + std::to_string(S.tab[i].len);
    for (uint64_t x : S.ops) o += (o.empty() ? "" : ",") + std::to_string(x);
    for (uint32_t j : S.taken) taken += (taken.empty() ? "" : ",") + std::to_string(j);
    printf("%s: n_tab=%zu tab=%s ops=%s taken=%s n_tapes=%llu n_ops=%llu\n", name, S.tab.size(), tab.empty() ? "-" : tab.c_str(), o.empty() ? "-" : o.c_str(),
           taken.empty() ? "-" : taken.c_str(), (unsigned long long)S.n_tapes, (unsigned long long)S.n_ops);
}

int main() {
    for (uint32_t depth = 0; depth <= 12; depth++)
        for (size_t n_ops : {255, 256, 6363})
            for (uint32_t n_choices : {0u, 5u})
                for (int option : {0, 256}) {
                    const SplitLevels s = split_levels(option, n_ops, n_choices, depth);
                    printf("levels_%u_%zu_%u_%d: l1=%u l2=%u\n", depth, n_ops, n_choices, option, s.l1, s.l2);
                }
    // first split, root tape of 10 ops: not ok, empty, as long as the root, longer, outside the level (below and above), accepted ones out of path order
    const size_t ROOT = 10;
    for (uint32_t level : {1u, 2u}) {
        const uint64_t b = level_base(level);
        const std::vector<Cand> c = {{b + 5, true, 3},      {b + 1, false, 4}, {b + 2, true, 0},  {b + 3, true, ROOT}, {b + 4, true, ROOT + 1}, {2 * b, true, 2},
                                     {b - 1, true, 2},      {b + 0, true, 9},  {b + 6, false, 0}, {b + 7, true, 1},    {16 * b + 3, true, 2},   {b + (level == 2 ? 63 : 2), true, 4}};
        print_pack(level == 1 ? "first_l1" : "first_l2", level, c, std::vector<size_t>(c.size(), ROOT), NO_OPS_LIMIT);
    }
    // where a split pays: kept = sub_ops / (sub_tapes * root_ops) against 0.25 (a tape the bulk interpreter takes) and 0.75
    for (int bulk = 0; bulk < 2; bulk++)
        for (uint64_t sub_ops : {0ull, 99ull, 100ull, 101ull, 299ull, 300ull, 301ull})
            for (uint64_t tapes : {0ull, 4ull})
                printf("worth_%d_%llu_%llu: use=%d\n", bulk, (unsigned long long)sub_ops, (unsigned long long)tapes, split_worth_using(sub_ops, tapes, 100, bulk != 0) ? 1 : 0);
    // the second split's gate: 128 ops on average, the first split in use with tapes kept, the choices within 3 GiB
    struct Gate { const char* name; bool in_use; size_t kept; uint64_t ops, tapes, cells; uint32_t nch; };
    for (const Gate& g : {Gate{"at", true, 3, 128 * 3, 3, 10, 7}, Gate{"below", true, 3, 128 * 3 - 1, 3, 10, 7}, Gate{"unused", false, 3, 1000, 3, 10, 7}, Gate{"none_kept", true, 0, 1000, 3, 10, 7},
                          Gate{"choices_at", true, 3, 1000, 3, 3ull << 20, 1024}, Gate{"choices_over", true, 3, 1000, 3, (3ull << 20) + 1, 1024}})
        printf("gate_%s: wanted=%d\n", g.name, second_split_wanted(g.in_use, g.kept, g.ops, g.tapes, g.cells, g.nch) ? 1 : 0);
    // second split, l1 = 1 and l2 = 3: the first split kept tapes of 8 and 6 ops for the octants 2 and 5 (sub_of: octant -> kept tape)
    {
        const uint32_t l1 = 1, l2 = 3;
        const std::vector<int32_t> sub_of = {-1, -1, 0, -1, -1, 1, -1, -1};
        const std::vector<size_t> kept_len = {8, 6};
        auto path = [](uint64_t o1, uint64_t o2, uint64_t o3) { return (((1ull << 3 | o1) << 3 | o2) << 3) | o3; };
        const std::vector<Cand> c = {{path(2, 0, 1), true, 7}, {path(3, 1, 1), true, 2}, {path(2, 7, 7), true, 8}, {path(5, 0, 0), true, 5}, {path(5, 0, 1), true, 6},
                                     {path(5, 3, 2), false, 2}, {path(2, 0, 0), true, 1}, {path(0, 0, 0), true, 1}, {path(7, 7, 7), true, 1}, {path(5, 7, 7), true, 0}};
        std::vector<size_t> parent_len;
        std::string parents;
        for (const Cand& x : c) {
            const int32_t k = split_parent(sub_of, x.path, l1, l2);
            parents += (parents.empty() ? "" : ",") + std::to_string(k);
            parent_len.push_back(k < 0 ? 0 : kept_len[(size_t)k]);      // (no parent: nothing is shorter than 0 ops, so never accepted)
        }
        printf("second_parents: k=%s outside=%d\n", parents.c_str(), split_parent(sub_of, 16ull << 6, l1, l2));
        print_pack("second", l2, c, parent_len, OPS_LIMIT_32);
    }
    // the 2^32 cap, with lengths no memory stands behind: a dropped candidate's ops are never read
    {
        const uint64_t one = 1;
        const uint64_t path[3] = {8 + 1, 8 + 2, 8 + 3};
        const uint64_t* ops[3] = {&one, &one, &one};
        const size_t len[3] = {1, (size_t)(OPS_LIMIT_32 - 1), 1};
        const SplitPack S = pack_split(1, 3, path, ops, len, OPS_LIMIT_32);
        printf("cap_pack: taken=%zu first=%u last=%u n_ops=%llu\n", S.taken.size(), S.taken.front(), S.taken.back(), (unsigned long long)S.n_ops);
        printf("cap_fit: below=%d at=%d none=%d\n", ops_fit(5, OPS_LIMIT_32 - 6, OPS_LIMIT_32) ? 1 : 0, ops_fit(5, OPS_LIMIT_32 - 5, OPS_LIMIT_32) ? 1 : 0,
               ops_fit(5, OPS_LIMIT_32 - 5, NO_OPS_LIMIT) ? 1 : 0);
    }
    return 0;
}
