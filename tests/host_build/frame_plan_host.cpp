// Host build of the frame plan (fidget_amd/csrc/frame_plan.hpp: no HIP, no device) for tests/test_frame_plan.py: plans named frames the
// way render3d_frame / render2d_frame do and prints what the plan decided, one line each: `name: key=value ...` (a refusal's text with
// '_' for its spaces; roots as first,n,stride,z,x joined by ';', in queue order).
#include <stdio.h>
#include <string.h>

#include <string>

#include "frame_plan.hpp"

struct Case {
    bool is3d = true;
    uint32_t w = 1024, h = 1024, d = 1024;
    std::vector<uint32_t> tiles;      // 3D: the caller's list (empty: the library's choice); 2D: the list prepare() is given
    PartSpec part;
    PlanInputs in;
    TapeFacts t;
    bool one_level_64 = false;
    bool raw_tiles = false;      // 3D: `tiles` goes to plan_frame as it is (not through choose_tiles_3d, which substitutes what the kernels do not take)
};

// A tape of prospero.vm's kind: 6363 ops, 72 registers, 3000 choices, reads x and y only; 16 term groups, a root chain
static TapeFacts prospero_kind() {
    TapeFacts t;
    t.n_ops = 6363; t.n_regs = 72; t.n_choices = 3000;
    t.input_slots = 3;
    t.n_groups = 16;
    for (uint32_t g = 0; g < t.n_groups; g++) t.group[g] = {400, 40, 190};
    t.n_terms = 64; t.n_top = 63; t.chain = true;
    return t;
}

static std::string list(const uint32_t* v, size_t n) {
    std::string s;
    for (size_t i = 0; i < n; i++) s += (i ? "/" : "") + std::to_string(v[i]);
    return s.empty() ? "-" : s;
}

static void print(const char* name, const Case& c) {
    RenderSetup R;
    memset(&R.S, 0, sizeof(R.S));
    FhRender& P = R.S.P;
    P.width = c.w; P.height = c.h; P.depth = c.is3d ? c.d : 0;
    for (int i = 0; i < 4; i++) P.mat[5 * i] = 1.0f;      // identity camera; x, y, z on slots 0, 1, 2
    for (uint32_t s = 0; s < FH_MAX_INPUTS; s++) P.in_kind[s] = s < 3 ? s : 3;
    R.one_level_64 = c.one_level_64;
    std::vector<uint32_t> ts = c.tiles;
    if (c.is3d) {
        column_facts(P, c.t, c.in, R);
        const uint32_t size[3] = {c.w, c.h, c.d};
        const TileChoice T = choose_tiles_3d(c.tiles.empty() ? nullptr : c.tiles.data(), (uint32_t)c.tiles.size(), size, c.part.n_shards * c.part.nx * c.part.ny, c.part.nz,
                                             R.column_inv, c.in.root32_max, c.in.no_zrep, linked_root_tape(c.t, c.in));
        if (!c.raw_tiles) ts = T.ts;
    }
    const PlanStatus ps = plan_frame(c.t, c.in, c.is3d, ts, c.part, R);
    std::string msg = ps.msg;
    for (char& ch : msg) if (ch == ' ') ch = '_';
    printf("%s: status=%d msg=%s", name, ps.status, msg.empty() ? "-" : msg.c_str());
    if (ps.status) { printf("\n"); return; }
    if (R.groups) plan_linked_prune(c.t, c.in, true, c.t.chain ? c.t.n_top : 0, R);
    const FhRenderState& S = R.S;
    const FrameBytes& B = R.bytes;
    printf(" tiles=%s tl=%u roots_x=%u roots_y=%u slab=%u n_slabs=%u n_layers=%u slab_lo=%u slab_hi=%u slab_stop=%u pre_levels=%u", list(P.tiles, P.n_levels).c_str(), R.tl,
           P.roots_x, P.roots_y, P.slab, R.n_slabs, R.n_layers, R.slab_lo, R.slab_hi, R.slab_stop, S.pre_levels);
    std::string roots;
    for (const FhGroup& g : R.roots) {
        if (g.tape.off != 0 || g.tape.len != c.t.n_ops || g.tape.n_regs != c.t.n_regs || g.tape.n_choices != c.t.n_choices || g.y != 0) roots += "BAD";
        roots += (roots.empty() ? "" : ";") + std::to_string(g.first) + "," + std::to_string(g.n) + "," + std::to_string(g.stride) + "," + std::to_string(g.z) + "," + std::to_string(g.x);
    }
    printf(" roots=%s groups_per_slab=%u qcap=%s squeue_cap=%u leaf_cap=%u table_words=%u n_footprints=%u hit_bucket_cap=%u hit_words=%zu mind_words=%zu slot_cap=%u",
           roots.empty() ? "-" : roots.c_str(), R.groups_per_slab, list(S.qcap, P.n_levels).c_str(), S.squeue_cap, S.leaf_cap, R.table_words, R.n_footprints, R.hit_bucket_cap,
           R.hit_words, R.mind_words, S.slot_cap[0]);
    std::string q;
    for (uint32_t l = 0; l < P.n_levels; l++) q += (l ? "/" : "") + std::to_string(B.queue[l]);
    printf(" b_gscratch=%zu b_queue=%s b_squeue=%zu b_leaves=%zu b_leaves_b=%zu b_leaf_table=%zu b_leaf_table_b=%zu b_zbuf=%zu b_normals=%zu b_fp_lists=%zu b_fp_lists_b=%zu b_mind=%zu"
           " b_tvals=%zu b_topch=%zu b_chwr=%zu b_chw=%zu/%zu b_slots=%zu",
           B.gscratch, q.c_str(), B.squeue, B.leaves, B.leaves_b, B.leaf_table, B.leaf_table_b, B.zbuf, B.normals, B.fp_lists, B.fp_lists_b, B.mind, B.tvals, B.topch, B.chwr, B.chw[0],
           B.chw[1], B.slots);
    printf(" lds_big=%zu lds_small=%zu lds_mid=%zu lds_points_big=%zu lds_normals_big=%zu lds_normals_small=%zu lds_group=%zu lds_prune2=%zu big_hbm=%d stride=%u hbm_waves=%u",
           R.lds_tiles_big, R.lds_tiles_small, R.lds_tiles_mid, R.lds_points_big, R.lds_normals_big, R.lds_normals_small, R.lds_tiles_group, R.lds_prune2, R.big_hbm, S.gscratch_stride,
           R.hbm_waves);
    printf(" xy_fixed=%d root_invariant=%d column_inv=%d root_zrep=%d front_only=%d zrep=%d full=%d split=%d asm_points=%d asm_points_t=%d asm_normals=%d asm_tiles=%d asm_tiles_t=%d"
           " hip_tiles_unasked=%d prune1=%d exp_levels=%u groups=%d prune2=%d leaf_asm_regs=%u norm_asm_regs=%u n_tgroups=%u arena_head=%u arena_root_end=%u arena_frame_end=%u"
           " arena_cap=%u smooth=%d\n",
           R.xy_fixed, R.root_invariant, R.column_inv, R.root_zrep, R.front_only, R.zrep, R.full, R.split, R.asm_points, R.asm_points_t, R.asm_normals, R.asm_tiles, R.asm_tiles_t,
           R.hip_tiles_unasked, R.prune1, R.exp_levels, R.groups, R.prune2, S.leaf_asm_regs, S.norm_asm_regs, S.n_tgroups, S.arena_head, S.arena_root_end, S.arena_frame_end,
           S.arena_cap, R.smooth_tape);
}

int main() {
    printf("sizes: group=%zu leaf=%zu leaf_ref=%zu slot=%zu\n", sizeof(FhGroup), sizeof(FhLeaf), sizeof(FhLeafRef), sizeof(FhSlot));
    Case d;
    d.t = prospero_kind();
    auto with = [&](auto f) { Case c = d; f(c); return c; };
    auto cube = [](Case& c, uint32_t n) { c.w = c.h = c.d = n; };
    // whole frames
    print("whole_1024", d);
    print("whole_1024_noinv", with([](Case& c) { c.in.no_column_inv = 1; }));
    print("whole_2048", with([&](Case& c) { cube(c, 2048); }));
    print("whole_2048_noinv", with([&](Case& c) { cube(c, 2048); c.in.no_column_inv = 1; }));
    print("whole_64", with([&](Case& c) { cube(c, 64); }));
    print("odd_200x120x72", with([](Case& c) { c.w = 200; c.h = 120; c.d = 72; }));
    print("odd_200x120x72_noinv", with([](Case& c) { c.w = 200; c.h = 120; c.d = 72; c.in.no_column_inv = 1; }));
    for (int z = 1; z <= 3; z++) print(("no_zrep" + std::to_string(z)).c_str(), with([&](Case& c) { c.in.no_zrep = z; }));
    for (int sl : {1, 8}) {
        print(("slab_layers" + std::to_string(sl)).c_str(), with([&](Case& c) { c.in.slab_layers = sl; }));
        print(("slab_layers" + std::to_string(sl) + "_noinv").c_str(), with([&](Case& c) { c.in.slab_layers = sl; c.in.no_column_inv = 1; }));
    }
    // parts of a frame
    print("shard_1_of_3", with([&](Case& c) { cube(c, 512); c.part.shard = 1; c.part.n_shards = 3; }));
    print("shard_1_of_3_noinv", with([&](Case& c) { cube(c, 512); c.part.shard = 1; c.part.n_shards = 3; c.in.no_column_inv = 1; }));
    auto block = [](Case& c) { c.part.ix = 1; c.part.nx = 2; c.part.iy = 0; c.part.ny = 2; c.part.iz = 1; c.part.nz = 2; };
    print("block_101", with([&](Case& c) { cube(c, 512); block(c); }));
    print("block_101_noinv", with([&](Case& c) { cube(c, 512); block(c); c.in.no_column_inv = 1; }));
    print("block_101_128", with([&](Case& c) { cube(c, 512); block(c); c.in.no_column_inv = 1; c.tiles = {128, 32, 8}; }));
    print("more_parts_than_layers", with([&](Case& c) { cube(c, 256); c.tiles = {128, 32, 8}; c.part.iz = 1; c.part.nz = 4; }));
    print("tall_block", with([](Case& c) { c.w = 64; c.h = 4096; c.d = 64; c.tiles = {32, 8}; c.part.ix = 1; c.part.nx = 2; c.in.no_column_inv = 1; }));
    // 2D
    print("2d_4096", with([](Case& c) { c.is3d = false; c.w = c.h = 4096; c.tiles = {128, 16}; }));
    print("2d_inserted_level", with([](Case& c) { c.is3d = false; c.w = c.h = 1024; c.tiles = {128, 16, 8}; }));
    print("2d_one_level_64", with([](Case& c) { c.is3d = false; c.w = c.h = 256; c.tiles = {16}; c.one_level_64 = true; }));
    print("2d_one_level_plain", with([](Case& c) { c.is3d = false; c.w = c.h = 256; c.tiles = {16}; }));
    // tapes
    print("regs_300", with([](Case& c) { c.t.n_regs = 300; }));
    print("regs_300_few_cus", with([](Case& c) { c.t.n_regs = 300; c.in.n_cu = 8; }));
    print("regs_200", with([](Case& c) { c.t.n_regs = 200; }));
    print("regs_140", with([](Case& c) { c.t.n_regs = 140; }));
    print("groups_do_not_fit", with([](Case& c) { c.in.arena_bytes = 100000; }));
    print("transcendental", with([](Case& c) { c.t.asm_ok = false; c.t.is_full = true; }));
    print("transcendental_mod", with([](Case& c) { c.t.asm_ok = false; c.t.is_full = true; c.t.has_mod = true; }));
    print("no_asm", with([](Case& c) { c.in.use_asm = false; }));
    print("no_split", with([](Case& c) { c.in.use_split = false; }));
    // refusals, in the order the plan checks them
    print("refuse_outputs", with([](Case& c) { c.t.n_outputs = 2; c.tiles = {8, 32}; }));
    print("refuse_no_levels", with([](Case& c) { c.is3d = false; c.tiles = {}; }));
    print("refuse_nine_levels", with([](Case& c) { c.is3d = false; c.tiles = {512, 256, 128, 64, 32, 16, 8, 4, 2}; }));
    print("refuse_ascending", with([](Case& c) { c.is3d = false; c.tiles = {8, 32}; }));
    print("refuse_not_a_multiple", with([](Case& c) { c.is3d = false; c.tiles = {128, 48}; }));
    print("refuse_fanout", with([](Case& c) { c.is3d = false; c.tiles = {128, 8}; }));
    print("refuse_3d_fanout", with([](Case& c) { c.raw_tiles = true; c.tiles = {128, 8}; }));
    print("refuse_leaves", with([](Case& c) { c.raw_tiles = true; c.tiles = {128, 32, 16}; c.t.n_regs = 4096; }));
    print("refuse_registers", with([](Case& c) { c.t.n_regs = 4096; c.t.n_ops = 1u << 24; }));
    print("accept_4095_registers", with([](Case& c) { c.t.n_regs = 4095; }));
    print("refuse_ops", with([](Case& c) { c.t.n_ops = 1u << 24; c.t.n_choices = 1u << 28; }));
    print("refuse_register_file", with([](Case& c) { c.t.n_choices = 1u << 28; c.w = 65536; }));
    print("refuse_65536_wide", with([](Case& c) { c.w = 65536; c.h = 8; c.d = 8; c.in.arena_bytes = 1000; }));
    print("refuse_65536_high", with([](Case& c) { c.w = 8; c.h = 65536; c.d = 8; }));
    print("refuse_2p29_pixels", with([](Case& c) { c.w = 32768; c.h = 16384; c.d = 8; c.in.arena_bytes = 1000; }));
    print("refuse_arena", with([](Case& c) { c.in.arena_bytes = (6363 + 64) * 8 - 1; }));
    print("accept_arena", with([](Case& c) { c.in.arena_bytes = (6363 + 64) * 8; }));
    print("refuse_arena_2d", with([](Case& c) { c.is3d = false; c.tiles = {128, 16}; c.in.arena_bytes = 1000; }));
    return 0;
}
