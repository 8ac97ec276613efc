// Host build of the 3D frame schedule (fidget_amd/csrc/frame_schedule.hpp: no HIP, no device) for tests/test_frame_schedule.py:
// fills the facts of named frames - the part of prepare()'s arithmetic the schedule reads, for a tape of prospero.vm's kind (every
// assembly path on, term groups, linked prune) - and prints their schedules, one line each; then a sweep for the edge property.
#include <stdio.h>
#include <string.h>

#include <string>

#include "frame_schedule.hpp"

struct Case {
    uint32_t size = 1024;
    int no_column_inv = 0, no_zrep = 0, no_pipeline = 0;
    ScheduleInputs in;
};

// What column_setup + choose_tiles_3d + prepare leave in a RenderSetup for a size^3 frame of a tape that reads no z (camera: identity)
static RenderSetup facts(const Case& c) {
    RenderSetup R;
    memset(&R.S, 0, sizeof(R.S));
    FhRender& P = R.S.P;
    P.width = P.height = P.depth = c.size;
    R.xy_fixed = true; R.root_invariant = !c.no_column_inv;
    R.column_inv = R.xy_fixed && R.root_invariant && (c.no_zrep == 0 || c.no_zrep == 3);
    const uint32_t size[3] = {c.size, c.size, c.size};
    const TileChoice T = choose_tiles_3d(nullptr, 0, size, 1, 1, R.column_inv, 4096, c.no_zrep, true);
    const std::vector<uint32_t>& ts = T.ts;
    P.n_levels = (uint32_t)ts.size();
    for (size_t i = 0; i < ts.size(); i++) P.tiles[i] = ts[i];
    P.max_regs = 72; P.max_choices = 3000;
    P.roots_x = P.roots_y = (c.size + ts[0] - 1) / ts[0];
    const uint32_t n_layers = (c.size + ts[0] - 1) / ts[0];
    const bool prepass_ok = ts.size() >= 2 && n_layers <= FH_MAX_SLABS;
    uint32_t SL = prepass_ok ? 4 * std::max<uint32_t>(1, 128 / ts[0]) : 1u;      // (option slab_layers = 4; as prepare())
    while (SL > 1 && (ts[0] * SL / 8 > 64 || SL * 2 > n_layers)) SL >>= 1;
    P.slab = ts[0] * SL;
    R.n_slabs = (c.size + P.slab - 1) / P.slab; R.n_layers = n_layers;
    R.S.pre_levels = prepass_ok ? std::min<uint32_t>(2, (uint32_t)ts.size() - 1) : 0;
    R.slab_lo = 0; R.slab_hi = prepass_ok ? (n_layers + SL - 1) / SL : n_layers;
    R.tl = 64; R.split = R.asm_tiles = R.asm_points = R.asm_normals = R.prune1 = R.groups = R.prune2 = true;
    R.exp_levels = std::min(R.S.pre_levels, 1u);
    R.root_zrep = R.S.pre_levels > 0 && R.column_inv;
    R.front_only = R.root_zrep && c.no_zrep == 0;
    R.slab_stop = R.front_only ? R.slab_hi - 1 : R.slab_lo;
    R.groups_per_slab = (P.roots_x * P.roots_y + 63) / 64;
    R.n_footprints = ((c.size + 7) / 8) * ((c.size + 7) / 8);
    R.table_words = R.n_footprints * (P.slab / 8);
    R.zrep = R.split && R.S.pre_levels > 0 && R.xy_fixed && !c.no_column_inv && c.no_zrep != 1;
    R.lds_tiles_big = 89856; R.lds_tiles_mid = 46336; R.lds_tiles_small = 20736; R.lds_points_big = 72 * 64 * 4; R.lds_normals_big = 72 * 64 * 16; R.lds_normals_small = 32 * 64 * 16;
    R.S.leaf_asm_regs = 40; R.S.norm_asm_regs = 40;
    return R;
}
static ScheduleInputs inputs(const Case& c) {
    ScheduleInputs in = c.in;
    in.no_zrep = c.no_zrep;
    if (c.no_pipeline) in.use_pipeline = false;
    if (!frame_pipelined(in)) in.frames_queued = false;      // (the driver only looks when the frame is pipelined)
    return in;
}

static const char* role(Role r) { static const char* const n[] = {"CALLER", "PRE", "SIDE", "TAIL"}; return r < N_ROLES ? n[r] : "?"; }
static std::string level_text(const LevelPlan& L) {
    static const char* const path[] = {"MONO", "GROUPS", "ASM", "HIP"};
    std::string s = path[L.path];
    if (L.exp) s += "+exp";
    if (L.v32) s += "+v32";
    if (L.small_lds) s += "+small";
    if (L.v64) s += L.both_lists ? "+v64both" : "+v64";
    if (L.mid) s += "+mid";
    if (L.rest) s += "+rest";
    if (L.rare) s += "+rare";
    if (L.fork_big) s += "+fork";
    return s;
}
static void print(const char* name, const Case& c) {
    const RenderSetup R = facts(c);
    const ScheduleInputs in = inputs(c);
    const FrameSchedule F = schedule_frame(R, in);
    static const char* const walk[] = {"HIP", "LIST", "COLUMNS", "BLOCKS"};
    printf("%s:", name);
    printf(" tiles=");
    for (uint32_t l = 0; l < R.S.P.n_levels; l++) printf("%s%u", l ? "/" : "", R.S.P.tiles[l]);
    printf(" slab=%u slabs=%u rendered=%d NC=%u fpipe=%d lone=%d alt_pre=%d takes_turn=%d", R.S.P.slab, R.slab_hi - R.slab_lo, F.n_rendered, F.NC, F.fpipe, F.lone, F.alt_pre, F.takes_turn);
    printf(" root=%s l1_flags=%s l1=%s fork_on=%s tiles_on=%s lists=%s leaf=%s normals=%s", role(F.root), role(F.l1_flags), role(F.l1), role(F.fork_on), role(F.tiles), role(F.lists),
           role(F.leaf), role(F.normals));
    printf(" pipe=%d tiles_first=%d fork_to_side=%d fork_to_tail=%d ev_pre=%d pre_implied=%d aux_edge=%d", F.pipe, F.tiles_first, F.fork_to_side, F.fork_to_tail, F.ev_pre, F.pre_implied, F.aux_edge);
    printf(" rare=%d by_list=%d walk=%s g=%u list_waves=%u table_words=%u reset_blocks=%d", F.rare, F.by_list, walk[F.leaf_walk], F.g, F.list_waves, F.table_words, F.reset_blocks);
    for (uint32_t l = 0; l < R.S.P.n_levels; l++) printf(" L%u=%s@%s", l, level_text(F.level[l]).c_str(), role(F.level[l].rest_on));
    printf("\n");
}

// Every stage that runs behind another role's work has an event edge from it or is on the same role
static int violations(const FrameSchedule& F, bool coarse_l1) {
    int bad = 0;
    const Role roles[] = {F.root, F.l1_flags, F.l1, F.fork_on, F.tiles, F.lists, F.leaf, F.normals};
    for (Role r : roles) bad += r >= N_ROLES;
    (void)coarse_l1;      // (root -> l1_flags -> l1 -> fork_on: consecutive stages, the driver's hop() records an event wherever the role changes)
    const bool to_caller = F.fork_on == CALLER || F.ev_pre || (F.pre_implied && F.pipe && F.tiles == F.fork_on && F.n_rendered > 0);
    bad += !to_caller;
    if (F.tiles != F.fork_on) bad += !((F.tiles == SIDE && F.fork_to_side) || (F.tiles == TAIL && F.fork_to_tail) || (F.tiles == CALLER && to_caller));
    if (F.leaf != F.tiles) bad += !F.pipe;
    if (F.lists != F.tiles) bad += !(F.lists == F.leaf ? F.pipe : F.aux_edge);
    if (F.normals != F.leaf) bad += !F.aux_edge;
    if (F.normals != CALLER) bad += !F.aux_edge;      // (k_finish3d, on the caller's stream, waits for the last slab's ev_leaves)
    if (F.leaf != CALLER) bad++;
    return bad;
}

int main() {
    Case d;      // prospero.vm 1024^3, default options, device output, queued behind another frame
    d.in.frames_queued = true; d.in.rare_seen = 0; d.in.last_leaves = 5500;
    auto with = [&](auto f) { Case c = d; f(c); return c; };
    print("default_queued", d);
    print("default_queued_turn", with([](Case& c) { c.in.pre_turn = 1; }));
    print("default_alone", with([](Case& c) { c.in.frames_queued = false; }));
    print("general_queued", with([](Case& c) { c.no_column_inv = 1; }));
    print("general_alone", with([](Case& c) { c.no_column_inv = 1; c.in.frames_queued = false; }));
    print("big_queued", with([](Case& c) { c.size = 2048; }));
    print("big_alone", with([](Case& c) { c.size = 2048; c.in.frames_queued = false; }));
    for (int g = 0; g < 3; g++) {
        const char* const tag[] = {"default", "general", "big"};
        auto kind = [&](Case& c) { if (g == 1) c.no_column_inv = 1; if (g == 2) c.size = 2048; };
        print((std::string(tag[g]) + "_no_pipeline").c_str(), with([&](Case& c) { kind(c); c.no_pipeline = 1; }));
        print((std::string(tag[g]) + "_profiling").c_str(), with([&](Case& c) { kind(c); c.in.profiling = true; }));
        // (a lane is a child context with no_pipeline = 1 that renders into an image of its own on the device)
        print((std::string(tag[g]) + "_lane").c_str(), with([&](Case& c) { kind(c); c.no_pipeline = 1; c.in.out_is_device = true; c.in.frames_queued = false; }));
        print((std::string(tag[g]) + "_host_output").c_str(), with([&](Case& c) { kind(c); c.in.out_is_device = false; }));
        print((std::string(tag[g]) + "_rare_seen").c_str(), with([&](Case& c) { kind(c); c.in.rare_seen = 1; }));
        for (int w : {0, 2, 3}) print((std::string(tag[g]) + "_column_walk" + std::to_string(w)).c_str(), with([&](Case& c) { kind(c); c.in.column_walk = w; }));
    }
    int n = 0, bad = 0;
    for (uint32_t size : {64u, 128u, 256u, 512u, 1024u, 2048u})
        for (int bits = 0; bits < 256; bits++)
            for (int w = 0; w < 4; w++)
                for (int zr : {0, 1, 2, 3}) {
                    Case c = d;
                    c.size = size; c.in.column_walk = w; c.no_zrep = zr;
                    c.no_column_inv = bits & 1; c.no_pipeline = (bits >> 1) & 1; c.in.profiling = (bits >> 2) & 1; c.in.out_is_device = !((bits >> 3) & 1);
                    c.in.rare_seen = (bits >> 4) & 1; c.in.frames_queued = (bits >> 5) & 1; c.in.pre_turn = (bits >> 6) & 1; c.in.huge = (bits >> 7) & 1;
                    const RenderSetup R = facts(c);
                    const int v = violations(schedule_frame(R, inputs(c)), R.S.pre_levels > 1);
                    if (v && bad < 5) print("VIOLATION", c);
                    n++; bad += v != 0;
                }
    printf("sweep: %d schedules, %d violations\n", n, bad);
    return bad != 0;
}
