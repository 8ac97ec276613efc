// Host build of the 3D frame schedule (fidget_amd/csrc/frame_schedule.hpp: no HIP, no device) for tests/test_frame_schedule.py:
// plans named frames as the driver does (frame_plan.hpp: column_facts, choose_tiles_3d, plan_frame, plan_linked_prune) for a tape of
// prospero.vm's kind (every assembly path on, term groups, linked prune) and prints their schedules, one line each; then a sweep for
// the edge property.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "frame_schedule.hpp"

struct Case {
    uint32_t size = 1024;
    int no_column_inv = 0, no_zrep = 0, no_pipeline = 0;
    ScheduleInputs in;
};

// A tape of prospero.vm's kind: 6363 ops, 72 registers, 3000 choices, reads x and y only; term groups, links and a root chain present
static TapeFacts prospero_kind() {
    TapeFacts t;
    t.n_ops = 6363; t.n_regs = 72; t.n_choices = 3000;
    t.input_slots = 3;
    t.n_groups = 16;
    for (uint32_t g = 0; g < t.n_groups; g++) t.group[g] = {400, 40, 190};
    t.n_terms = 64; t.n_top = 63; t.chain = true;
    return t;
}
// What the driver leaves in a RenderSetup for a size^3 frame of that tape (camera: identity; x, y, z on slots 0, 1, 2): render3d_frame's steps
static RenderSetup facts(const Case& c) {
    const TapeFacts t = prospero_kind();
    PlanInputs pin;
    pin.no_column_inv = c.no_column_inv; pin.no_zrep = c.no_zrep;
    RenderSetup R;
    memset(&R.S, 0, sizeof(R.S));
    FhRender& P = R.S.P;
    P.width = P.height = P.depth = c.size;
    for (int i = 0; i < 4; i++) P.mat[5 * i] = 1.0f;
    for (uint32_t s = 0; s < FH_MAX_INPUTS; s++) P.in_kind[s] = s < 3 ? s : 3;
    column_facts(P, t, pin, R);
    const uint32_t size[3] = {c.size, c.size, c.size};
    const TileChoice T = choose_tiles_3d(nullptr, 0, size, 1, 1, R.column_inv, pin.root32_max, pin.no_zrep, linked_root_tape(t, pin));
    const PlanStatus ps = plan_frame(t, pin, true, T.ts, PartSpec{}, R);
    if (ps.status) { fprintf(stderr, "plan refused: %s\n", ps.msg); exit(2); }
    if (R.groups) plan_linked_prune(t, pin, true, 63, R);
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
