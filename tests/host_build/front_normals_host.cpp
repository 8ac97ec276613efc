// Host build of the rule that says which 3D frames run their normals kernels (fidget_amd/csrc/frame_schedule.hpp FrameSchedule::normals_on - no
// HIP, no device) for tests/test_front_normals.py: not a WHOLE front-slab-only frame, every hit of which k_finish3d clamps to (0, 0, 1, depth).
// Frames are planned as tests/host_build/frame_schedule_host.cpp plans them, for tapes of three kinds, whole and in parts; the driver's
// launches behind the leaf kernel are modelled from capi_render.hpp render_slabs (normals_work, or k_rare_leaves3d alone).  Prints named frames
// and a sweep over all combinations of the schedule inputs: the rule against its restatement, the points of large leaves never lost, and
// nothing else of a schedule moved by it.  Meant to be built with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "frame_schedule.hpp"

enum Kind { PLAIN, TRANSCENDENTAL, READS_Z, SMALL };
struct Case {
    uint32_t w = 1024, h = 1024, d = 1024;
    Kind kind = PLAIN;
    int no_column_inv = 0, no_zrep = 0, no_pipeline = 0, no_asm = 0;
    float tilt = 0.0f;      // a z coefficient in the model's y row: the camera tilted about x
    PartSpec part;
    ScheduleInputs in;
};

// prospero.vm's kind (frame_schedule_host.cpp); the same with a transcendental opcode; the same reading z; a tape within the leaf kernel's file
static TapeFacts tape_of(Kind k) {
    TapeFacts t;
    t.n_ops = 6363; t.n_regs = k == SMALL ? 30 : 72; t.n_choices = 3000;
    t.input_slots = k == READS_Z ? 7 : 3;
    t.n_groups = 16;
    for (uint32_t g = 0; g < t.n_groups; g++) t.group[g] = {400, 30, 190};
    t.n_terms = 64; t.n_top = 63; t.chain = true;
    if (k == TRANSCENDENTAL) t.asm_ok = false;
    return t;
}
static RenderSetup facts(const Case& c) {
    const TapeFacts t = tape_of(c.kind);
    PlanInputs pin;
    pin.no_column_inv = c.no_column_inv; pin.no_zrep = c.no_zrep; pin.slab_contexts = c.in.slab_contexts; pin.use_asm = !c.no_asm;
    RenderSetup R;
    memset(&R.S, 0, sizeof(R.S));
    FhRender& P = R.S.P;
    P.width = c.w; P.height = c.h; P.depth = c.d;
    for (int i = 0; i < 4; i++) P.mat[5 * i] = 1.0f;
    P.mat[6] = c.tilt;
    for (uint32_t s = 0; s < FH_MAX_INPUTS; s++) P.in_kind[s] = s < 3 ? s : 3;
    column_facts(P, t, pin, R);
    const uint32_t size[3] = {c.w, c.h, c.d};
    const TileChoice T = choose_tiles_3d(nullptr, 0, size, c.part.n_shards * c.part.nx * c.part.ny, c.part.nz, R.column_inv, pin.root32_max, pin.no_zrep, linked_root_tape(t, pin));
    const PlanStatus ps = plan_frame(t, pin, true, T.ts, c.part, R);
    if (ps.status) { fprintf(stderr, "plan refused: %s\n", ps.msg); exit(2); }
    if (R.groups) plan_linked_prune(t, pin, true, 63, R);
    return R;
}
static bool whole(const Case& c) { return c.part.n_shards == 1 && c.part.nx * c.part.ny * c.part.nz == 1; }
static ScheduleInputs inputs(const Case& c) {
    ScheduleInputs in = c.in;
    in.no_zrep = c.no_zrep;
    in.whole = whole(c);
    if (c.no_pipeline) in.use_pipeline = false;
    if (!frame_pipelined(in)) in.frames_queued = false;
    return in;
}

// What a slab launches behind its leaf kernel (capi_render.hpp render_slabs): the normals kernels with what rides on them, or k_rare_leaves3d alone
struct Behind { bool normals, rare_leaves; };
static Behind behind_leaf_kernel(const FrameSchedule& F) { return Behind{F.normals_on, F.rare_leaves}; }
// The slabs a frame renders lie at the volume's top and are all of it that is rendered: the rule's reason, restated from the plan's numbers
static bool every_hit_is_clamped(const RenderSetup& R, const Case& c) {
    return whole(c) && R.column_inv && c.no_zrep == 0 && R.slab_stop + 1 == R.slab_hi && R.slab_hi == R.n_slabs && R.root_zrep;
}
// every field of a schedule but normals_on as text
static std::string rest_of(const FrameSchedule& F, uint32_t n_levels) {
    char b[1024];
    snprintf(b, sizeof b, "%d%d%d%d|%d%d%d%d%d%d%d%d|%d%d%d%d%d%d|%d%d%d%u|%d %d %d|%d%u|%d%d%d%u|%d|%u %u %d", F.fpipe, F.lone, F.alt_pre, F.takes_turn, F.root, F.l1_flags, F.l1, F.fork_on, F.tiles,
             F.lists, F.leaf, F.normals, F.fork_to_side, F.fork_to_tail, F.ev_pre, F.pre_implied, F.aux_edge, F.rec_fork, F.coarse, F.pipe, F.tiles_first, F.NC, F.slab_first, F.slab_stop,
             F.n_rendered, F.rare, F.rare_stride, (int)F.leaf_walk, F.by_list, F.by_columns, F.g, F.rare_leaves, F.list_waves, F.table_words, F.reset_blocks);
    std::string s = b;
    for (uint32_t l = 0; l < n_levels; l++) {
        const LevelPlan& L = F.level[l];
        snprintf(b, sizeof b, " L%d%d%d%d%d%d%d%d%d%d%d%d%u%d", (int)L.path, L.rest_on, L.per_slab, L.exp, L.v32, L.small_lds, L.v64, L.both_lists, L.mid, L.rest, L.rare, L.fork_big, L.rare_stride, L.push_mul);
        s += b;
    }
    return s;
}
static void print(const char* name, const Case& c) {
    const RenderSetup R = facts(c);
    const FrameSchedule F = schedule_frame(R, inputs(c));
    const Behind b = behind_leaf_kernel(F);
    printf("%s: tiles=%u/%u front_only=%d column_inv=%d whole=%d rendered=%d normals_on=%d by_list=%d rare=%d rare_leaves=%d normals_launches=%d rare_leaves_launch=%d clamped=%d\n", name,
           R.S.P.tiles[0], R.S.P.tiles[1], R.front_only, R.column_inv, whole(c), F.n_rendered, F.normals_on, F.by_list, F.rare, F.rare_leaves, b.normals, b.rare_leaves, every_hit_is_clamped(R, c));
}

int main() {
    Case d;      // prospero.vm's kind at 1024^3, default options, device output, queued behind another frame
    d.in.frames_queued = true; d.in.rare_seen = 0; d.in.last_leaves = 5500;
    auto with = [&](auto f) { Case c = d; f(c); return c; };
    print("default_queued", d);
    print("default_alone", with([](Case& c) { c.in.frames_queued = false; }));
    print("default_host_output", with([](Case& c) { c.in.out_is_device = false; }));
    print("default_profiling", with([](Case& c) { c.in.profiling = true; }));
    print("default_lane", with([](Case& c) { c.no_pipeline = 1; c.in.frames_queued = false; }));
    print("default_rare_seen", with([](Case& c) { c.in.rare_seen = 1; }));
    print("default_by_table", with([](Case& c) { c.in.column_walk = 3; }));
    print("default_no_asm", with([](Case& c) { c.no_asm = 1; }));
    for (uint32_t n : {64u, 128u, 256u, 512u, 2048u}) print(("size_" + std::to_string(n)).c_str(), with([&](Case& c) { c.w = c.h = c.d = n; }));
    print("size_96x64x40", with([](Case& c) { c.w = 96; c.h = 64; c.d = 40; }));
    print("small_tape", with([](Case& c) { c.kind = SMALL; }));
    print("transcendental", with([](Case& c) { c.kind = TRANSCENDENTAL; }));
    print("shard", with([](Case& c) { c.part.n_shards = 2; }));
    print("block_xy", with([](Case& c) { c.part.nx = c.part.ny = 2; }));
    print("block_z_front", with([](Case& c) { c.part.nz = 2; c.part.iz = 1; }));
    print("block_z_back", with([](Case& c) { c.part.nz = 2; c.part.iz = 0; }));
    print("every_slab", with([](Case& c) { c.no_zrep = 3; }));
    print("no_column_inv", with([](Case& c) { c.no_column_inv = 1; }));
    print("tilted", with([](Case& c) { c.tilt = 0.25f; }));
    print("reads_z", with([](Case& c) { c.kind = READS_Z; }));
    long n = 0, off = 0, bad_rule = 0, bad_points = 0, moved = 0;
    for (uint32_t size : {64u, 256u, 1024u, 2048u})
        for (int bits = 0; bits < 256; bits++)
            for (int w = 0; w < 4; w++)
                for (int zr : {0, 1, 2, 3})
                    for (int part = 0; part < 4; part++)
                        for (Kind k : {PLAIN, SMALL, TRANSCENDENTAL, READS_Z}) {
                            Case c = d;
                            c.w = c.h = c.d = size; c.in.column_walk = w; c.no_zrep = zr; c.kind = k;
                            if (part == 1) c.part.n_shards = 2;
                            if (part == 2) { c.part.nz = 2; c.part.iz = 0; }
                            if (part == 3) { c.part.nx = 2; c.part.ix = 1; }
                            c.no_column_inv = bits & 1; c.no_pipeline = (bits >> 1) & 1; c.in.profiling = (bits >> 2) & 1; c.in.out_is_device = !((bits >> 3) & 1);
                            c.in.rare_seen = (bits >> 4) & 1; c.in.frames_queued = (bits >> 5) & 1; c.in.pre_turn = (bits >> 6) & 1; c.in.huge = (bits >> 7) & 1;
                            const RenderSetup R = facts(c);
                            const FrameSchedule F = schedule_frame(R, inputs(c));
                            const Behind b = behind_leaf_kernel(F);
                            n++; off += !F.normals_on;
                            // no normals exactly where every hit is clamped, and never in a part of a frame
                            bad_rule += F.normals_on == every_hit_is_clamped(R, c);
                            bad_rule += !F.normals_on && !whole(c);
                            // the points of the leaves beyond the leaf kernel's file are k_rare_leaves3d's in a rare_leaves frame: launched with or without the normals
                            bad_points += F.rare_leaves && !b.rare_leaves;
                            // nothing else of the schedule depends on `whole` but the root levels' turns (alt_pre), which no whole frame changes: the same frame as a
                            // part differs from it only there and in normals_on - so a whole frame's schedule, normals_on aside, is what it was
                            if (whole(c)) {
                                ScheduleInputs as_part = inputs(c);
                                as_part.whole = false;
                                FrameSchedule G = schedule_frame(R, as_part);
                                if (!F.alt_pre) moved += rest_of(F, R.S.P.n_levels) != rest_of(G, R.S.P.n_levels) || G.normals_on != true;
                            }
                        }
    printf("sweep: %ld schedules, %ld without normals, %ld against the rule, %ld large leaves without their points, %ld moved otherwise\n", n, off, bad_rule, bad_points, moved);
    return bad_rule != 0 || bad_points != 0 || moved != 0;
}
