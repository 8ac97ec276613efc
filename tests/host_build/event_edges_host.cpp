// Host build of the part of the 3D frame schedule that says which EVENTS a frame records (fidget_amd/csrc/frame_schedule.hpp: rec_fork,
// records_leaves, waits_leaves, StagingRing, SlotGuard - no HIP, no device) for tests/test_event_edges.py.  Frames are planned as
// tests/host_build/frame_schedule_host.cpp plans them; the driver's waits are modelled here from capi_render.hpp (tile_step: the tile chain
// of slab idx waits for ev_leaves[idx - NC]; render_slabs: the caller's stream waits for the last slab's ev_leaves in an aux_edge frame;
// coarse_levels: the side / tail stream waits for ev_fork under fork_to_side / fork_to_tail).  Then the staging ring: 20 frames, some of
// which end early, against a device that remembers when it read a slot - meant to be built with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "frame_schedule.hpp"

struct Case {
    uint32_t size = 1024;
    int no_column_inv = 0, no_zrep = 0, no_pipeline = 0;
    ScheduleInputs in;
};

// A tape of prospero.vm's kind (frame_schedule_host.cpp)
static TapeFacts prospero_kind() {
    TapeFacts t;
    t.n_ops = 6363; t.n_regs = 72; t.n_choices = 3000;
    t.input_slots = 3;
    t.n_groups = 16;
    for (uint32_t g = 0; g < t.n_groups; g++) t.group[g] = {400, 40, 190};
    t.n_terms = 64; t.n_top = 63; t.chain = true;
    return t;
}
static RenderSetup facts(const Case& c) {
    const TapeFacts t = prospero_kind();
    PlanInputs pin;
    pin.no_column_inv = c.no_column_inv; pin.no_zrep = c.no_zrep; pin.slab_contexts = c.in.slab_contexts;
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
    if (!frame_pipelined(in)) in.frames_queued = false;
    return in;
}
static FrameSchedule plan(const Case& c) { return schedule_frame(facts(c), inputs(c)); }

// ---- the driver's waits -----------------------------------------------------------------------------------------------------
static std::set<int> leaves_waited(const FrameSchedule& F) {
    std::set<int> w;
    for (int idx = 0; idx < F.n_rendered; idx++)
        if (F.pipe && idx >= (int)F.NC) w.insert(idx - (int)F.NC);      // tile_step: the slab context is free again
    if (F.aux_edge && F.n_rendered > 0) w.insert(F.n_rendered - 1);     // render_slabs: the last slab's normals, on the tail stream
    return w;
}
static std::set<int> leaves_recorded(const FrameSchedule& F, bool parents_rule) {
    std::set<int> r;
    for (int idx = 0; idx < F.n_rendered; idx++)
        if (parents_rule ? F.pipe : records_leaves(F, idx)) r.insert(idx);
    return r;
}
// records without a waiter + waits without a record (ev_leaves, ev_fork), + what the schedule's own wait function says against the model
static int violations(const FrameSchedule& F, bool parents_rule = false) {
    int bad = 0;
    const std::set<int> w = leaves_waited(F), r = leaves_recorded(F, parents_rule);
    for (int i : r) bad += !w.count(i);
    for (int i : w) bad += !r.count(i);
    for (int idx = 0; idx < F.n_rendered + 2; idx++) bad += waits_leaves(F, idx) != (F.pipe && idx >= (int)F.NC && idx < F.n_rendered);
    bad += records_leaves(F, -1) || records_leaves(F, F.n_rendered);
    const bool fork_waited = F.fork_to_side || F.fork_to_tail, fork_recorded = parents_rule ? F.pipe : F.rec_fork;
    bad += fork_waited != fork_recorded;
    bad += fork_recorded && !F.pipe;      // (the driver records it with the fork of the slab contexts, which a frame without them does not make)
    return bad;
}
static std::string list(const std::set<int>& s) {
    std::string t;
    for (int i : s) t += (t.empty() ? "" : ",") + std::to_string(i);
    return t.empty() ? "-" : t;
}
static void print(const char* name, const Case& c) {
    const FrameSchedule F = plan(c);
    printf("%s: rendered=%d NC=%u pipe=%d aux_edge=%d fork_to_side=%d fork_to_tail=%d rec_fork=%d leaves=%s waited=%s violations=%d parents_rule=%d rare=%d by_list=%d rare_leaves=%d\n", name,
           F.n_rendered, F.NC, F.pipe, F.aux_edge, F.fork_to_side, F.fork_to_tail, F.rec_fork, list(leaves_recorded(F, false)).c_str(), list(leaves_waited(F)).c_str(), violations(F),
           violations(F, true), F.rare, F.by_list, F.rare_leaves);
}

// ---- the staging ring --------------------------------------------------------------------------------------------------------
// The device of the model: one clock; a slot remembers when k_frame_begin that reads it was queued and when its event was recorded last.
struct Device {
    uint64_t clock = 0, read_at[FH_STAGING_SLOTS] = {}, guard_at[FH_STAGING_SLOTS] = {};
    std::vector<unsigned char> mem[FH_STAGING_SLOTS];
};
struct Record {
    Device* dev = nullptr; StagingRing* ring = nullptr; uint32_t slot = 0; int* records = nullptr;
    void operator()() const { dev->guard_at[slot] = ++dev->clock; ring->used[slot] = true; ++*records; }
};
enum Exit { LEAVES_ROOT, STAYS, CANCELLED_EARLY, LAUNCH_FAILED, REFUSED_BEFORE_LAUNCH };
// One frame as upload_frame / coarse_levels / render3d_frame go about the slot; returns the violations it saw
static int frame(Device& dev, StagingRing& ring, Exit how, size_t bytes, int& records, int& armed) {
    int bad = 0;
    const uint32_t slot = ring.take();
    // the slot's next user: waits for the slot's event, if one counts - and then no read may be younger than that record
    if (ring.used[slot]) bad += dev.guard_at[slot] < dev.read_at[slot];
    else bad += dev.read_at[slot] != 0;      // (read once and never guarded)
    if (dev.mem[slot].size() < bytes) dev.mem[slot].assign(bytes + 4096, 0);
    memset(dev.mem[slot].data(), (int)(ring.next & 0xff), bytes);      // the frame's state and root groups
    SlotGuard<Record> guard(Record{});
    if (how == REFUSED_BEFORE_LAUNCH) return bad;      // (hold_bound refused: nothing queued, nothing armed)
    dev.read_at[slot] = ++dev.clock;                   // k_frame_begin queued
    guard.record_now = Record{&dev, &ring, slot, &records}; guard.arm(); armed++;
    if (how == LAUNCH_FAILED || how == CANCELLED_EARLY) return bad;     // (the guard's destructor)
    ++dev.clock;                                       // the root level
    if (how == LEAVES_ROOT) { guard.record(); ++dev.clock; }     // the hop's record beside it
    ++dev.clock;                                       // slabs, k_finish3d, ev_done
    guard.record();
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
    print("default_host_output", with([](Case& c) { c.in.out_is_device = false; }));
    print("default_profiling", with([](Case& c) { c.in.profiling = true; }));
    print("big_queued", with([](Case& c) { c.size = 2048; }));
    print("default_rare_seen", with([](Case& c) { c.in.rare_seen = 1; }));
    print("default_column_walk3", with([](Case& c) { c.in.column_walk = 3; }));
    // more slabs than slab contexts: every slab of a 2048^3 frame rendered (no_zrep 3: four), two or three contexts; queued (no aux_edge
    // where the normals stay on the caller's stream) and with a host output (aux_edge)
    for (uint32_t nc : {1u, 2u, 3u}) {
        print(("slabs4_nc" + std::to_string(nc) + "_general_queued").c_str(), with([&](Case& c) { c.size = 2048; c.no_zrep = 3; c.no_column_inv = 1; c.in.slab_contexts = nc; }));
        print(("slabs4_nc" + std::to_string(nc) + "_host_output").c_str(), with([&](Case& c) { c.size = 2048; c.no_zrep = 3; c.in.out_is_device = false; c.in.slab_contexts = nc; }));
        print(("slabs4_nc" + std::to_string(nc) + "_default_queued").c_str(), with([&](Case& c) { c.size = 2048; c.no_zrep = 3; c.in.slab_contexts = nc; }));
    }
    long n = 0, bad = 0, bad_parent = 0;
    for (uint32_t size : {64u, 128u, 256u, 512u, 1024u, 2048u})
        for (int bits = 0; bits < 256; bits++)
            for (int w = 0; w < 4; w++)
                for (int zr : {0, 1, 2, 3})
                    for (uint32_t nc : {1u, 2u, 3u, 4u}) {
                        Case c = d;
                        c.size = size; c.in.column_walk = w; c.no_zrep = zr; c.in.slab_contexts = nc;
                        c.no_column_inv = bits & 1; c.no_pipeline = (bits >> 1) & 1; c.in.profiling = (bits >> 2) & 1; c.in.out_is_device = !((bits >> 3) & 1);
                        c.in.rare_seen = (bits >> 4) & 1; c.in.frames_queued = (bits >> 5) & 1; c.in.pre_turn = (bits >> 6) & 1; c.in.huge = (bits >> 7) & 1;
                        const FrameSchedule F = plan(c);
                        const int v = violations(F);
                        if (v && bad < 5) print("VIOLATION", c);
                        n++; bad += v != 0; bad_parent += violations(F, true) != 0;
                    }
    printf("sweep: %ld schedules, %ld violations, %ld under the rule 'recorded whenever pipe'\n", n, bad, bad_parent);

    // the staging ring: 20 frames, the ring of 8 comes round twice; early exits of every kind in the middle; slots grow (a larger frame)
    Device dev;
    StagingRing ring;
    int records = 0, armed = 0, sbad = 0;
    for (int i = 0; i < 20; i++) {
        const Exit how = i == 9 ? CANCELLED_EARLY : i == 10 ? LAUNCH_FAILED : i == 11 ? REFUSED_BEFORE_LAUNCH : i % 3 == 2 ? STAYS : LEAVES_ROOT;
        sbad += frame(dev, ring, how, (size_t)3000 + (i >= 12 ? 9000 : 0) + 64 * (size_t)i, records, armed);
    }
    // at the end every read lies in front of its slot's record
    for (uint32_t s = 0; s < FH_STAGING_SLOTS; s++) sbad += dev.read_at[s] != 0 && !(ring.used[s] && dev.guard_at[s] > dev.read_at[s]);
    printf("staging: frames=20 armed=%d records=%d violations=%d\n", armed, records, sbad);
    return bad != 0 || sbad != 0 || records != armed;
}
