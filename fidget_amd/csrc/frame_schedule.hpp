// The schedule of a 3D frame: which stream every stage goes to, which launches exist and how the slabs are arranged - decided ONCE per
// frame by schedule_frame() below from facts alone: the frame's plan (frame_plan.hpp: the RenderSetup that plan_frame and plan_linked_prune
// leave), a few options, what the context has, three observations of the moment; capi_render.hpp runs it.  No HIP call, no global: this
// header compiles with plain g++ next to render_state.h, and tests/test_frame_schedule.py pins the schedules of named frames, planned by
// the same functions the driver calls (tests/host_build/frame_schedule_host.cpp).
// How to read one: a frame is root level -> level 1 (flags, evaluate) -> `fork_on` (flags of the parked parents, frame mark, fork of the
// slab contexts) -> per slab: tile chain, footprint lists, leaf kernel, normals -> k_finish3d on the caller's stream.  Wherever two
// consecutive stages have different roles there is an event between them; the edges that are not a plain hop are the fork_* / ev_pre fields.
// An event is recorded where somebody waits for it and nowhere else: a record between two dependent kernels of one stream costs that chain
// a gap and the host a runtime call (profiles/event_edges), so WHICH events a frame records is part of its schedule - rec_fork and
// records_leaves() below, next to the fields that say who waits - and the driver keeps no condition of its own.  The one record that guards
// host memory, the pinned staging slot's, is made where the root stream leaves the root level or the frame ends (SlotGuard, at the end).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "frame_plan.hpp"
#include "render_state.h"

// register-file shapes of the VGPR tile kernels (gen_tilesv.py): registers, choices
static const uint32_t V32_REGS = 32, V32_CHOICES = 256, V64_REGS = 64, V64_CHOICES = 512;
// Rare mode: blocks per folded launch (a slab context's blocks keep their register files in rare_scratch: capi_render.hpp rare_file)
static const uint32_t FH_RARE_BLOCKS = 8;

// ---- the schedule ----------------------------------------------------------------------------------------------------------
// Which stream of the context: the caller's, the pre-pass stream, the side stream (high priority), the tail stream
enum Role : uint8_t { CALLER = 0, PRE, SIDE, TAIL, N_ROLES };

struct ScheduleInputs {
    int no_tiles_v = 0, no_zrep = 0, column_walk = 1, column_group = 2;      // options (FH_OPTION_LIST)
    // what the context has: its switches, the streams that exist, the pinned host words, slab contexts
    bool frame_pipeline = true, use_pipeline = true, profiling = false, has_side = true, has_tail = true, has_flags = true;
    uint32_t slab_contexts = 4;
    // the call; huge: the tape's register files live in HBM - nothing of the frame runs beside anything else; whole: not a part of a frame (shard, block)
    bool out_is_device = true, huge = false, whole = true;
    // observed when the frame is queued
    bool frames_queued = false;                    // the frame before this one is still under way (looked at only if frame_pipelined())
    uint32_t pre_turn = 0;                         // whose turn the alternating root level is
    uint32_t rare_seen = 1, last_leaves = 0;       // host_flags[2], host_flags[3]: the last finished frame met a large tape; its leaf count
};

// One tile level (launch_tiles): which evaluate + prune launches it makes, between set-up and push
struct LevelPlan {
    enum Path : uint8_t { MONO, GROUPS, ASM, HIP } path = MONO;   // monolithic k_tiles; root level by term groups + linked prune; assembly tile kernels; HIP tile kernels
    Role rest_on = CALLER;   // where the launches behind fh_tiles_v64 (LDS layouts' rest, prune, push) go: the level's own role but for level 1 of a `tiles_first` frame
    bool per_slab = false, exp = false;    // a level of the per-slab chains (not of the pre-pass); the forward pass exports its choices, the prune runs as one wave per child (fh_prune1)
    // the small slot list: fh_tiles_v32, or fh_tiles with the small LDS layout (neither: both lists in fh_tiles_v64); fh_tiles_v64 for the other list (or both)
    bool v32 = false, small_lds = false, v64 = false, both_lists = false;
    bool mid = false, rest = false;        // fh_tiles with the medium / the root-sized LDS layout
    bool rare = false;       // rare mode: nothing for the other list, FH_RARE_BLOCKS more blocks of k_tpush3d
    bool fork_big = false;   // the other list's launches run on the side stream beside the small list's (ev_rest_fork / ev_rest_join)
    uint32_t rare_stride = 0; int push_mul = 2;      // the frame's FrameSchedule::rare_stride, for the push kernel; waves per CU of the leaf level's push (FH_PUSH_MUL: tools/build_lib_variant.py)
};

struct FrameSchedule {
    bool fpipe = false, lone = false, alt_pre = false, takes_turn = false;
    // roles: upload + root level; level 1's flags and its evaluate launches; what follows level 1 / the root push (flags, frame mark, fork);
    // the slabs' tile chains; footprint lists; leaf kernel; normals
    Role root = CALLER, l1_flags = CALLER, l1 = CALLER, fork_on = CALLER, tiles = CALLER, lists = CALLER, leaf = CALLER, normals = CALLER;
    // edges that are not a hop between consecutive stages: ev_fork to the side / tail stream, ev_pre to the caller's stream - or implied by
    // the first tile chain's event; per slab, if `pipe`, ev_tiles (tile chain -> lists, leaf kernel); ev_aux (leaf kernel -> normals), ev_leaves (context free, image complete)
    bool fork_to_side = false, fork_to_tail = false, ev_pre = false, pre_implied = false, aux_edge = false;
    bool rec_fork = false;      // ev_fork is recorded: the side or the tail stream waits for it (a frame whose tile chain runs where the fork went records none)
    // there is a pre-pass (and something to render); slab contexts in flight, NC of them; every slab's tile chain queued before the first slab's tail work
    bool coarse = false, pipe = false, tiles_first = false; uint32_t NC = 1;
    int slab_first = 0, slab_stop = 0, n_rendered = 0;      // slabs rendered: slab_first down to slab_stop
    bool rare = false; uint32_t rare_stride = 0;            // rare mode; bytes of a rare block's register file
    enum LeafWalk : uint8_t { HIP_LEAVES, BY_LIST, BY_COLUMNS, BY_BLOCKS } leaf_walk = HIP_LEAVES;
    bool by_list = false, by_columns = false; uint32_t g = 0;      // the leaf kernel's walk; group of 2^g layers
    bool rare_leaves = false;    // rare mode of a by_list frame: ONE launch (k_rare_leaves3d) for the points and the normals of the leaves beyond the leaf kernel's file
    uint32_t list_waves = 0, table_words = 0; int reset_blocks = 1;
    bool normals_on = true;      // the slabs' normals kernels run: not in a whole front-slab-only frame, whose hits are all clamped (below; FH_EXP_SKIP_NORMALS)
    LevelPlan level[FH_MAX_LEVELS];
};

static bool frame_pipelined(const ScheduleInputs& in) { return in.frame_pipeline && in.use_pipeline && !in.profiling && in.out_is_device && !in.huge; }

// `on`: the role the level starts on; `rest_on`: see LevelPlan (== on for every level but one)
static LevelPlan plan_level(const RenderSetup& R, const ScheduleInputs& in, int level, bool is3d, uint32_t rare_stride, Role on, Role rest_on) {
    LevelPlan L;
#ifdef FH_PUSH_MUL
    L.push_mul = FH_PUSH_MUL;
#endif
    L.rare_stride = rare_stride; L.rest_on = rest_on;
    const uint32_t pre = R.S.pre_levels, l = (uint32_t)level;
    const FhRender& P = R.S.P;
    if (!R.split) return L;
    L.per_slab = pre > 0 && l >= pre;
    // pre-pass levels: long tapes, few parents -> the forward pass exports its choices and the prune runs as one wave per child (fh_prune1)
    L.exp = R.prune1 && l < R.exp_levels;      // level 0 only: 8 parents, 6363-op tape (measured)
    // Rare mode (schedule_frame): at a per-slab level the two launches for parents outside the small slot list are not made; the push kernel's last
    // blocks evaluate such parents in C++ (none, nearly always)
    L.rare = rare_stride && is3d && R.asm_tiles && !in.no_tiles_v && level > 0 && L.per_slab && !L.exp;
    if (R.groups && level == 0) { L.path = LevelPlan::GROUPS; return L; }
    if (!R.asm_tiles) { L.path = LevelPlan::HIP; return L; }
    L.path = LevelPlan::ASM;
    // Pre-pass levels below the root: the small-layout parents and the others are different slot lists;
    // their launches run side by side (second stream) instead of one after the other.
    // (Only for a frame alone, whose coarse levels are on the caller's stream: in a pipelined frame they are off the critical
    // path, and the side stream carries the previous frame's tile chains, where this frame's level-1 kernel sat for 170 us
    // of every frame - 1.64 -> 1.60 ms without the fork.  Forking to the tail stream instead: 2.0 ms; to streams of their
    // own, also for the per-slab levels' nearly always empty big-list launches: 3.5 ms - streams beyond four share
    // hardware queues (GPU_MAX_HW_QUEUES) and serialise against each other.)
    // (A fifth stream for the per-slab levels' nearly always empty big-list launches, with GPU_MAX_HW_QUEUES=8 in the
    // environment: 2.3 ms per frame instead of 1.03 - more than four streams in flight cost far more than two kernel
    // boundaries per slab, whatever the number of hardware queues.)
    L.fork_big = level > 0 && l < pre && in.use_pipeline && !in.profiling && in.has_side && on == CALLER && is3d;
    // Tapes of <= 32 registers / 256 choices (the small slot list: every parent of the leaf level) and, from the other
    // list, those of <= 64 / 512 go to the kernels that keep the interval file, the choices and the prune's register
    // map in VGPRs (fh_tiles_v32: 16 waves per CU, fh_tiles_v64: 8; no LDS); what is left takes the LDS layouts.
    const bool vk = !in.no_tiles_v && !L.exp;
    // (a pre-pass level has a few hundred parents in the two lists together: fh_tiles_v64 takes both in ONE launch
    // - the level's time is its slowest parent's either way, and a launch of its own for the small list put
    // another 130 us on the coarse levels' chain)
    L.both_lists = level > 0 && vk && l < pre && !L.fork_big;
    L.v32 = level > 0 && vk && !L.both_lists; L.small_lds = level > 0 && !vk;
    // (leaving the per-slab levels' big-list parents to the root-sized LDS launch alone - one launch less on the slab's tile
    // chain - was measured: 1.02 vs 1.04 ms per frame, within the noise; not done)
    if (L.rare) return L;      // (the parents outside the small list: the blocks behind k_tpush3d's)
    // (a ROOT tape that fits fh_tiles_v64 - 64 registers, 512 choices - and is not pruned through exported choices takes it too:
    // bear.vm's 23 registers, 512^3: the root level 255 -> 160 us with the interval file in VGPRs instead of LDS)
    const bool root_v64 = vk && level == 0 && is3d && P.max_regs <= V64_REGS && P.max_choices <= V64_CHOICES;
    L.v64 = vk && (level > 0 || root_v64);
    L.rest = !L.v64 || P.max_regs > V64_REGS || P.max_choices > V64_CHOICES;      // anything left for the root-sized LDS layout?
    // Pre-pass levels below the root: a few hundred parents whose tapes are far smaller than the
    // root's.  With the root-sized LDS layout only one wave fits a CU (256 at a time); a medium
    // layout takes those that fit it three to a CU, the root-sized launch takes the rest.
    L.mid = !vk && level > 0 && l < pre && R.lds_tiles_mid * 2 <= R.lds_tiles_big;
    return L;
}

static FrameSchedule schedule_frame(const RenderSetup& R, const ScheduleInputs& in) {
    FrameSchedule F;
    const FhRender& P = R.S.P;
    const uint32_t pre = R.S.pre_levels, n_groups = R.groups_per_slab, slabs = R.slab_hi - R.slab_lo;
    // Frame pipelining (asynchronous renders): this frame takes the buffer set the previous frame did not use, and everything up
    // to and including its coarse levels is queued on a stream of its own - it depends on nothing the previous frame does, so it
    // runs beside that frame's slabs.  The slabs' tile chains follow on the side stream (after the previous frame's), the leaf
    // chains and the final image on the caller's stream as before.
    F.fpipe = frame_pipelined(in);
    // Two root levels side by side.  A frame of one coarse level whose tapes read no z (front slab only: one light tile chain, a leaf
    // stage of 5 k leaves) is its root level and little else: 165 us of kernels in one dependent chain on the pre-pass stream against
    // 100 on the side stream and 100 for lists + leaves + normals together - and that chain set the rate of queued frames.  Such frames
    // take the pre-pass stream and the tail stream IN TURN for their root level, and keep what the tail stream carried (lists, normals)
    // on the caller's stream around the leaf kernel: still four streams (a fifth shares a hardware queue with one of them and
    // serialises against it, measured in round 2), two frames' root levels in flight.
    F.alt_pre = F.fpipe && P.n_levels == 2 && R.column_inv && in.no_zrep == 0 && in.has_tail && in.whole;
    // A frame ALONE - nothing of the frame before it is under way - keeps its coarse levels on the caller's stream: there is nothing to run
    // beside, and every change of stream is an event's latency (prospero.vm 1024^3, one frame alone: 0.388 -> 0.33 ms).  The frame queued
    // behind it takes the pre-pass stream as before and overlaps with it.
    F.lone = F.fpipe && !in.frames_queued;
#ifdef FH_EXP_NO_LONE      // experiment (tools/build_lib_variant.py): every frame's coarse levels on the pre-pass stream, as until round 6
    F.lone = false;
#endif
    F.takes_turn = F.fpipe && !F.lone && F.alt_pre;
    F.root = !F.fpipe || F.lone ? CALLER : (F.takes_turn && (in.pre_turn & 1u) ? TAIL : PRE);
    F.coarse = pre && n_groups;
    // Two-stream pipeline over the z-slabs: the tile stage of a slab runs on the side stream while
    // the leaves of the slab in front of it are evaluated on the caller's stream.  The occlusion
    // pyramid is then one slab stale, which is still exact (depths only grow).  The slab contexts
    // (dS, dS + 1, ..) take turns; each owns its leaves, leaf table, footprint lists and arena share.
    F.pipe = in.use_pipeline && !in.profiling && slabs > 1 && n_groups > 0 && !R.big_hbm;
    F.NC = F.pipe ? std::min<uint32_t>(in.slab_contexts, slabs) : 1;     // (no more contexts than slabs: each takes its share of the arena)
    F.slab_first = (int)R.slab_hi - 1; F.slab_stop = (int)R.slab_stop;
    F.n_rendered = n_groups ? std::max(0, F.slab_first - F.slab_stop + 1) : 0;
    // Pipelined frames: the root level stays on the pre-pass stream, the level below it moves to the head of this frame's tile
    // chains on the side stream.  The two coarse levels of a frame are one dependent chain of ~0.9 ms that, on one stream, set
    // the frame rate; split, the root level of frame n + 1 runs beside level 1 and the slabs of frame n, and the side stream
    // carries level 1 + the (now few) slab steps of its own frame.  (A frame alone sees no difference: the same chain.)
    const bool l1_side = F.fpipe && !F.lone && pre > 1 && in.has_side && slabs > 1 && n_groups > 0;
    // Where a slab's tile chain goes: the side stream, or (pipelined frames of at most as many slabs as there are slab contexts) the
    // tail stream, every slab's chain queued there BEFORE the tail work of the first slab - the side stream then carries level 1 of
    // the coarse levels alone, the pre-pass stream the root level, and the three chains of consecutive frames run beside each other.
    // (there when the ROOT tape reads no input that changes along a pixel column - then no tape of the frame does,
    // the leaf stage is light and the tail stream has room; a frame whose leaf kernels fill the machine wants its tile chains on
    // the high-priority side stream: prospero.vm 1024^3 0.77 -> 0.64 ms per frame there, the same frames with the column-invariance
    // short cuts off 1.86 -> 2.01)
    F.tiles_first = F.pipe && l1_side && R.root_invariant && in.has_tail && R.asm_points && slabs <= F.NC;
    // (and in such a frame the side stream - the busiest one of a pipelined frame, 0.43 ms of the 0.526 - carries level 1's evaluate + prune
    // launches and nothing else: the flags of level 1's tapes are set at the end of the root level on the pre-pass stream, and what follows
    // level 1 - the flags of its children, the frame mark, the fork of the slab contexts - goes to the stream the tile chains run on;
    // a frame with heavy leaf kernels keeps its tile chains on the side stream, and its fork must not queue behind the previous frame's tail work)
    F.l1 = l1_side ? SIDE : F.root;
    F.l1_flags = F.tiles_first ? F.root : F.l1;
    // (one coarse level - root tiles of 32^3 - in a pipelined frame: that level IS the frame's longest chain and the pre-pass stream the
    // pacemaker of the pipeline, so what follows its push - the flags of the parked parents, the frame mark, the fork of the slab
    // contexts - goes to the head of the tile chains on the side stream, which has no level 1 to carry in such a frame)
    const bool tail_to_side = F.fpipe && !F.lone && F.pipe && pre == 1 && in.has_side;
    F.fork_on = F.tiles_first ? TAIL : tail_to_side ? SIDE : F.l1;
    F.tiles = !F.pipe ? CALLER : F.tiles_first ? TAIL : SIDE;
    F.fork_to_side = F.pipe && F.fork_on != SIDE;
    F.fork_to_tail = F.tiles_first;
    F.rec_fork = F.fork_to_side || F.fork_to_tail;
    // the rest of the frame is the caller's stream's (and the tile stream's, which waits for the fork)
    // (one coarse level, its tail on the side stream, and tile chains to follow there: the caller's stream waits for the first tile
    // chain's event, which lies behind everything queued so far - no event of its own for that)
    F.pre_implied = F.fpipe && F.pipe && pre == 1 && in.has_side && F.fork_on == SIDE;
    F.ev_pre = F.fpipe && F.fork_on != CALLER && !F.pre_implied;
    // The leaf kernel is the slab's critical chain.  What surrounds it - the footprint lists (needed by the normals and the
    // LDS-class leaves only), those leaves (any order with the others: atomic-max z-buffer) and the normals of the slab's
    // hits - are small launches that leave the machine mostly idle, so in the pipelined frame they run on a third stream
    // beside the leaf kernel of the NEXT slab: the normals kernel only takes hits of its own slab's depth range, and a hit
    // behind them can never replace them.  (Measured with three slab contexts, ms per frame: everything on the caller's stream 2.44, the normals only on the third stream 2.30, lists + normals 2.16 - once the min-depth pyramid kernel of the tile chain ran in blocks of four waves: its 16-wave blocks found no room beside a leaf kernel that is never interrupted, 166 us instead of 10.)
    // (lists + normals on the tail stream; normals only and off were measured slower: DESIGN_HISTORY.md)
    // (when the tile chains run on the tail stream and frames are queued back to back, the
    // slab's small kernels stay on the caller's stream around its leaf kernel - otherwise the tail stream, serial, waits for every leaf
    // kernel with the NEXT frame's tile chains queued behind: 0.45 ms of it per frame for 0.40 of work.  A frame alone is 70 us
    // quicker with them beside its leaf kernels, hence the test)
    const bool on_main = F.tiles_first && in.frames_queued;
    F.aux_edge = F.pipe && in.has_tail && R.asm_points && !on_main && !F.alt_pre;   // (the HIP leaf kernels walk the footprint lists)
    F.lists = F.normals = F.aux_edge ? TAIL : CALLER;
    // Rare mode.  Four launches of a slab exist for tapes too large for the assembly kernels' register files - a leaf of more than 32
    // registers (its points, then its normals, in the C++ kernels with an LDS file), a parent of a per-slab tile level outside the small
    // slot list (fh_tiles_v64, then fh_tiles) - and find nothing to do in nearly every frame: prospero.vm 1024^3 0.138 -> 0.126 ms per
    // frame without them.  While the last finished frame of this context met no such tape (k_finish3d: host_flags[2]) the slab does not
    // make them: the last FH_RARE_BLOCKS blocks of k_classify3d, k_hits3d (or k_rare_leaves3d for both: rare_leaves below) and k_tpush3d do their work - correct for any number of such
    // tapes, slow for many (a wave per block, the register files in HBM), and the first frame that meets one puts the launches back.
    const size_t stride = (std::max(std::max(R.lds_tiles_big, R.lds_points_big), R.lds_normals_big) + 255) / 256 * 256;
    // (a root tape of <= 32 registers has no large leaves, but its per-slab levels still launch fh_tiles_v64 for the other slot list)
    F.rare = R.split && R.asm_tiles && R.asm_points && R.asm_normals && !R.big_hbm && in.has_flags && in.rare_seen == 0 &&
             stride * FH_RARE_BLOCKS * 4 <= ((size_t)256 << 20);      // (a set's state buffer holds four slab contexts)
    F.rare_stride = F.rare ? (uint32_t)stride : 0u;
    // Sparse columns (option column_walk): the frames whose tapes guarantee at most one leaf per pixel
    // column and slab.  `by_list` (column_walk 1): their leaf stage is driven by the slab's FhLeaf records themselves - wave i of fh_columns
    // and of fh_normals takes leaf i - instead of by the [layer][footprint] table, which for 5.5 k leaves in 1 M entries was cleared, scanned
    // whole by k_classify3d, scanned whole again by fh_columns and walked per footprint by k_hits3d in every frame.  The push then writes no
    // table (render_state.h leaf_list), k_classify3d and k_hits3d shrink to their rare-mode blocks, and both kernels' grids follow the leaf
    // count the last finished frame of this context reported (host_flags[3]: a hint - waves loop over the list, any grid is right).
    const uint32_t layers = P.slab / 8;
    F.by_list = in.column_walk == 1 && R.column_inv && R.split && R.zrep && R.asm_points && R.asm_normals && layers <= 64 && in.has_flags;
    F.table_words = F.by_list ? 0u : R.table_words;
    // Rare mode in such a frame: all that is left of k_classify3d and k_hits3d are their FH_RARE_BLOCKS blocks for the leaves beyond the assembly
    // kernels' files - two launches that read n_leaves_lds == 0 and leave, in nearly every frame (5.4 + 5.6 us of the caller's stream, prospero.vm
    // 1024^3).  A column of a by_list frame has one leaf per slab or none, so a large leaf's hits are final when its own points are through and
    // its gradient can follow in the same wave: one launch, behind the leaf kernel.  Only where the leaf kernel's and the normals kernel's files
    // are the same size (40 / 40; with transcendental opcodes 44 / 40): a leaf between the two has its points from fh_columns_t and its normals
    // from k_hits3d's blocks, and keeps both launches as they are.
    F.rare_leaves = F.by_list && F.rare && P.max_regs > R.S.leaf_asm_regs && R.S.leaf_asm_regs == R.S.norm_asm_regs;
#ifdef FH_EXP_TWO_RARE_LAUNCHES      // experiment (tools/build_lib_variant.py): the rare-only k_classify3d and k_hits3d launches as until profiles/event_edges
    F.rare_leaves = false;
#endif
    F.list_waves = (R.n_footprints + 63) / 64 * 64;      // (no frame has reported yet: what the column walk launches)
    if (F.by_list && in.last_leaves) F.list_waves = std::min(F.list_waves, (in.last_leaves + in.last_leaves / 8 + 63) / 64 * 64);
    F.reset_blocks = (int)std::max<uint32_t>(1, std::min<uint32_t>(1024, (std::max(F.table_words, n_groups) + 255) / 256));
    // Column walk: one footprint COLUMN of the slab's leaf table per wave instead of one block of four footprints
    // of one layer.  A frame whose tapes read nothing that changes along a pixel column queues at most one leaf per column
    // and slab (the nearest of a stack), so its table is nearly empty - prospero 1024^3: 5.5 k leaves in 1 M entries - and
    // the (blocks, layers) grid is 262 144 workgroups of which 98 % load four empty entries and leave: 66 of the launch's
    // 71 us.  By columns it is 16 384 waves, each with its column's 64 entries in one load.  Leaves of a column are then
    // taken one after the other by one wave, front to back, which is wrong for frames with a leaf in most layers (the
    // launch would last as long as its fullest column: measured in round 3, bear.vm 2.40 -> 4.07 ms): option column_walk
    // 1 = only where the tapes guarantee sparse columns - and then by the list of leaves, `by_list` above -, 3 = the same frames
    // by the table (parity runs), 0 never, 2 always (tests).
    F.by_columns = in.column_walk == 2 || ((in.column_walk == 1 || in.column_walk == 3) && R.column_inv);
    // ... and for every other frame, round 6: the column walk by GROUPS of 2^g layers (grid y = the group,
    // front group first; option column_group = g, 0: the block walk).  A wave keeps its footprint: the pixels' set-up,
    // their matrix products and their z-buffer words are loaded once per wave instead of once per leaf (the z-buffer words
    // were two thirds of the launch's HBM traffic), hits stay in registers from leaf to leaf and leave in one atomic.
    // (a blend - few min / max, nothing to prune: bear.vm's leaves keep 350 of the root's 650 ops - wants half the group: a wave's
    // leaves are taken one after the other, and the launch lasts as long as its fullest waves - 512^3, ms per frame by g = 0 / 1 /
    // 2 / 3: 1.24 / 0.97 / 1.09 / 1.33; prospero.vm's 22-op leaves on the general path: 0.433 / 0.424 ms per launch by g = 1 / 2)
    const uint32_t g_opt = (uint32_t)std::min(std::max(in.column_group, 0), 6);
    F.g = F.by_columns ? 6u : (R.smooth_tape && g_opt > 1 ? g_opt - 1 : g_opt);
    F.leaf_walk = !R.asm_points ? FrameSchedule::HIP_LEAVES : F.by_list ? FrameSchedule::BY_LIST
                : ((F.by_columns && layers <= 64) || (!F.by_columns && F.g > 0)) ? FrameSchedule::BY_COLUMNS : FrameSchedule::BY_BLOCKS;
    // The normals of a WHOLE front-slab-only frame were computed and thrown away.  No tape of such a frame reads anything that changes along
    // a pixel column, so a pixel that is inside is inside at every z: its hit is the top voxel of the top leaf layer of the volume, its depth
    // >= the image's depth, and k_finish3d writes (0, 0, 1, depth) for every pixel of depth >= depth - 1 whatever its normal (the reference's
    // clamp: voxel.rs:533-539) - fh_normals evaluated a gradient for every hit of the slab, 25 us of the caller's stream and a launch, and
    // nothing read it.  The frame makes no normals launch; its hits keep their leaf's number in the z-buffer word, which k_finish3d does not
    // look at.  What stays is k_rare_leaves3d where the frame has it: the POINTS of the leaves beyond the leaf kernel's file are that
    // launch's (its gradients follow in the same wave and are clamped like the others).  A part of a frame (shard, block: `whole` false)
    // keeps its normals - a back z-block's hits lie below the volume's top -, and so does every frame with z in a tape.
    F.normals_on = !(R.front_only && in.whole);
#ifdef FH_EXP_SKIP_NORMALS      // experiment (tools/build_lib_variant.py): a frame without its normals kernels - what they cost beside the leaf kernels
    F.normals_on = false;
#endif
    for (uint32_t l = 0; l < P.n_levels && l < FH_MAX_LEVELS; l++) {
        const Role on = l >= pre ? F.tiles : l == 0 ? F.root : F.l1;
        F.level[l] = plan_level(R, in, (int)l, true, F.rare_stride, on, l == 1 && l < pre ? F.fork_on : on);
    }
    return F;
}

// ev_leaves[idx], behind the normals of the idx-th slab rendered, has two waiters: the tile chain of slab idx + NC, which takes the same
// slab context (capi_render.hpp tile_step), and - for the LAST slab of a frame whose normals run on the tail stream - the caller's stream
// before k_finish3d.  It is recorded for those and for nobody: the front-slab frame (n_rendered 1) records none.
static bool waits_leaves(const FrameSchedule& F, int idx) { return F.pipe && idx >= (int)F.NC && idx < F.n_rendered; }      // (the tile chain of slab idx: for ev_leaves[idx - NC])
static bool records_leaves(const FrameSchedule& F, int idx) {
    if (!F.pipe || idx < 0 || idx >= F.n_rendered) return false;
    return idx + (int)F.NC < F.n_rendered || (F.aux_edge && idx == F.n_rendered - 1);
}

// ---- the pinned staging ring and its guards ---------------------------------------------------------------------------------
// A frame's state and root groups reach the device through one of FH_STAGING_SLOTS pinned slots, which k_frame_begin reads on the frame's
// root stream; the slot's next user, FH_STAGING_SLOTS frames later, waits for the slot's event first.  That event has to lie at or behind
// k_frame_begin on the root stream - and not between k_frame_begin and the root level's first kernel, where it was until profiles/event_edges:
// it is recorded when the root stream is left for the first time (beside the hop's own record, at the end of the root level) or, for a
// frame that never leaves its root stream, beside the frame's last record - and on EVERY other way out of the frame, which is why it is
// an object: whatever returns early (a cancelled frame, a failed launch, a refused level) records it on the way.
static const uint32_t FH_STAGING_SLOTS = 8;
struct StagingRing {
    uint32_t next = 0;
    bool used[FH_STAGING_SLOTS] = {};      // the slot's event has been recorded at least once: its next user waits for it
    uint32_t take() { return next++ % FH_STAGING_SLOTS; }
};
// `Record`: what records the slot's event behind everything queued on the root stream so far (the driver: hipEventRecord)
template <class Record> struct SlotGuard {
    Record record_now;
    bool armed = false;
    explicit SlotGuard(Record r) : record_now(r) {}
    SlotGuard(const SlotGuard&) = delete;
    SlotGuard& operator=(const SlotGuard&) = delete;
    void arm() { armed = true; }                                        // k_frame_begin has been queued: the device reads the slot
    void record() { if (armed) { armed = false; record_now(); } }       // once
    ~SlotGuard() { record(); }
};
