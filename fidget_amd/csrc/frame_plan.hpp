// The plan of a frame's set-up: everything a 2D or 3D frame decides before its first launch - which tiles, which slabs and layers of a part,
// the root groups, every queue capacity and buffer size, which kernel paths the tape takes - as pure functions of facts: the tape's numbers
// (TapeFacts), the context's options and sizes (PlanInputs), the image and the part of it.  capi_render.hpp prepare() runs the plan: it
// allocates what FrameBytes names, uploads the tape's root tables and binds the pointers.  No HIP call, no global: this header compiles with
// plain g++ next to render_state.h, and tests/test_frame_plan.py checks it against the rules restated in Python
// (tests/host_build/frame_plan_host.cpp).  frame_schedule.hpp decides, from the finished plan, where every launch goes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "render_state.h"

static const uint32_t VM_TILES_2D[] = {128, 32, 8};        // fidget-core/src/vm/mod.rs:255-257
static const uint32_t VM_TILES_3D[] = {128, 64, 32, 16, 8};  // fidget-core/src/vm/mod.rs:251-253
static const uint32_t FH_LEAF_REGS = 40, FH_LEAF_REGS_T = 44;      // (gen_interp.py gen_columns: fh_columns' 40 x 2 shape, fh_columns_t's 44 x 4)
static const uint32_t FH_NORMAL_REGS = 40;                         // (gen_normals.py NR)
// 2D hint of the HIP shape: 128 -> 16 with 16 x 16 pixel leaves - what fidget-jit uses (fidget-jit/src/lib.rs:984-986); a fan-out
// of 64 children per parent fills a wavefront of the tile-stage kernels (the VM's 128 / 32 / 8 fans out by 16)
static const uint32_t HIP_TILES_2D[] = {128, 16};
// medium LDS layout of the tile stage (pre-pass levels below the root): 48 KB, three waves per CU
static const uint32_t MID_REGS = 64, MID_CHOICES = 768;
static size_t tiles_lds(uint32_t regs, uint32_t choices, uint32_t TL) {
    size_t b = (size_t)regs * TL * 8 + (size_t)((choices + 15) / 16) * TL * 4 + (size_t)regs * TL + 256;
    return (b + 15) & ~(size_t)15;
}

// Which part of the volume a render covers (multi-GPU): root-tile columns round robin (index % n_shards == shard, full
// depth), or a block of an nx x ny x nz split of the root-tile grid and of the z-slabs (octants: 2 x 2 x 2)
struct PartSpec {
    uint32_t shard = 0, n_shards = 1;
    uint32_t ix = 0, nx = 1, iy = 0, ny = 1, iz = 0, nz = 1;
};

// What the plan needs to know of a tape (capi_tapes.hpp tape_facts)
struct TapeFacts {
    size_t n_ops = 0;
    uint32_t n_regs = 0, n_choices = 0, n_outputs = 1;
    bool asm_ok = true, is_full = false, has_mod = false, tiles_t_ok = true;      // capi_tapes.hpp tape_class
    uint32_t input_slots = 0;      // the input slots the tape reads, bit per slot
    uint32_t n_groups = 0;         // term groups (host_graph.hpp plan_terms), and per group: ops, registers, choices
    struct Group { uint32_t n_ops, n_regs, n_choices; } group[FH_MAX_GROUPS] = {};
    uint32_t n_terms = 0, n_top = 0;
    bool chain = false;
};
// ... and of the context: the options it reads (FH_OPTION_LIST), the context's switches and sizes
struct PlanInputs {
    int slab_layers = 4, no_zrep = 0, no_column_inv = 0, no_columns_t = 0, no_asm_normals = 0, no_asm_tiles = 0, no_asm_tiles_t = 0, no_tape_groups = 0, prune2 = 1,
        root32_max = 4096;
    bool use_asm = true, use_split = true;
    uint32_t n_cu = 256, slab_contexts = 4;
    size_t arena_bytes = (size_t)128 << 20;      // of the arena the frame runs in (arena_bytes_for: after the growth a frame before it asked for)
};

// Bytes of every buffer a frame needs, in the order prepare() grows them (0: not needed; the state block and the arena are the context's)
struct FrameBytes {
    size_t gscratch = 0, queue[FH_MAX_LEVELS] = {0}, squeue = 0, leaves = 0, leaves_b = 0, leaf_table = 0, leaf_table_b = 0, zbuf = 0, normals = 0, fp_lists = 0, fp_lists_b = 0,
           mind = 0, tvals = 0, topch = 0, chwr = 0, chw[2] = {0, 0}, slots = 0;
};

struct RenderSetup {
    FhRenderState S;
    std::vector<FhGroup> roots;
    FrameBytes bytes;
    uint32_t n_slabs = 1, n_layers = 1;      // z-slabs (steps of the per-slab chains), root-tile layers
    uint32_t slab_lo = 0, slab_hi = 1;   // z-slabs this render covers (all of them unless the volume is split in z: octant shards)
    size_t lds_tiles_mid = 0, lds_tiles_big = 0, lds_tiles_small = 0, lds_points_big = 0, lds_normals_big = 0, lds_normals_small = 0;
    uint32_t table_words = 0, n_footprints = 0, groups_per_slab = 0;
    bool smooth_tape = false;      // the root tape has a choice in fewer than every tenth op (and more than 200 ops): a blend whose leaves stay long
    uint32_t hit_bucket_cap = 0;   // the normals kernel's work lists (k_hits3d): entries per bucket, words of the whole thing per slab context
    size_t hit_words = 0;
    size_t mind_words = 0;      // words of the min-depth pyramid (cleared at the head of the frame)
    uint32_t tl = 16;  // sibling tiles per wave in the tile kernel (16 or 64)
    bool full = false;  // tape uses transcendental / modulo ops -> FULL kernel variants
    bool asm_points = false;  // leaf stage on the assembly interpreters
    bool asm_points_t = false;  // ... on fh_columns_t (tapes with transcendental / modulo / rng opcodes)
    bool asm_normals = false;   // normals by the assembly gradient interpreter fh_normals (gen_normals.py): footprints of leaves of <= 32 registers
    bool split = false;       // 3D tile stage as setup / evaluate+prune / push kernels
    bool asm_tiles = false;   // ... with the evaluate+prune step in assembly (fh_tiles)
    bool asm_tiles_t = false; // ... by the *_t variants (transcendental opcodes)
    bool hip_tiles_unasked = false;   // ... or by the HIP kernels although nobody switched the assembly ones off (fhip_render_counters out[6] counts such frames)
    uint32_t group_regs = 0, group_choices = 0;  // bounds over the tape's groups
    size_t lds_tiles_group = 0;
    bool groups = false;      // ... and level 0 evaluated as the tape's independent groups (tape parallelism)
    bool prune1 = false;      // ... and, on the first exp_levels levels, the prune as one wave per child (fh_prune1)
    bool prune2 = false;      // ... by the linked prune (prune2.hip k_prune2: visits only the ops a child keeps) where the tape qualifies
    const uint64_t* d_links = nullptr;
    const uint64_t* d_ctab = nullptr;
    size_t lds_prune2 = 0;
    uint32_t n_chain = 0;          // ops of the root chain (their table lies behind d_ctab's t.n_choices entries)
    uint32_t p2_cap_kept = 0;      // kept ops per child the linked prune's LDS areas are sized for (children beyond: the scalar sweep behind it)
    uint32_t exp_levels = 0;
    uint32_t col_slots = 0, col_depmask = 0, col_flags = 0;   // 3D: axis slots x | y << 8 | z << 16 (0xFF none), inputs varying along a pixel column, bit 16 projective
    bool zrep = false;        // ... column-invariant parents are evaluated for one z-layer only (k_tape_flags)
    bool xy_fixed = false, root_invariant = false;   // 3D, set before plan_frame: x and y do not move along a pixel column; the ROOT tape reads nothing that does
    // ... both, and the short cut is on (option no_zrep 0 or 3): no tape of the frame reads anything that changes along a pixel column, so at most
    // one leaf per pixel column and slab.  Computed HERE ONLY (column_facts); read by the tile choice, by plan_frame (root_zrep) and by the schedule
    bool column_inv = false;
    bool one_level_64 = false;   // 2D, a one-level list: root groups of 64 tiles through the split tile stage (render2d_frame's small-image passes)
    bool classify_only = false;  // ... and the pass that only classifies its tiles and writes their fills (no prune, no leaves)
    bool root_zrep = false;   // ... then the root level evaluates ONE layer of root tiles per z-slab and hands the result to the layers stacked on it
    bool front_only = false;  // ... and only the front slab is rendered (slab_stop = slab_hi - 1)
    uint32_t slab_stop = 0;   // the slabs rendered: slab_hi - 1 down to slab_stop (= slab_lo unless front_only)
    bool big_hbm = false;     // the root-sized register files live in HBM (S.gscratch): hbm_waves workgroups per root-sized launch
    uint32_t hbm_waves = 0;
};

// A refusal of the plan: status (fidget_hip.h fhip_status: 0 none, 5 bad tape, 6 unsupported) and the message
struct PlanStatus { int status = 0; const char* msg = ""; };
static const int PLAN_BAD_TAPE = 5, PLAN_UNSUPPORTED = 6;

// ---- the tile list of a 3D frame ----------------------------------------------------------------------------------------
// fidget-raster/src/lib.rs:59-66
static std::vector<uint32_t> trim_tiles(const uint32_t* tiles, uint32_t n, uint32_t max_size) {
    uint32_t i = n;
    for (uint32_t k = 0; k < n; k++) if (tiles[k] < max_size) { i = k; break; }
    i = i ? i - 1 : 0;
    return std::vector<uint32_t>(tiles + i, tiles + n);
}
// RenderHints of the HIP shape (the reference lets every shape type pick its own, shape.rs RenderHints): a fan-out of 4^3 = 64 children
// fills a wavefront (128 -> 32 -> 8).  The root tile stays the one the reference's VmShape hints give for the image size, so that exactly
// the same voxels are covered (a root tile overhanging the image in z is evaluated there by the reference too).
static std::vector<uint32_t> hip_tiles_3d(uint32_t max_size) {
    std::vector<uint32_t> v = trim_tiles(VM_TILES_3D, 5, max_size);
    std::vector<uint32_t> out{v[0]};
    for (uint32_t t = v[0]; t > 8;) { t = std::max<uint32_t>(t / 4, 8); out.push_back(t); }
    return out;
}
// Split + assembly on, and the tape is one the groups + linked prune path takes (what a root level of many tiles needs: choose_tiles_3d's
// 32^3 root tiles, render2d_frame's one-level passes, plan_linked_prune)
static bool linked_root_tape(const TapeFacts& t, const PlanInputs& in) {
    return in.use_split && in.use_asm && t.n_groups > 0 && !in.no_tape_groups && in.prune2 && t.asm_ok && t.n_ops <= FH_P2_MAX_OPS && t.n_choices <= FH_P2_MAX_CHOICES;
}
// valid = false: the caller's list is not one the reference accepts; substituted: it is, but not one the kernels take - rendered with the library's
struct TileChoice { std::vector<uint32_t> ts; bool valid = true, substituted = false; };
// The caller's list (or null) for an image of `size`; columns_split, nz: parts of a frame - n_shards * nx * ny, nz (1, 1: a whole frame); column_inv:
// RenderSetup::column_inv; the options; root32_tape: linked_root_tape
static TileChoice choose_tiles_3d(const uint32_t* tile_sizes, uint32_t n_tile_sizes, const uint32_t (&size)[3], uint32_t columns_split, uint32_t nz, bool column_inv,
                                  int root32_max, int no_zrep, bool root32_tape) {
    const uint32_t width = size[0], height = size[1], depth = size[2];
    TileChoice T;
    const uint32_t image = std::max(width, height);
    T.ts = tile_sizes ? trim_tiles(tile_sizes, n_tile_sizes, image) : hip_tiles_3d(image);
    bool own_tiles = !tile_sizes;
    if (tile_sizes) {
        // Any list the reference accepts (TileSizes::new, fidget-core/src/render/mod.rs:181-251: descending, each a multiple of the next;
        // fidget-jit's own hint is [64, 16, 8], a caller's [64, 16, 4] is valid there) is accepted here: what the device's kernels cannot
        // take as given - leaves other than 8^3 (one 8 x 8 footprint per wavefront), a fan-out above 64 children (one per lane) - is
        // rendered with the library's list instead.  A 3D image does not depend on the tile sizes, so the caller
        // cannot tell, except by the time; fhip_render_counters out[7] counts such frames.
        T.valid = n_tile_sizes >= 1 && tile_sizes[n_tile_sizes - 1] >= 1;
        for (uint32_t i = 1; i < n_tile_sizes && T.valid; i++)
            T.valid = tile_sizes[i - 1] > tile_sizes[i] && tile_sizes[i] > 0 && tile_sizes[i - 1] % tile_sizes[i] == 0;
        if (!T.valid) return T;
        bool native = T.ts.back() == 8 && T.ts.size() <= FH_MAX_LEVELS;
        for (size_t i = 1; i < T.ts.size() && native; i++) { const uint32_t n = T.ts[i - 1] / T.ts[i]; native = n * n * n <= 64; }
        if (!native) { T.ts = hip_tiles_3d(image); own_tiles = T.substituted = true; }
    }
    // Few tiles, long tape (a small image, a part of a frame on one rank of several, a model without z): root tiles of 32^3 straight
    // above the leaves.  With 128^3 root tiles such a frame is a handful of one-wave chains over tapes that a 128^3 tile barely prunes
    // (prospero.vm at 512^3: a root tile keeps up to 1 795 of 6 363 ops - beyond the linked prune's and fh_tiles_v64's limits, so the
    // LDS-file kernel and the scalar sweep walk them: 3.3 ms for one frame).  The root level's forward pass is parallel over the tape
    // (term groups) however many tiles there are, and the linked prune handles a thousand children in one round, each a wave: pruning
    // the ROOT tape per 32^3 tile costs what pruning it per 128^3 tile costs, its tapes are what level 1 would have arrived at, and
    // level 1 - the longest kernel of the frame - is not run at all: 512^3 3.25 -> 1.45 ms alone.  A 3D image does not depend on the
    // tile sizes, so this is the library's choice whenever the caller gave none: taken while the root level has at
    // most `root32_max` children - counting one layer per z-slab when the root tape reads nothing that changes along a pixel column
    // (root_zrep, plan_frame) - and the tape is one the groups + linked prune path takes.
    if (own_tiles && root32_max > 0 && T.ts.size() == 3 && T.ts[0] == 128 && root32_tape) {
        const uint64_t cols = (uint64_t)((width + 31) / 32) * ((height + 31) / 32) / std::max<uint32_t>(1, columns_split);
        const uint64_t layers = column_inv ? (no_zrep == 0 ? 1u : (uint64_t)std::max<uint32_t>(2, (depth + 511) / 512))      // (one layer per slab; the front slab only)
                                             : (uint64_t)((depth + 31) / 32) / std::max<uint32_t>(1, nz);
        // (measured, profiles/r05c: up to two rounds of the linked prune's workgroups - 2 048 children - always; up to root32_max when a
        // 128^3 root tile is a quarter of the image or more - there the 128^3 tiles' tapes stay long whatever is done: 512^3 with z in
        // every tape, 4 096 children, 3.65 -> 1.72 ms; an octant of a 1024^3 frame, as many children of a model twice the size: 1.10 -> 1.33)
        const uint64_t children = cols * std::max<uint64_t>(layers, 1);
        if ((children <= 2048 || (children <= (uint64_t)root32_max && image <= 512)) && (depth + 31) / 32 <= FH_MAX_SLABS)
            T.ts = {32, 8};
    }
    return T;
}

// ---- column invariance ------------------------------------------------------------------------------------------------------
// 3D: input slots of the axes, which inputs change along a pixel column (a z coefficient in the axis' matrix row, or a projective
// matrix), and whether the root tape reads any of them - from the camera matrix, the input binding and the tape's input slots alone
static void column_facts(const FhRender& P, const TapeFacts& t, const PlanInputs& in, RenderSetup& R) {
    uint32_t u[16];
    memcpy(u, P.mat, sizeof(u));
    const bool proj = (((u[12] | u[13] | u[14]) & 0x7FFFFFFFu) | (u[15] ^ 0x3F800000u)) != 0;
    int slot[3] = {-1, -1, -1};
    for (int sl = 0; sl < FH_MAX_INPUTS; sl++) if (P.in_kind[sl] < 3) slot[P.in_kind[sl]] = sl;   // (the last slot of an axis)
    for (int ax = 0; ax < 3; ax++) {
        R.col_slots |= (uint32_t)(slot[ax] < 0 ? 0xFF : slot[ax]) << (8 * ax);
        const bool dep = proj || (u[4 * ax + 2] & 0x7FFFFFFFu) != 0;
        if (dep && slot[ax] >= 0) R.col_depmask |= 1u << slot[ax];
        if (dep) R.col_flags |= 0x20000u << ax;     // (bits 17 .. 19: this axis of the model changes along a pixel column - from the camera alone)
    }
    R.col_flags |= proj ? 0x10000u : 0u;
    // tiles of a tape that reads nothing varying along z repeat along z: worth looking for when x and y do not vary with it
    R.xy_fixed = !proj && (slot[0] < 0 || !((R.col_depmask >> slot[0]) & 1)) && (slot[1] < 0 || !((R.col_depmask >> slot[1]) & 1));
    // (option no_column_inv, diagnostics / bench: no column-invariance short cut anywhere - every input counts as varying
    // along z - which is what a model with z in every tape gets)
    if (in.no_column_inv) R.col_depmask = 0xFFFFFFFFu;
    R.root_invariant = !in.no_column_inv && R.col_depmask != 0xFFFFFFFFu && (t.input_slots & R.col_depmask & 0x7FFFFFFFu) == 0;
    R.column_inv = R.xy_fixed && R.root_invariant && (in.no_zrep == 0 || in.no_zrep == 3);
}

// ---- the arena ----------------------------------------------------------------------------------------------------------------
// A frame before this one ran out of tape arena (`overflowed`: k_finish3d / k_latch_arena said so in the pinned host word): the sets come
// back twice as large, up to `cap` (option arena_mb).  The frames that overflowed were right (their tiles kept their parents' tapes), only slower.
// `volume_hint`: voxels of a 3D frame whose ROOT tape reads an input that changes along a pixel column (0: none such, or 2D): every
// tile of every slab then keeps a tape of its own, and the first 128 MB overflow in the first frame - which is then right but many
// times slower (children keep their parents' tapes), as are the frames until the growth has caught up.  Sized at about a byte
// per voxel from the start instead (prospero.vm 1024^3 with z in every tape: peak 0.9 GB per set), before anything is in flight.
// Returns the bytes the frame's arena has (`have`: nothing to do).
static size_t arena_bytes_for(size_t have, size_t cap, size_t first_step_below, bool overflowed, size_t tape_ops, uint64_t volume_hint) {
    size_t need = ((tape_ops + 64) * 8 + 4096) * 4;       // (root tape + its groups, with room to prune into)
    if (volume_hint) need = std::max<size_t>(need, std::min<uint64_t>(volume_hint, cap));
    bool grow = overflowed && have < cap;
    size_t want = grow ? have * (have <= first_step_below ? 4 : 2) : have;      // (the first step is the big one: a frame that outgrows the first 128 MB is usually one with z in every tape, at 4 x the ops and more)
    if (want < need) { want = need; grow = have < std::min(need, cap); }
    return grow ? std::min(cap, want) : have;
}

// ---- the frame ------------------------------------------------------------------------------------------------------------------
// Everything of a frame's set-up that is arithmetic or a decision.  R comes with the image (S.P width, height, depth, the matrix and
// the inputs), column_facts' fields and the 2D passes' one_level_64 / classify_only; `ts`: the tile list; `part`: the part of the volume.
// Leaves: S.P's tile fields, every size, capacity and offset of S (no pointer, no counter: prepare() bind_state), the root groups in queue
// order, R.bytes and every path flag but the linked prune's (plan_linked_prune, once the tape's links are known to exist).
static PlanStatus plan_frame(const TapeFacts& t, const PlanInputs& in, bool is3d, const std::vector<uint32_t>& ts, const PartSpec& part, RenderSetup& R) {
    auto refuse = [](int status, const char* msg) { PlanStatus s; s.status = status; s.msg = msg; return s; };
    FhRenderState& S = R.S;
    FhRender& P = S.P;
    FrameBytes& B = R.bytes;
    if (t.n_outputs != 1) return refuse(PLAN_BAD_TAPE, "shape tapes have exactly one output");
    if (ts.empty() || ts.size() > FH_MAX_LEVELS) return refuse(PLAN_UNSUPPORTED, "1..8 tile levels supported");
    P.n_levels = (uint32_t)ts.size();
    uint32_t fanout = 1;
    for (size_t i = 0; i < ts.size(); i++) {
        P.tiles[i] = ts[i];
        if (i) {
            if (ts[i - 1] <= ts[i] || ts[i - 1] % ts[i]) return refuse(PLAN_UNSUPPORTED, "bad tile size list");
            const uint32_t n = ts[i - 1] / ts[i];
            fanout = std::max(fanout, is3d ? n * n * n : n * n);
        }
    }
    if (fanout > 64) return refuse(PLAN_UNSUPPORTED, "tile fan-out above 64 children");
    // (a one-level 2D list - the small-image passes of render2d_frame: root groups of 64 tiles - takes the 64-lane tile stage too)
    const uint32_t TL = R.tl = (fanout > 16 || (!is3d && ts.size() == 1 && R.one_level_64)) ? 64 : 16;
    if (is3d && ts.back() != 8) return refuse(PLAN_UNSUPPORTED, "3D leaves must be 8^3 (one 8x8 footprint per wave)");
    // (register numbers are 12-bit fields of a tape word.  The device prunes keep old -> new register maps in bytes with 0xFF =
    // dead: a CHILD tape has 255 registers at most - one that would need more keeps its parent's tape; the root tape may have
    // more, its register file then lives in HBM: gscratch below)
    if (t.n_regs >= FH_MAX_REGS) return refuse(PLAN_UNSUPPORTED, "renders support up to 4095 registers");
    if (t.n_ops >= (1u << 24)) return refuse(PLAN_UNSUPPORTED, "renders support tapes of up to 2^24 ops");   // (FhLeafRef packs length | registers << 24)
    P.max_regs = std::max<uint32_t>(t.n_regs, 1);
    P.max_choices = t.n_choices;
    P.roots_x = (P.width + ts[0] - 1) / ts[0];
    P.roots_y = (P.height + ts[0] - 1) / ts[0];
    // z-slabs: the per-slab chains (tile stage, leaf kernel, tail) take `slab_layers` root-tile layers per step when the coarse
    // levels are evaluated for the whole volume up front (the length of the tile chain is its number of steps: every step's
    // launches leave most of the machine idle); one layer per step otherwise
    const uint32_t n_layers = is3d ? (P.depth + ts[0] - 1) / ts[0] : 1;
    // (a two-level list - root tiles of 32^3 straight above the leaves, what small images and parts of a frame take - gets a pre-pass of
    // its ONE coarse level; option slab_layers counts layers of 128 voxels, whatever the root tile)
    const bool prepass_ok = is3d && ts.size() >= 2 && n_layers <= FH_MAX_SLABS;
    uint32_t SL = prepass_ok ? (uint32_t)std::max(1, std::min(8, in.slab_layers)) * std::max<uint32_t>(1, 128 / ts[0]) : 1u;
    // (the leaf table: <= 64 eight-voxel layers per slab; at least two slabs, so that the tile stage of one still runs beside the
    // leaf kernel of the other - bear.vm at 512^3, four layers: 3.68 ms per frame as two slabs, 3.77 as one)
    while (SL > 1 && (ts[0] * SL / 8 > 64 || SL * 2 > n_layers)) SL >>= 1;
    P.slab = ts[0] * SL;
    R.n_slabs = is3d ? (P.depth + P.slab - 1) / P.slab : 1;
    R.n_layers = n_layers;
    R.full = t.is_full;
    // assembly leaf kernels: supported opcodes only (any 4x4 screen-to-model matrix, projective ones included)
    R.asm_points = in.use_asm && is3d && (t.asm_ok || !in.no_columns_t);
    R.asm_points_t = R.asm_points && !t.asm_ok;   // transcendental / modulo / rng opcodes: the variant that calls the compiled routines
    // (the most registers of a leaf the leaf kernel takes - gen_interp.py gen_columns: the largest register-file shape of fh_columns / fh_columns_t)
    S.leaf_asm_regs = !R.asm_points ? 32u : (R.asm_points_t ? FH_LEAF_REGS_T : FH_LEAF_REGS);
    // (fh_normals_t has the transcendental, rng and atan2 handlers; a modulo's gradient - div_euclid - keeps the C++ kernel)
    R.asm_normals = R.asm_points && !in.no_asm_normals && (!R.asm_points_t || !t.has_mod);
    S.norm_asm_regs = R.asm_normals ? FH_NORMAL_REGS : 32u;

    // LDS budgets: BIG = bounded by the root tape (children never need more); SMALL = fixed
    R.lds_tiles_big = tiles_lds(P.max_regs, P.max_choices, TL);
    R.lds_tiles_small = tiles_lds(SMALL_REGS, SMALL_CHOICES, TL);
    R.lds_tiles_mid = tiles_lds(MID_REGS, MID_CHOICES, TL);
    R.lds_points_big = (size_t)P.max_regs * WAVE * 4;
    R.lds_normals_big = (size_t)P.max_regs * WAVE * 16;
    R.lds_normals_small = (size_t)32 * WAVE * 16;
    // A register file that does not fit LDS (more than ~160 registers for the gradients, ~280 for the intervals) lives in HBM:
    // the reference spills registers beyond its file to memory slots (compiler/alloc.rs:116-125), this is the device's form of
    // it - the root-sized kernel variants take a region of `gscratch` per workgroup instead of LDS.  A slow path by design
    // (a few hundred workgroups, no pipelining: render3d_part), for tapes the fast paths cannot take anyway.
    S.gscratch_stride = 0;
    R.big_hbm = R.lds_tiles_big > FH_LDS_MAX || R.lds_normals_big > FH_LDS_MAX || R.lds_points_big > FH_LDS_MAX;
    if (R.big_hbm) {
        const size_t stride = (std::max(std::max(R.lds_tiles_big, R.lds_normals_big), R.lds_points_big) + 255) & ~(size_t)255;
        if (stride >= ((size_t)1 << 31)) return refuse(PLAN_UNSUPPORTED, "register file too large");
        R.hbm_waves = (uint32_t)std::max<size_t>(64, std::min<size_t>((size_t)in.n_cu * 4, ((size_t)1 << 30) / stride));
        B.gscratch = (size_t)R.hbm_waves * stride;
        S.gscratch_stride = (uint32_t)stride;
        R.lds_tiles_big = R.lds_normals_big = R.lds_points_big = 0;      // (no dynamic LDS for those launches; grids: blocks_big)
    }

    // pre-pass: with >= 3 levels the two coarsest levels are evaluated for all z-slabs at once
    S.n_slabs = R.n_slabs;
    S.pre_levels = prepass_ok ? std::min<uint32_t>(2, (uint32_t)ts.size() - 1) : 0;

    // root-tile layers of this part: layer k of the block split belongs to iz = k * nz / n_layers (iz = nz - 1: the front);
    // its z-slabs are those that hold one of its layers (a slab shared with another part has work for this part's layers only)
    uint32_t layer_lo = 0, layer_hi = n_layers;
    if (part.nz > 1) {
        layer_lo = n_layers; layer_hi = 0;
        for (uint32_t k = 0; k < n_layers; k++)
            if ((uint64_t)k * part.nz / n_layers == part.iz) { layer_lo = std::min(layer_lo, k); layer_hi = std::max(layer_hi, k + 1); }
        if (layer_lo >= layer_hi) layer_lo = layer_hi = 0;   // more parts than layers: nothing to do
    }
    R.slab_lo = layer_lo / SL; R.slab_hi = (layer_hi + SL - 1) / SL;
    if (!S.pre_levels) { R.slab_lo = layer_lo; R.slab_hi = layer_hi; }
    // root groups: runs of <= TL root tiles of this part, index = first + lane * stride (one set per slab in pre-pass mode)
    struct Run { uint32_t first, n, stride; };
    std::vector<Run> runs;
    if (part.nx > 1 || part.ny > 1) {       // a block of root-tile columns: per x, the run of its y range (x-major numbering)
        for (uint32_t tx = 0; tx < P.roots_x; tx++) {
            if ((uint64_t)tx * part.nx / P.roots_x != part.ix) continue;
            uint32_t y0 = P.roots_y, y1 = 0;
            for (uint32_t ty = 0; ty < P.roots_y; ty++)
                if ((uint64_t)ty * part.ny / P.roots_y == part.iy) { y0 = std::min(y0, ty); y1 = std::max(y1, ty + 1); }
            for (uint32_t ty = y0; ty < y1; ty += TL) runs.push_back(Run{tx * P.roots_y + ty, std::min<uint32_t>(TL, y1 - ty), 1});
        }
    } else {       // every n_shards-th root tile from `shard` on
        const uint32_t n_roots = P.roots_x * P.roots_y, mine = part.shard < n_roots ? (n_roots - part.shard + part.n_shards - 1) / part.n_shards : 0;
        for (uint32_t i = 0; i < mine; i += TL) runs.push_back(Run{part.shard + i * part.n_shards, std::min<uint32_t>(TL, mine - i), part.n_shards});
    }
    const FhTapeRef root{0, (uint32_t)t.n_ops, (uint16_t)t.n_regs, (uint16_t)t.n_choices};
    R.smooth_tape = t.n_ops > 200 && (size_t)t.n_choices * 10 < t.n_ops;
    // Column invariance at the ROOT: a root tape that reads no input varying along a pixel column, under a camera
    // that keeps x and y fixed along it, has the same interval, the same choices and the same pruned tape in every root tile of a
    // column of root tiles.  One layer per z-slab is evaluated (the slab's back-most: FhGroup::x = how many layers of the slab it stands
    // for) and the push stage hands the result to the stack - a fill with the nearest copy's depth, ONE queue entry carrying the copies,
    // exactly what the levels below do for column-invariant parents.  prospero.vm at 1024^3: 64 root tiles instead of 512.
    R.root_zrep = is3d && S.pre_levels > 0 && in.use_split && TL == 64 && R.column_inv;
    // ... and of such a frame ONLY THE FRONT SLAB is rendered at all.  Nothing the frame evaluates depends on z: every tile, every leaf of
    // a slab further back repeats the front slab's result for its column with a smaller depth - a filled tile is filled in front of it, a
    // leaf's hits are the front leaf's hits, a pixel the front slab left empty is outside the model at every z - and the image takes the
    // largest depth.  The slabs behind the first (prospero.vm at 1024^3: half the root level's children - the linked prune then runs
    // its workgroups in one round instead of two -, one of two tile chains, one of two leaf launches) are not queued.  (no_zrep 3: every
    // slab, as before.)
    R.front_only = R.root_zrep && in.no_zrep == 0;
    R.slab_stop = R.front_only && R.slab_hi > R.slab_lo ? R.slab_hi - 1 : R.slab_lo;
    uint32_t q0_layers = S.pre_levels ? layer_hi - layer_lo : 1;
    auto push_groups = [&](uint32_t z, uint32_t copies) {
        for (const Run& r : runs) {
            FhGroup g{};
            g.tape = root;
            g.first = r.first; g.n = r.n; g.stride = r.stride;
            g.z = z; g.x = copies;
            R.roots.push_back(g);
        }
    };
    if (R.root_zrep) {
        q0_layers = 0;
        for (uint32_t sb = R.slab_hi; sb-- > R.slab_stop;) {       // front slabs first
            const uint32_t lo = std::max(layer_lo, sb * SL), hi = std::min(layer_hi, (sb + 1) * SL);
            if (lo >= hi) continue;
            q0_layers++;
            push_groups(lo * ts[0], hi - lo);
        }
    } else
        for (uint32_t k = 0; k < q0_layers; k++) push_groups((layer_hi - 1 - k) * ts[0], 0);      // front layers first
    R.groups_per_slab = (uint32_t)(R.roots.size() / std::max<uint32_t>(q0_layers, 1));
    if (layer_lo >= layer_hi) { R.roots.clear(); R.groups_per_slab = 0; }

    // capacities (exact upper bounds): queue[l] holds the tiles of size ts[l-1] that can be
    // ambiguous, per slab for the per-slab levels and for the whole volume for pre-pass levels
    uint32_t qcaps[FH_MAX_LEVELS] = {0};
    qcaps[0] = std::max<uint32_t>((uint32_t)R.roots.size(), 1);
    for (size_t l = 1; l < ts.size(); l++) {
        const uint64_t tp = ts[l - 1];
        uint64_t c = (uint64_t)((P.width + tp - 1) / tp) * ((P.height + tp - 1) / tp) * (is3d ? P.slab / tp : 1);
        if (l < S.pre_levels) c *= R.n_slabs;
        qcaps[l] = (uint32_t)std::max<uint64_t>(c, 1);
    }
    for (size_t l = 0; l < ts.size(); l++) { S.qcap[l] = qcaps[l]; B.queue[l] = (size_t)qcaps[l] * sizeof(FhGroup); }
    S.squeue_cap = qcaps[S.pre_levels];
    if (S.pre_levels) B.squeue = (size_t)qcaps[S.pre_levels] * R.n_slabs * sizeof(FhGroup);
    const uint64_t tl = ts.back();
    const uint64_t fw = (P.width + tl - 1) / tl, fhh = (P.height + tl - 1) / tl;
    const uint64_t leaf_cap = fw * fhh * (is3d ? P.slab / tl : 1);
    R.table_words = is3d ? (uint32_t)leaf_cap : 0;
    R.n_footprints = (uint32_t)(fw * fhh);
    S.leaf_cap = (uint32_t)leaf_cap;
    B.leaves = leaf_cap * sizeof(FhLeaf);
    const size_t extra = std::min<uint32_t>(in.slab_contexts, std::max<uint32_t>(R.n_slabs, 1)) - 1;      // (slab contexts beyond the first)
    if (is3d) {
        if (P.width > 65535 || P.height > 65535) return refuse(PLAN_UNSUPPORTED, "3D renders support images up to 65535 x 65535");
        // (the assembly leaf and normals kernels address the z-buffer as base + a 32-bit byte offset of 8 bytes per pixel)
        if ((uint64_t)P.width * P.height >= ((uint64_t)1 << 29)) return refuse(PLAN_UNSUPPORTED, "3D renders support images of fewer than 2^29 pixels");
        B.leaves_b = extra * leaf_cap * sizeof(FhLeaf);
        B.leaf_table = leaf_cap * sizeof(FhLeafRef);
        B.leaf_table_b = extra * leaf_cap * sizeof(FhLeafRef);
        B.zbuf = (size_t)P.width * P.height * 8;
        B.normals = (size_t)P.width * P.height * 12;
        // (three footprint lists and the normals kernel's list of leaves with a hit: at most every leaf of a slab)
        // (a footprint's pixels name at most one leaf per layer of the slab; footprint i of the class lists goes to bucket i % 64)
        R.hit_bucket_cap = (uint32_t)(((size_t)R.n_footprints + FH_HIT_BUCKETS - 1) / FH_HIT_BUCKETS * (P.slab / tl));
        R.hit_words = (size_t)FH_HIT_BUCKETS * (FH_HIT_STRIDE + R.hit_bucket_cap);
        B.fp_lists = ((size_t)R.n_footprints * 3 + R.hit_words) * 4;
        B.fp_lists_b = extra * B.fp_lists;
        for (size_t l = 0; l < ts.size(); l++) R.mind_words += (size_t)((P.width + ts[l] - 1) / ts[l]) * ((P.height + ts[l] - 1) / ts[l]);
        B.mind = R.mind_words * 4;   // (cleared - empty image: nothing occluded - by the frame's first launch, upload_frame)
    }
    S.arena_cap = (uint32_t)std::min<size_t>(in.arena_bytes / 8 - 64, 0x7FFFFFE0u);  // slack: the interpreters prefetch up to 12 ops past a tape's end
    S.arena_head = S.arena_root_end = (uint32_t)t.n_ops;
    R.split = in.use_split && R.tl == 64;
    // (tapes with sin cos tan asin acos atan exp ln: the *_t variants of the tile kernels, which carry those interval handlers;
    // and, since round 5, those for atan2, mod, mix, rand)
    R.asm_tiles_t = !t.asm_ok && t.tiles_t_ok && !in.no_asm_tiles_t;
    // (not with a register file in HBM: the assembly tile kernels - fh_prune1, the groups path and the linked prune with them - keep
    // registers AND choices in LDS, and a tape of few registers can still outgrow it by its choices alone, ~5 600 of them)
    R.asm_tiles = R.split && in.use_asm && !in.no_asm_tiles && (t.asm_ok || R.asm_tiles_t) && t.n_regs <= 128 && !R.big_hbm;
    R.asm_tiles_t = R.asm_tiles_t && R.asm_tiles;
    // (left to the HIP kernels: tapes of more than 128 registers and register files in HBM)
    R.hip_tiles_unasked = !R.asm_tiles && R.split && in.use_asm && !in.no_asm_tiles;
    // levels whose forward pass exports its choices to the one-wave-per-child prune (fh_prune1): long tapes, few parents.
    // 3D: of the pre-pass levels, level 0 (measured); 2D: level 0
    R.exp_levels = is3d ? std::min(S.pre_levels, 1u) : 1u;
    R.prune1 = R.asm_tiles && !R.asm_tiles_t && R.exp_levels > 0;      // (the *_t kernels have no export mode)
    // tape parallelism: level 0 evaluates the root tree's terms as independent groups on different
    // waves, then the tree itself; the prune sees the root tape with its usual choices
    R.groups = R.prune1 && t.n_groups > 0 && !in.no_tape_groups;
    S.n_tgroups = 0;
    if (R.groups) {
        uint32_t off = (uint32_t)t.n_ops + 16, mr = 1, mc = 0;
        for (uint32_t g = 0; g < t.n_groups; g++) {
            const TapeFacts::Group& gt = t.group[g];
            S.tgroup[g] = FhTapeRef{off, gt.n_ops, (uint16_t)gt.n_regs, (uint16_t)gt.n_choices};
            off += gt.n_ops + 16;  // slack: the interpreters prefetch past a tape's end
            mr = std::max(mr, gt.n_regs); mc = std::max(mc, gt.n_choices);
        }
        R.group_regs = mr; R.group_choices = mc;
        R.lds_tiles_group = tiles_lds(mr, mc, TL);
        R.groups = mr <= 128 && R.lds_tiles_group <= FH_LDS_MAX && (size_t)off * 8 + 4096 <= in.arena_bytes;
        if (R.groups) {
            S.n_tgroups = t.n_groups;
            S.n_terms = t.n_terms; S.n_top = t.n_top; S.top_chain = t.chain ? 1 : 0;
            S.troot_len = (uint32_t)t.n_ops; S.troot_choices = t.n_choices; S.troot_regs = std::max<uint32_t>(t.n_regs, 1);
            S.arena_head = S.arena_root_end = off;
            const size_t blocks = qcaps[0];
            B.tvals = blocks * S.n_terms * WAVE * 8;
            B.topch = blocks * S.n_top * WAVE;
            B.chwr = blocks * S.n_tgroups * ((t.n_choices + 15) / 16) * WAVE * 4 + 256;
        }
    }
    if (R.prune1) {  // choice words of the pre-pass levels' forward passes: [slot][word][lane]
        uint32_t cap = 1;
        for (uint32_t l = 0; l < std::max(S.pre_levels, R.exp_levels); l++) cap = std::max(cap, qcaps[l] * (l == 0 && R.groups ? S.n_tgroups : 1u));
        const size_t words[2] = {(SMALL_CHOICES + 15) / 16, ((size_t)P.max_choices + 15) / 16};
        for (int k = 0; k < 2; k++) B.chw[k] = std::max<size_t>(cap * words[k] * 256, 256);
    }
    if (R.split) {
        uint32_t cap = 1;
        for (size_t l = 0; l < ts.size(); l++) cap = std::max(cap, qcaps[l] * (l == 0 && R.groups ? S.n_tgroups : 1u));
        B.slots = (size_t)cap * sizeof(FhSlot);
        S.slot_cap[0] = S.slot_cap[1] = cap;
    }
    S.arena_frame_end = S.arena_root_end;
    // (tiles of column-invariant parents are evaluated for one z-layer only: k_tape_flags)
    R.zrep = R.split && S.pre_levels > 0 && R.xy_fixed && !in.no_column_inv && in.no_zrep != 1;
    if (((size_t)t.n_ops + 64) * 8 > in.arena_bytes) return refuse(PLAN_UNSUPPORTED, "tape larger than the arena");
    // level-0 groups sit at the back of queue[0] (the "big" half), in reverse order
    std::reverse(R.roots.begin(), R.roots.end());
    return PlanStatus{};
}

// The linked prune of the root level (option prune2; prune2.hip): 0.275 ms against fh_prune1's 0.344 per 1024^3 frame of prospero.vm (a
// child of that root tape keeps ~580 ops, up to 1011); fh_prune1 stays behind it for the children it leaves marked (more than 64
// registers / FH_P2_MAX_KEPT ops).  For a frame plan_frame gave the groups path; `has_links`, `n_chain`: the tape's links and choice table
// exist on the device, the ops of its root chain - known once the tape's root tables have been made (prepare() ensure_root_tables).
static void plan_linked_prune(const TapeFacts& t, const PlanInputs& in, bool has_links, uint32_t n_chain, RenderSetup& R) {
    R.p2_cap_kept = (uint32_t)FH_P2_MAX_KEPT;
    R.lds_prune2 = (size_t)FH_P2_WPB * fh_p2_wave_lds(t.n_choices, R.p2_cap_kept) + (((size_t)n_chain * 4 + 15) & ~(size_t)15);
    R.n_chain = n_chain;
    // (one workgroup of FH_P2_WPB children per CU: beyond two rounds of them - 2048^3 has 4 096 root tiles - the scalar sweep,
    // whose waves all fit the machine at once, is the faster one again: 2.09 against 2.17 ms per frame)
    R.prune2 = R.groups && has_links && linked_root_tape(t, in) && R.lds_prune2 <= FH_LDS_MAX &&
               R.roots.size() * 64 <= (size_t)2 * in.n_cu * FH_P2_WPB;      // (a root group = up to 64 root tiles)
}

// ---- clean buffer sets ---------------------------------------------------------------------------------------------------------
// A 3D frame starts from a z-buffer, normals and a min-depth pyramid that are all zero.  k_finish3d, the last kernel to touch them, reads
// every z-buffer word anyway and can hand the set back that way (`leave_clean`: it zeroes what the frame wrote); the next frame of the
// set then clears nothing (k_frame_begin: 20 MB of stores at 1024^2, at the head of the frame's longest chain).  What a set was left clean
// FOR is recorded with the set on the host: the pixels and the pyramid words k_finish3d went over.  A frame whose own numbers are the
// record's skips the clears; any other frame clears everything, as a set's first frame does.  The record is dropped when a frame starts
// and written when the frame has been queued to its end with a k_finish3d that cleans: a frame that was cancelled or failed half way, a
// frame whose image goes to the host and a profiled frame leave none.
struct CleanSig {
    bool valid = false;
    uint64_t pixels = 0, mind_words = 0;
};
// What kind of frame it is, for the rule
struct CleanFrame {
    bool out_is_device = true, profiling = false;
};
// Does this frame's k_finish3d clean behind itself (and, queued to its end, leave a record)?
static bool leaves_set_clean(const CleanFrame& f) { return f.out_is_device && !f.profiling; }
// May the frame skip its clears?  `left`: the set's record; `want`: what this frame needs cleared
static bool set_is_clean(const CleanSig& left, const CleanSig& want) {
    return left.valid && want.valid && left.pixels == want.pixels && left.mind_words == want.mind_words;
}
// The record a frame leaves: none unless it ran to its end (`queued_whole`) with a cleaning k_finish3d
static CleanSig set_left_by(const CleanFrame& f, const CleanSig& want, bool queued_whole) {
    CleanSig s = want;
    s.valid = want.valid && queued_whole && leaves_set_clean(f);
    return s;
}
