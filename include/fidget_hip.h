/* fidget_hip.h — C ABI of libfidget_hip.so: the MI355X (gfx950) backend for Fidget's
 * evaluation hot path.
 *
 * This is the drop-in boundary.  A Rust crate `fidget-hip` binds these symbols
 *  and implements fidget_core::eval::{Function, MathFunction,
 * Tape, TracingEvaluator, BulkEvaluator} + render::RenderHints on top of them, the
 * same way `fidget-jit` wraps `VmData` and replaces only tapes and evaluators
 * (/root/reference/fidget-jit/src/lib.rs:872-998).  Every entry point names the
 * reference interface it replaces.
 *
 * Conventions: plain C, no unwinding; every call returns an fhip_status; all
 * `const T*` / `T*` arguments are CALLER-OWNED HOST buffers unless a parameter is
 * documented as a device pointer; one fhip_ctx per host thread / HIP stream
 * (evaluators in the reference are per-thread too, fidget-raster/src/lib.rs:129-133).
 */
#ifndef FIDGET_HIP_H
#define FIDGET_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fhip_status {
    FHIP_OK = 0,
    FHIP_ERR_BAD_VAR_SLICE = 1,     /* var/mod.rs:151-165  TracingArgError / BulkArgError::BadVarSlice */
    FHIP_ERR_MISMATCHED_SLICES = 2, /* var/mod.rs:167-197  BulkArgError::MismatchedSlices */
    FHIP_ERR_BAD_CHOICE_SLICE = 3,  /* vm/data.rs:129-134  BadTrace(BadChoiceSlice) */
    FHIP_ERR_MISSING_VAR = 4,       /* shape/mod.rs:391-396 MissingVar */
    FHIP_ERR_BAD_TAPE = 5,          /* malformed bytecode / bad node (context BadNode) */
    FHIP_ERR_UNSUPPORTED = 6,       /* e.g. > 256 live registers, tile fan-out > 64 */
    FHIP_ERR_HIP = 7,               /* a HIP runtime call failed; see fhip_last_error */
    FHIP_ERR_CANCELLED = 8,         /* render/config.rs:38-80 CancelToken */
    FHIP_ERR_PARSE = 9,             /* context/mod.rs ParseError */
    FHIP_ERR_OVERFLOW = 10          /* a device work queue overflowed (sizes are bounds; should not happen) */
} fhip_status;

typedef struct fhip_ctx fhip_ctx;     /* device, stream, scratch pools        */
typedef struct fhip_tape fhip_tape;   /* one compiled function (host + device) */
typedef struct fhip_graph fhip_graph; /* host mirror of fidget_core::Context   */

/* ---- context ------------------------------------------------------------------------ */
/* `stream` is a hipStream_t (NULL = the default stream), e.g. torch's current stream. */
fhip_status fhip_ctx_create(int device, void* stream, fhip_ctx** out);
void fhip_ctx_destroy(fhip_ctx* ctx);
const char* fhip_last_error(const fhip_ctx* ctx);
fhip_status fhip_ctx_sync(fhip_ctx* ctx);
/* Gives back the device and pinned memory a context keeps between calls for speed alone: the mesher's leaf records (17 GB after a
 * depth-10 build) - the same buffer holds the scratch of fhip_triangles_voxels, 64 bytes per triangle of the largest mesh so far -
 * its landing area, the frame lanes (child contexts with buffers of their own - up to four, each a context's worth of
 * buffers: option frame_lanes).  Waits for the context's work; whatever is needed again is made again by the call that needs it. */
fhip_status fhip_ctx_trim(fhip_ctx* ctx);
/* The tape arena of a buffer set is sized by need: 128 MB, or about a byte per voxel for a 3D frame whose root tape reads an input that
 * changes along a pixel column, grown when a frame ran out (that frame is still right: its tiles kept their parents' tapes - and many
 * times slower), never beyond option arena_mb.  A caller that knows better - a sequence of frames of a heavier model to come - says
 * so here: every set's arena is at least `megabytes` from the next frame on (capped by arena_mb).  Waits for the context's own work. */
fhip_status fhip_ctx_reserve_arena(fhip_ctx* ctx, size_t megabytes);
/* The device evaluates sin cos tan asin acos atan atan2 exp ln with the routines of glibc 2.35's x86-64 libm (its FMA variants)
 * restated operation by operation (fidget_amd/csrc/trans_libm.hpp) - the libm the reference's f32 methods call on the deployment
 * image, whose values its own bulk test demands bit for bit (fidget-core/src/eval/test/float_slice.rs:404-412).  On a host with
 * ANOTHER libm (glibc >= 2.41's CORE-MATH routines, a CPU without FMA, musl) the reference's CPU evaluators - and this repository's
 * oracle - return other bits for some arguments, and a comparison of device against host values fails for that reason alone.
 * This call says so: 32 arguments per routine (ordinary values, the reduction's range boundaries, tiny and huge ones) through the
 * restated routines compiled for the host against the RUNNING libm; returns the number that differ (0: this host's libm is the one
 * the device restates) and, when `msg` is given, the first difference by name - "sinf(0x1.8p+1): device family 0x..., host libm
 * 0x...".  No device is touched.  fhip_ctx_create runs it once per process and prints the message to stderr if there is one
 * (FHIP_QUIET=1: does not). */
int fhip_libm_probe(char* msg, size_t cap);
/* render/config.rs:38-80: cooperative cancellation, honoured between kernel waves */
void fhip_cancel(fhip_ctx* ctx);
void fhip_cancel_reset(fhip_ctx* ctx);
/* A cancel flag of the caller's - one byte, non-zero = cancel - that the context's checks read beside its own until fhip_cancel_watch(ctx,
 * NULL): fidget_core::render::CancelToken (render/config.rs:38-78) is an Arc<AtomicBool> whose address into_raw() hands out, so the
 * Rust crate passes the EvalConfig's token for the duration of a render (voxel.rs:52-61; its cancel_render test, voxel.rs:573-590) and
 * a cancel from any thread ends the render with FHIP_ERR_CANCELLED.  The byte must stay valid while it is watched. */
void fhip_cancel_watch(fhip_ctx* ctx, const void* flag);
/* Behaviour switches of a context (the role of the reference's config structs - ThreadPool / TileSizes / RenderConfig carry
 * the reference's knobs; these carry the back end's own: which kernels, how many slab contexts, the column-invariance short
 * cuts ...).  A context reads FHIP_<NAME> from the environment ONCE, when it is created; afterwards only this call changes
 * a switch - a render never consults the environment.  It waits for the context's frames in flight first.  Names and
 * defaults: FH_OPTION_LIST in fidget_amd/csrc/capi_core.hpp; e.g. "no_column_inv", "frame_lanes",
 * "arena_mb".  Unknown names (and the two that are fixed at creation) return FHIP_ERR_UNSUPPORTED. */
fhip_status fhip_ctx_set_option(fhip_ctx* ctx, const char* name, int value);
fhip_status fhip_ctx_get_option(const fhip_ctx* ctx, const char* name, int* value);

/* ---- tapes -------------------------------------------------------------------------- */
/* The wire format produced by fidget_bytecode::Bytecode::new(&VmData)
 * (fidget-bytecode/src/lib.rs:11-42, 203-332).  Replaces JitFunction's
 * `point_tape/interval_tape/float_slice_tape/grad_slice_tape` compilation
 * (fidget-jit/src/lib.rs:875-908): one device tape serves all four evaluators.
 * Variable slots are the reference's VarMap indices, any number of them (input slots below 2^20).  The evaluators and
 * fhip_solve take every tape; renders and meshes of a tape that reads more than 16 input slots run its bound tape, the same
 * ops with the bound variables as immediates (BOUND_TAPES.md): the same image, FHIP_ERR_MISSING_VAR before any launch. */
fhip_status fhip_tape_from_bytecode(fhip_ctx* ctx, const uint32_t* words, size_t n_words, fhip_tape** out);
void fhip_tape_free(fhip_tape* tape);
uint32_t fhip_tape_len(const fhip_tape* tape);          /* Function::size      eval/mod.rs:171 */
uint32_t fhip_tape_choice_count(const fhip_tape* tape); /* Function::can_simplify != 0 */
uint32_t fhip_tape_reg_count(const fhip_tape* tape);
uint32_t fhip_tape_var_count(const fhip_tape* tape);    /* Tape::vars().len()  eval/mod.rs:41 */
uint32_t fhip_tape_output_count(const fhip_tape* tape); /* Tape::output_count  eval/mod.rs:47 */
/* Copy the device-format ops (8 bytes each, evaluation order) to `ops`; returns the length */
uint32_t fhip_tape_ops(const fhip_tape* tape, uint64_t* ops, uint32_t cap);
/* The tape as the reference's VmData<N> holds it: RegTape::new::<N> (fidget-core/src/compiler/reg_tape.rs:26-32) - the
 * single-pass RegisterAllocator<N> with its LRU eviction and Load / Store spills to memory slots >= N
 * (compiler/alloc.rs:13-708, compiler/lru.rs:19-76) - over this tape's ops, and Bytecode::new of that
 * (fidget-bytecode/src/lib.rs:203-332).  Host side only; what the device runs is the library's own dense allocation.
 * reg_ops (may be NULL): 4 words per RegOp in evaluation order (VmData::iter_asm, vm/data.rs:320-323): opcode (tape_format.h FhOp; 52
 * Load, 53 Store), out, a (lhs / the stored register), then b, or the immediate bits, or the input / output / memory slot.
 * words (may be NULL): the bytecode, start and end markers included.  info = { RegTape::len(), RegTape::slot_count(),
 * Bytecode::reg_count, Bytecode::mem_count }.  1 <= n_regs <= 255.  FHIP_ERR_UNSUPPORTED: the reserved register 255 would be in
 * use (lib.rs ReservedRegister); info[0..1] are valid then. */
fhip_status fhip_tape_reg_tape(const fhip_tape* tape, uint32_t n_regs, uint32_t* reg_ops, uint32_t cap_ops, uint32_t* words,
                               uint32_t cap_words, uint32_t info[4]);

/* Tape parallelism (no counterpart in the reference): when the root of the function is a min / max
 * of many parts, the same function as `count` independent tapes whose outputs combine, in order,
 * with FH_MIN_RR (30) / FH_MAX_RR (31).  The renderers evaluate the root level that way; exposed
 * for tests.  0 groups = the tape does not split. */
uint32_t fhip_tape_group_count(const fhip_tape* tape);
int fhip_tape_group_op(const fhip_tape* tape);
fhip_status fhip_tape_group(fhip_ctx* ctx, const fhip_tape* tape, uint32_t g, fhip_tape** out);
/* The form of that split the 3D renderer uses at its root level: groups that output the terms of the
 * root min / max tree, the tree as a small program over them, and a table saying where each choice of
 * the full tape is recorded.  Returns the number of groups (0: not split);
 * info = { terms, tree ops, tree registers, choices covered (= fhip_tape_choice_count) }. */
uint32_t fhip_tape_term_plan(const fhip_tape* tape, uint32_t info[4]);
/* ... its parts, for tests: group g as a tape of its own (its OUTPUT ops carry the term index);
 * the tree, 3 words per op: op | out << 8 | a_kind << 16 | b_kind << 24 (kinds: 0 tree register, 1 term,
 * 2 immediate bits), a, b (returns the number of ops); and per choice of the full tape, in tape order,
 * where it is recorded: group << 24 | choice index there, group 255 = op index of the tree. */
fhip_status fhip_tape_term_group(fhip_ctx* ctx, const fhip_tape* tape, uint32_t g, fhip_tape** out);
uint32_t fhip_tape_term_tree(const fhip_tape* tape, uint32_t* words, uint32_t cap_ops);
uint32_t fhip_tape_term_choice_src(const fhip_tape* tape, uint32_t* src, uint32_t cap);

/* Function::simplify (eval/mod.rs:147-160; VmData::simplify vm/data.rs:123-318).
 * `choices` is one byte per choice op in evaluation order, values 1/2/3 = Left/Right/Both. */
fhip_status fhip_simplify(fhip_ctx* ctx, const fhip_tape* tape, const uint8_t* choices, uint32_t n_choices,
                          fhip_tape** child);

/* ---- evaluators (trait surface; batched over n samples) ----------------------------- */
/* TracingEvaluator<Data = Interval>::eval (eval/tracing.rs:26-64, vm/mod.rs:325-538).
 * vars: [n][n_vars][2] (lo,hi); out: [n][n_outputs][2]; choices: [n][choice_count] or NULL;
 * simplify: [n] (1 = a trace would be returned) or NULL.  n_vars may exceed the tape's. */
fhip_status fhip_interval_eval(fhip_ctx* ctx, const fhip_tape* tape, const float* vars, uint32_t n_vars, uint32_t n,
                               float* out, uint8_t* choices, uint8_t* simplify);
/* TracingEvaluator<Data = f32>::eval (vm/mod.rs:543-760).  vars: [n][n_vars]; out: [n][n_outputs] */
fhip_status fhip_point_eval(fhip_ctx* ctx, const fhip_tape* tape, const float* vars, uint32_t n_vars, uint32_t n,
                            float* out, uint8_t* choices, uint8_t* simplify);
/* BulkEvaluator<Data = f32>::eval (eval/bulk.rs:23-58, vm/mod.rs:794-1086).
 * vars[i] -> lens[i] floats (all lens must be equal, else MISMATCHED_SLICES);
 * out[o] -> n floats for each of the tape's outputs. */
fhip_status fhip_float_eval(fhip_ctx* ctx, const fhip_tape* tape, const float* const* vars, const uint32_t* lens,
                            uint32_t n_vars, float* const* out);
/* BulkEvaluator<Data = Grad>::eval (vm/mod.rs:1091-1397).  Grad = {v,dx,dy,dz} (types/grad.rs:4-13) */
fhip_status fhip_grad_eval(fhip_ctx* ctx, const fhip_tape* tape, const float* const* vars, const uint32_t* lens,
                           uint32_t n_vars, float* const* out);

/* ---- constraint solver ---------------------------------------------------------------
 * fidget::solver::solve (fidget-solver/src/lib.rs:191-289), batched: n_instances independent Levenberg-Marquardt solves of the
 * same constraints, in one launch.  Residual i is output 0 of constraints[i].  Parameter p names a variable as fhip_graph_var
 * does (param_axis 0 X, 1 Y, 2 Z, 3 Var::V(param_index[p])); param_free[p] != 0 makes it free.  A variable a tape reads that no
 * parameter names evaluates as 0.  values: [n_instances][n_params], the start of a free parameter or the value of a fixed one.
 * out: [n_instances][n_free], the free parameters in parameter order; err: [n_instances] the error sum_i r_i^2 at the result
 * (0 after FHIP_SOLVE_ZERO_RESIDUAL, +inf if no step was accepted); iterations: accepted steps; exit_reason: FHIP_SOLVE_*.
 * err, iterations and exit_reason may be NULL.  max_iterations = 0: 1000.  Differences from the reference (the free
 * variables' order, the caps, the linear solve): SOLVER.md.  FHIP_ERR_UNSUPPORTED: more than 64 free parameters;
 * FHIP_ERR_BAD_VAR_SLICE: a variable named twice, an axis outside 0..3; FHIP_ERR_BAD_TAPE: a constraint with no output -
 * each returned before any launch.  Blocking; host buffers. */
#define FHIP_SOLVE_ZERO_RESIDUAL 0   /* every residual exactly 0 */
#define FHIP_SOLVE_NO_CHANGE 1       /* the accepted step changed no free parameter */
#define FHIP_SOLVE_ZERO_ERROR 2      /* the error of the accepted step is 0 */
#define FHIP_SOLVE_ZERO_DAMPING 3    /* the damping underflowed to 0 */
#define FHIP_SOLVE_STALLED 4         /* the last four errors are equal */
#define FHIP_SOLVE_MAX_ITERATIONS 5  /* max_iterations steps accepted */
#define FHIP_SOLVE_MAX_RETRIES 6     /* 128 trial steps in a row rejected */
fhip_status fhip_solve(fhip_ctx* ctx, const fhip_tape* const* constraints, uint32_t n_constraints, const int32_t* param_axis,
                       const uint64_t* param_index, const uint8_t* param_free, uint32_t n_params, const float* values,
                       uint32_t n_instances, uint32_t max_iterations, float* out, float* err, uint32_t* iterations,
                       int32_t* exit_reason);

/* ---- batched renders (the throughput path) ------------------------------------------ */
/* fidget_raster::pixel::{RenderConfig, EvalConfig} (fidget-raster/src/pixel.rs:27-57) */
typedef struct fhip_render2d_config {
    uint32_t width, height;
    const float* world_to_model;   /* row-major 3x3, NULL = identity */
    float z;
    int pixel_perfect;
    const uint32_t* tile_sizes;    /* NULL = RenderHints::tile_sizes_2d() of the HIP shape: {128,16}, as fidget-jit (fidget-jit/src/lib.rs:984-986):
                                    * 64 children per parent.  Fills carry the level they were decided at (pixel.rs:225-229), so images
                                    * compare bit for bit with the reference rendered with the same tile sizes */
    uint32_t n_tile_sizes;
    const uint64_t* var_keys;      /* ShapeVars<f32>: Var::V index -> value */
    const float* var_values;
    uint32_t n_vars;
    const int32_t* axis_slots;     /* VarMap slot of X, Y, Z (-1 = absent); NULL = use the tape's own map */
} fhip_render2d_config;
/* fidget_raster::voxel::{RenderConfig, EvalConfig} (fidget-raster/src/voxel.rs:25-54) */
typedef struct fhip_render3d_config {
    uint32_t width, height, depth;
    const float* world_to_model;   /* row-major 4x4, NULL = identity */
    const uint32_t* tile_sizes;    /* NULL = RenderHints::tile_sizes_3d() of the HIP shape: the root tile the VmShape hints give for this
                                    * image size, then fan-out 4^3: {128,32,8} - or {32,8} when the root level has few tiles (a small
                                    * image, a part of a frame, a model without z).  Any list TileSizes::new accepts
                                    * (render/mod.rs:181-251) is accepted; one the kernels cannot take as given (leaves other than 8,
                                    * fan-out above 64) is replaced by the library's: a 3D image does not depend on the tile sizes */
    uint32_t n_tile_sizes;
    const uint64_t* var_keys;
    const float* var_values;
    uint32_t n_vars;
    const int32_t* axis_slots;
} fhip_render3d_config;

/* fidget_raster::pixel::render (pixel.rs:452-492).  out: width*height RawDistancePixel (f32
 * bit patterns, pixel.rs:159-241); a device pointer when out_is_device != 0, in which case
 * the call is asynchronous on the context's stream. */
fhip_status fhip_render2d(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render2d_config* cfg, float* out,
                          int out_is_device);
/* fidget_raster::voxel::render (voxel.rs:500-553).  out: width*height GeometryPixel
 * {f32 normal[3]; u32 depth} (voxel.rs:122-134).
 * Asynchronous renders (out_is_device) of one context are pipelined across frames: the context keeps four sets of device
 * buffers, and the coarse tile levels of a frame run on an internal stream beside the slabs of the frame before it.  For the
 * caller nothing changes: `out` is written on the context's stream, in call order; fhip_ctx_sync waits for every frame. */
fhip_status fhip_render3d(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                          int out_is_device);
/* Multi-GPU 3D, partition A: render only the root-tile columns whose index (x-major, lib.rs:116-123) satisfies
 * index % n_shards == shard, at full depth (front-to-back culling intact).  Other pixels are left {0,0,0,0}: every pixel is
 * produced by exactly one shard, so the partial images combine with an integer SUM of the raw words (or a gather). */
fhip_status fhip_render3d_shard(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                                int out_is_device, uint32_t shard, uint32_t n_shards);
/* Multi-GPU 3D, partition B (the octant split): block `index` = ix + split[0] * (iy + split[1] * iz) of a
 * split[0] x split[1] x split[2] division of the volume: blocks of root-tile columns in x and y, of z-slabs (root-tile
 * layers) in z; iz = split[2] - 1 is nearest the camera.  Pixels outside the block's columns stay {0,0,0,0}.  Blocks
 * that differ only in iz cover the same pixels and combine with fhip_merge_depth, front range first. */
fhip_status fhip_render3d_block(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                                int out_is_device, uint32_t index, const uint32_t split[3]);
/* The stitch rule of voxel.rs:527-550 across z ranges, in place on `front` (device pointers, n_pixels GeometryPixel each):
 * the larger depth wins, a tie keeps `front` (a hit there carries the normal; the equal depth on the other side is a
 * filled tile's z + T + 1, which has none), then depth >= image_depth - 1 -> (image_depth, [0, 0, 1]). */
fhip_status fhip_merge_depth(fhip_ctx* ctx, void* front, const void* back, uint64_t n_pixels, uint32_t image_depth);

/* ---- post-processing: fidget_raster::effects (fidget-raster/src/effects.rs) --------------------
 * The step right after a render; images are width*height arrays as the renders produce them.  With on_device != 0
 * every pointer is a device pointer and the call is asynchronous on the context's stream (the image a render just
 * left in HBM is consumed in place); otherwise host buffers. */
/* denoise_normals (effects.rs:17-36, denoise_pixel 252-326): GeometryPixel image -> GeometryPixel image */
fhip_status fhip_denoise_normals(fhip_ctx* ctx, const void* image, uint32_t width, uint32_t height, void* out, int on_device);
/* compute_ssao (effects.rs:73-95, compute_pixel_ssao 156-250): out = width*height f32, NaN where depth == 0.  The
 * reference draws the sampling kernel (3 x n_kernel, ssao_kernel 395-424) and the rotation noise (2 x n_noise,
 * ssao_noise 430-448) from rand::rng(); here the caller passes them: kernel[i*3 + {0,1,2}], noise[i*2 + {0,1}]. */
fhip_status fhip_compute_ssao(fhip_ctx* ctx, const void* image, uint32_t width, uint32_t height, uint32_t depth, const float* kernel,
                              uint32_t n_kernel, const float* noise, uint32_t n_noise, float* out, int on_device);
/* blur_ssao (effects.rs:98-115, compute_pixel_blur 329-392) */
fhip_status fhip_blur_ssao(fhip_ctx* ctx, const float* ssao, uint32_t width, uint32_t height, float* out, int on_device);
/* apply_shading (effects.rs:42-67, shade_pixel 118-153): ssao = blurred occlusion map or NULL; out = width*height*3 bytes */
fhip_status fhip_apply_shading(fhip_ctx* ctx, const void* image, uint32_t width, uint32_t height, uint32_t depth, const float* ssao,
                               uint8_t* out_rgb, int on_device);
/* RawDistancePixel image -> RGBA8: mode 0 to_rgba_bitmap (effects.rs:443-464), 1 the same with transparent = true,
 * 2 to_debug_bitmap (467-496), 3 to_rgba_distance (506-547) */
fhip_status fhip_to_rgba(fhip_ctx* ctx, const float* image, uint32_t width, uint32_t height, int mode, uint8_t* out_rgba, int on_device);

/* ---- meshing: the evaluation side of fidget_mesh::Octree::build (fidget-mesh/src/octree.rs) -----------------
 * Octree cells of [-1, 1]^3 to `depth` (Settings::depth), classified by interval evaluation (recurse, octree.rs:521-583), and
 * every ambiguous cell of the last level sampled as leaf() does (octree.rs:590-862): corner mask, Manifold Dual Contouring
 * edges, 4 x 16-point edge search, intersections, gradients, one QEF vertex per cell vertex.  What has no evaluation in it
 * (cell collapse, the dual walk) stays with the caller.  Leaf record (fhip_mesh_counts out[4] bytes, 528): f32 bounds[6]
 * (x.lo x.hi y.lo y.hi z.lo z.hi); u64 path (3 bits per level, leading 1); u32 mask, n_edges, n_verts, pad; u16 inter[12][3]
 * (+ 4 u16 pad); f32 pos[12][3]; f32 grad[12][4] (dx dy dz v); f32 vert[4][3]; f32 qef_err[4].  mask 0 / 255: the cell turned
 * out Empty / Full at its corners (n_edges = 0). */
typedef struct fhip_mesh fhip_mesh;
fhip_status fhip_mesh_sample(fhip_ctx* ctx, const fhip_tape* tape, uint32_t depth, const float* world_to_model, const int32_t* axis_slots,
                             const uint64_t* var_keys, const float* var_values, uint32_t n_vars, fhip_mesh** out);
/* fidget_mesh::Octree::build + Octree::walk_dual (octree.rs:48-68, 219-225; Settings: depth, world_to_model): fhip_mesh_sample, then
 * the octree assembled from the device's results - cell collapse (check_done / try_collapse, octree.rs:256-385) with the merged
 * Hermite data included - ON THE DEVICE, level by level, and the dual walk (dc.rs, builder.rs) on the device too: the recursion's calls
 * as level arrays in call order, MeshBuilder's numbering by first use through atomic minima and prefix sums (neither the leaf records
 * nor the octree leave HBM: the host receives the mesh) -> Mesh { vertices, triangles } (lib.rs:64-69): the cells, vertices and
 * triangles of the single-threaded recursion, in its order.  Tapes of 256 ops and more are simplified once on the way down
 * (octree.rs:546-553; option "mesh_simplify_min_ops", 0 = never): the mesh does not depend on it.  Context option "mesh_device_walk" 0:
 * the walk on the host's threads (independent sub-walks; FHIP_MESH_THREADS, default: all cores up to 32); "mesh_device_assembly" 0: the assembly on the
 * host's threads too (independent subtrees, as build_inner_mt octree.rs:94-210), from copies of the levels and the leaf records -
 * the path fhip_mesh_merge takes; same per-cell functions, same octree.  The leaf records are not kept with the mesh
 * (fhip_mesh_leaves after a build copies nothing). */
fhip_status fhip_mesh_build(fhip_ctx* ctx, const fhip_tape* tape, uint32_t depth, const float* world_to_model, const int32_t* axis_slots,
                            const uint64_t* var_keys, const float* var_values, uint32_t n_vars, fhip_mesh** out);
void fhip_mesh_vertices(const fhip_mesh* mesh, float* out);        /* counts[6] x 3 floats */
void fhip_mesh_triangles(const fhip_mesh* mesh, uint64_t* out);    /* counts[7] x 3 vertex indices */
/* The same arrays where the mesh holds them, without a copy (15 M triangles are 360 MB: a tenth of a second of a 0.35 s build) - what
 * `Mesh { vertices, triangles }` (fidget-mesh/src/mesh.rs) can borrow or take; valid until fhip_mesh_free. */
const float* fhip_mesh_vertices_ptr(const fhip_mesh* mesh);
const uint64_t* fhip_mesh_triangles_ptr(const fhip_mesh* mesh);
void fhip_mesh_free(fhip_mesh* mesh);
/* out = {cells interval-evaluated, Full, Empty, ambiguous cells at the leaf depth, bytes per leaf record, levels visited,
 *        mesh vertices, mesh triangles} */
void fhip_mesh_counts(const fhip_mesh* mesh, uint64_t out[8]);
void fhip_mesh_leaves(const fhip_mesh* mesh, void* out);
/* The build sharded by the root's octants, as Octree::build_inner_mt hands the root's eight children to its workers
 * (octree.rs:94-123) - here to up to eight GPUs.  fhip_mesh_sample_part runs the device side (cell classification, leaf
 * sampling) for the octants o with o * n_parts / 8 == part (8 parts: one octant each; 2 parts: the z halves); every part
 * evaluates the root cell itself.  Its results - per level the cells' classes and slots, and the leaf records - are written
 * as one flat buffer by fhip_mesh_part_export (fhip_mesh_part_bytes long), which is what travels between processes.
 * fhip_mesh_merge takes the buffers of ALL parts (parts[k] = part k), puts the level arrays together (build_inner_mt's index
 * remapping, octree.rs:176-195: slots of later parts shifted by the ambiguous cells before them), and runs octree assembly
 * (check_done on the merged tree, octree.rs:197-208) and the dual walk: the mesh is the one fhip_mesh_build gives on one GPU,
 * vertex for vertex and triangle for triangle.  The buffers (8-byte aligned) are only read during the call.  A merge needs no
 * device; with a context it reuses the context's host-side caches. */
fhip_status fhip_mesh_sample_part(fhip_ctx* ctx, const fhip_tape* tape, uint32_t depth, const float* world_to_model, const int32_t* axis_slots,
                                  const uint64_t* var_keys, const float* var_values, uint32_t n_vars, uint32_t part, uint32_t n_parts, fhip_mesh** out);
uint64_t fhip_mesh_part_bytes(const fhip_mesh* mesh);
void fhip_mesh_part_export(const fhip_mesh* mesh, void* out);
fhip_status fhip_mesh_merge(fhip_ctx* ctx, const void* const* parts, const uint64_t* part_bytes, uint32_t n_parts, const float* world_to_model,
                            fhip_mesh** out);
/* The mesh where the device left it.  Context option "mesh_keep_device" (default 0) = 1: a mesh that fhip_mesh_build makes with the
 * device walk keeps `Mesh { vertices, triangles }` (fidget-mesh/src/lib.rs:64-69) in device memory as well - n x 3 f32 and n x 3 u64,
 * the arrays of fhip_mesh_vertices_ptr / fhip_mesh_triangles_ptr - for a consumer on the device.  They belong to the mesh:
 * fhip_mesh_free frees them, fhip_ctx_trim does not touch them.  NULL when the arrays are not resident: the option was off, the walk
 * ran on the host ("mesh_device_walk" 0, an octree beyond the device walk's limits), the mesh came from fhip_mesh_merge, or it is empty. */
const float* fhip_mesh_vertices_dev(const fhip_mesh* mesh);
const uint64_t* fhip_mesh_triangles_dev(const fhip_mesh* mesh);
/* Mesh::write_stl (fidget-mesh/src/output.rs:5-38) on the device: the binary STL file of the mesh, byte for byte - the 44 bytes of header
 * text zero-padded to 80, the triangle count as a little-endian u32, then 50 bytes per triangle: normal = (b - a) x (c - a) in f32, not
 * normalised (output.rs:20-26), the corners a, b, c, two zero bytes (output.rs:27-35).  The cross product is nalgebra's, which is not
 * vendored with the reference: x = u.y v.z - u.z v.y, y = u.z v.x - u.x v.z, z = u.x v.y - u.y v.x, each product and each difference
 * rounded to f32, is recalled from its source and could not be verified against it; another order of the same operands can only change
 * the sign of a zero.  fhip_mesh_stl_bytes = 84 + 50 x triangles is the size of `out`.  Resident arrays (above) are read in place; a mesh
 * without them has its host arrays uploaded first.  out_is_device != 0: `out` is a device pointer (4-byte aligned) and the call is
 * asynchronous on the context's stream; otherwise the bytes arrive in the host buffer through the context's pinned landing area.
 * FHIP_ERR_UNSUPPORTED before any launch: 2^32 triangles or more (the format's count is 32 bits wide). */
uint64_t fhip_mesh_stl_bytes(const fhip_mesh* mesh);
fhip_status fhip_mesh_stl(fhip_ctx* ctx, const fhip_mesh* mesh, void* out, int out_is_device);
/* BulkEvaluator<Data = Grad>::eval (VmGradSliceEval::eval, vm/mod.rs:1091-1397) at the mesh's vertices, without the round trip through
 * the host that fhip_grad_eval needs: out = n_vertices x Grad {v, dx, dy, dz} (types/grad.rs:4-13) of `tape` at vertex i, x / y / z
 * seeded (1,0,0) / (0,1,0) / (0,0,1), every Var::V bound to its value with a zero gradient.  The vertices are in model space already
 * (octree.rs:58-65), so no transform is applied: the gradient is the model-space one, unnormalised as GeometryPixel::normal
 * (voxel.rs:122-134), and v says how far the vertex sits from the surface.  `tape`: any one-output tape (FHIP_ERR_BAD_TAPE otherwise), of
 * any number of input slots; the variable arguments are fhip_mesh_build's (FHIP_ERR_MISSING_VAR likewise).  The whole tape runs at every
 * vertex.  out_is_device != 0: a device pointer (16-byte aligned), asynchronous on the context's stream when the arrays are resident. */
fhip_status fhip_mesh_vertex_grads(fhip_ctx* ctx, const fhip_tape* tape, const fhip_mesh* mesh, const int32_t* axis_slots,
                                   const uint64_t* var_keys, const float* var_values, uint32_t n_vars, float* out, int out_is_device);

/* ---- shape occupancy: volume, centroid, second moments and bounds of a solid, as exact integer sums ----------
 * The region is the mesher's cube [-1, 1]^3 (carried into model space by world_to_model as fhip_mesh_build does), divided into a
 * regular grid of N = 4 << depth voxels per axis.  Voxel (i, j, k) is inside iff the tape's value is < 0 (NaN: not inside) at its
 * centre, c(i) = float(2 i + 1 - N) * (1.0f / N) - both factors and the product are exact in f32 - taken through the f32 point
 * transform of the mesher's leaf samples.  The grid is not visited voxel by voxel: the octree of fhip_mesh_sample is descended (the
 * same interval evaluations, the same tape simplification on the way down), a Full cell (interval result hi < 0) counts as entirely
 * inside by closed forms, an Empty one (lo > 0) as entirely outside, and only the ambiguous cells of level `depth` are sampled, at
 * their 4 x 4 x 4 voxels.  The result is what this recursion gives; it is the count over all N^3 centres whenever interval
 * inclusion holds for the tape.  All sums are integers: exact, independent of summation order and of "mesh_simplify_min_ops",
 * identical from run to run.
 *   n: inside voxels;  s1: sum of i, j, k over them;  s2: sum of i^2, j^2, k^2, ij, ik, jk;  lo / hi: the smallest and largest inside
 *   index per axis, inclusive (n == 0: lo = N, hi = 0);  grid: N;  cells: {cells interval-evaluated, Full, Empty, ambiguous cells of
 *   the last level}, what fhip_mesh_counts reports after fhip_mesh_sample at the same depth.
 * With h = 2 / N: volume = n h^3, centroid_x = -1 + (s1[0] / n + 0.5) h, and so on.  Arguments, variable binding and statuses are
 * fhip_mesh_build's (tapes of more than 16 input slots run their bound tape; one output; FHIP_ERR_UNSUPPORTED when the register file
 * exceeds LDS); depth > 10 is FHIP_ERR_UNSUPPORTED before any launch (at depth 10 the largest sum is below N^5 = 2^60).  Blocking;
 * `out` points to a host fhip_occupancy, the struct below; it is declared void* so that bindings generated from this header need no new type. */
typedef struct fhip_occupancy { uint64_t n, s1[3], s2[6]; uint32_t lo[3], hi[3]; uint32_t grid, pad; uint64_t cells[4]; } fhip_occupancy;
fhip_status fhip_shape_occupancy(fhip_ctx* ctx, const fhip_tape* tape, uint32_t depth, const float* world_to_model, const int32_t* axis_slots,
                                 const uint64_t* var_keys, const float* var_values, uint32_t n_vars, void* out);

/* ---- shape voxels: the inside voxels themselves, as a packed bitmap, and what is made of one ----------
 * The grid, the voxel centres and "inside" are fhip_shape_occupancy's, recursion included: a Full cell of the octree is all inside, an
 * Empty one all outside, an ambiguous cell of level `depth` is sampled at the 64 centres of its 4 x 4 x 4 voxels.  The bitmap stores
 * exactly that, one 64-bit word per such brick: B^3 little-endian uint64_t with B = 1 << depth (fhip_voxels_words; N = 4 B voxels per
 * axis).  Word (bz * B + by) * B + bx is the brick of the voxels (4 bx + lx, 4 by + ly, 4 bz + lz), lx, ly, lz in 0..3, and its bit
 * lx + 4 ly + 16 lz is set iff that voxel is inside.  The number of set bits is fhip_occupancy.n at the same depth; the bitmap does not
 * depend on "mesh_simplify_min_ops" and is identical from run to run.
 * fhip_shape_voxels: arguments, variable binding, bound tapes and statuses are fhip_shape_occupancy's; depth > 10 (a bitmap beyond
 * 8 GiB) is FHIP_ERR_UNSUPPORTED before any launch.  `out` holds fhip_voxels_words words and is written completely, zeros included:
 * the caller need not clear it.  out_is_device != 0: a device pointer, 8-byte aligned (a 16-byte aligned one lets the Full cells be
 * stored 16 bytes per lane); otherwise a host buffer, filled through the context's pinned landing area as fhip_mesh_stl does.  Blocking
 * either way.  `cells`: NULL, or the four counters fhip_occupancy.cells holds.
 * fhip_voxels_slices: layer images for k0 <= k < k1, out[((k - k0) * N + j) * N + i] = 255 where voxel (i, j, k) is inside and 0 where
 * not.  k0 > k1, k1 > N and depth > 10 are FHIP_ERR_UNSUPPORTED; k0 == k1 is FHIP_OK and writes nothing.
 * fhip_voxels_layer_counts: out[k], k < N, = the number of inside voxels with third index k; their sum is the number of set bits.
 * Both follow the effects' convention: on_device != 0, every pointer is a device pointer (bricks and counts 8-byte, slices 16-byte
 * aligned) and the call is asynchronous on the context's stream; otherwise every pointer is a host buffer. */
uint64_t fhip_voxels_words(uint32_t depth);
fhip_status fhip_shape_voxels(fhip_ctx* ctx, const fhip_tape* tape, uint32_t depth, const float* world_to_model, const int32_t* axis_slots,
                              const uint64_t* var_keys, const float* var_values, uint32_t n_vars, uint64_t* out, int out_is_device,
                              uint64_t cells[4]);
fhip_status fhip_voxels_slices(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, uint32_t k0, uint32_t k1, uint8_t* out, int on_device);
fhip_status fhip_voxels_layer_counts(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, uint64_t* out, int on_device);

/* ---- contours of a 2D slice: the outlines of the shape's cross-section at cfg->z, by marching squares ----------
 * The image is the PIXEL-PERFECT fhip_render2d image of `cfg` (size, z, world_to_model, variables, axis slots; cfg->pixel_perfect is
 * taken as 1): v[j * W + i], `inside` = v < 0, so NaN is outside.  Coordinates are pixel units: the centre of pixel (i, j) is the point
 * (float(i), float(j)).
 * Lattice edges, in index order: horizontal h(i, j) from (i, j) to (i + 1, j), 0 <= i < W - 1, 0 <= j < H, index j * (W - 1) + i; then
 * vertical u(i, j) from (i, j) to (i, j + 1), 0 <= i < W, 0 <= j < H - 1, index (W - 1) * H + j * W + i.  An edge crosses when `inside`
 * differs at its ends, and vertex k sits on the k-th crossing edge: with a, b the values at its first and other end,
 * t = a / (a - b) in f32 (t = 0.5 unless 0 <= t <= 1: NaN and infinite ends), at (float(i) + t, float(j)) or (float(i), float(j) + t).
 * Cell c(i, j), 0 <= i < W - 1, 0 <= j < H - 1, in the order j * (W - 1) + i, has the mask bit 0 in(i, j), 1 in(i + 1, j),
 * 2 in(i + 1, j + 1), 3 in(i, j + 1) and the edges B = h(i, j), R = u(i + 1, j), T = h(i, j + 1), L = u(i, j).  Its segments are pairs
 * of vertex ids {from, to}, the inside on their left (x to the right, j upward):
 *   1 B-L   2 R-B   4 T-R   8 L-T   3 R-L   6 T-B   14 L-B   13 B-R   11 R-T   7 T-L   12 L-R   9 B-T   (0, 15: none)
 *   5: B-R, T-L when ((v00 + v10) + (v11 + v01)) * 0.25f < 0, else B-L, T-R;   10: L-B, R-T when it is, else R-B, L-T
 * in cell order, a saddle's two in the order written.  next[k] is the `to` of the one segment with `from` k, 0xFFFFFFFF where there is
 * none (only on the image's border); no vertex has more than one segment leaving or arriving.  With W < 2 or H < 2 there are no cells,
 * so no segments: what is left is the crossing edges of the single row or column, vertices nothing joins; W or H = 0 gives no vertices.
 * fhip_contour2d: blocking.  The frame and four passes over it run on the context's stream; two totals come back to size the arrays;
 * vertices, segments and next stay in device memory, owned by the result.  Statuses as fhip_render2d's (FHIP_ERR_MISSING_VAR before
 * any launch); W * H or the number of edges at 2^32 or above is FHIP_ERR_UNSUPPORTED.
 * fhip_contours_counts: {vertices, segments, W, H}.  _vertices (2 floats each), _segments (2 ids each), _next (one id per vertex) copy
 * to host buffers of the caller's; _vertices_dev / _segments_dev are the device arrays (NULL when empty), valid until fhip_contours_free.
 * fhip_contour_loops: host only, no GPU call.  Follows next[0 .. n - 1] into chains of vertex ids: open chains first - from the
 * vertices no segment arrives at, in ascending order - then closed loops, each from its smallest id, in ascending order of that.
 * order: n ids; loop_start: n_loops + 1 offsets into it (at most n + 1); closed: n_loops flags (at most n); each may be NULL - call
 * once for *n_loops, then again.  FHIP_ERR_UNSUPPORTED: not a link array (an id >= n, two segments arriving at one vertex). */
/* (the result's handle, a `fhip_contours`, is declared void* here, as fhip_shape_occupancy's `out` is) */
fhip_status fhip_contour2d(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render2d_config* cfg, void** out);
void fhip_contours_counts(const void* contours, uint64_t out[4]);
fhip_status fhip_contours_vertices(const void* contours, float* out);
fhip_status fhip_contours_segments(const void* contours, uint32_t* out);
fhip_status fhip_contours_next(const void* contours, uint32_t* out);
const float* fhip_contours_vertices_dev(const void* contours);
const uint32_t* fhip_contours_segments_dev(const void* contours);
void fhip_contours_free(void* contours);
fhip_status fhip_contour_loops(const uint32_t* next, uint64_t n, uint32_t* order, uint64_t* loop_start, uint8_t* closed, uint64_t* n_loops);

/* ---- connected components of a voxel bitmap: is the solid one body or several, does it enclose voids ----------
 * (No counterpart in the reference, which has no voxel bitmap: the definitions below are the specification.)
 * The grid is fhip_shape_voxels': B = 1 << depth bricks and N = 4 B voxels per axis, nothing beyond it and no wrap-around.  The
 * FOREGROUND is the set bits, or with complement != 0 the clear bits.  Two foreground voxels are neighbours when they share a face
 * (connectivity 6) or a face, an edge or a corner (connectivity 26); any other connectivity is FHIP_ERR_UNSUPPORTED.  A component is a
 * class of the foreground under "joined by a chain of neighbours".  The key of a voxel is word_index * 64 + bit; a component's seed is
 * its voxel of smallest key, and the components are numbered 0, 1, ... by ascending seed key.  Per component: size, its number of voxels;
 * seed (i, j, k); lo, hi, its inclusive bounds per axis; border, 1 when some voxel of it has a coordinate equal to 0 or N - 1.  With
 * complement, the components with border == 0 are the voids the solid encloses.
 * fhip_voxels_components: blocking.  on_device != 0: `bricks` is a device pointer (8-byte aligned), otherwise a host buffer of
 * fhip_voxels_words(depth) words, staged.  Every brick's word is split into its own components (its nodes), which a lock-free union-find
 * joins across the bricks' faces (edges and corners); no pass waits for another workgroup.  depth > 10 is FHIP_ERR_UNSUPPORTED, more
 * than 2^32 - 2 nodes FHIP_ERR_OVERFLOW; an empty foreground gives 0 components and FHIP_OK.  The result owns two device arrays (a
 * brick's first node, a node's component) and the table; it records connectivity, complement and depth.
 * fhip_components_counts: {components, nodes, foreground voxels, depth}.
 * fhip_components_table: copies the table to host arrays of the caller's - size [c], seed, lo, hi [c][3], border [c]; any may be NULL.
 * The two calls below take the bitmap again: it MUST be the one that was labelled, unchanged (the result holds no copy of it).
 * fhip_components_label_slices: label images for k0 <= k < k1, out[((k - k0) * N + j) * N + i] = the component of voxel (i, j, k), -1
 * for background.  k0 > k1, k1 > N and more than 2^31 - 1 components are FHIP_ERR_UNSUPPORTED; k0 == k1 writes nothing.
 * fhip_components_extract: the bitmap of the components ids[0 .. n_ids - 1] (a host array; an id >= the number of components is
 * FHIP_ERR_UNSUPPORTED): fhip_voxels_words words, all of them written, their set bits the voxels of those components - of the foreground,
 * so with complement the voids come out as set bits.  `out` must not overlap `bricks`.
 * Buffers follow fhip_voxels_slices' convention, separately for the bitmap and the output: a device pointer (bricks 8-byte, label
 * images 16-byte aligned; the call is then asynchronous on the context's stream) or a host buffer. */
/* (the result's handle, a `fhip_components`, is declared void* here, as fhip_contour2d's is) */
fhip_status fhip_voxels_components(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t connectivity, int complement,
                                   void** out);
void fhip_components_counts(const void* comps, uint64_t out[4]);
fhip_status fhip_components_table(const void* comps, uint64_t* size, uint32_t* seed, uint32_t* lo, uint32_t* hi, uint8_t* border);
fhip_status fhip_components_label_slices(fhip_ctx* ctx, const void* comps, const uint64_t* bricks, int bricks_on_device, uint32_t k0,
                                         uint32_t k1, int32_t* out, int out_on_device);
fhip_status fhip_components_extract(fhip_ctx* ctx, const void* comps, const uint64_t* bricks, int bricks_on_device, const uint32_t* ids,
                                    uint64_t n_ids, uint64_t* out, int out_on_device);
void fhip_components_free(void* comps);

/* ---- exact Euclidean distance transform of a voxel bitmap: how far, in voxels, from the nearest foreground voxel ----------
 * (No counterpart in the reference, which has no voxel bitmap: the definitions below are the specification.  A shape's own value is no
 * distance - min, max, scaling and mix all break |grad f| = 1 - but between voxel centres the squared distance is an integer.)
 * The grid is fhip_shape_voxels': N = 4 << depth voxels per axis, voxel (i, j, k) bit lx + 4 ly + 16 lz of bricks[bz][by][bx].  The
 * FOREGROUND is the set bits, or with complement != 0 the clear bits.  The field d2 is N^3 uint32, d2[(k * N + j) * N + i] = the minimum
 * over the foreground voxels (i', j', k') of (i - i')^2 + (j - j')^2 + (k - k')^2: 0 on the foreground itself.  Outside the grid there is
 * nothing, neither foreground nor background.  Without any foreground voxel every value is 0xFFFFFFFF, "no distance" (-1 as an int32).
 * fhip_voxels_distance: blocking.  on_device != 0: `bricks` is a device pointer (8-byte aligned), otherwise a host buffer of
 * fhip_voxels_words(depth) words, staged.  Three separable passes, exact in integers: along i from the rows' bit masks, then along j and
 * along k the lower envelope of the parabolas f(q) + (p - q)^2; no pass waits for another workgroup.  depth > 8 is FHIP_ERR_UNSUPPORTED,
 * refused before anything is allocated: at depth 8 the field is 4 GiB, and the call holds a workspace of up to 1 GiB beside it while it
 * runs.  The result owns the field in device memory and records depth and complement; it keeps no reference to the bitmap.
 * fhip_distance_info: {the largest finite d2, the smallest index (k * N + j) * N + i that has it, foreground voxels, depth}.  With every
 * voxel foreground: 0 at index 0.  Without foreground: 0 and, for the index, UINT64_MAX ("none").
 * fhip_distance_slices: the layers k0 <= k < k1, out[((k - k0) * N + j) * N + i] = d2 of voxel (i, j, k).  k0 > k1 and k1 > N are
 * FHIP_ERR_UNSUPPORTED; k0 == k1 writes nothing.  Only these layers are copied to a host buffer.
 * fhip_distance_dev: the device pointer of the whole field, N^3 uint32, valid until fhip_distance_free.
 * fhip_distance_threshold: a bitmap of fhip_voxels_words(depth) words, all of them written: with beyond == 0 a bit is set where
 * d2 <= t ("within"), otherwise where d2 > t ("beyond").  t <= 0xFFFFFFFE, 0xFFFFFFFF is FHIP_ERR_UNSUPPORTED: "no distance" is never
 * within and always beyond.  Within t of the set bits is the solid grown by a ball of radius sqrt(t); beyond t of the clear bits
 * (complement) is the solid shrunk by it.
 * Output buffers follow fhip_voxels_slices' convention: a device pointer (a bitmap 8-byte, layers 16-byte aligned; the call is then
 * asynchronous on the context's stream) or a host buffer, filled when the call returns. */
/* (the result's handle, a `fhip_distance`, is declared void* here, as fhip_voxels_components' is) */
fhip_status fhip_voxels_distance(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, int complement, void** out);
void fhip_distance_info(const void* dist, uint64_t out[4]);
fhip_status fhip_distance_slices(fhip_ctx* ctx, const void* dist, uint32_t k0, uint32_t k1, uint32_t* out, int out_on_device);
const uint32_t* fhip_distance_dev(const void* dist);
fhip_status fhip_distance_threshold(fhip_ctx* ctx, const void* dist, uint32_t t, int beyond, uint64_t* out_bricks, int out_on_device);
void fhip_distance_free(void* dist);

/* ---- local thickness of a distance field: per voxel the largest ball that fits and holds it ----------
 * (Hildebrand & Rueegsegger's local thickness, BoneJ's Tb.Th.  No counterpart in the reference; the definition below is the specification.)
 * Let F be a finished field of fhip_voxels_distance.  For every voxel p of the grid T(p) = max { F(c) : c a voxel of the grid,
 * F(c) > |p - c|^2 }, and 0 where there is no such c: the open ball of squared radius F(c) around c holds no foreground voxel, so
 * T(p) > 0 exactly where F(p) > 0, and there T(p) >= F(p).  T is in squared voxels like F.  Balls that poke out of the grid are clipped;
 * outside the grid there is neither foreground nor a centre.  Of the field to the clear bits (complement != 0) T is the wall thickness of
 * the solid - a slab w voxels thick reads ceil(w / 2)^2, so 2 sqrt(T) is the wall in voxels, rounded up to even; of the field to the set
 * bits it is the local width of the empty space.
 * fhip_distance_thickness: blocking.  The result is a distance handle whose field is T: fhip_distance_slices, _threshold, _dev, _free
 * and _info ({largest T, its smallest index, voxels with T == 0, depth}) apply unchanged.  It allocates one more field of N^3 uint32 and,
 * while it runs, N^3 / 8 bytes of flags and three tables of max F + 1 words.  A centre whose ball lies inside the ball of one of its 26
 * neighbours is not painted - that leaves T as it is; the kept balls are scattered with integer atomic maxima, so T does not depend on
 * the order of arrival.  FHIP_ERR_UNSUPPORTED: a field on another device, a field without foreground (all 0xFFFFFFFF: no bounded
 * ball), a field that is itself a thickness.
 * fhip_thickness_info: {largest T, its smallest index (k * N + j) * N + i, smallest positive T, its smallest index, voxels with T > 0,
 * depth, centres (F > 0), balls painted}.  With T all 0: {0, 0, 0, UINT64_MAX, 0, ...}.  A null handle: zeros and UINT64_MAX twice.
 * fhip_thickness_thin: fhip_distance_threshold's bitmap of the voxels with 0 < T <= t, the parts thinner than 2 sqrt(t).
 * fhip_thickness_histogram: counts[b] = the voxels with edges[b] <= T < edges[b + 1] for b < n_edges - 1; 2 <= n_edges <= 1024, the
 * edges ascending (equal neighbours make an empty bin; on the host this is checked).  on_device != 0: edges (4-byte aligned) and counts
 * (8-byte aligned) are device pointers and the call is asynchronous on the context's stream. */
fhip_status fhip_distance_thickness(fhip_ctx* ctx, const void* dist, void** out);
void fhip_thickness_info(const void* thick, uint64_t out[8]);
fhip_status fhip_thickness_thin(fhip_ctx* ctx, const void* thick, uint32_t t, uint64_t* out_bricks, int out_on_device);
fhip_status fhip_thickness_histogram(fhip_ctx* ctx, const void* thick, const uint32_t* edges, uint32_t n_edges, uint64_t* counts, int on_device);

/* ---- boundary mesh of a voxel bitmap: the solid's faces as triangles, its surface area, its Euler number ----------
 * (No counterpart in the reference, which has no voxel bitmap: the definitions below are the specification, exact and in integers.)
 * GRID.  fhip_shape_voxels': B = 1 << depth bricks and N = 4 B voxels per axis, voxel (i, j, k) bit lx + 4 ly + 16 lz of word
 * (bz B + by) B + bx.  Outside the grid every voxel counts as clear: faces on the grid's border exist and the surface is closed.
 * FACE.  A set voxel and a direction d = 0 .. 5 = -x, +x, -y, +y, -z, +z in which its neighbour is clear; its axis is a = d / 2.  With
 * (u, v) the unit vectors of the next two axes cyclically (x -> y, z; y -> z, x; z -> x, y), its four lattice corners, counter-clockwise
 * seen from outside, are o, o + u, o + u + v, o + v with o = (i, j, k) + e_a on the + side, and o, o + v, o + u + v, o + u with
 * o = (i, j, k) on the - side.  Faces are ordered by brick word index, then d, then the voxel's bit in its brick.  Face f gives the
 * triangles 2 f = (c0, c1, c2) and 2 f + 1 = (c0, c2, c3), so that the STL normal (b - a) x (c - a) points from set to clear.
 * VERTEX.  A lattice corner (a, b, c), 0 <= a, b, c <= N, is used iff the eight voxels around it are not all equal - the same set as
 * the corners of all faces.  One vertex per used corner, shared by every face there, also where the surface pinches (voxels touching
 * only along an edge or at a corner).  Vertices are numbered ascending by corner brick ((c >> 2) (B + 1) + (b >> 2)) (B + 1) + (a >> 2),
 * then by local bit (a & 3) + 4 (b & 3) + 16 (c & 3).  A coordinate is float(2 a - N) * (1.0f / N), exact in f32: the frame is the
 * cube [-1, 1]^3 that the bitmap was sampled in.
 * EDGE.  A lattice edge is used iff the four voxels around it are not all equal.
 * fhip_voxels_surface: the counting pass alone; blocking.  out = {faces per direction [6], V used corners, E used edges, F = the sum of
 * the six, n set voxels}, a host array.  The area is F h^2 with h = 2 / N, and V - E + F the Euler number of the surface complex.
 * fhip_voxels_mesh: blocking.  The counting pass, two prefix sums, one pass that writes the vertices and one that writes the faces;
 * no pass waits for another workgroup.  The result is a fhip_mesh like fhip_mesh_build's: vertices (3 f32 each) and triangles (3 u64
 * each) resident in device memory and copied to the host, so that fhip_mesh_counts (entries 6 and 7; the octree's counters are 0),
 * _vertices(_ptr, _dev), _triangles(_ptr, _dev), _stl_bytes, _stl, _vertex_grads and _free apply unchanged.  An empty bitmap gives an
 * empty mesh (no device arrays) and FHIP_OK.
 * Both: on_device != 0: `bricks` is a device pointer (8-byte aligned), otherwise a host buffer of fhip_voxels_words(depth) words,
 * staged.  A NULL argument, a misaligned device pointer and depth > 10 are refused before any launch.  2^32 triangles or more, or
 * 2^32 vertices or more, are FHIP_ERR_OVERFLOW, decided from the counting pass's 64-bit totals before an array of the result is
 * allocated or written; a failed allocation is FHIP_ERR_HIP. */
fhip_status fhip_voxels_surface(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint64_t out[10]);
fhip_status fhip_voxels_mesh(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, fhip_mesh** out);

/* ---- a voxel bitmap along a direction: shadows, overhangs, supports, heights ---------------------------------------
 * (No counterpart in the reference, which has no voxel bitmap: the definitions below are the specification, exact and in integers.)
 * GRID.  fhip_shape_voxels': B = 1 << depth bricks and N = 4 B voxels per axis, depth <= 10, voxel (i, j, k) bit lx + 4 ly + 16 lz of
 * word (bz B + by) B + bx.  Outside the grid every bitmap is clear.
 * DIRECTION.  d = 0 .. 5 is -x, +x, -y, +y, -z, +z, the numbering of fhip_voxels_mesh's faces; e(d) is its unit vector and d ^ 1 its
 * opposite.  An axis a = 0, 1, 2 is x, y, z.
 * FLOW.  Given seeds S, blockers K and a direction d, the flow is the bitmap R with R(p) = (R(p - e) | S(p - e)) & ~K(p), R and S false
 * outside the grid; a NULL K means none.  Equivalently R(p) holds iff there is t >= 1 with S(p - t e) and ~K(p - s e) for all
 * 0 <= s < t: a seed that is itself blocked still emits, and a blocked voxel is never in R.  With FHIP_FLOW_WITH_SEEDS (bit 0 of
 * `flags`) the result is R | S.  The shadow of a solid A towards d is flow(S = A, K = A, d), the clear voxels with a set voxel behind
 * them; the solid swept to the border is flow(A, none, d, WITH_SEEDS); the space trapped along an axis - reachable from neither side,
 * an undercut of a two-part mould - is the AND of the two opposite shadows, which the caller takes.
 * OVERHANGS.  Given a solid A, a build direction `up`, an integer reach2 in 0 .. 16 and a flag `bed`: p is supported iff there is a set
 * q one layer below, (q - p) . e(up) = -1, whose squared perpendicular offset - the squared length of q - p projected on the two other
 * axes - is at most reach2: a Euclidean disc, reach2 = 0 straight below only, 1 a plus of five, 2 the 3 x 3 square.  For p in the first
 * layer (p - e(up) outside the grid) every q counts as set iff `bed`, and as clear otherwise.  The overhangs are the set voxels that
 * are not supported.  With reach2 <= 16 every q lies in p's brick or in a brick adjacent to it: hence the limit.
 * SUPPORTS are flow(S = overhangs, K = A, d = up ^ 1): the clear columns under every overhanging voxel, down to the next set voxel or
 * the grid's border - two calls.
 * HEIGHTS.  Given an axis a, the result is int32 [3][N][N], indexed by the two remaining coordinates, the lower axis fastest: a = 2
 * gives [j][i], a = 1 [k][i], a = 0 [k][j].  Plane 0: the smallest coordinate along a of a set voxel in that column, -1 in an empty
 * column; plane 1: the largest, -1 likewise; plane 2: the number of set voxels in the column.
 * All three: one launch on the context's stream.  on_device != 0: the inputs are device pointers (8-byte aligned) - `seeds` and
 * `blockers` live in the same place - and otherwise host buffers of fhip_voxels_words(depth) words, staged; out_on_device likewise
 * for `out`, which is written completely: fhip_voxels_words(depth) words, or 3 N N int32.  With device pointers throughout the call
 * is asynchronous, as fhip_voxels_slices is; with a host `out` it returns when `out` is filled.  Refused before any launch, `out`
 * untouched: a NULL context or `out` (FHIP_ERR_BAD_TAPE); a NULL input, depth > 10, dir or up > 5, axis > 2, reach2 > 16, unknown flag
 * bits, a misaligned device pointer, an `out` that is the same pointer as an input (FHIP_ERR_UNSUPPORTED). */
#define FHIP_FLOW_WITH_SEEDS 1u
fhip_status fhip_voxels_flow(fhip_ctx* ctx, const uint64_t* seeds, const uint64_t* blockers /* NULL: none */, uint32_t depth,
                             int on_device, uint32_t dir, uint32_t flags, uint64_t* out, int out_on_device);
fhip_status fhip_voxels_overhangs(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t up,
                                  uint32_t reach2, int bed, uint64_t* out, int out_on_device);
fhip_status fhip_voxels_heights(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t axis,
                                int32_t* out, int out_on_device);

/* ---- a triangle mesh to a voxel bitmap: solid voxelization by parity along +x --------------------------------------
 * (No counterpart in the reference, which has no voxel bitmap: the definition below is the specification, exact and in integers after
 * the snap, and the result is the same from run to run and under any order of the triangles - XOR commutes.)
 * GRID.  fhip_shape_voxels': B = 1 << depth bricks and N = 4 B voxels per axis over [-1, 1]^3, depth <= 10, voxel (i, j, k) bit
 * lx + 4 ly + 16 lz of word (bz B + by) B + bx.  Each triangle writes one toggle bit per column (j, k) it covers; a prefix XOR along x
 * turns the toggles into the solid (even-odd: two nested closed sheets enclose a cavity).
 * SNAP.  A vertex coordinate v (float32) goes through the optional `mesh_to_world`, a row-major 3 x 4 matrix of doubles (NULL: the
 * identity), evaluated in binary64 as ((m0 x + m1 y) + m2 z) + m3 with no contraction: w.  q = llrint(w (128 N) + 128 N), rounding to
 * nearest-even, in lattice units of 1/256 voxel: voxel i has its centre at 256 i + 128, and a vertex that fhip_voxels_mesh makes at
 * float(2 a - N) / N snaps to exactly 256 a.
 * REJECTED.  A triangle is skipped, and counted in `rejected`, if any vertex coordinate w is not finite or lies outside [-1.5, 1.5] -
 * decided on w, before any conversion to an integer - or if one of its indices is at or beyond n_vertices, which is never read.
 * FLAT.  Projected to the yz plane, D = (b.y - a.y)(c.z - a.z) - (b.z - a.z)(c.y - a.y).  D == 0: the triangle is edge-on or
 * degenerate, skipped and counted in `flat`.  D < 0: b and c change places and D its sign, so that the inside lies to the left of
 * every edge.
 * COVER.  Column (j, k) is the point P = (256 j + 128, 256 k + 128).  For each directed edge p -> r of (b -> c, c -> a, a -> b),
 * e = (r.y - p.y)(P.z - p.z) - (r.z - p.z)(P.y - p.y).  P is covered iff every e > 0, or e == 0 and the edge owns its points: an edge
 * owns its points when r.y - p.y > 0, or when r.y - p.y == 0 and r.z - p.z < 0 - the rasterizer's fill rule: a point on an edge or a
 * vertex that two or more triangles share is counted once per sheet.  Only columns with 0 <= j, k < N are visited.
 * CROSSING.  With the three e as weights (w_a = e(b -> c), w_b = e(c -> a), w_c = e(a -> b), sum = D), xmin = min(a.x, b.x, c.x) and
 * num = w_a (a.x - xmin) + w_b (b.x - xmin) + w_c (c.x - xmin), the crossing lies at xmin + num / D and toggles every voxel whose centre
 * is at or beyond it: i* = ceil((num - (128 - xmin) D) / (256 D)), the exact quotient rounded up.  i* <= 0 toggles voxel (0, j, k);
 * i* >= N toggles the column's bit in an exit plane of N x N bits and counts the crossing in `clipped`; otherwise (i*, j, k).
 * FILL.  inside(i, j, k) = the XOR of the toggles at (0 .. i, j, k).  `open_rows` is the number of columns where inside(N - 1, j, k)
 * XOR the exit plane's bit is 1: a row with an odd number of crossings shows that the mesh is not closed.  A closed mesh gives 0, also
 * where it pokes out of the cube.
 * BIT BUDGET.  Everything in int64: coordinates in [-64 N, 320 N], spans at most 384 N = 1.5 2^20 at depth 10, D <= span^2 < 2^41.2,
 * edge values off the triangle below 2^42.2, num <= span^3 < 2^61.8, |(128 - xmin) D| < 2^61.5, their difference below 2^63, the
 * divisor 256 D below 2^50.  The division is made once per covered column.
 * fhip_triangles_voxels: `vertices` 3 f32 each; `triangles` 3 u64 indices each, or NULL for a soup in which every three vertices are
 * a triangle.  on_device != 0: both are device pointers (4- and 8-byte aligned), otherwise host arrays, which get device memory of
 * their own for the call.  `out`: fhip_voxels_words(depth) words, written completely - a device pointer (8-byte aligned) with
 * out_on_device != 0, otherwise a host buffer, staged.  info = {triangles, rejected, flat, crossings (covered columns, clipped ones
 * included), clipped, open_rows, set voxels, W = the columns under the triangles' boxes, the items of work}, a host array: the call
 * blocks.  n_triangles == 0 gives an all-zero bitmap.  A set-up pass, prefix sums, a pass over the W (triangle, column) items with one
 * 64-bit atomic XOR per covered column, the fill; no pass waits for another workgroup.  Refused before `out` is touched: a NULL
 * context, `out` or `info` (FHIP_ERR_BAD_TAPE); depth > 10, NULL vertices with triangles to read, a misaligned device pointer
 * (FHIP_ERR_UNSUPPORTED); n_triangles >= 2^32 (FHIP_ERR_OVERFLOW).  W >= 2^40 is FHIP_ERR_OVERFLOW too, decided after the set-up: a
 * device `out` has then been cleared to zeros and holds no result, a host `out` has not been written.  The call's scratch, 64 bytes
 * per triangle, stays with the context afterwards, in the buffer of the mesher's leaf records: fhip_ctx_trim gives it back.
 * fhip_mesh_voxels: the same for a fhip_mesh, from its device arrays where they are resident (fhip_mesh_vertices_dev), otherwise
 * from its host arrays. */
fhip_status fhip_triangles_voxels(fhip_ctx* ctx, const float* vertices, uint64_t n_vertices, const uint64_t* triangles /* NULL: a soup */,
                                  uint64_t n_triangles, int on_device, const double* mesh_to_world /* 3 x 4 or NULL */, uint32_t depth,
                                  uint64_t* out, int out_on_device, uint64_t info[8]);
fhip_status fhip_mesh_voxels(fhip_ctx* ctx, const fhip_mesh* mesh, const double* mesh_to_world, uint32_t depth,
                             uint64_t* out, int out_on_device, uint64_t info[8]);

/* ---- the check of a triangle mesh: weld, edges, shells, volume ------------------------------------------------------
 * (No counterpart in the reference, which never asks what kind of mesh it made: the definition below is the specification.  Every
 * integer result is the same bits from run to run and does not depend on how the hardware orders the threads; the two float64 sums per
 * shell, volume6 and area2, add the same terms in an order of arrival that may differ from run to run, and nothing else does.)
 * INPUT.  As fhip_triangles_voxels takes it: `vertices` 3 f32 each; `triangles` 3 u64 indices each, or NULL for a soup in which every
 * three vertices are a triangle.  Corner c = 3 t + k is corner k of triangle t.  A triangle is REJECTED if a coordinate of one of its
 * corners is not finite, or one of its indices is at or beyond n_vertices (never read).  With any triangle rejected the call makes
 * no arrays: it returns FHIP_OK and a handle whose counts hold `triangles` and `rejected` alone.
 * WELD.  weld != 0: two corners are the same vertex iff their three coordinates are equal as floats after x + 0.0f (-0 equals +0; no
 * NaN gets here).  The welded vertices are numbered in the order of their first corners, vertices[v] holds that first corner's
 * coordinates, bits unchanged, and a vertex that no triangle uses does not appear.  weld == 0 (indexed meshes only; a soup is refused):
 * a vertex is its index, and the vertex array is handed through as given, all n_vertices rows of it.  Either way `triangles` holds
 * every triangle in the order given, as vertex ids, and counts[3] is the number of distinct vertices that a triangle uses.
 * DEGENERATE.  A triangle with two equal vertex ids: counted, kept in `triangles`, no part of edges or shells, its shell 0xFFFFFFFF.
 * EDGES.  An edge is a set {a, b}, a < b, used by the triangles that are not degenerate: f uses in the direction a -> b, r in b -> a.
 * boundary: f + r == 1; flipped: f + r == 2 and f != r; nonmanifold: f + r >= 3; unbalanced: f != r.  A mesh is closed iff no edge is
 * unbalanced - its triangles form a cycle, what parity filling needs - and manifold iff no edge is boundary, flipped or nonmanifold;
 * its Euler number is vertices - edges + (triangles - degenerate).  fhip_topology_edges: the edges of one class (kind 0 boundary, 1
 * flipped, 2 nonmanifold, 3 unbalanced) as counts[5 + kind] pairs (a, b) of u32, in the order of the first corners that use them.
 * SHELLS.  Two triangles that are not degenerate are in the same shell iff a chain of shared edges, of any class, joins them.  Shells
 * are numbered in the order of their first (smallest) triangles; triangle_shells[t] is a triangle's shell.  Per shell: `triangles`;
 * `first`, its first triangle; `unbalanced`, its unbalanced edges - an edge lies in one shell, so the shell is closed iff this is 0;
 * lo, hi [3]: the exact minimum and maximum of its corners, -0 taken as +0; volume6 and area2, each the sum over the shell's
 * triangles of a binary64 term of the corners a, b, c - rows of `vertices` - converted to binary64, evaluated in the order written,
 * no contraction: with n = (b.y c.z - b.z c.y, b.z c.x - b.x c.z, b.x c.y - b.y c.x) the term of volume6 is (a.x n.x + a.y n.y) + a.z n.z;
 * with u = b - a, v = c - a and m = u x v in the same component order the term of area2 is sqrt((m.x m.x + m.y m.y) + m.z m.z).  A
 * shell with volume6 < 0 is an inward-facing cavity; the mesh's volume is the sum of volume6 over 6, its area that of area2 over 2.
 * THE PASSES.  Three lock-free tables.  Vertices: open addressing over u32 slots that hold the corner that claimed them (CAS from
 * empty); a corner that meets a claimed slot compares its key with the claimant's, read from the input - it never waits for another
 * thread's data - and a second word per slot takes the minimum of the corners: the first.  Edges: slots of a key a << 32 | b claimed
 * by a 64-bit CAS, the two counts in one 64-bit word (an add of 1 or 1 << 32), the first corner by a minimum.  Shells: a union-find
 * over the triangles that links towards the smaller root, every triangle united with the first triangle of each of its edges.  The
 * lists and numbers come from flags and prefix sums over the corners and triangles, never from the order of the slots.  A probe
 * sequence visits every slot at most once; one that finds no room makes the call return FHIP_ERR_OVERFLOW.  No pass waits for
 * another workgroup.  table_log2 == 0: the library sizes the tables (the least power of two at or above 4 T slots each; 8 bytes a
 * vertex slot, 32 an edge slot); otherwise both get exactly 1 << table_log2 slots (at most 32).  The scratch stays with the context in
 * the buffer of the mesher's leaf records, as fhip_triangles_voxels' does: fhip_ctx_trim gives it back.
 * Limits: 3 n_triangles <= 2^32 - 2 and, indexed, n_vertices <= 2^32 - 2, beyond them FHIP_ERR_OVERFLOW.  n_triangles == 0 is valid:
 * all counts zero, no arrays.  The calls block.  counts = {triangles, rejected, degenerate, vertices, edges, boundary, flipped,
 * nonmanifold, unbalanced, shells, vertex-table slots, edge-table slots, 0, 0, 0, 0}.  The getters copy to host arrays of the sizes the
 * counts give (`vertices`: fhip_topology_vertex_rows rows - counts[3] welded, n_vertices otherwise); the _dev getters return the
 * handle's device arrays, NULL where there are none; any array pointer of fhip_topology_shells may be NULL.  fhip_mesh_topology: the
 * same for a fhip_mesh, from its device arrays where they are resident. */
fhip_status fhip_triangles_topology(fhip_ctx* ctx, const float* vertices, uint64_t n_vertices, const uint64_t* triangles /* NULL: a soup */,
                                    uint64_t n_triangles, int on_device, int weld, uint32_t table_log2, void** out);
fhip_status fhip_mesh_topology(fhip_ctx* ctx, const fhip_mesh* mesh, int weld, uint32_t table_log2, void** out);
void fhip_topology_counts(const void* topo, uint64_t out[16]);
uint64_t fhip_topology_vertex_rows(const void* topo);
fhip_status fhip_topology_vertices(const void* topo, float* out);
fhip_status fhip_topology_triangles(const void* topo, uint64_t* out);
fhip_status fhip_topology_triangle_shells(const void* topo, uint32_t* out);
const float* fhip_topology_vertices_dev(const void* topo);
const uint64_t* fhip_topology_triangles_dev(const void* topo);
const uint32_t* fhip_topology_triangle_shells_dev(const void* topo);
fhip_status fhip_topology_shells(const void* topo, uint64_t* triangles, uint32_t* first, uint64_t* unbalanced, float* lo, float* hi,
                                 double* volume6, double* area2);
fhip_status fhip_topology_edges(fhip_ctx* ctx, const void* topo, uint32_t kind, uint32_t* out, int out_on_device);
void fhip_topology_free(void* topo);

/* ---- the outlines of a voxel bitmap's layers: closed rectilinear loops per layer ------------------------------------
 * (No counterpart in the reference, which has no voxel bitmap: the definitions below are the specification, exact and in integers,
 * and the result is the same from run to run.)
 * LAYER IMAGE.  Layers are along z, as for fhip_voxels_slices.  Layer k is the image P(i, j) = voxel (i, j, k), 0 <= i, j < N = 4 << depth,
 * clear outside the grid: every loop is closed and the grid's borders produce edges.
 * CORNERS (a, b), 0 <= a, b <= N.  The corner mask is m = P(a-1, b-1) | P(a, b-1) << 1 | P(a, b) << 2 | P(a-1, b) << 3.
 * UNIT BOUNDARY EDGES separate a set pixel from a clear one and are directed with the inside on the left, x to the right and y upward:
 * the bottom side of a set pixel runs +x and its top -x, its right side runs +y and its left side -y.  Headings are numbered as the
 * directions of fhip_voxels_flow: 0 = -x, 1 = +x, 2 = -y, 3 = +y.
 * VERTICES lie only where the outline turns.  As (incoming heading, outgoing heading) a corner holds: m = 0, 15, 3, 6, 9, 12: none (the
 * last four are straight runs); m = 1: (3, 0); m = 2: (0, 2); m = 4: (2, 1); m = 8: (1, 3); m = 7: (2, 0); m = 11: (0, 3); m = 13: (3, 1);
 * m = 14: (1, 2).  The saddles m = 5 and m = 10 hold two vertices, in ascending order of the outgoing heading.  With connectivity 4
 * diagonal pixels are separate and both loops turn left: m = 5: (3, 0), (2, 1); m = 10: (0, 2), (1, 3).  With connectivity 8 diagonal
 * pixels are joined and both loops turn right: m = 5: (2, 0), (3, 1); m = 10: (1, 2), (0, 3).  Any other connectivity is
 * FHIP_ERR_UNSUPPORTED.
 * NUMBERING.  Layers ascend; inside a layer the corners are in the order b (N + 1) + a; a saddle's two vertices in the order above.  Ids
 * are global uint32; vertex_start[K + 1] (K = k1 - k0) gives each layer's range.  2^32 vertices or more is FHIP_ERR_OVERFLOW, decided
 * from the counting pass's 64-bit totals before anything is written.
 * xy[v] is the corner as two uint16 (a, b).  next[v] is the id of the first vertex met from v along its outgoing heading: the nearest
 * corner on that lattice line that holds a vertex with that incoming heading - everything between is a straight corner.  next is a
 * permutation inside each layer: every vertex has exactly one successor and one predecessor.
 * LOOPS.  A loop's leader is its smallest vertex id; loops are numbered by ascending leader, so a layer's loops are contiguous:
 * loop_start[K + 1] gives each layer's range and loop_of[v] each vertex's loop.  The loop table holds per loop: leader and n_vertices;
 * area2, the int64 shoelace sum of x_v y_next - x_next y_v over its vertices, positive for an outer boundary and negative for a hole;
 * perimeter, its Manhattan length; lo[2] and hi[2], its corner bounds.  Per layer, area2 is the sum over the layer's loops, which
 * equals twice the layer's count of set voxels (fhip_voxels_layer_counts), and perimeter the number of its unit boundary edges.
 * WORLD.  Corner a is at float(2 a - N) / N, as fhip_voxels_mesh places it; a layer's z is its centre float(2 k + 1 - N) / N.
 * on_device != 0: `bricks` is a device pointer (8-byte aligned), read in place; otherwise a host buffer of fhip_voxels_words(depth)
 * words, staged.  The call blocks, as fhip_contour2d does: the counting pass's totals come back to size the arrays.  xy, next and
 * loop_of stay in device memory, owned by the handle (the _dev getters; NULL where there are no vertices); the getters copy ranges to
 * the host, any output pointer may be NULL, and a range beyond the counts is FHIP_ERR_UNSUPPORTED.  counts = {vertices, loops, layers,
 * N, k0, connectivity, 0, 0}.  Refused before any launch: k0 > k1, k1 > N, depth > 10 (FHIP_ERR_UNSUPPORTED).  k0 == k1 is FHIP_OK
 * with an empty result.  No kernel waits for another workgroup; the sums are integer atomics. */
fhip_status fhip_voxels_outlines(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t k0, uint32_t k1,
                                 uint32_t connectivity, void** out);
void fhip_outlines_counts(const void* outlines, uint64_t out[8]);
fhip_status fhip_outlines_layers(const void* outlines, uint64_t* vertex_start, uint64_t* loop_start, int64_t* area2, uint64_t* perimeter);
fhip_status fhip_outlines_vertices(const void* outlines, uint64_t first, uint64_t count, uint16_t* xy, uint32_t* next, uint32_t* loop_of);
fhip_status fhip_outlines_loops(const void* outlines, uint64_t first, uint64_t count, uint32_t* leader, uint32_t* n_vertices,
                                int64_t* area2, uint64_t* perimeter, uint16_t* lo, uint16_t* hi);
const uint16_t* fhip_outlines_xy_dev(const void* outlines);
const uint32_t* fhip_outlines_next_dev(const void* outlines);
const uint32_t* fhip_outlines_loop_dev(const void* outlines);
void fhip_outlines_free(void* outlines);

/* ---- the nesting of those outlines: which hole belongs to which outer boundary, which island lies in which hole -----
 * (No counterpart in the reference.  The definitions below are the specification, exact and in integers, and the result is the same
 * from run to run.)  Take a result of fhip_voxels_outlines (layers k0 <= k < k1, connectivity 4 or 8) and the bitmap it was made
 * from.  For loop l of layer k let (a0, b0) be the corner of its leader and P the layer image, clear outside the grid.
 * THE LEADER.  The unit boundary edge (a0, b0)-(a0, b0 + 1) belongs to l.  If area2[l] > 0, pixel (a0, b0) is set; if area2[l] < 0,
 * pixel (a0, b0) is clear and pixel (a0 - 1, b0) is set.  area2 is never 0.
 * LEFT.  Take the largest a < a0 with P(a - 1, b0) != P(a, b0); a = 0 compares the clear outside with P(0, b0).  left[l] is the loop
 * that owns the unit boundary edge (a, b0)-(a, b0 + 1); without such an a, left[l] is NONE = 0xFFFFFFFF.  left[l] lies in the same
 * layer, and left[l] < l.
 * PARENT.  parent[l] is the first loop in the chain left[l], left[left[l]], ... whose area2 has the opposite sign to l's, NONE if the
 * chain ends first.  parent[l] < l.  A loop without a parent is an outer boundary; a parent's sign is opposite to its child's.
 * Equivalently: a loop e != l encloses l iff e has an odd number of vertical unit edges on pixel row b0 with a < a0, and parent[l] is
 * the enclosing loop of smallest |area2|.
 * DEPTH.  depth[l] is 0 without a parent, otherwise depth[parent[l]] + 1: even exactly for outer boundaries.
 * CHILDREN AND REGIONS.  n_children[l] is the number of loops whose parent is l.  region_area2[l] is the int64 sum of area2[l] and the
 * area2 of the children of l: for an outer boundary twice the number of set pixels of one connected component of the layer under
 * `connectivity`; for a hole minus twice the number of clear pixels of one component of the clear pixels under the dual connectivity
 * (8 for 4, 4 for 8), the outside component excluded.
 * PER LAYER.  outer: its loops with area2 > 0; top: its loops without a parent; max_depth.
 * `bricks`: a host buffer, or with bricks_on_device != 0 a device pointer (8-byte aligned), as for fhip_components_label_slices.  It MUST
 * be the bitmap that was outlined, unchanged: the handle holds no copy of it.  With another bitmap the result is unspecified, but
 * nothing is read or written outside the arrays: the row scan ends at a = 0, the column walk at the lattice's border, the vertex
 * search inside the layer's own id range, and only a loop of the same layer with a smaller id is kept as left[l].
 * THE PASSES.  A lane per loop: the row scan, the column walk against the edge's heading to the corner where its straight run begins, a
 * lower bound search for that corner's word a | b << 16 among the layer's vertices (a saddle's two share the word; only m = 10 has
 * vertical outgoing headings, 2 then 3), loop_of.  Parents by pointer doubling over the links of equal sign, depths by the same
 * doubling over (ancestor, hops), double-buffered, ceil(log2(the largest layer's loop count)) rounds each, fixed by the host from
 * loop_start.  The sums are integer atomics; no kernel waits for another workgroup.
 * The call blocks, as fhip_voxels_outlines does.  parent and depth stay in device memory, owned by the handle (the _dev getters; NULL
 * where there are no loops); everything is also on the host: the getters copy, any output pointer may be NULL, and a range beyond the
 * counts is FHIP_ERR_UNSUPPORTED.  counts = {loops, outer, top, max depth, layers, k0, connectivity, 0}.  Outlines with no loops, or
 * with k0 == k1, give FHIP_OK and an empty nesting.  Refused before any launch: no context, outlines or result (FHIP_ERR_BAD_TAPE), no
 * bitmap, outlines of another device's context (FHIP_ERR_UNSUPPORTED).  The outlines are read and not changed.
 * fhip_nesting_children is host code and needs no context: a counting sort of the n loops by parent into CSR - child_start[n + 1],
 * children[child_start[n]], each list ascending; loops without a parent are in no list; a parent >= n that is not NONE is
 * FHIP_ERR_UNSUPPORTED. */
fhip_status fhip_outlines_nesting(fhip_ctx* ctx, const void* outlines, const uint64_t* bricks, int bricks_on_device, void** out);
void fhip_nesting_counts(const void* nest, uint64_t out[8]);
fhip_status fhip_nesting_layers(const void* nest, uint64_t* outer, uint64_t* top, uint32_t* max_depth);
fhip_status fhip_nesting_loops(const void* nest, uint64_t first, uint64_t count, uint32_t* left, uint32_t* parent, uint32_t* depth,
                               uint32_t* n_children, int64_t* region_area2);
const uint32_t* fhip_nesting_parent_dev(const void* nest);
const uint32_t* fhip_nesting_depth_dev(const void* nest);
fhip_status fhip_nesting_children(const uint32_t* parent, uint64_t n, uint64_t* child_start, uint32_t* children);
void fhip_nesting_free(void* nest);

/* ---- the slices of a triangle mesh: closed contour loops per plane z = const ----------------------------------------
 * (No counterpart in the reference, which never cuts a mesh: the definition below is the specification.  Every output but one is the
 * same bits from run to run and does not depend on how the hardware orders the threads; a loop's area2 is a float64 sum of the same
 * terms in an order of arrival that may differ from run to run, and it alone.)
 * INPUT.  `topology`: a handle of fhip_triangles_topology or fhip_mesh_topology with its device arrays - the vertices, 3 f32 each, and
 * the triangles as vertex ids, welded or as given, no coordinate that is not finite.  A topology that rejected triangles holds no mesh
 * and is FHIP_ERR_UNSUPPORTED.  `zs`: n_planes f32 on the host.  The planes must be finite and strictly ascending: anything else is
 * FHIP_ERR_UNSUPPORTED, and nothing is written.  n_planes == 0 is FHIP_OK with empty results, as is a mesh without triangles.  A
 * triangle with two equal vertex ids is skipped.  Planes are always z = const; other directions are the caller's transform of the
 * vertices.
 * SIDE.  Vertex v is above plane p iff z_v >= zs[p], by float comparison, so -0 equals +0.  a(v) is the number of planes v is above,
 * an upper bound search in zs; everything after it is integer arithmetic.  Edge {u, v} crosses exactly the planes
 * min(a_u, a_v) <= p < max(a_u, a_v); triangle t crosses the planes from the smallest to the largest a of its corners.  A solid
 * spanning [z0, z1] is therefore cut by the planes in (z0, z1].
 * CROSSINGS.  A crossing is a pair (undirected mesh edge, plane): a vertex of the slice, the same one from whichever triangle reaches
 * it.  The crossing edges are taken in the order of their first corners - the smallest corner 3 t + i that uses the edge, from i to
 * i + 1 - and within an edge the crossings by ascending plane; ids come from one exclusive prefix sum over the corners, never from the
 * order of the table's slots.  2^32 - 1 crossings or more is FHIP_ERR_OVERFLOW, and so is 2^32 - 1 segments or more.  edge[X] = (u, v),
 * u < v, and plane[X].  Position: with u the end with the smaller vertex id, t = (zs[p] - z_u) / (z_v - z_u), x = x_u + t (x_v - x_u)
 * and y likewise, in binary64 from the floats converted, every operation rounded on its own, no contraction, the result rounded to
 * float32: xy[X].  z_u == zs[p] gives the mesh vertex itself.  Coincident crossings and zero-length segments are legal.
 * SEGMENTS.  A crossing triangle has one corner alone on its side of the plane; name the corners (A, B, C) in the triangle's order
 * with A the lone one.  If A is above, the segment runs from the crossing on edge A -> B to the crossing on edge C -> A; if A is below,
 * the other way.  For a mesh that is counter-clockwise seen from outside the inside is then on the left seen from +z: outer boundaries
 * have area2 > 0 and holes area2 < 0, as for fhip_voxels_outlines and fhip_contour2d.  Vertices are not reduced to turns.
 * PER CROSSING.  out and in are the numbers of segments that leave a crossing and arrive at it; degree[X] is one byte, out | in << 4,
 * each saturating at 15.  A crossing is irregular iff out != 1 or in != 1: on a boundary edge, a nonmanifold edge, a flipped
 * triangle.  next[X] is the end of the segment leaving X in the triangle with the smallest index, 0xFFFFFFFF when out == 0.
 * LOOPS.  A loop is a connected part of the crossings under all segments.  A loop's leader is its smallest crossing id; loops are
 * numbered in ascending order of leader; loop_of[X].  Per loop: leader; plane; the numbers of its crossings, segments and irregular
 * crossings; area2, the float64 sum over its segments s -> d of x_s y_d - x_d y_s from the float32 positions converted, each product
 * and the difference rounded on their own; lo[2] and hi[2], the exact bounds of its positions, -0 taken as +0.  A loop is a closed
 * polygon iff it has no irregular crossing: next then walks it from the leader back to the leader.  Per plane: the counts of
 * crossings, segments and loops.
 * THE PASSES.  Levels per vertex; the crossing edges alone into a lock-free edge table as fhip_triangles_topology's (a topology does
 * not keep its own), sized from the count of crossing corners: the least power of two at or above 4/3 of them, or exactly
 * 1 << table_log2 slots (at most 32); a probe sequence that finds no room is FHIP_ERR_OVERFLOW, nothing spins.  Counts at the first
 * corners and per triangle, prefix sums; then a lane per crossing and a lane per segment, each finding its corner or triangle by a
 * search in the sums, so that a coarse mesh under thousands of planes fills the device; a union-find towards the smaller root; the
 * loops' table by atomics.  No pass waits for another workgroup.  The scratch stays with the context in the buffer of the mesher's leaf
 * records: fhip_ctx_trim gives it back.  The call blocks.
 * counts = {planes, crossings, segments, loops, irregular crossings, edge-table slots, 0, 0}.  fhip_slices_planes: zs and the three
 * counts per plane; fhip_slices_loops: a row per loop; fhip_slices_vertices: host copies of the arrays per crossing (xy 2 f32, edge 2
 * u32); any output pointer may be NULL.  The _dev getters return the handle's device arrays, NULL where there are no crossings. */
fhip_status fhip_topology_slices(fhip_ctx* ctx, const void* topology, const float* zs, uint32_t n_planes, uint32_t table_log2, void** out);
void fhip_slices_counts(const void* slices, uint64_t out[8]);
fhip_status fhip_slices_planes(const void* slices, float* zs, uint64_t* crossings, uint64_t* segments, uint64_t* loops);
fhip_status fhip_slices_loops(const void* slices, uint32_t* leader, uint32_t* plane, uint32_t* crossings, uint32_t* segments, uint32_t* irregular,
                              double* area2, float* lo, float* hi);
fhip_status fhip_slices_vertices(const void* slices, float* xy, uint32_t* plane, uint32_t* edge, uint32_t* next, uint32_t* loop_of, uint8_t* degree);
const float* fhip_slices_xy_dev(const void* slices);
const uint32_t* fhip_slices_next_dev(const void* slices);
const uint32_t* fhip_slices_loop_dev(const void* slices);
const uint32_t* fhip_slices_plane_dev(const void* slices);
void fhip_slices_free(void* slices);

/* ---- the nesting of those slices: polygons with holes per plane ---------------------------------------------------
 * (fhip_outlines_nesting's counterpart for a mesh's slices.  No bitmap lies under these loops: they are float32 polygons, and which
 * contains which is decided by a ray cast from each loop's leader towards -x against the polygons themselves.  No counterpart in the
 * reference; the definition below is the specification.)
 * All of it is over one handle of fhip_topology_slices: its xy, plane, next and loop_of per crossing where they are in device memory,
 * and its loops' table - leader, plane, crossings, irregular, area2.
 * LOOPS THAT TAKE PART.  The regular loops: those without an irregular crossing, the closed polygons.  An irregular loop takes no
 * part: parent = depth = 0xFFFFFFFF (NONE), n_children = 0, region_area2 = 0, and its segments are ignored.  The segments of a regular
 * loop are v -> next[v] for each of its crossings v, one per crossing.
 * A HIT.  Leader position q = xy[leader[l]], and a segment s -> d of another regular loop m != l of the same plane.  The segment is hit
 * iff (1) it straddles q's row under the half-open rule (s.y <= q.y) != (d.y <= q.y), by float32 comparison - each vertex's y is
 * compared once, so two segments that share a vertex on the row cannot both count or both miss where the loop passes through the row
 * - and (2) its crossing of the row lies strictly left of q, decided by the sign of
 * c = (d.x - s.x) * (q.y - s.y) - (q.x - s.x) * (d.y - s.y), the float32 values converted to binary64, every operation rounded on its
 * own, no contraction: hit iff c < 0 for an upward segment (s.y <= q.y), c > 0 for a downward one; c == 0 is not a hit.  This binary64
 * sequence IS the definition.  It is not exact for arbitrary float32 input - the differences may round - so a leader within rounding
 * of another loop's boundary may fall either side, but always the same side: the result is a function of the six floats alone.
 * CONTAINMENT AND DEPTH.  m contains l iff the number of hit segments of m is odd.  depth[l] is the number of loops that contain l.
 * PARENT.  parent[l] is the containing loop with the largest depth, the smallest id among equals; NONE if there is none.  For loops that
 * do not cross each other the containing loops form a chain and depth[parent[l]] == depth[l] - 1; `improper` counts the loops with a
 * parent where that equation fails, so a caller learns that loops cross without testing it.
 * MISORIENTED.  The regular loops whose orientation disagrees with their depth: (depth even) != (area2 > 0).  A shell turned inside out
 * shows up here.  This is the one integer that inherits area2's order of arrival, and only for loops of area near zero.
 * CHILDREN AND REGIONS.  n_children[l]: the loops whose parent is l.  region_area2[l] (float64): area2[l] plus its children's area2,
 * added in ascending child id - deterministic given area2.  A region is a loop of even depth with its children: even-odd filling.
 * PER PLANE.  regular; outer (even depth); top (no parent); max_depth; improper; misoriented - and the number of bands used.
 * Everything but misoriented and region_area2 is the same bits from run to run; nothing depends on the order of arrival of atomics,
 * on the number of bands, or on the order of the triangles beyond what the slices fix.
 * THE PASSES.  The segments of every plane are indexed by bands of y.  band(y) = clamp(floor((y - y0) * scale), 0, nb - 1) in float32,
 * each operation rounded on its own, NaN -> 0: monotone non-decreasing in y, which alone guarantees that a segment that straddles q's
 * row is listed in band(q.y).  y0 and scale = nb / (y1 - y0) come from the y-extent of the plane's regular loops (lo, hi); an empty
 * extent is one band.  CSR: a count pass - a lane per regular segment adds to each band from that of its lower to that of its upper
 * end - a prefix sum, a fill pass; entries arrive in any order and no result depends on it.  `bands` == 0 is the host's rule: a plane
 * gets one band per 32 regular segments, at least 1 and at most 2^20; if the count pass reports more than 4 entries per regular segment,
 * every plane's number is halved and the count repeated, until it fits or all are 1.  `bands` != 0: that many for every plane, used as
 * given.  2^32 - 1 bands, band entries or hits or more is FHIP_ERR_OVERFLOW.  Then a wave per leader: its lanes stride over the entries
 * of the leader's band and apply the predicate; hits are counted, prefix-summed over the leaders, and written - the hit loop's id per
 * hit - at places from ballot and popcount, no atomics: a list of at most 512 stays in the wave's LDS, a longer one goes to global memory.
 * The ids of odd multiplicity of a leader's list are its containing loops (any length: nothing of fixed size is overrun), their number
 * its depth; after all depths, the parent and the integer sums.  A band's entry is the segment itself, 20 bytes, read in order.  No kernel waits for another workgroup,
 * nothing spins, and every loop is bounded by the arrays' sizes.  The scratch stays with the context, as for the slices.
 * The call blocks.  Refused before any launch: no context, slices or result (FHIP_ERR_BAD_TAPE), slices of another device's context
 * (FHIP_ERR_UNSUPPORTED).  Zero planes, zero loops, or irregular loops alone give FHIP_OK, an empty result and no device arrays.
 * counts = {loops, regular, outer, top, max depth, improper, misoriented, planes, bands, band entries, hits, 0 ..}.
 * fhip_slice_nesting_planes: the six counts (uint64) and the bands per plane; fhip_slice_nesting_loops: a row per loop; any output
 * pointer may be NULL.  parent and depth stay in device memory with the handle (the _dev getters; NULL for an empty result).  Children
 * lists: fhip_nesting_children over `parent`. */
fhip_status fhip_slices_nesting(fhip_ctx* ctx, const void* slices, uint32_t bands, void** out);
void fhip_slice_nesting_counts(const void* nest, uint64_t out[16]);
fhip_status fhip_slice_nesting_planes(const void* nest, uint64_t* regular, uint64_t* outer, uint64_t* top, uint64_t* max_depth, uint64_t* improper,
                                      uint64_t* misoriented, uint32_t* bands);
fhip_status fhip_slice_nesting_loops(const void* nest, uint32_t* parent, uint32_t* depth, uint32_t* n_children, double* region_area2);
const uint32_t* fhip_slice_nesting_parent_dev(const void* nest);
const uint32_t* fhip_slice_nesting_depth_dev(const void* nest);
void fhip_slice_nesting_free(void* nest);

/* ---- profiling ----------------------------------------------------------------------- */
/* When enabled, every kernel launch of a render is bracketed by HIP events on the context's
 * stream; fhip_profile_read returns per-kernel-class totals of the last render. */
enum { FHIP_K_TILES = 0, FHIP_K_POINTS = 1, FHIP_K_NORMALS = 2, FHIP_K_OTHER = 3, FHIP_K_COUNT = 4 };
void fhip_profile_enable(fhip_ctx* ctx, int on);
fhip_status fhip_profile_read(fhip_ctx* ctx, double ms[4], uint32_t launches[4]);
/* ... and per assembly kernel, each launch bracketed by its own pair of events:
 * index 0 fh_columns, 1 / 2 fh_float_eval_{16x4, 32x2}, 3 fh_tiles, 4 fh_prune1 */
fhip_status fhip_profile_read_kernels(fhip_ctx* ctx, double ms[8], uint32_t launches[8]);
/* Counters of the last render: [0] arena ops used (peak), [1] arena overflows, [2] leaves of the last slab, [3] queue overflows,
 * [4..5] queue entries per tile level below the root; [6] (context total) frames whose tile stage ran on the HIP C++ kernels without a
 * switch asking for it (tapes beyond the assembly kernels' register files); [7] (context total) 3D frames whose tile_sizes were valid but not a list the
 * kernels take - leaves other than 8^3, a fan-out above 64 - and were rendered with the library's own list (same image) */
fhip_status fhip_render_counters(fhip_ctx* ctx, uint64_t out[8]);

/* Diagnostics (wave statistics, arena / queue dumps, micro-benchmarks, the tape-group plans) are declared in
 * fidget_hip_debug.h: they are not part of the surface a binding needs. */

/* ---- host mirror of fidget_core::Context (no Rust toolchain here; tests + demos) ------ */
/* Opcode numbers = declaration order of UnaryOpcode / BinaryOpcode (context/op.rs:11-48). */
fhip_graph* fhip_graph_new(void);
void fhip_graph_free(fhip_graph* g);
uint32_t fhip_graph_len(const fhip_graph* g);
uint32_t fhip_graph_var(fhip_graph* g, int axis_or_3, uint64_t index); /* 0 X, 1 Y, 2 Z, 3 Var::V(index) */
uint32_t fhip_graph_constant(fhip_graph* g, float v);
uint32_t fhip_graph_unary(fhip_graph* g, int opcode, uint32_t a);              /* 0xFFFFFFFF = BadNode */
uint32_t fhip_graph_binary(fhip_graph* g, int opcode, uint32_t a, uint32_t b);
uint32_t fhip_graph_from_text(fhip_graph* g, const char* text);               /* Context::from_text */
/* MathFunction::new (eval/mod.rs:203-208) */
fhip_status fhip_tape_from_graph(fhip_ctx* ctx, const fhip_graph* g, const uint32_t* roots, uint32_t n_roots,
                                 fhip_tape** out);
/* VarMap of a graph-built tape: slot of X/Y/Z (axis 0..2) or of Var::V(index); -1 if absent */
int fhip_tape_axis_slot(const fhip_tape* tape, int axis);
int fhip_tape_var_slot(const fhip_tape* tape, uint64_t index);

/* RegionSize::screen_to_world (render/region.rs:87-108); n = 2 -> 3x3, n = 3 -> 4x4, row major */
void fhip_screen_to_world(const uint32_t* size, int n, float* out);

#ifdef __cplusplus
}
#endif
#endif
