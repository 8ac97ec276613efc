// Fragment of capi.hip (the 2D / 3D tile renderers: frame set-up, the coarse levels, slabs, streams and frame pipelining); not a stand-alone header: included by capi.hip only.
// ---- renders ---------------------------------------------------------------------------
static fhip_status bind_inputs(fhip_ctx* ctx, const fhip_tape* tape, const int32_t* axis_slots, const uint64_t* keys,
                               const float* vals, uint32_t n, FhRender& P) {
    const fh::HostTape& t = tape->t;
    std::vector<char> bound(FH_MAX_INPUTS, 0);
    for (uint32_t s = 0; s < FH_MAX_INPUTS; s++) { P.in_kind[s] = 3; P.in_value[s] = 0.0f; }
    for (int a = 0; a < 3; a++) {
        const int s = axis_slots ? axis_slots[a] : t.vars.axis[a];
        if (s >= 0 && s < FH_MAX_INPUTS) { P.in_kind[s] = (uint32_t)a; bound[s] = 1; }
    }
    for (uint32_t i = 0; i < n; i++) {
        // graph-built tapes: keys are Var::V indices; bytecode tapes (axis_slots given): keys are slots
        const int s = axis_slots ? (int)keys[i] : t.vars.slot_of(3, keys[i]);
        if (s >= 0 && s < FH_MAX_INPUTS) { P.in_value[s] = vals[i]; bound[s] = 1; }
    }
    for (uint32_t s = 0; s < t.n_vars; s++)
        if (!bound[s]) return fail(ctx, FHIP_ERR_MISSING_VAR, "a variable of the shape has no value");
    return FHIP_OK;
}

// (option stats, bit 1: where the host thread's time of a 3D frame goes - set-up, prepare, state upload, coarse levels, slabs, finish -
// printed every 200 frames; tools/host_enqueue.py)
struct HostSpans {
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t n = 0;
    std::chrono::steady_clock::time_point last;
    void start() { last = std::chrono::steady_clock::now(); }
    void mark(int k) { const auto now = std::chrono::steady_clock::now(); t[k] += std::chrono::duration<double, std::micro>(now - last).count(); last = now; }
    void frame() {
        if (++n % 200 == 0) {
            fprintf(stderr, "fidget-hip host us per frame: set-up %.1f prepare %.1f upload %.1f coarse %.1f slabs %.1f finish %.1f\n", t[0] / 200, t[1] / 200, t[2] / 200, t[3] / 200, t[4] / 200, t[5] / 200);
            for (double& x : t) x = 0;
        }
    }
};
static thread_local HostSpans g_spans;      // (one context per thread: each thread's frames, not a mix)
#define FH_SPAN(k) do { if (ctx->opt.stats & 2) g_spans.mark(k); } while (0)

// The facts of a context the frame plan is made from (frame_plan.hpp); arena_bytes: the caller's (prepare: what the frame's arena will have)
static PlanInputs plan_inputs(const fhip_ctx* ctx) {
    PlanInputs in;
    in.slab_layers = ctx->opt.slab_layers; in.no_zrep = ctx->opt.no_zrep; in.no_column_inv = ctx->opt.no_column_inv; in.no_columns_t = ctx->opt.no_columns_t;
    in.no_asm_normals = ctx->opt.no_asm_normals; in.no_asm_tiles = ctx->opt.no_asm_tiles; in.no_asm_tiles_t = ctx->opt.no_asm_tiles_t;
    in.no_tape_groups = ctx->opt.no_tape_groups; in.prune2 = ctx->opt.prune2; in.root32_max = ctx->opt.root32_max;
    in.use_asm = ctx->use_asm; in.use_split = ctx->use_split; in.n_cu = (uint32_t)ctx->n_cu; in.slab_contexts = ctx->slab_contexts; in.arena_bytes = ctx->arena_bytes;
    return in;
}

// Wait for the work of THIS context - its own streams and its lanes' - and nobody else's: other contexts on the device keep running
// (hipDeviceSynchronize here stalled every thread's context for an arena that belongs to one).
static hipError_t sync_own_streams(fhip_ctx* ctx) {
    hipError_t e = hipSuccess;
    for (hipStream_t s : {ctx->stream, ctx->stream2, ctx->stream3, ctx->stream_pre}) {
        const hipError_t r = hipStreamSynchronize(s);       // (ctx->stream is the caller's stream at all times - no render assigns it -, so the caller's stream is waited for too; null: the device's default stream, the caller chose it)
        if (r != hipSuccess && e == hipSuccess) e = r;
    }
    for (fhip_ctx* L : ctx->lanes)
        if (L) { const hipError_t r = sync_own_streams(L); if (r != hipSuccess && e == hipSuccess) e = r; }
    return e;
}
// The arena of the context's sets becomes `want` bytes (frame_plan.hpp arena_bytes_for: a frame before this one ran out, or this frame
// needs more from the start): wait for what is in flight and let the sets come back larger
static fhip_status grow_arena_if_asked(fhip_ctx* ctx, size_t want) {
    if (want == ctx->arena_bytes) return FHIP_OK;
    HIP_TRY(ctx, sync_own_streams(ctx));       // (every stream of the context, its lanes included: a set's arena is about to be replaced)
    if (ctx->host_flags) ctx->host_flags[0] = 0;
    ctx->arena_bytes = want;
    return FHIP_OK;
}

// The root tables of a tape on the device, made once per tape by the first frame that takes the groups path: top ops and choice sources, and
// (option prune2) the links of the root tape with its choice table and root chain for the linked prune
static fhip_status ensure_root_tables(fhip_ctx* ctx, const fhip_tape* tape) {
    const fh::HostTape& t = tape->t;
    std::lock_guard<std::mutex> guard(tape->upload_lock);
    if (tape->device >= 0 && tape->device != ctx->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "this tape's device copies belong to another device: build the tape per device");
    tape->device = ctx->device;
    if (!tape->d_top) {
        static_assert(sizeof(FhTopOp) == sizeof(fh::TopOp), "top op layout");
        HIP_TRY(ctx, hipMalloc((void**)&tape->d_top, tape->plan.top.size() * sizeof(FhTopOp)));
        HIP_TRY(ctx, hipMemcpy(tape->d_top, tape->plan.top.data(), tape->plan.top.size() * sizeof(FhTopOp), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMalloc((void**)&tape->d_chsrc, std::max<size_t>(tape->plan.choice_src.size(), 1) * 4));
        HIP_TRY(ctx, hipMemcpy(tape->d_chsrc, tape->plan.choice_src.data(), tape->plan.choice_src.size() * 4, hipMemcpyHostToDevice));
    }
    if (ctx->opt.prune2 && !tape->links_tried) {
        tape->links_tried = true;
        std::vector<uint64_t> lk;
        std::vector<uint64_t> cops;
        if (fh::compute_links(t, lk, cops)) {
            // (published together or not at all: a failure half way must not leave links without their choice table)
            uint64_t *dl = nullptr, *dc = nullptr;
            // the root chain's ops (plan.chain: acc = min / max(acc, term) all the way to the OUTPUT op) in evaluation order, behind the choice
            // table: the linked prune's liveness pass starts from every kept op of the chain at once instead of walking it link by link
            std::vector<uint32_t> chain = chain_table(tape, cops);
            const size_t n_cops = std::max<size_t>(cops.size(), 1);
            cops.resize(n_cops + (chain.size() + 1) / 2, 0);
            if (!chain.empty()) memcpy(cops.data() + n_cops, chain.data(), chain.size() * 4);
            hipError_t e = hipMalloc((void**)&dl, lk.size() * 8);
            if (e == hipSuccess) e = hipMemcpy(dl, lk.data(), lk.size() * 8, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMalloc((void**)&dc, std::max<size_t>(cops.size(), 1) * 8);
            if (e == hipSuccess) e = hipMemcpy(dc, cops.data(), cops.size() * 8, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                if (dl) (void)hipFree(dl);
                if (dc) (void)hipFree(dc);
                HIP_TRY(ctx, e);
            }
            tape->d_links = dl; tape->d_ctab = dc; tape->n_chain = (uint32_t)chain.size();
        }
    }
    return FHIP_OK;
}

// The frame's pointers into the context's buffers, its counters at zero, its stamp
static void bind_state(fhip_ctx* ctx, const fhip_tape* tape, bool is3d, RenderSetup& R) {
    FhRenderState& S = R.S;
    const FhRender& P = S.P;
    S.frame_stamp = ++ctx->frame_stamp;
    if (R.hip_tiles_unasked) ctx->hip_tile_frames++;
    S.gscratch = R.big_hbm ? (char*)ctx->gscratch.p : nullptr;
    if (is3d) {
        uint32_t* mp = (uint32_t*)ctx->mind.p;
        for (uint32_t l = 0; l < P.n_levels; l++) {
            S.mind[l] = mp;
            mp += (size_t)((P.width + P.tiles[l] - 1) / P.tiles[l]) * ((P.height + P.tiles[l] - 1) / P.tiles[l]);
        }
        for (int c = 0; c < 3; c++) S.fp_list[c] = (uint32_t*)ctx->fp_lists.p + (size_t)c * R.n_footprints;
        S.hit_list = (uint32_t*)ctx->fp_lists.p + (size_t)3 * R.n_footprints;
    }
    S.arena = (uint64_t*)ctx->arena.p;
    S.arena_overflow = 0;
    for (int l = 0; l < FH_MAX_LEVELS; l++) {
        S.queue[l] = (FhGroup*)ctx->queue[l].p;
        S.count[l] = S.cursor[l] = S.count_big[l] = S.cursor_big[l] = 0;
    }
    S.count_big[0] = (uint32_t)R.roots.size();  // the root tape always takes the large LDS layout
    if (R.groups) {
        S.ttop = tape->d_top; S.chsrc = tape->d_chsrc;
        R.d_ctab = tape->d_ctab; R.d_links = tape->d_links;
        S.tvals = (float*)ctx->tvals.p; S.topch = (uint8_t*)ctx->topch.p; S.chwr = (uint32_t*)ctx->chwr.p;
    }
    if (R.prune1) for (int k = 0; k < 2; k++) S.chw[k] = (uint32_t*)ctx->chw[k].p;
    if (R.split) for (int k = 0; k < 2; k++) S.slots[k] = (FhSlot*)ctx->slots[k].p;
    S.squeue = (FhGroup*)ctx->squeue.p;
    for (int k = 0; k < FH_MAX_SLABS; k++) S.scount[k] = S.scount_big[k] = 0;
    S.queue_overflow = 0;
    S.leaves = (FhLeaf*)ctx->leaves.p;
    S.n_leaves = S.leaf_cursor = S.leaf_cursor_big = S.normal_cursor = S.normal_cursor_big = 0;
    S.leaf_table = (FhLeafRef*)ctx->leaf_table.p;
    for (int c = 0; c < 3; c++) S.fp_count[c] = S.fp_cursor[c] = 0;
    S.zbuf = (uint64_t*)ctx->zbuf.p;
    S.normals = (float*)ctx->normals.p;
    S.image2d = nullptr;
    memset(S.stat, 0, sizeof(S.stat));
    memset(S.leaf_stat, 0, sizeof(S.leaf_stat));
    S.want_stats = (ctx->profiling || ctx->probe || (ctx->opt.stats & 1)) ? 1 : 0;
}

// A frame's set-up: the plan (frame_plan.hpp: every check, size and path), then the device's part of it in a fixed order - the arena's
// growth, the buffers, the tape's root tables, the pointers
static fhip_status prepare(fhip_ctx* ctx, const fhip_tape* tape, const TapeFacts& facts, bool is3d, const std::vector<uint32_t>& ts,
                           const PartSpec& part, RenderSetup& R) {
    static_assert(PLAN_BAD_TAPE == FHIP_ERR_BAD_TAPE && PLAN_UNSUPPORTED == FHIP_ERR_UNSUPPORTED, "the plan's refusals are fhip_status values");
    const FhRender& P = R.S.P;
    PlanInputs in = plan_inputs(ctx);
    in.arena_bytes = arena_bytes_for(ctx->arena_bytes, ctx->arena_cap_bytes, (size_t)FH_ARENA_START_MB << 20, ctx->host_flags && ctx->host_flags[0] != 0, facts.n_ops,
                                     is3d && !R.root_invariant ? (uint64_t)P.width * P.height * P.depth : 0);
    const PlanStatus ps = plan_frame(facts, in, is3d, ts, part, R);
    if (ps.status) return fail(ctx, (fhip_status)ps.status, ps.msg);
    { const fhip_status gs = grow_arena_if_asked(ctx, in.arena_bytes); if (gs) return gs; }
    const FrameBytes& B = R.bytes;
    HIP_TRY(ctx, ctx->gscratch.ensure(B.gscratch));
    HIP_TRY(ctx, ctx->state.ensure(4 * sizeof(FhRenderState)));
    { void* const before = ctx->arena.p; HIP_TRY(ctx, ctx->arena.ensure(ctx->arena_bytes)); if (ctx->arena.p != before) ctx->resident_serial = 0; }
    for (size_t l = 0; l < ts.size(); l++) HIP_TRY(ctx, ctx->queue[l].ensure(B.queue[l]));
    const std::pair<DevBuf*, size_t> list[] = {{&ctx->squeue, B.squeue}, {&ctx->leaves, B.leaves}, {&ctx->leaves_b, B.leaves_b}, {&ctx->leaf_table, B.leaf_table},
                                               {&ctx->leaf_table_b, B.leaf_table_b}, {&ctx->zbuf, B.zbuf}, {&ctx->normals, B.normals}, {&ctx->fp_lists, B.fp_lists},
                                               {&ctx->fp_lists_b, B.fp_lists_b}, {&ctx->mind, B.mind}, {&ctx->tvals, B.tvals}, {&ctx->topch, B.topch}, {&ctx->chwr, B.chwr},
                                               {&ctx->chw[0], B.chw[0]}, {&ctx->chw[1], B.chw[1]}, {&ctx->slots[0], B.slots}, {&ctx->slots[1], B.slots}};
    for (const auto& b : list) HIP_TRY(ctx, b.first->ensure(b.second));      // (0 bytes: not needed by this frame, left as it is)
    if (R.groups) {
        const fhip_status us = ensure_root_tables(ctx, tape);
        if (us) return us;
        plan_linked_prune(facts, in, tape->d_links && tape->d_ctab, tape->n_chain, R);
    }
    bind_state(ctx, tape, is3d, R);
    return FHIP_OK;
}

static int blocks_for(const fhip_ctx* ctx, size_t lds, int max_per_cu);
// ... of a root-sized launch: as many workgroups as LDS lets run, or the number of HBM register-file regions
static int blocks_big(const fhip_ctx* ctx, const RenderSetup& R, size_t lds, int max_per_cu) {
    return R.big_hbm ? (int)R.hbm_waves : blocks_for(ctx, lds, max_per_cu);
}
static int blocks_for(const fhip_ctx* ctx, size_t lds, int max_per_cu) {
    int per_cu = lds ? (int)std::min<size_t>((size_t)max_per_cu, FH_LDS_MAX / std::max<size_t>(lds, 1)) : max_per_cu;
    per_cu = std::max(per_cu, 1);
    return ctx->n_cu * per_cu;
}

static fhip_status finish_render(fhip_ctx* ctx) {
    HIP_TRY(ctx, hipMemcpyAsync(&ctx->last_state, ctx->state.p, sizeof(FhRenderState), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 1; k < ctx->forked; k++) {  // the other slab contexts keep their own counters
        HIP_TRY(ctx, hipMemcpy(&ctx->last_state_b, (char*)ctx->state.p + k * sizeof(FhRenderState), sizeof(FhRenderState), hipMemcpyDeviceToHost));
        ctx->last_state.queue_overflow += ctx->last_state_b.queue_overflow;
        ctx->last_state.arena_overflow += ctx->last_state_b.arena_overflow;
        for (int i = 0; i < 64; i++) ctx->last_state.stat[i] += ctx->last_state_b.stat[i];
        for (int i = 0; i < 8; i++) ctx->last_state.leaf_stat[i] += ctx->last_state_b.leaf_stat[i];
    }
    ctx->have_last_state = true;
    if (ctx->last_state.queue_overflow) return fail(ctx, FHIP_ERR_OVERFLOW, "device work queue overflow");
    return FHIP_OK;
}

struct FrameClear { void* p = nullptr; size_t bytes = 0; uint32_t fill = 0; };   // a buffer the frame starts from cleared (bytes: a multiple of 4)
// The record that guards a staging slot (frame_schedule.hpp SlotGuard): the slot's event, behind what `st` - the frame's root stream - has been given so far
struct RecordSlot {
    fhip_ctx* ctx = nullptr; uint32_t slot = 0; hipStream_t st = nullptr;
    void operator()() const { if (hipEventRecord(ctx->staging[slot].ev, st) == hipSuccess) ctx->ring.used[slot] = true; else (void)hipGetLastError(); }
};
typedef SlotGuard<RecordSlot> StagingGuard;
// (`later`: the frame records the slot's guard itself, where its root stream leaves the root level or the frame ends - armed here once
// k_frame_begin is queued; none: recorded here, behind k_frame_begin)
static fhip_status upload_frame(fhip_ctx* ctx, hipStream_t st, const fhip_tape* tape, RenderSetup& R, const FrameClear (&clear)[3], StagingGuard* later = nullptr) {
    // The frame's state and root groups go through pinned staging slots (a ring of eight, each guarded by an event): a copy from
    // pageable memory would make the host wait for everything queued on the stream before it, i.e. for the previous frame.
    const size_t roots_bytes = R.roots.size() * sizeof(FhGroup);
    const uint32_t slot = ctx->ring.take();
    fhip_ctx::Staging& sg = ctx->staging[slot];
    if (sg.ev && ctx->ring.used[slot]) HIP_TRY(ctx, hipEventSynchronize(sg.ev));
    if (!sg.ev) HIP_TRY(ctx, hipEventCreateWithFlags(&sg.ev, hipEventDisableTiming));
    if (sg.cap < sizeof(FhRenderState) + roots_bytes) {
        if (sg.p) (void)hipHostFree(sg.p);
        sg.p = nullptr; sg.cap = 0;
        HIP_TRY(ctx, hipHostMalloc(&sg.p, sizeof(FhRenderState) + roots_bytes + 4096, hipHostMallocDefault));
        sg.cap = sizeof(FhRenderState) + roots_bytes + 4096;
    }
    memcpy(sg.p, &R.S, sizeof(FhRenderState));
    if (roots_bytes) memcpy((char*)sg.p + sizeof(FhRenderState), R.roots.data(), roots_bytes);
    { const fhip_status hs = hold_bound(ctx, tape); if (hs) return hs; }
    // The root tape and its groups sit below arena_root_end, where no frame writes: a shape rendered
    // again finds them there (17 small copies, 0.1 ms of a 4 ms frame, otherwise).
    if (ctx->resident_serial != tape->serial || ctx->resident_groups != R.S.n_tgroups) {
        ctx->resident_serial = 0;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->arena.p, tape->t.ops.data(), tape->t.ops.size() * 8, hipMemcpyHostToDevice, st));
        for (uint32_t g = 0; g < R.S.n_tgroups; g++)  // the group tapes follow the root tape
            HIP_TRY(ctx, hipMemcpyAsync((uint64_t*)ctx->arena.p + R.S.tgroup[g].off, tape->tgroups[g].ops.data(),
                                        tape->tgroups[g].ops.size() * 8, hipMemcpyHostToDevice, st));
        ctx->resident_serial = tape->serial;
        ctx->resident_groups = R.S.n_tgroups;
    }
    // state, root groups and the cleared buffers in one launch (k_frame_begin reads the pinned slot itself)
    static_assert(sizeof(FhRenderState) % 4 == 0 && sizeof(FhGroup) % 4 == 0, "copied as 32-bit words");
    FhFrameBegin fb;
    memset(&fb, 0, sizeof(fb));
    fb.state_dst = (uint32_t*)ctx->state.p; fb.state_src = (const uint32_t*)sg.p; fb.state_words = (uint32_t)(sizeof(FhRenderState) / 4);
    if (!R.roots.empty()) {
        fb.roots_dst = (uint32_t*)((FhGroup*)ctx->queue[0].p + (R.S.qcap[0] - R.roots.size()));
        fb.roots_src = (const uint32_t*)((const char*)sg.p + sizeof(FhRenderState));
        fb.roots_words = (uint32_t)(roots_bytes / 4);
    }
    size_t most = 0;
    for (int k = 0; k < 3; k++) {
        fb.clear[k] = (uint32_t*)clear[k].p; fb.clear_words[k] = clear[k].bytes / 4; fb.fill[k] = clear[k].fill;
        if (clear[k].p) most = std::max(most, clear[k].bytes);
    }
    const unsigned blocks = (unsigned)std::max<size_t>(8, std::min<size_t>((size_t)ctx->n_cu * 32, (most + 64 * 64 - 1) / (64 * 64)));
    FH_KLAUNCH(k_frame_begin, dim3(blocks), dim3(WAVE), 0, st, fb);
    // (armed before the launch's status is looked at: a launch that failed may still have been queued)
    if (later) { later->record_now = RecordSlot{ctx, slot, st}; later->arm(); }
    else RecordSlot{ctx, slot, st}();
    HIP_TRY(ctx, hipGetLastError());
    for (auto& e : ctx->prof_events) { (void)hipEventDestroy(e.second.first); (void)hipEventDestroy(e.second.second); }
    ctx->prof_events.clear();
    for (auto& e : ctx->asm_events) { (void)hipEventDestroy(e.second.first); (void)hipEventDestroy(e.second.second); }
    ctx->asm_events.clear();
    return FHIP_OK;
}

// One level of the tile hierarchy: the small-LDS variant for the bulk of the groups and the
// root-sized variant for the few large tapes (both always launched; empty queues exit at once).
#define FH_LAUNCH_TILES(IS3D, FULL, BIG, grid, lds)                                                                  \
    do {                                                                                                            \
        if (R.tl == 64) FH_KLAUNCH((k_tiles<IS3D, FULL, BIG, 64>), dim3(grid), dim3(WAVE), lds, st, dS, level); \
        else FH_KLAUNCH((k_tiles<IS3D, FULL, BIG, 16>), dim3(grid), dim3(WAVE), lds, st, dS, level);            \
    } while (0)
// Kernarg blocks of the assembly kernels: one struct per layout, each beside the generator function that reads it
struct KaTiles { FhRenderState* S; uint32_t level, big, max_regs, max_choices, n_waves, flags, skip_regs, skip_choices; };            // gen_tiles.py gen_tiles, gen_tilesv.py gen_tilesv
struct KaPrune1 { FhRenderState* S; uint32_t level, big, max_choices, mode; };                                                        // gen_prune.py gen_prune1
struct KaColumns { FhRenderState* S; uint32_t n_waves, slots, depmask, flags, pad[2]; const void* table; uint32_t nfpl, layers; };    // gen_interp.py gen_columns
struct KaNormals { FhRenderState* S; uint32_t n_waves, slots, z_lo, z_hi, bucket_cap, mode; };                                        // gen_normals.py gen_normals

// The streams of a context by role (frame_schedule.hpp), and the role the host thread is queueing on
struct FrameStreams { hipStream_t s[N_ROLES]; Role cur; hipStream_t on() const { return s[cur]; } };
static FrameStreams frame_streams(const fhip_ctx* ctx, Role at = CALLER) { return FrameStreams{{ctx->stream, ctx->stream_pre, ctx->stream2, ctx->stream3}, at}; }
// The next stage goes to another stream: that stream waits for what has been queued here so far
static hipError_t hop(FrameStreams& fs, Role to, hipEvent_t ev) {
    if (to == fs.cur) return hipSuccess;
    const hipError_t e = hipEventRecord(ev, fs.on());
    fs.cur = to;
    return e != hipSuccess ? e : hipStreamWaitEvent(fs.on(), ev, 0);
}
// The facts of a context the schedule is made from (frame_schedule.hpp; the caller adds what it observes)
static ScheduleInputs schedule_inputs(const fhip_ctx* ctx, int out_is_device) {
    ScheduleInputs in;
    in.no_tiles_v = ctx->opt.no_tiles_v; in.no_zrep = ctx->opt.no_zrep; in.column_walk = ctx->opt.column_walk; in.column_group = ctx->opt.column_group;
    in.frame_pipeline = ctx->frame_pipeline; in.use_pipeline = ctx->use_pipeline; in.profiling = ctx->profiling; in.slab_contexts = ctx->slab_contexts;
    in.has_side = ctx->stream2 != nullptr; in.has_tail = ctx->stream3 != nullptr; in.has_flags = ctx->host_flags != nullptr; in.out_is_device = out_is_device != 0;
    return in;
}
// Rare mode: where a slab context's blocks keep their register files (a slab context = one FhRenderState of the set)
static char* rare_file(const fhip_ctx* ctx, const FhRenderState* dS, uint32_t rare_stride) {
    if (!rare_stride) return nullptr;
    return (char*)ctx->rare_scratch.p + (size_t)(dS - (const FhRenderState*)ctx->state.p) * FH_RARE_BLOCKS * rare_stride;
}
// 3D tile stage of one level as three kernels (see kernels.hip "Split 3D tile stage"): set-up, evaluate + prune - one of the three below,
// LevelPlan::path -, push
// Tape parallelism: the root tree's terms by independent groups, one wave per (block of root
// tiles, group) -> the tree over the terms (result, marks, arena) -> the root tape's choice words
// gathered from both -> one wave per ambiguous child prunes the root tape -> push.
static void tiles_by_groups(fhip_ctx* ctx, const RenderSetup& R, FhRenderState* dS, hipStream_t st) {
    const int gg = blocks_for(ctx, R.lds_tiles_group, 8);
    KaTiles ka = {dS, 0, 1, R.group_regs, R.group_choices, (uint32_t)gg, (ctx->probe ? 1u : 0u) | 2u | 4u | 8u, 0, 0};
    (void)launch_asm(ctx, st, FH_ASM_TILES, (uint32_t)gg, &ka, sizeof(ka), R.lds_tiles_group);
    const uint32_t blocks = R.S.qcap[0], root_words = (R.S.troot_choices + 15) / 16, group_words = (R.group_choices + 15) / 16;
    if (R.S.top_chain && R.S.n_top > 64u * FH_CHAIN_SEG) FH_KLAUNCH(k_tchain3d_chunks, dim3(WAVE, blocks), dim3(WAVE), 0, st, dS);
    else if (R.S.top_chain) FH_KLAUNCH(k_tchain3d, dim3(WAVE, blocks), dim3(WAVE), 0, st, dS);
    else FH_KLAUNCH(k_ttop3d, dim3(blocks), dim3(WAVE), 0, st, dS);
    // (the marks and the gather of the root tape's choice words do not depend on each other: one launch, the marks in the blocks
    // behind the gather's)
    if (R.classify_only || !root_words) FH_KLAUNCH(k_tmark3d, dim3(blocks), dim3(WAVE), 0, st, dS);
    if (R.classify_only) return;       // (the fills of the decided tiles follow in the push; nothing is pruned or queued)
    if (root_words) FH_KLAUNCH(k_tscatter3d, dim3(root_words + 1, blocks), dim3(WAVE), 0, st, dS, group_words, root_words);
    KaPrune1 kp = {dS, 0, 1, R.S.troot_choices, 2};
    if (!R.prune2) { (void)launch_asm(ctx, st, FH_ASM_PRUNE1, blocks * 64, &kp, sizeof(kp)); return; }
    hipEvent_t ea = nullptr, eb = nullptr;      // (timed under the fh_prune1 slot of the per-kernel profile: it replaces that launch)
    if (ctx->profiling) { (void)hipEventCreate(&ea); (void)hipEventCreate(&eb); (void)hipEventRecord(ea, st); }
    FH_KLAUNCH(k_prune2, dim3(blocks * FH_P2_PER_SLOT), dim3(FH_P2_WPB * FH_P2_WPC * 64), R.lds_prune2, st, dS, 0u, 1u, root_words,
                       (const uint2*)R.d_links, (const uint2*)R.d_ctab, 2u, R.S.troot_len, R.S.troot_choices, R.p2_cap_kept,
                       (const uint32_t*)(R.d_ctab + std::max<uint32_t>(R.S.troot_choices, 1)), R.n_chain);
    // ... and the scalar sweep behind it for the children it left marked (more than 64 registers or FH_P2_MAX_KEPT kept ops:
    // none for the models here; a wave whose child is done leaves at once)
    size_t kp_bytes = sizeof(kp);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &kp, HIP_LAUNCH_PARAM_BUFFER_SIZE, &kp_bytes, HIP_LAUNCH_PARAM_END};
    (void)hipModuleLaunchKernel(ctx->asm_fn[FH_ASM_PRUNE1], blocks * 64, 1, 1, WAVE, 1, 1, 0, st, nullptr, extra);
    if (ctx->profiling) { (void)hipEventRecord(eb, st); ctx->asm_events.push_back({FH_ASM_PRUNE1, {ea, eb}}); }
}
// The assembly tile kernels, as the level's plan says (frame_schedule.hpp plan_level: why each launch is there)
static void tiles_asm(fhip_ctx* ctx, const RenderSetup& R, const LevelPlan& L, FhRenderState* dS, int level, FrameStreams& fs) {
    // Persistent waves with a static round robin over the parents (one short workgroup per parent was measured slower in the
    // pipelined frame: the tile stage then takes more of the machine from the leaf kernel it overlaps with).
    const int gs = blocks_for(ctx, R.lds_tiles_small, 8), gb = blocks_big(ctx, R, R.lds_tiles_big, 8);
    const int K_TILES = R.asm_tiles_t ? FH_ASM_TILES_T : FH_ASM_TILES;
    auto big_stream = [&] { return L.fork_big ? fs.s[SIDE] : fs.on(); };      // where the launches for the other slot list go
    KaTiles ka = {dS, (uint32_t)level, 0, SMALL_REGS, SMALL_CHOICES, (uint32_t)gs, (ctx->probe ? 1u : 0u) | (L.exp ? 2u : 0u), 0, 0};
    if (L.fork_big) { (void)hipEventRecord(ctx->ev_rest_fork, fs.on()); (void)hipStreamWaitEvent(fs.s[SIDE], ctx->ev_rest_fork, 0); }
    if (L.v32) {
        // (32 waves per compute unit: twice what fits at once - the waves take the slots round robin, and with as many waves as
        // fit a launch of 1.5 slots per wave lasted two rounds of its longest parents: 0.213 -> 0.192 ms on the general path)
        ka.n_waves = (uint32_t)(ctx->n_cu * 32);
        (void)launch_asm(ctx, fs.on(), R.asm_tiles_t ? FH_ASM_TILES_V32_T : FH_ASM_TILES_V32, ka.n_waves, &ka, sizeof(ka));
    } else if (L.small_lds)
        (void)launch_asm(ctx, fs.on(), K_TILES, (uint32_t)gs, &ka, sizeof(ka), R.lds_tiles_small);
    ka.big = 1;
    if (L.exp) ka.flags |= ((R.S.P.max_choices + 15) / 16) << 16;  // one stride in chw[1] for the medium and the large layout
    if (L.rare) return;
    if (L.v64) {
        // (per-slab levels: the parents' tapes fit fh_tiles_v32 but for a rare one - an empty launch of 2048 waves of 176
        // VGPRs each, queued behind the leaf kernel of the slab in front, was measured to hold the tile chain up for
        // 130 us: a small persistent grid there)
        ka.max_regs = V64_REGS; ka.max_choices = V64_CHOICES;
        ka.n_waves = L.per_slab ? 128u : (uint32_t)(ctx->n_cu * 8);
        if (L.both_lists) ka.flags |= 16u;
        (void)launch_asm(ctx, big_stream(), R.asm_tiles_t ? FH_ASM_TILES_V64_T : FH_ASM_TILES_V64, ka.n_waves, &ka, sizeof(ka));
        (void)hop(fs, L.rest_on, ctx->ev_l1);      // (level 1 of a `tiles_first` frame: its remaining launches - the LDS layouts' rest, the push - leave the side stream)
        ka.flags &= ~16u;
        ka.skip_regs = V64_REGS; ka.skip_choices = V64_CHOICES;
    }
    if (L.mid) {
        const int gm = blocks_for(ctx, R.lds_tiles_mid, 8);
        ka.max_regs = MID_REGS; ka.max_choices = MID_CHOICES; ka.n_waves = (uint32_t)gm;
        (void)launch_asm(ctx, big_stream(), K_TILES, (uint32_t)gm, &ka, sizeof(ka), R.lds_tiles_mid);
        ka.skip_regs = MID_REGS; ka.skip_choices = MID_CHOICES;
    }
    ka.max_regs = R.S.P.max_regs; ka.max_choices = R.S.P.max_choices; ka.n_waves = (uint32_t)gb;
    if (L.rest) (void)launch_asm(ctx, big_stream(), K_TILES, (uint32_t)gb, &ka, sizeof(ka), R.lds_tiles_big);
    if (L.fork_big) { (void)hipEventRecord(ctx->ev_rest_join, fs.s[SIDE]); (void)hipStreamWaitEvent(fs.on(), ctx->ev_rest_join, 0); }
    if (L.exp) {
        KaPrune1 kp = {dS, (uint32_t)level, 0, SMALL_CHOICES, 0};
        const uint32_t bound = R.S.qcap[level] * 64;  // 64 waves per possible parent; unmarked children exit at once
        if (level > 0) (void)launch_asm(ctx, fs.on(), FH_ASM_PRUNE1, bound, &kp, sizeof(kp));
        kp.big = 1; kp.max_choices = R.S.P.max_choices;
        (void)launch_asm(ctx, fs.on(), FH_ASM_PRUNE1, bound, &kp, sizeof(kp));
    }
}
static void tiles_hip(fhip_ctx* ctx, const RenderSetup& R, FhRenderState* dS, int level, hipStream_t st) {
    const int gs = blocks_for(ctx, R.lds_tiles_small, 8), gb = blocks_big(ctx, R, R.lds_tiles_big, 8);
    if (level > 0 && R.full) FH_KLAUNCH((k_teval3d<true, false>), dim3(gs), dim3(WAVE), R.lds_tiles_small, st, dS, level);
    else if (level > 0) FH_KLAUNCH((k_teval3d<false, false>), dim3(gs), dim3(WAVE), R.lds_tiles_small, st, dS, level);
    if (R.full) FH_KLAUNCH((k_teval3d<true, true>), dim3(gb), dim3(WAVE), R.lds_tiles_big, st, dS, level);
    else FH_KLAUNCH((k_teval3d<false, true>), dim3(gb), dim3(WAVE), R.lds_tiles_big, st, dS, level);
}
// The monolithic tile kernel (option no_split)
static void launch_tiles_mono(fhip_ctx* ctx, const RenderSetup& R, FhRenderState* dS, int level, bool is3d, hipStream_t st) {
    const int gs = blocks_for(ctx, R.lds_tiles_small, 8), gb = blocks_big(ctx, R, R.lds_tiles_big, 8);
    launch(ctx, st, FHIP_K_TILES, [&] {
        if (is3d) { if (R.full) FH_LAUNCH_TILES(true, true, true, gb, R.lds_tiles_big); else FH_LAUNCH_TILES(true, false, true, gb, R.lds_tiles_big); }
        else { if (R.full) FH_LAUNCH_TILES(false, true, true, gb, R.lds_tiles_big); else FH_LAUNCH_TILES(false, false, true, gb, R.lds_tiles_big); }
    });
    if (level > 0)
        launch(ctx, st, FHIP_K_TILES, [&] {
            if (is3d) { if (R.full) FH_LAUNCH_TILES(true, true, false, gs, R.lds_tiles_small); else FH_LAUNCH_TILES(true, false, false, gs, R.lds_tiles_small); }
            else { if (R.full) FH_LAUNCH_TILES(false, true, false, gs, R.lds_tiles_small); else FH_LAUNCH_TILES(false, false, false, gs, R.lds_tiles_small); }
        });
}
// ... on the stream fs is at; fs moves only where the plan says so (LevelPlan::rest_on)
// (`head`: the level is the first of a frame's first tile chain and its set-up kernel carries the chain's head - tile_head below)
static void launch_tiles(fhip_ctx* ctx, const RenderSetup& R, const LevelPlan& L, FhRenderState* dS, int level, bool is3d, FrameStreams& fs, const FhHead* head = nullptr) {
    if (L.path == LevelPlan::MONO) return launch_tiles_mono(ctx, R, dS, level, is3d, fs.on());
    const int gp = ctx->n_cu * 8;
    launch(ctx, fs.on(), FHIP_K_TILES, [&] {
        if (is3d) FH_KLAUNCH(k_tsetup3d, dim3(gp), dim3(WAVE), 0, fs.on(), dS, level, head ? *head : FhHead{});
        else FH_KLAUNCH(k_tsetup2d, dim3(gp), dim3(WAVE), 0, fs.on(), dS, level);
    });
    launch(ctx, fs.on(), FHIP_K_TILES, [&] {
        if (L.path == LevelPlan::GROUPS) tiles_by_groups(ctx, R, dS, fs.on());
        else if (L.path == LevelPlan::ASM) tiles_asm(ctx, R, L, dS, level, fs);
        else tiles_hip(ctx, R, dS, level, fs.on());
    });
    // (last level: fewer waves, several parents each - one leaf reservation per wave)
    const bool last = level + 1 == (int)R.S.P.n_levels;
    const int gpush = last ? ctx->n_cu * L.push_mul : gp;
    launch(ctx, fs.on(), FHIP_K_TILES, [&] {
        // (above the leaf level: 16 more waves per parent for the fills of its interval-full children - kernels.hip tfill3d_body)
        const uint32_t rb = L.rare ? FH_RARE_BLOCKS : 0u;
        if (is3d) FH_KLAUNCH(k_tpush3d, dim3(gpush + rb, last ? 1 : 17), dim3(WAVE), 0, fs.on(), dS, level, rb, rare_file(ctx, dS, L.rare_stride), L.rare_stride);
        else {
            if (!R.classify_only) FH_KLAUNCH(k_tpush2d, dim3(gpush), dim3(WAVE), 0, fs.on(), dS, level);
            const uint32_t slots_max = R.S.qcap[level] * ((level == 0 && R.groups) ? R.S.n_tgroups : 1u);
            FH_KLAUNCH(k_tfill2d, dim3(64, slots_max), dim3(256), 0, fs.on(), dS, level);
        }
    });
}

static fhip_status render2d_frame(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render2d_config* cfg, float* out,
                                  int out_is_device) {
    if (ctx->is_cancelled()) return fail(ctx, FHIP_ERR_CANCELLED, "cancelled");
    RenderSetup R;
    memset(&R.S, 0, sizeof(R.S));
    FhRender& P = R.S.P;
    P.width = cfg->width; P.height = cfg->height; P.depth = 0; P.z = cfg->z; P.pixel_perfect = cfg->pixel_perfect ? 1 : 0;
    fhip_status st = bind_inputs(ctx, tape, cfg->axis_slots, cfg->var_keys, cfg->var_values, cfg->n_vars, P);
    if (st) return st;
    // mat = world_to_model * screen_to_world, lifted to 4x4 preserving Z (pixel.rs:122-124, 281-285)
    const uint32_t size[2] = {cfg->width, cfg->height};
    float s2w[9], m3[9];
    const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    fhip_screen_to_world(size, 2, s2w);
    mat_product(cfg->world_to_model ? cfg->world_to_model : ident, s2w, 3, m3);
    const float m4[16] = {m3[0], m3[1], 0, m3[2], m3[3], m3[4], 0, m3[5], 0, 0, 1, 0, m3[6], m3[7], 0, m3[8]};
    memcpy(P.mat, m4, sizeof(m4));
    std::vector<uint32_t> ts = cfg->tile_sizes ? trim_tiles(cfg->tile_sizes, cfg->n_tile_sizes, std::max(cfg->width, cfg->height))
                                               : trim_tiles(HIP_TILES_2D, 2, std::max(cfg->width, cfg->height));
    // A 2D fill says at which level of the caller's list it was decided (pixel.rs:225-229), so the list is part of the result and is kept -
    // but a step of the list whose fan-out exceeds the 64 lanes of a wavefront (128 -> 8: 256 children) is taken in two: a level in between
    // that the caller does not see.  A tile decided there is what its children of the caller's next level would ALL have been decided as
    // (interval arithmetic is inclusion monotone), so its fill carries THEIR level; an undecided one hands them a tape pruned once more,
    // which changes no value.  The image is the one the caller's list gives, fill tags included.
    std::vector<uint32_t> tags;
    {
        std::vector<uint32_t> out;
        for (size_t i = 0; i < ts.size(); i++) {
            if (i) {
                uint32_t a = ts[i - 1];
                const uint32_t b = ts[i];
                if (a <= b || a % b) return fail(ctx, FHIP_ERR_UNSUPPORTED, "bad tile size list");
                while (a / b > 8) {       // the largest tile below `a` that takes at most 8 x 8 of `a` and is made of whole `b`s
                    uint32_t c = 0;
                    for (uint32_t k = 8; k >= 2 && !c; k--) if (a % k == 0 && (a / k) % b == 0 && a / k > b) c = a / k;
                    if (!c) break;        // (no such divisor: left to the plan, which refuses the fan-out)
                    out.push_back(c); tags.push_back((uint32_t)i);
                    a = c;
                }
            }
            out.push_back(ts[i]); tags.push_back((uint32_t)i);
        }
        if (out.size() > FH_MAX_LEVELS) return fail(ctx, FHIP_ERR_UNSUPPORTED, "1..8 tile levels supported");
        ts = out;
    }
    const size_t npix = (size_t)cfg->width * cfg->height;
    float* d_out = out;
    if (!out_is_device) { HIP_TRY(ctx, ctx->tmp_out.ensure(npix * 4)); d_out = (float*)ctx->tmp_out.p; }
    const TapeFacts facts = tape_facts(tape);
    // One pass over a tile list: the tile levels, then the leaf pixels (`classify_only`: the root level's fills, nothing else)
    auto pass = [&](RenderSetup& Q, const std::vector<uint32_t>& tiles, const std::vector<uint32_t>& tg) -> fhip_status {
        for (size_t i = 0; i < FH_MAX_LEVELS; i++) Q.S.P.tag[i] = i < tg.size() ? tg[i] : (uint32_t)i;
        fhip_status ps = prepare(ctx, tape, facts, false, tiles, PartSpec{}, Q);
        if (ps) return ps;
        Q.S.image2d = d_out;
        FhRenderState* dS = (FhRenderState*)ctx->state.p;
        const FrameClear no_clear[3] = {};
        FrameStreams fs = frame_streams(ctx);       // (a 2D frame is one chain on the caller's stream)
        hipStream_t const st = fs.on();
        ps = upload_frame(ctx, st, tape, Q, no_clear);
        if (ps) return ps;
        for (uint32_t l = 0; l < Q.S.P.n_levels; l++) {
            if (ctx->is_cancelled()) return fail(ctx, FHIP_ERR_CANCELLED, "cancelled");
            launch_tiles(ctx, Q, plan_level(Q, schedule_inputs(ctx, out_is_device), (int)l, false, 0u, CALLER, CALLER), dS, (int)l, false, fs);
        }
        if (Q.classify_only) return FHIP_OK;
        launch(ctx, st, FHIP_K_POINTS, [&] {
            if (Q.full) FH_KLAUNCH((k_pixels2d<32, true>), dim3(ctx->n_cu * 8), dim3(WAVE), 0, st, dS);
            else FH_KLAUNCH((k_pixels2d<32, false>), dim3(ctx->n_cu * 16), dim3(WAVE), 0, st, dS);
        });
        if (Q.S.P.max_regs > 32)
            launch(ctx, st, FHIP_K_POINTS, [&] {
                const int g = blocks_big(ctx, Q, Q.lds_points_big, 16);
                if (Q.full) FH_KLAUNCH((k_pixels2d<0, true>), dim3(g), dim3(WAVE), Q.lds_points_big, st, dS);
                else FH_KLAUNCH((k_pixels2d<0, false>), dim3(g), dim3(WAVE), Q.lds_points_big, st, dS);
            });
        if (ctx->host_flags) FH_KLAUNCH(k_latch_arena, dim3(1), dim3(1), 0, st, dS, 1u, ctx->host_flags);    // (an arena that ran out: grown before the next frame)
        return FHIP_OK;
    };
    // Small images of a large tape (round 5).  With 128 x 128 root tiles a 256 x 256 image is FOUR one-wave chains over a tape that a quarter
    // of the image barely prunes: 4.1 ms for prospero.vm, where the 4096 x 4096 image takes 0.5.  The root level's forward pass is parallel
    // over the tape whatever the number of tiles (term groups) and the linked prune takes a thousand children in a round, so the ROOT tape
    // is pruned per leaf tile directly - a one-level pass over the list's last entry - and the pixels are evaluated from those tapes;
    // values and decisions are the two-level recursion's (inclusion monotone intervals).  What the caller's list
    // still decides is the level a fill SAYS it was decided at (pixel.rs:225-229): a leaf tile's fill is tagged with the last level, and a
    // second, classify-only pass over the root tiles writes the fills of the decided ones - level 0 - over whatever their leaf tiles
    // wrote (a decided root tile's leaf tiles are all decided the same way, so nothing else is overwritten).
    const bool small_ok = ts.size() == 2 && tags.size() == 2 && ts[1] >= 8 && ts[0] / ts[1] <= 8 && ctx->opt.root32_max > 0 && linked_root_tape(facts, plan_inputs(ctx)) &&
                          (uint64_t)((P.width + ts[1] - 1) / ts[1]) * ((P.height + ts[1] - 1) / ts[1]) <= 2048u &&
                          (uint64_t)((P.width + ts[0] - 1) / ts[0]) * ((P.height + ts[0] - 1) / ts[0]) <= 64u;
    if (small_ok) {
        RenderSetup A = R;
        A.one_level_64 = true;
        st = pass(A, std::vector<uint32_t>{ts[1]}, std::vector<uint32_t>{1u});
        if (st) return st;
        if (!P.pixel_perfect) {       // (pixel-perfect renders have no fills: pixel.rs:345-368)
            RenderSetup B = R;
            B.one_level_64 = true; B.classify_only = true;
            st = pass(B, std::vector<uint32_t>{ts[0]}, std::vector<uint32_t>{0u});
            if (st) return st;
        }
    } else {
        st = pass(R, ts, tags);
        if (st) return st;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_done, ctx->stream));     // (a later pipelined 3D frame that takes this buffer set waits for it)
    ctx->ev_done_valid = true; ctx->last_end = ctx->ev_done;
    if (!out_is_device) {
        HIP_TRY(ctx, hipMemcpyAsync(out, d_out, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
        return finish_render(ctx);
    }
    return FHIP_OK;
}

// ---- a 3D frame: the stages of a slab, each on the stream it is given; then the frame in the order of its schedule ---------------------
// Head of a slab's tile chain: the slab's counters and table reset, the min-depth pyramid rebuilt from the slabs in front
static void slab_begin(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FhRenderState* dS, int k, hipStream_t st) {
    const FhRender& P = R.S.P;
    const uint32_t pre = R.S.pre_levels, n_groups = R.groups_per_slab, n32 = ((P.width + 31) / 32) * ((P.height + 31) / 32);
    launch(ctx, st, FHIP_K_OTHER, [&] {
        // the usual pyramid (three levels, 4 x 4 each, 8 x 8 leaf tiles) has a kernel of its own
        // (up to 1024 x 1024: at 2048 x 2048 it was measured SLOWER than the generic kernel - 11.2 vs 8.2 ms per frame)
        const bool pyr3 = P.n_levels == 3 && P.tiles[2] == 8 && P.tiles[1] == 32 && P.tiles[0] == 128 && n32 <= 1024;
        const bool rebuild = k != F.slab_first;  // the first slab sees an empty image (pyramid pre-zeroed)
        // (32 / 8 with its one pre-pass level: both pyramid levels rebuilt and the slab reset in one launch as well)
        const bool pyr2 = P.n_levels == 2 && P.tiles[1] == 8 && P.tiles[0] == 32 && pre == 1;
        if (rebuild && pyr2) { FH_KLAUNCH(k_slab_begin2, dim3(n32 + F.reset_blocks), dim3(256), 0, st, dS, n32, F.table_words, (uint32_t)k, n_groups); return; }
        if (rebuild && pyr3 && pre == 2) { FH_KLAUNCH(k_slab_begin3, dim3(n32 + F.reset_blocks), dim3(256), 0, st, dS, n32, F.table_words, (uint32_t)k, n_groups); return; }
        // (workgroups of one wave: they find room beside a leaf kernel that fills the machine - 73 us per launch on the general path with four)
        FH_KLAUNCH(k_reset_slab, dim3(F.reset_blocks * 4), dim3(WAVE), 0, st, dS, F.table_words, (uint32_t)k, n_groups, (pyr3 && rebuild) ? 1u : 0u);
        if (rebuild && pyr3) FH_KLAUNCH(k_minpyramid3, dim3(n32), dim3(256), 0, st, dS);
        else if (rebuild) FH_KLAUNCH(k_minpyramid, dim3(P.roots_x * P.roots_y), dim3(256), 0, st, dS);
    });
}
// The tile chain of slab k (the idx-th slab rendered) on the schedule's tile stream
static fhip_status tile_step(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FrameStreams& fs, FhRenderState* dS, int k, int idx, const FhHead* head) {
    fs.cur = F.tiles;
    if (waits_leaves(F, idx)) HIP_TRY(ctx, hipStreamWaitEvent(fs.on(), ctx->ev_leaves[idx - (int)F.NC], 0));  // context free again
    const FhHead* const mine = head && idx == 0 ? head : nullptr;      // (the frame's first tile chain: no launch for the slab's reset - in its set-up kernel)
    if (!mine) slab_begin(ctx, R, F, dS, k, fs.on());
    for (uint32_t l = R.S.pre_levels; l < R.S.P.n_levels; l++) launch_tiles(ctx, R, F.level[l], dS, (int)l, true, fs, l == R.S.pre_levels ? mine : nullptr);
    if (F.pipe) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles[idx], fs.on()));
    fs.cur = CALLER;
    return FHIP_OK;
}
// The footprint lists of a slab, and its leaves beyond the leaf kernel's register file
static void classify_work(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FhRenderState* dS, hipStream_t st) {
    const uint32_t class_blocks = (R.n_footprints + FH_CLASSIFY_FP - 1) / FH_CLASSIFY_FP;
    // (by_list: nothing to classify - what is left of the launch is rare mode's blocks for the leaves beyond the leaf kernel's file)
    if (F.rare_leaves) {}      // (... and those blocks' work is k_rare_leaves3d's, behind the leaf kernel: normals_work)
    else if (F.by_list && F.rare && R.S.P.max_regs > R.S.leaf_asm_regs)
        launch(ctx, st, FHIP_K_OTHER, [&] { ctx->rare_launches++; FH_KLAUNCH(k_classify3d, dim3(FH_RARE_BLOCKS), dim3(WAVE), 0, st, dS, 1, 0u, rare_file(ctx, dS, F.rare_stride), F.rare_stride); });
    else if (!F.by_list) launch(ctx, st, FHIP_K_OTHER, [&] {
        FH_KLAUNCH(k_classify3d, dim3(class_blocks + (F.rare ? FH_RARE_BLOCKS : 0u)), dim3(R.S.P.slab / 8 > 16 ? 256 : WAVE), 0, st, dS, R.asm_points ? 1 : 0, class_blocks,
                   rare_file(ctx, dS, F.rare_stride), F.rare_stride);
    });
    if (R.S.P.max_regs > R.S.leaf_asm_regs && !F.rare)      // (rare mode: in the blocks behind k_classify3d's)
        launch(ctx, st, FHIP_K_POINTS, [&] {
            const int g = blocks_big(ctx, R, R.lds_points_big, 16);
            if (R.full) FH_KLAUNCH((k_leaves3d<2, 0, 1, true>), dim3(g), dim3(WAVE), R.lds_points_big, st, dS);
            else FH_KLAUNCH((k_leaves3d<2, 0, 1, false>), dim3(g), dim3(WAVE), R.lds_points_big, st, dS);
        });
}
// The leaf kernel of slab context `sk`, by the walk the schedule chose (frame_schedule.hpp leaf_walk: why)
static void leaf_work(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FhRenderState* dS, uint32_t sk, hipStream_t st) {
    launch(ctx, st, FHIP_K_POINTS, [&] {
        // class 0: <= 16 registers, 4 voxels per lane; class 1: <= 32 registers, 2 per lane; class 2: LDS file
        if (F.leaf_walk == FrameSchedule::HIP_LEAVES) {
            const int per_cu = R.full ? 8 : 16;
            if (R.full) { FH_KLAUNCH((k_leaves3d<0, 16, 4, true>), dim3(ctx->n_cu * per_cu), dim3(WAVE), 0, st, dS); FH_KLAUNCH((k_leaves3d<1, 32, 2, true>), dim3(ctx->n_cu * per_cu), dim3(WAVE), 0, st, dS); }
            else { FH_KLAUNCH((k_leaves3d<0, 16, 4, false>), dim3(ctx->n_cu * per_cu), dim3(WAVE), 0, st, dS); FH_KLAUNCH((k_leaves3d<1, 32, 2, false>), dim3(ctx->n_cu * per_cu), dim3(WAVE), 0, st, dS); }
            return;
        }
        // one launch for classes 0 and 1: 128 VGPRs -> 4 waves per SIMD
        // per-frame constants of the leaf kernel (gen_interp.py gen_columns): input slots of the axes, the inputs that change
        // along a pixel column (a z coefficient in the axis' matrix row, or a projective matrix), projective flag
        const int which = R.asm_points_t ? FH_ASM_COLUMNS_T : FH_ASM_COLUMNS;
        const uint32_t layers = R.S.P.slab / 8;
        // (the slab context's leaf table and leaf records, as k_fork_state lays the contexts out: the kernel takes them - with the table's shape - from its
        // kernarg, so that a wave whose part of the table is empty leaves after one dependent load)
        const void* const slab_table = sk == 0 ? (const void*)R.S.leaf_table : (const void*)((const FhLeafRef*)ctx->leaf_table_b.p + (size_t)(sk - 1) * R.S.leaf_cap);
        const void* const slab_leaves = sk == 0 ? (const void*)R.S.leaves : (const void*)((const FhLeaf*)ctx->leaves_b.p + (size_t)(sk - 1) * R.S.leaf_cap);
        KaColumns ka = {dS, 0u, R.col_slots, R.col_depmask, R.col_flags, {0, 0}, slab_table, R.n_footprints, layers};
        if (F.leaf_walk == FrameSchedule::BY_LIST) {      // (flags bit 21: table = the slab context's FhLeaf records, nfpl = their capacity, pad[0] = the launch's waves)
            ka.flags |= (3u << 20) | (6u << 24); ka.pad[0] = F.list_waves; ka.table = slab_leaves; ka.nfpl = R.S.leaf_cap;
            (void)launch_asm(ctx, st, which, F.list_waves, &ka, sizeof(ka));
        } else if (F.leaf_walk == FrameSchedule::BY_COLUMNS) {      // (flags bit 20: a footprint column per wave; bits 24 .. 27: in groups of 2^g layers, grid y = the group)
            ka.flags |= (1u << 20) | (F.g << 24);
            (void)launch_asm(ctx, st, which, (R.n_footprints + 63) / 64 * 64, &ka, sizeof(ka), 0, (layers + (1u << F.g) - 1) >> F.g);
        } else {
            // one workgroup per block of 4 footprints (gen_interp.py FH_BLKL = 2) of one 8-voxel layer, front layers first
            // (pad[0]: floor(2^32 / blocks per layer) - the kernel rotates a layer's blocks by a per-layer offset, which is what balances
            // the launch, and takes the remainder by this reciprocal instead of a subtraction loop)
            const uint32_t n_blocks = (R.n_footprints + 3) / 4;
            ka.pad[0] = n_blocks > 1 ? (uint32_t)(((uint64_t)1 << 32) / n_blocks) : 0u;
            (void)launch_asm(ctx, st, which, n_blocks, &ka, sizeof(ka), 0, layers);
        }
    });
}
// Rare mode of a by-list frame (frame_schedule.hpp rare_leaves): the points of the leaves beyond the leaf kernel's file and the normals of their hits
// in one launch, driven by the slab's leaves - behind the leaf kernel, whether the frame's normals kernels run or not
static void rare_leaves_launch(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FhRenderState* dS, int k, hipStream_t st) {
    const uint32_t z_lo = (uint32_t)k * R.S.P.slab, z_hi = z_lo + R.S.P.slab;
    ctx->rare_launches++;
    FH_KLAUNCH(k_rare_leaves3d, dim3(FH_RARE_BLOCKS), dim3(WAVE), 0, st, dS, z_lo, z_hi, rare_file(ctx, dS, F.rare_stride), F.rare_stride);
}
// The normals of slab k's hits
static void normals_work(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FhRenderState* dS, int k, hipStream_t st) {
    const uint32_t z_lo = (uint32_t)k * R.S.P.slab, z_hi = z_lo + R.S.P.slab;
    launch(ctx, st, FHIP_K_NORMALS, [&] {
        const int gs = blocks_for(ctx, R.lds_normals_small, 8), gb = blocks_big(ctx, R, R.lds_normals_big, 8);
        const int which = R.asm_points_t ? FH_ASM_NORMALS_T : FH_ASM_NORMALS;
        if (F.by_list) {
            // (the leaf that owns a pixel's hit is its column's leaf or nobody: fh_normals takes the slab's leaves one per wave pass and
            // looks at the z-buffer itself; k_hits3d: rare mode's blocks for the footprints the push put on list 2)
            if (F.rare_leaves) rare_leaves_launch(ctx, R, F, dS, k, st);
            else if (F.rare && R.S.P.max_regs > R.S.norm_asm_regs) {
                ctx->rare_launches++;
                FH_KLAUNCH(k_hits3d, dim3(FH_RARE_BLOCKS), dim3(WAVE), 0, st, dS, z_lo, z_hi, R.hit_bucket_cap, 0u, rare_file(ctx, dS, F.rare_stride), F.rare_stride);
            }
            KaNormals kn = {dS, F.list_waves, R.col_slots, z_lo, z_hi, R.hit_bucket_cap, 1u};
            (void)launch_asm(ctx, st, which, kn.n_waves, &kn, sizeof(kn));
        }
        else if (R.asm_normals) {
            // (lists 0 and 1 of k_classify3d hold every footprint whose leaves need <= 32 registers - the assembly interpreter's file:
            // k_hits3d turns them into the list of leaves that own a hit, the normals kernel takes one leaf per wave pass)
            const uint32_t hb = std::min<uint32_t>(R.n_footprints, (uint32_t)ctx->n_cu * 64);
            FH_KLAUNCH(k_hits3d, dim3(hb + (F.rare ? FH_RARE_BLOCKS : 0u)), dim3(WAVE), 0, st, dS, z_lo, z_hi, R.hit_bucket_cap, hb, rare_file(ctx, dS, F.rare_stride), F.rare_stride);
            // (wave w walks bucket w % 64 with a stride of n_waves / 64)
            KaNormals kn = {dS, std::max<uint32_t>((uint32_t)(ctx->n_cu * 8) / FH_HIT_BUCKETS, 1u) * FH_HIT_BUCKETS, R.col_slots, z_lo, z_hi, R.hit_bucket_cap, 0};
            (void)launch_asm(ctx, st, which, kn.n_waves, &kn, sizeof(kn));
        }
        else if (R.full) FH_KLAUNCH((k_normals3d<true, false>), dim3(gs), dim3(WAVE), R.lds_normals_small, st, dS, z_lo, z_hi);
        else FH_KLAUNCH((k_normals3d<false, false>), dim3(gs), dim3(WAVE), R.lds_normals_small, st, dS, z_lo, z_hi);
        if (R.S.P.max_regs > R.S.norm_asm_regs && !(F.rare && R.asm_normals)) {      // (rare mode: in the blocks behind k_hits3d's)
            if (R.full) FH_KLAUNCH((k_normals3d<true, true>), dim3(gb), dim3(WAVE), R.lds_normals_big, st, dS, z_lo, z_hi);
            else FH_KLAUNCH((k_normals3d<false, true>), dim3(gb), dim3(WAVE), R.lds_normals_big, st, dS, z_lo, z_hi);
        }
    });
}
// The coarse levels of every slab in one go, then what follows them - the flags of the parked parents, the frame mark, the fork of the slab
// contexts - and the edges to the streams the slabs run on; leaves fs on the caller's stream
// What follows the root push of a frame of ONE coarse level whose leaf stage goes by the list - the flags of the parked parents, the frame
// mark, the fork of the slab contexts - and the first slab's reset (no table to clear in such a frame) were two launches at the head of the
// tile chain: both are the work of the chain's first kernel now, the set-up of level 1 (kernels.hip FhHead).  A frame of two coarse levels
// keeps its launches: its frames are bound by level 1 and the leaf kernels, not by the host's launch count, and level 1's own flags launch stays either way.
// What makes the head see the push's final counts: the tile chain's stream waits for the root level's - ev_l0 (hop to `fork_on`) where the
// chain runs on the stream the fork went to, ev_fork (fork_to_side) where it does not; on one stream, the order of the launches.
static FhHead tile_head(const fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F) {
    FhHead h{};
    FhFork& fork = h.fork;
    fork.n = F.NC; fork.mark = F.coarse ? 1u : 0u;
    fork.leaves = (FhLeaf*)ctx->leaves_b.p; fork.leaf_table = (FhLeafRef*)ctx->leaf_table_b.p; fork.fp_lists = (uint32_t*)ctx->fp_lists_b.p;
    fork.leaf_cap = (size_t)R.S.leaf_cap; fork.n_footprints = (size_t)R.n_footprints; fork.hit_words = R.hit_words;
    h.on = F.coarse && R.zrep && R.S.pre_levels == 1 && F.by_list && F.n_rendered > 0 && F.level[1].path != LevelPlan::MONO ? 1u : 0u;
    h.slab = (uint32_t)F.slab_first; h.n_root_groups = R.groups_per_slab; h.depmask = R.col_depmask;
    return h;
}
// (`slot`: the staging slot's guard, recorded where the host leaves the root stream for the first time - beside that hop's own record, behind
// the root level; a frame that stays on its root stream keeps it armed for render3d_frame)
static fhip_status coarse_levels(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FrameStreams& fs, FhRenderState* dS, const FhHead& head, StagingGuard& slot) {
    const uint32_t pre = R.S.pre_levels;
    const FhFork& fork = head.fork;
    const bool forked_here = F.coarse && R.zrep;      // (by the flags launch below, or by the head of the tile chain)
    auto leave = [&](Role to, hipEvent_t ev) { if (to != fs.cur) slot.record(); return hop(fs, to, ev); };
    if (F.coarse) {
        launch_tiles(ctx, R, F.level[0], dS, 0, true, fs);
        if (pre > 1) {
            HIP_TRY(ctx, leave(F.l1_flags, ctx->ev_l0));
            if (R.zrep) launch(ctx, fs.on(), FHIP_K_OTHER, [&] { FH_KLAUNCH(k_tape_flags, dim3(ctx->n_cu * 4), dim3(WAVE), 0, fs.on(), dS, 1, R.col_depmask, 0, FhFork{}); });
            HIP_TRY(ctx, leave(F.l1, ctx->ev_l0));
            launch_tiles(ctx, R, F.level[1], dS, 1, true, fs);
        }
        HIP_TRY(ctx, leave(F.fork_on, pre > 1 ? ctx->ev_l1 : ctx->ev_l0));      // (level 1 did not go through fh_tiles_v64; or one coarse level whose tail goes to the side stream)
        // (the fork of a pipelined frame's slab contexts - or, with ONE context, the frame mark alone - in the same launch)
        if (R.zrep && !head.on) launch(ctx, fs.on(), FHIP_K_OTHER, [&] { FH_KLAUNCH(k_tape_flags, dim3(ctx->n_cu * 8 + 1), dim3(WAVE), 0, fs.on(), dS, (int)pre, R.col_depmask, 1, fork); });
        if (!F.pipe && !forked_here) launch(ctx, fs.on(), FHIP_K_OTHER, [&] { FH_KLAUNCH(k_mark_frame, dim3(1), dim3(1), 0, fs.on(), dS); });
    }
    if (F.pipe) {
        if (!forked_here) FH_KLAUNCH(k_fork_state, dim3(1), dim3(1), 0, fs.on(), dS, fork);
        if (F.rec_fork) HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, fs.on()));
        if (F.fork_to_side) HIP_TRY(ctx, hipStreamWaitEvent(fs.s[SIDE], ctx->ev_fork, 0));
    }
    if (F.ev_pre) HIP_TRY(ctx, leave(CALLER, ctx->ev_pre));     // (from the stream the last coarse-level kernel went to)
    fs.cur = CALLER;
    if (F.fork_to_tail) HIP_TRY(ctx, hipStreamWaitEvent(fs.s[TAIL], ctx->ev_fork, 0));
    return FHIP_OK;
}
// The slabs, front to back (voxel.rs:252-261): tile chain, footprint lists, leaf kernel, normals - each on its role's stream, slab
// contexts in turn
static fhip_status render_slabs(fhip_ctx* ctx, const RenderSetup& R, const FrameSchedule& F, FrameStreams& fs, FhRenderState* dS0, const FhHead& head) {
    const FhHead* const hd = head.on ? &head : nullptr;
    auto slab_state = [&](int idx) { return dS0 + (F.pipe ? (uint32_t)idx % F.NC : 0u); };
    for (int idx = 0; F.tiles_first && idx < F.n_rendered; idx++) { const fhip_status st = tile_step(ctx, R, F, fs, slab_state(idx), F.slab_first - idx, idx, hd); if (st) return st; }
    for (int idx = 0; idx < F.n_rendered; idx++) {
        if (ctx->is_cancelled()) {
            if (hd && idx == 0 && !F.tiles_first) ctx->forked = 0;      // (the fork rides on the first tile chain, which is not queued now: nobody reads the other slab contexts' states)
            return fail(ctx, FHIP_ERR_CANCELLED, "cancelled");
        }
        const int k = F.slab_first - idx;
        FhRenderState* const dS = slab_state(idx);
        if (!F.tiles_first) { const fhip_status st = tile_step(ctx, R, F, fs, dS, k, idx, hd); if (st) return st; }
        if (F.pipe) HIP_TRY(ctx, hipStreamWaitEvent(fs.s[F.leaf], ctx->ev_tiles[idx], 0));
        if (F.aux_edge) HIP_TRY(ctx, hipStreamWaitEvent(fs.s[F.lists], ctx->ev_tiles[idx], 0));
        classify_work(ctx, R, F, dS, fs.s[F.lists]);
        leaf_work(ctx, R, F, dS, (uint32_t)(dS - dS0), fs.s[F.leaf]);
        if (F.aux_edge) { HIP_TRY(ctx, hipEventRecord(ctx->ev_aux[idx], fs.s[F.leaf])); HIP_TRY(ctx, hipStreamWaitEvent(fs.s[F.normals], ctx->ev_aux[idx], 0)); }     // the slab's leaf kernel is through
        if (F.normals_on) normals_work(ctx, R, F, dS, k, fs.s[F.normals]);
        else if (F.rare_leaves) launch(ctx, fs.s[F.normals], FHIP_K_NORMALS, [&] { rare_leaves_launch(ctx, R, F, dS, k, fs.s[F.normals]); });      // (a frame without normals: the large leaves' points all the same)
        if (records_leaves(F, idx)) HIP_TRY(ctx, hipEventRecord(ctx->ev_leaves[idx], fs.s[F.normals]));       // slab context free again for slab idx + NC; the last one of an aux_edge frame: image complete
    }
    // (the tail stream is serial: the last slab's normals)
    if (F.aux_edge && F.n_rendered > 0) HIP_TRY(ctx, hipStreamWaitEvent(fs.s[CALLER], ctx->ev_leaves[F.n_rendered - 1], 0));
    return FHIP_OK;
}

// "Is the frame before this one still under way?" - what decides lanes or stage pipeline (lanes_possible) and, under the stage pipeline,
// whether the frame is alone (frame_schedule.hpp `lone`).  Asked of the event that frame recorded at its end on the caller's stream
// (fhip_ctx::last_end), at most once per frame: new_frame() at every entry point forgets the last answer.
static void new_frame(fhip_ctx* ctx) { ctx->before_asked = false; }
static bool frame_before_under_way(fhip_ctx* ctx) {
    if (!ctx->before_asked) {
        ctx->before_asked = true;
        ctx->before_busy = ctx->last_end && hipEventQuery(ctx->last_end) == hipErrorNotReady;
        (void)hipGetLastError();
    }
    return ctx->before_busy;
}
static fhip_status render3d_frame(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                                  int out_is_device, const PartSpec& part) {
    if (ctx->is_cancelled()) return fail(ctx, FHIP_ERR_CANCELLED, "cancelled");
    if (ctx->opt.stats & 2) g_spans.start();
    (void)hipSetDevice(ctx->device);
    // bind and camera
    RenderSetup R;
    memset(&R.S, 0, sizeof(R.S));
    FhRender& P = R.S.P;
    P.width = cfg->width; P.height = cfg->height; P.depth = cfg->depth; P.z = 0; P.pixel_perfect = 0;
    fhip_status st = bind_inputs(ctx, tape, cfg->axis_slots, cfg->var_keys, cfg->var_values, cfg->n_vars, P);
    if (st) return st;
    const uint32_t size[3] = {cfg->width, cfg->height, cfg->depth};
    float s2w[16];
    const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    fhip_screen_to_world(size, 3, s2w);
    mat_product(cfg->world_to_model ? cfg->world_to_model : ident, s2w, 4, P.mat);  // voxel.rs:107-109
    const TapeFacts facts = tape_facts(tape);
    const PlanInputs pin = plan_inputs(ctx);
    column_facts(P, facts, pin, R);
    // choose the tiles
    const TileChoice tiles = choose_tiles_3d(cfg->tile_sizes, cfg->n_tile_sizes, size, part.n_shards * part.nx * part.ny, part.nz, R.column_inv, pin.root32_max, pin.no_zrep,
                                             linked_root_tape(facts, pin));
    if (!tiles.valid) return fail(ctx, FHIP_ERR_UNSUPPORTED, "bad tile size list");
    if (tiles.substituted) ctx->substituted_tiles++;
    // pick the buffer set: a pipelined frame takes the set used longest ago
    ScheduleInputs in = schedule_inputs(ctx, out_is_device);
    // (a tape whose register files live in HBM takes the slow path: one region per workgroup, shared by the launches of a frame, so
    // nothing of the frame runs beside anything else)
    in.huge = (size_t)std::max<uint32_t>(tape->t.n_regs, 1) * WAVE * 16 > FH_LDS_MAX || tiles_lds(std::max<uint32_t>(tape->t.n_regs, 1), tape->t.n_choices, 64) > FH_LDS_MAX;
    in.whole = part.n_shards == 1 && part.nx * part.ny * part.nz == 1;
    if (frame_pipelined(in)) {
        // (rotate: the current set goes to the back of the ring, the set used longest ago comes forward)
        for (uint32_t i = 0; i < ctx->extra_sets; i++) std::swap(static_cast<FrameBufs&>(*ctx), ctx->others[i]);
        // the frame before this one is still under way (the caller queues frames back to back)
        in.frames_queued = ctx->extra_sets > 0 && frame_before_under_way(ctx);
    }
    // (clean buffer sets, frame_plan.hpp: what the set's last frame left it clean for - taken off the set before anything of this frame can
    // touch its buffers, prepare()'s growing them included: whatever ends this frame early leaves no record)
    const CleanSig left_clean = ctx->clean;
    ctx->clean = CleanSig();
    FH_SPAN(0);
    st = prepare(ctx, tape, facts, true, tiles.ts, part, R);
    if (st) return st;
    FH_SPAN(1);
    // schedule: every decision about streams, launches and slabs of this frame (frame_schedule.hpp)
    in.pre_turn = ctx->pre_turn;
    if (ctx->host_flags) { in.rare_seen = ctx->host_flags[2]; in.last_leaves = ctx->host_flags[3]; }
    const FrameSchedule F = schedule_frame(R, in);
    if (F.takes_turn) ctx->pre_turn++;
    if (F.rare) { HIP_TRY(ctx, ctx->rare_scratch.ensure((size_t)F.rare_stride * FH_RARE_BLOCKS * 4)); ctx->rare_frames++; }      // (a set's state buffer holds four slab contexts)
    R.S.leaf_list = F.by_list ? 1u : 0u; ctx->forked = F.pipe ? F.NC : 0;      // (what the device and the set are told of it)
    FrameStreams fs = frame_streams(ctx, F.root);
    if (F.fpipe && ctx->ev_done_valid) HIP_TRY(ctx, hipStreamWaitEvent(fs.on(), ctx->ev_done, 0));   // the set's previous frame has left it
    // upload
    const size_t npix = (size_t)cfg->width * cfg->height;
    FhGeometryPixel* d_out = (FhGeometryPixel*)out;
    if (!out_is_device) { HIP_TRY(ctx, ctx->tmp_out.ensure(npix * sizeof(FhGeometryPixel))); d_out = (FhGeometryPixel*)ctx->tmp_out.p; }
    FhRenderState* const dS0 = (FhRenderState*)ctx->state.p;
    const CleanFrame kind = {out_is_device != 0, ctx->profiling};
    CleanSig want_clean;
    want_clean.valid = true; want_clean.pixels = npix; want_clean.mind_words = R.mind_words;
    const bool is_clean = set_is_clean(left_clean, want_clean);      // (then the clears are skipped)
    const FrameClear clear3[3] = {{ctx->zbuf.p, npix * 8, 0u}, {ctx->normals.p, npix * 12, 0u}, {ctx->mind.p, R.mind_words * 4, 0u}}, no_clear[3] = {};
    // (the staging slot's guard: recorded by coarse_levels where the root stream is left, or below beside ev_done - or by whatever returns before that)
    StagingGuard slot(RecordSlot{});
    st = upload_frame(ctx, fs.on(), tape, R, is_clean ? no_clear : clear3, &slot);
    if (st) return st;
    FH_SPAN(2);
    const FhHead head = tile_head(ctx, R, F);
    st = coarse_levels(ctx, R, F, fs, dS0, head, slot);
    if (st) return st;
    FH_SPAN(3);
    st = render_slabs(ctx, R, F, fs, dS0, head);
    if (st) return st;
    FH_SPAN(4);
    // finish: the image, the overflow latches and the pinned host words, on the caller's stream
    launch(ctx, ctx->stream, FHIP_K_OTHER, [&] { FH_KLAUNCH(k_finish3d, dim3(ctx->n_cu * 16), dim3(WAVE), 0, ctx->stream, dS0, d_out, std::max<uint32_t>(ctx->forked, 1u), (uint32_t*)ctx->sticky.p, ctx->host_flags,
                                                            leaves_set_clean(kind) ? 1u : 0u, (uint32_t)R.mind_words); });
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->launch_failed) { ctx->launch_failed = false; return FHIP_ERR_HIP; }   // (message in fhip_last_error)
    ctx->async_pending = out_is_device != 0;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_done, ctx->stream));     // (a later pipelined frame that takes this set waits for it; the next frame asks it whether this one is under way)
    ctx->ev_done_valid = true; ctx->last_end = ctx->ev_done;
    slot.record();      // (a frame that never left its root stream - the caller's: the slot's guard at the end of its chain)
    ctx->clean = set_left_by(kind, want_clean, true);
    if (ctx->opt.stats & 2) { g_spans.mark(5); g_spans.frame(); }
    if (!out_is_device) {
        HIP_TRY(ctx, hipMemcpyAsync(out, d_out, npix * sizeof(FhGeometryPixel), hipMemcpyDeviceToHost, ctx->stream));
        return finish_render(ctx);
    }
    return FHIP_OK;
}
// Frame lanes (option frame_lanes, default 4; 0 / 1: off).  The stage pipeline above runs the stages of consecutive frames beside
// each other, each stage on its stream; how far that goes is set by the busiest stream.  The other arrangement for frames that the
// caller queues back to back (the frame before is still under way): WHOLE frames beside each other - lane i % K is a child context
// that keeps to one stream (no_pipeline) and renders into an image of its own; the caller's stream waits for it and copies the image
// out, so `out` is only ever touched on the caller's stream, in order.  First measured with separate contexts driven in turn
// (tools/two_contexts.py under FHIP_NO_PIPELINE=1, profiles/r04r): bear.vm 512^3 - fh_columns_t with its 256 VGPRs, two waves per SIMD,
// 3.2 ms of kernels in a frame of 1.86 ms - 1.38 ms with three contexts; which arrangement a 3D frame takes is decided by lane_mode
// below.  A frame alone, a host output buffer or a profiled frame take the stage pipeline as before.  Parts of a frame (shards, blocks: what a rank of a
// multi-GPU job renders) are frames like any other here (option lanes_parts): one octant of prospero.vm 1024^3, queued, 0.72 -> 0.31 ms; a
// column shard of eight stays where it is, 0.43 (profiles/r04r/lanes_parts.txt).
static bool lanes_possible(fhip_ctx* ctx, int out_is_device) {
    if (ctx->opt.frame_lanes < 2 || ctx->is_lane || !out_is_device || ctx->profiling || ctx->probe || (ctx->opt.stats & 1)) return false;
    return frame_before_under_way(ctx);
}
static void lane_tune_release(fhip_ctx* ctx);
static void lanes_release(fhip_ctx* ctx, bool keep_measurements) {
    if (!keep_measurements) lane_tune_release(ctx);       // (what was measured was measured under the options of the moment)
    for (fhip_ctx* L : ctx->lanes) if (ctx->last_end == L->lane_copied) ctx->last_end = nullptr;      // (the event goes with its lane)
    for (fhip_ctx* L : ctx->lanes) {
        hipStream_t const s = L->lane_stream_owned ? L->stream : nullptr;
        if (L->lane_done) (void)hipEventDestroy(L->lane_done);
        if (L->lane_copied) (void)hipEventDestroy(L->lane_copied);
        L->lane_img.release();
        fhip_ctx_destroy(L);
        if (s) (void)hipStreamDestroy(s);
    }
    ctx->lanes.clear();
}
// One frame on the next lane: render(lane, image) queues it on the lane's stream into the lane's own image of `bytes` bytes
static fhip_status run_on_lane_(fhip_ctx* ctx, uint32_t max_lanes, size_t bytes, void* out, const std::function<fhip_status(fhip_ctx*, void*)>& render) {
    const uint32_t K = std::min((uint32_t)std::min(ctx->opt.frame_lanes, 8), max_lanes);
    if (ctx->opt.lanes_fail) return fail(ctx, FHIP_ERR_HIP, "frame lanes: failure provoked (option lanes_fail)");
    while (ctx->lanes.size() < K) {
        // (the first three lanes ride on the streams of the stage pipeline, which is idle while the lanes run: the runtime shares a few
        // hardware queues - four by default - among all streams that have work, and lanes on streams of their own ended up two to a
        // queue behind the idle ones: bear.vm 512^3 1.55 ms per frame instead of 1.4)
        hipStream_t const mine[3] = {ctx->stream_pre, ctx->stream3, ctx->stream2};
        const size_t k = ctx->lanes.size();
        hipStream_t s = k < 3 ? mine[k] : nullptr;
        const bool owned = !s;
        if (owned) HIP_TRY(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        fhip_ctx* L = nullptr;
        const fhip_status st = fhip_ctx_create(ctx->device, (void*)s, &L);
        if (st) { if (owned) (void)hipStreamDestroy(s); return fail(ctx, st, "frame lanes: no child context"); }
        L->lane_stream_owned = owned;
        L->opt = ctx->opt;
        L->opt.no_pipeline = 1;
        L->opt.frame_lanes = 0;
        apply_options(L);
        L->is_lane = true;
        (void)hipEventCreateWithFlags(&L->lane_done, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&L->lane_copied, hipEventDisableTiming);
        ctx->lanes.push_back(L);
    }
    fhip_ctx* const L = ctx->lanes[ctx->lane_next++ % K];
    L->cancel_src = &ctx->cancelled;
    L->watch.store(ctx->watch.load(std::memory_order_relaxed), std::memory_order_relaxed);
    HIP_TRY(ctx, L->lane_img.ensure(bytes));
    if (L->lane_copied_valid) HIP_TRY(ctx, hipStreamWaitEvent(L->stream, L->lane_copied, 0));   // (its previous image has been copied out)
    const fhip_status st = render(L, L->lane_img.p);
    if (st) { ctx->err = L->err; return st; }
    HIP_TRY(ctx, hipEventRecord(L->lane_done, L->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, L->lane_done, 0));
    HIP_TRY(ctx, hipMemcpyAsync(out, L->lane_img.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(L->lane_copied, ctx->stream));
    L->lane_copied_valid = true; ctx->last_end = L->lane_copied;      // (the end of this frame on the caller's stream)
    ctx->lane_frames++;
    if (ctx->tune_cur < 0) ctx->lane_frames_wanted++;      // (not a frame of a measuring window: somebody's arrangement of choice)
    return FHIP_OK;
}
// (FHIP_LANE_FALLBACK: the lanes' own resources could not be had - device memory for a child context's buffers, say: the caller renders the
// frame under the stage pipeline instead, and the context gives its lanes up for good; option lanes_fail provokes it, for the test)
static const fhip_status FHIP_LANE_FALLBACK = (fhip_status)1000;
static fhip_status run_on_lane(fhip_ctx* ctx, uint32_t max_lanes, size_t bytes, void* out, const std::function<fhip_status(fhip_ctx*, void*)>& render) {
    ctx->last_hip_error = 0;
    for (fhip_ctx* L : ctx->lanes) if (L) L->last_hip_error = 0;
    const fhip_status st = run_on_lane_(ctx, max_lanes, bytes, out, render);
    if (st != FHIP_ERR_HIP) return st;
    // Only what says "the lanes' resources cannot be had" sends the frame back to the stage pipeline: out of memory (a child context's
    // buffers, its image), a child context or stream that could not be made, the provoked failure of the test.  Any other HIP error - a
    // fault inside the lane's render - is the caller's to see, with the lane's message.
    bool resources = ctx->opt.lanes_fail != 0 || ctx->last_hip_error == (int)hipErrorOutOfMemory || ctx->err.rfind("frame lanes:", 0) == 0;
    for (fhip_ctx* L : ctx->lanes) if (L && L->last_hip_error == (int)hipErrorOutOfMemory) resources = true;
    if (!resources) return st;
    if (ctx->mesh_leaves.cap) {       // (a mesh build's leaf records - gigabytes kept for the next build - may be what the lanes had no room beside)
        (void)hipDeviceSynchronize();
        ctx->mesh_leaves.release();
    }
    fprintf(stderr, "fidget-hip: frame lanes given up for this context (%s); frames keep to the stage pipeline\n", ctx->err.c_str());
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);      // (nothing of the lanes may be pending on the caller's stream when they go)
    ctx->opt.frame_lanes = 0;
    lanes_release(ctx);
    ctx->err.clear();
    return FHIP_LANE_FALLBACK;
}
// Stage pipeline or lanes?  Measured with three lanes on the stage pipeline's streams (ms per queued frame, profiles/r04r/lanes_all.txt):
// prospero.vm 1024^3 0.505 / 0.570 (0.540 with four), with the column short cuts off 1.625 / 1.73 - but 512^3 1.66 / 1.15, 2048^3 2.18 / 1.99,
// colonnade.vm 1024^3 0.605 / 0.454, 512^3 0.334 / 0.248, bear.vm 512^3 1.84 / 1.37.  The stage pipeline wins where a frame's stages happen to be
// of equal length, which is a property of the model AND the size; nothing the host knows before the frame predicts it.  So it is measured:
// consecutive queued frames of one kind (tape, image size) run TUNE_SKIP + TUNE_WIN frames under the stage pipeline, as many on the lanes and as many
// under the stage pipeline again (a burst of frames starts on a machine whose clocks are still coming up, which counted against whatever
// was measured first: the general path's stage pipeline read 2.0 ms in the first window and runs at 1.63), each window timed between two
// events on the caller's stream after TUNE_SKIP frames of settling; the lanes are kept if they beat the better of the two stage windows
// by 3 %, for the life of the context (or until an option changes).  Frames that break the sequence - another kind, a frame alone - restart the
// window, so a queue of mixed frames never decides and keeps the prior: lanes for tapes with transcendental opcodes, the stage pipeline
// otherwise.  Both arrangements give the same image, bit for bit (tests/test_gpu_parity.py).
static constexpr uint32_t TUNE_SKIP = 4, TUNE_WIN = 8;       // (round 6: 40 frames to a verdict instead of 48)
// The lanes' window is followed by more frames on the lanes: K lanes finish their frames K at a time (heavy frames: every 5.5 ms four
// images of the general path of prospero.vm 1024^3), and a window whose last frame is the last frame ON the lanes ends with a group of one -
// a lone frame that takes half the time: such a window read 1.07 ms per frame where the lanes run at 1.38 and the stage pipeline at 1.34
// (profiles/r06b/experiments.txt 8).  With frames queued behind it the window's last group is a whole one.
// (with K lanes - option frame_lanes, 4 - the lanes' window is K frames of settling, 2 K frames timed, K frames behind them)
static uint32_t tune_lanes(const fhip_ctx* ctx) { return (uint32_t)std::min(std::max(ctx->opt.frame_lanes, 2), 8); }
static void lane_tune_release(fhip_ctx* ctx) {
    for (auto& t : ctx->lane_tune)
        for (hipEvent_t& e : t.ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    ctx->lane_tune.clear();
    ctx->tune_last_key = 0;
    ctx->tune_cur = -1;
}
static bool lane_mode(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, int out_is_device, const PartSpec& part) {
    ctx->tune_cur = -1;
    const bool whole = part.n_shards == 1 && part.nx * part.ny * part.nz == 1;
    const bool possible = lanes_possible(ctx, out_is_device) && ctx->use_pipeline && ctx->frame_pipeline;
    const bool prior = ctx->use_asm && !ctx->opt.no_columns_t && !tape_asm_ok(tape->t);
    if (!possible) { ctx->tune_last_key = 0; return false; }       // (a frame alone, a profiled frame, ...: the stage pipeline; the sequence is broken)
    uint64_t key = (tape->parent_serial ? tape->parent_serial : tape->serial) * 0x9E3779B97F4A7C15ull;   // (a bound tape: its parent's entry)
    key ^= ((uint64_t)cfg->width << 42) ^ ((uint64_t)cfg->height << 21) ^ (uint64_t)cfg->depth;
    key ^= (((uint64_t)part.shard * 64 + part.n_shards) * 0xD6E8FEB86659FD93ull) ^ ((((uint64_t)part.ix * 16 + part.iy) * 16 + part.iz) * 4096 + (part.nx * 16 + part.ny) * 16 + part.nz) * 0xA24BAED4963EE407ull;
    key |= 1;
    int at = -1;
    for (size_t i = 0; i < ctx->lane_tune.size(); i++) if (ctx->lane_tune[i].key == key) at = (int)i;
    if (at < 0) {
        if (ctx->lane_tune.size() < 32) { ctx->lane_tune.emplace_back(); at = (int)ctx->lane_tune.size() - 1; }
        else {      // the entry used longest ago makes room
            at = 0;
            for (size_t i = 1; i < ctx->lane_tune.size(); i++) if (ctx->lane_tune[i].used < ctx->lane_tune[at].used) at = (int)i;
            for (hipEvent_t& e : ctx->lane_tune[at].ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
            ctx->lane_tune[at] = fhip_ctx::LaneTune();
        }
        ctx->lane_tune[at].key = key;
    }
    fhip_ctx::LaneTune& T = ctx->lane_tune[at];
    T.used = ++ctx->tune_clock;
    if (T.phase == 4) { ctx->tune_last_key = key; return T.lanes; }
    if (ctx->tune_last_key != key) {       // the first frame of a run of this kind: the window starts again behind it, and it goes where the prior says
        ctx->tune_last_key = key;
        if (T.phase < 3) { T.n = 0; return prior; }
    }
    if (T.phase == 3) {
        const hipError_t q = hipEventQuery(T.ev[5]);
        (void)hipGetLastError();
        if (q != hipSuccess) return false;        // (under the stage pipeline until the last window's last event has passed)
        bool ok = true;
        for (int w = 0; w < 3; w++) {
            float t = 0.0f;
            ok = ok && hipEventElapsedTime(&t, T.ev[2 * w], T.ev[2 * w + 1]) == hipSuccess && t > 0.0f;
            T.ms[w] = t / (w == 1 ? 2 * tune_lanes(ctx) : TUNE_WIN);
        }
        (void)hipGetLastError();
        T.lanes = ok ? T.ms[1] < 0.97f * std::min(T.ms[0], T.ms[2]) : prior;
        T.phase = 4;
        // Memory by need: the child contexts exist since the measuring windows (a buffer set each, 0.5 GB).  When the verdict is the stage
        // pipeline, nothing else has ever used them and no other kind of frame is being measured, they go back - all windows' frames are
        // through (the last window's last event has passed, above), their images copied out before it.  A later frame that wants lanes
        // (a 2D queue, another kind's verdict) makes them again.
        if (!T.lanes && ctx->lane_frames_wanted == 0) {
            bool others = false;
            for (const fhip_ctx::LaneTune& o : ctx->lane_tune) others = others || (&o != &T && (o.phase != 4 || o.lanes));
            if (!others) lanes_release(ctx, true);
        }
        return T.lanes;
    }
    ctx->tune_cur = at;
    return T.phase == 1;
}
// (a queued frame's end: the marks of the tuner's windows.  What the next frame's lanes_possible asks is `last_end`, which the frame set itself.)
static fhip_status frame_queued(fhip_ctx* ctx, int out_is_device) {
    if (!out_is_device || ctx->is_lane || ctx->opt.frame_lanes < 2) return FHIP_OK;
    if (ctx->tune_cur >= 0) {       // a frame of a measuring window: its marks
        fhip_ctx::LaneTune& T = ctx->lane_tune[(size_t)ctx->tune_cur];
        ctx->tune_cur = -1;
        T.n++;
        const uint32_t K = tune_lanes(ctx);
        const uint32_t skip = T.phase == 1 ? K : TUNE_SKIP, win = T.phase == 1 ? 2 * K : TUNE_WIN, tail = T.phase == 1 ? K : 0u;
        if (T.n == skip || T.n == skip + win) {
            hipEvent_t& e = T.ev[2 * T.phase + (T.n == skip ? 0 : 1)];
            if (!e) HIP_TRY(ctx, hipEventCreate(&e));
            HIP_TRY(ctx, hipEventRecord(e, ctx->stream));
        }
        if (T.n == skip + win + tail) { T.phase++; T.n = 0; }
    }
    return FHIP_OK;
}
static fhip_status render3d_part(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                                 int out_is_device, const PartSpec& part) {
    (void)hipSetDevice(ctx->device);
    std::shared_ptr<const fhip_tape> bound;     // (more input slots than a render binds: its bound tape, capi_bound.hpp)
    fhip_render3d_config bcfg;
    if (tape->t.n_vars > FH_MAX_INPUTS) {
        const fhip_status bs = bound_tape(ctx, tape, cfg->axis_slots, cfg->var_keys, cfg->var_values, cfg->n_vars, bound);
        if (bs) return bs;
        tape = bound.get();
        bcfg = *cfg; bcfg.axis_slots = BOUND_AXES; bcfg.var_keys = nullptr; bcfg.var_values = nullptr; bcfg.n_vars = 0;
        cfg = &bcfg;
    }
    new_frame(ctx);
    fhip_status st = lane_mode(ctx, tape, cfg, out_is_device, part)
        ? run_on_lane(ctx, 8, (size_t)cfg->width * cfg->height * sizeof(FhGeometryPixel), out,
                      [&](fhip_ctx* L, void* img) { return render3d_frame(L, tape, cfg, img, 1, part); })
        : render3d_frame(ctx, tape, cfg, out, out_is_device, part);
    if (st == FHIP_LANE_FALLBACK) st = render3d_frame(ctx, tape, cfg, out, out_is_device, part);
    if (st) ctx->tune_cur = -1;
    return st ? st : frame_queued(ctx, out_is_device);
}
// (Four lanes by default, the fourth on a stream of its own: against three, prospero.vm 512^3 1.14 -> 0.91 ms per frame, colonnade.vm 1024^3 /
// 512^3 0.441 / 0.252 -> 0.413 / 0.212, bear.vm the same, gyroid-sphere 1024^3 1.14 -> 1.18; 2D frames keep to the three on the stage
// pipeline's streams: 4096^2 0.266 with three, 0.306 with four - profiles/r04r/lanes_3_or_4.txt.)
// 2D frames have no stage pipeline at all - a frame is one chain of tile levels and a pixel kernel on the caller's stream - so every
// queued 2D frame with a device output takes a lane: prospero.vm 4096^2 0.475 -> 0.333 ms per frame, 1024^2 0.83 -> 0.50 with three
// one-stream contexts in turn (profiles/r04r/frame_major3.txt)
fhip_status fhip_render2d(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render2d_config* cfg, float* out, int out_is_device) {
    (void)hipSetDevice(ctx->device);
    std::shared_ptr<const fhip_tape> bound;     // (as render3d_part)
    fhip_render2d_config bcfg;
    if (tape->t.n_vars > FH_MAX_INPUTS) {
        const fhip_status bs = bound_tape(ctx, tape, cfg->axis_slots, cfg->var_keys, cfg->var_values, cfg->n_vars, bound);
        if (bs) return bs;
        tape = bound.get();
        bcfg = *cfg; bcfg.axis_slots = BOUND_AXES; bcfg.var_keys = nullptr; bcfg.var_values = nullptr; bcfg.n_vars = 0;
        cfg = &bcfg;
    }
    new_frame(ctx);
    ctx->tune_cur = -1;
    ctx->tune_last_key = 0;       // (a 2D frame between two 3D frames of one kind: their window starts again)
    fhip_status st = lanes_possible(ctx, out_is_device)
        ? run_on_lane(ctx, 3, (size_t)cfg->width * cfg->height * 4, out, [&](fhip_ctx* L, void* img) { return render2d_frame(L, tape, cfg, (float*)img, 1); })
        : render2d_frame(ctx, tape, cfg, out, out_is_device);
    if (st == FHIP_LANE_FALLBACK) st = render2d_frame(ctx, tape, cfg, out, out_is_device);
    return st ? st : frame_queued(ctx, out_is_device);
}
fhip_status fhip_render3d(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                          int out_is_device) {
    return render3d_part(ctx, tape, cfg, out, out_is_device, PartSpec{});
}
fhip_status fhip_render3d_shard(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                                int out_is_device, uint32_t shard, uint32_t n_shards) {
    if (n_shards == 0 || shard >= n_shards) return fail(ctx, FHIP_ERR_UNSUPPORTED, "bad shard");
    PartSpec p;
    p.shard = shard; p.n_shards = n_shards;
    return render3d_part(ctx, tape, cfg, out, out_is_device, p);
}
// Octant-style shards: block `index` = ix + nx * (iy + ny * iz) of an nx x ny x nz split of the volume (root-tile
// columns in x and y, z-slabs in z; iz = nz - 1 is the front).  Pixels outside the block's columns stay {0,0,0,0}.
fhip_status fhip_render3d_block(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render3d_config* cfg, void* out,
                                int out_is_device, uint32_t index, const uint32_t split[3]) {
    if (!split || !split[0] || !split[1] || !split[2] || index >= split[0] * split[1] * split[2]) return fail(ctx, FHIP_ERR_UNSUPPORTED, "bad block");
    PartSpec p;
    p.nx = split[0]; p.ny = split[1]; p.nz = split[2];
    p.ix = index % p.nx; p.iy = (index / p.nx) % p.ny; p.iz = index / (p.nx * p.ny);
    return render3d_part(ctx, tape, cfg, out, out_is_device, p);
}
// Merge of two partial images of the same pixels from different z ranges (the stitch rule of voxel.rs:527-550 applied
// across shards): the larger depth wins, a tie goes to `front` (the range nearer the camera: a hit there carries the
// normal, the other side's equal depth is a filled tile's z + T + 1 with no normal); then the clamp depth >= D - 1 ->
// (D, [0, 0, 1]).  In place on `front`; device pointers; n pixels.
fhip_status fhip_merge_depth(fhip_ctx* ctx, void* front, const void* back, uint64_t n_pixels, uint32_t image_depth) {
    if (!n_pixels) return FHIP_OK;
    (void)hipSetDevice(ctx->device);
    FH_KLAUNCH(k_merge_depth, dim3((unsigned)std::min<uint64_t>((n_pixels + 255) / 256, 65535)), dim3(256), 0, ctx->stream,
                       (FhGeometryPixel*)front, (const FhGeometryPixel*)back, (size_t)n_pixels, image_depth);
    HIP_TRY(ctx, hipGetLastError());
    return FHIP_OK;
}
