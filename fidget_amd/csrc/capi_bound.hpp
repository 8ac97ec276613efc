// Fragment of capi.hip (bound tapes: renders and meshes of tapes that read more input slots than the render state binds); not a stand-alone
// header: included by capi.hip only.
// ---- bound tapes ------------------------------------------------------------------------
// A render or a mesh binds every variable but the axes to one constant for the whole call, and its kernels take FH_MAX_INPUTS input slots
// (render_state.h in_kind / in_value, the assembly input handlers, the columns kernel's decode table).  A tape that reads more slots is
// rendered as its BOUND tape: the same ops one for one, every INPUT of a bound slot turned into COPY_IMM of the value's bits and every INPUT
// of an axis into INPUT of slot 0 / 1 / 2 for x / y / z - in the tape, its groups and its term groups.  Registers, choice order, the term
// plan and the groups stay the parent's (copied, not computed again).  An INPUT of a bound constant and a COPY_IMM of it produce the same
// interval [v, v], point v and gradient (v, 0, 0, 0), so the image is the parent's.  BOUND_TAPES.md has the rest.
static const int32_t BOUND_AXES[3] = {0, 1, 2};
static const size_t BOUND_CACHE_ENTRIES = 8;   // bound tapes kept per parent (the bindings used last)

// The binding of every input slot of `tape` (key[1 + slot]: axis << 32, or 3 << 32 | the value's bits; key[0]: the device), as bind_inputs
// reads axis_slots, keys and values: the axes first, then the values (an axis' slot stays the axis).  Keys the tape does not read are ignored.
static fhip_status bound_key(fhip_ctx* ctx, const fhip_tape* tape, const int32_t* axis_slots, const uint64_t* keys, const float* vals, uint32_t n,
                             std::vector<uint64_t>& key) {
    const fh::HostTape& t = tape->t;
    const uint64_t NONE = ~0ull;
    key.assign((size_t)t.n_vars + 1, NONE);
    key[0] = ctx ? (uint64_t)(uint32_t)ctx->device : 0;
    for (int a = 0; a < 3; a++) {
        const int s = axis_slots ? axis_slots[a] : t.vars.axis[a];
        if (s >= 0 && (uint32_t)s < t.n_vars) key[1 + s] = (uint64_t)a << 32;
    }
    for (uint32_t i = 0; i < n; i++) {
        const int64_t s = axis_slots ? (keys[i] < t.n_vars ? (int64_t)keys[i] : -1) : t.vars.slot_of(3, keys[i]);
        if (s < 0) continue;
        uint64_t& k = key[1 + s];
        if (k == NONE || (k >> 32) == 3) k = (3ull << 32) | fh::bits_of(vals[i]);
    }
    for (size_t s = 1; s < key.size(); s++)
        if (key[s] == NONE) return fail(ctx, FHIP_ERR_MISSING_VAR, "a variable of the shape has no value");
    return FHIP_OK;
}

// The rewrite itself, for one tape's ops (slot = word 1 of an INPUT op, < n_vars)
static void bind_ops(std::vector<uint64_t>& ops, const std::vector<uint64_t>& key) {
    for (uint64_t& w : ops) {
        if (FH_W_OP((uint32_t)w) != FH_INPUT) continue;
        const uint64_t k = key[1 + (size_t)(w >> 32)];
        if ((k >> 32) < 3) w = (w & 0xFFFFFFFFull) | ((k >> 32) << 32);
        else w = (w & 0xFFF00ull) | FH_COPY_IMM | ((k & 0xFFFFFFFFull) << 32);    // (the out register kept, a = 0 as fh_pack gives)
    }
}
static void bind_host_tape(fh::HostTape& t, const std::vector<uint64_t>& key) {
    bind_ops(t.ops, key);
    t.vars = fh::VarTable();
    for (int a = 0; a < 3; a++) t.vars.axis[a] = a;
    t.vars.count = 3;
    t.n_vars = 3;
    t.op_class = 0;
}
static fhip_tape* make_bound(const fhip_tape* parent, const std::vector<uint64_t>& key) {
    fhip_tape* b = new fhip_tape();
    b->t = parent->t;
    bind_host_tape(b->t, key);
    b->groups = parent->groups;
    for (fh::HostTape& g : b->groups) bind_host_tape(g, key);
    b->group_op = parent->group_op;
    b->plan = parent->plan;
    b->tgroups = parent->tgroups;
    for (fh::HostTape& g : b->tgroups) bind_host_tape(g, key);
    b->parent_serial = parent->parent_serial ? parent->parent_serial : parent->serial;
    return b;
}

// The tape a render or mesh of `tape` with this binding runs: `tape` itself when it reads at most FH_MAX_INPUTS slots (today's path:
// `hold` stays empty), otherwise its bound tape, found in or added to the parent's cache, in `hold`.  FHIP_ERR_MISSING_VAR before anything
// is built when a slot has no value.
static fhip_status bound_tape(fhip_ctx* ctx, const fhip_tape* tape, const int32_t* axis_slots, const uint64_t* keys, const float* vals, uint32_t n,
                              std::shared_ptr<const fhip_tape>& hold) {
    hold.reset();
    if (tape->t.n_vars <= FH_MAX_INPUTS) return FHIP_OK;
    std::vector<uint64_t> key;
    fhip_status st = bound_key(ctx, tape, axis_slots, keys, vals, n, key);
    if (st) return st;
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint64_t k : key) h = (h ^ k) * 0x100000001B3ull;
    BoundCache& C = tape->bound;
    {
        std::lock_guard<std::mutex> guard(C.lock);
        for (BoundCache::Entry& e : C.entries)
            if (e.hash == h && e.key == key) { e.used = ++C.clock; hold = e.tape; return FHIP_OK; }
    }
    // (built outside the lock: another thread that wants the same binding may build it too - the first one in is kept)
    std::shared_ptr<fhip_tape> b(make_bound(tape, key), [](fhip_tape* p) { fhip_tape_free(p); });
    b->self = b;
    std::shared_ptr<const fhip_tape> evicted;     // (let go of after the lock: freeing a tape frees its device copies)
    std::lock_guard<std::mutex> guard(C.lock);
    for (BoundCache::Entry& e : C.entries)
        if (e.hash == h && e.key == key) { e.used = ++C.clock; hold = e.tape; return FHIP_OK; }
    size_t at = C.entries.size();
    if (at < BOUND_CACHE_ENTRIES) C.entries.emplace_back();
    else {
        at = 0;
        for (size_t i = 1; i < C.entries.size(); i++) if (C.entries[i].used < C.entries[at].used) at = i;
        evicted = std::move(C.entries[at].tape);
    }
    BoundCache::Entry& e = C.entries[at];
    e.hash = h; e.key = std::move(key); e.used = ++C.clock; e.tape = b;
    hold = b;
    return FHIP_OK;
}

// A frame of this set is about to read `tape` (upload_frame): a bound tape is held by the set until the set's next frame, and the set
// lets go of it only once the frame that read it is over (ev_done) - a queued copy or kernel may still read its ops.  A parent's cache
// may drop the tape meanwhile (another binding took its place, or the parent was freed); the set's hold keeps it.
static fhip_status hold_bound(fhip_ctx* ctx, const fhip_tape* tape) {
    if (ctx->bound_hold.get() == tape || (!ctx->bound_hold && !tape->parent_serial)) return FHIP_OK;
    if (ctx->bound_hold && ctx->ev_done_valid) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_done));
    ctx->bound_hold = tape->parent_serial ? tape->self.lock() : nullptr;
    return FHIP_OK;
}

// fidget_hip_debug.h: the bound tape of `tape` for a binding, as a tape of its own (not cached; fhip_tape_free frees it)
fhip_status fhip_debug_bound_tape(fhip_ctx* ctx, const fhip_tape* tape, const int32_t* axis_slots, const uint64_t* keys, const float* vals,
                                  uint32_t n, fhip_tape** out) {
    std::vector<uint64_t> key;
    fhip_status st = bound_key(ctx, tape, axis_slots, keys, vals, n, key);
    if (st) return st;
    *out = make_bound(tape, key);
    return FHIP_OK;
}
