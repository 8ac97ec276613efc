// Fragment of capi.hip (the constraint solver: fidget-solver's solve for a batch of parameter sets, solve.hip); not a stand-alone header: included by capi.hip only.
// ---- solver ----------------------------------------------------------------------------
// fidget-solver/src/lib.rs:191 (solve), batched: every instance is an independent Levenberg-Marquardt loop over the same tapes.
fhip_status fhip_solve(fhip_ctx* ctx, const fhip_tape* const* constraints, uint32_t n_constraints, const int32_t* param_axis,
                       const uint64_t* param_index, const uint8_t* param_free, uint32_t n_params, const float* values,
                       uint32_t n_instances, uint32_t max_iterations, float* out, float* err, uint32_t* iterations,
                       int32_t* exit_reason) {
    // ---- checks, all before any launch
    std::vector<int32_t> free_of(n_params, -1), param_of;
    for (uint32_t p = 0; p < n_params; p++) {
        if (param_axis[p] < 0 || param_axis[p] > 3) return fail(ctx, FHIP_ERR_BAD_VAR_SLICE, "parameter axis must be 0..3");
        for (uint32_t q = 0; q < p; q++)
            if (param_axis[q] == param_axis[p] && (param_axis[p] < 3 || param_index[q] == param_index[p]))
                return fail(ctx, FHIP_ERR_BAD_VAR_SLICE, "a variable is given twice");
        if (param_free[p]) { free_of[p] = (int32_t)param_of.size(); param_of.push_back((int32_t)p); }
    }
    const uint32_t n = (uint32_t)param_of.size();
    if (n > fhsolve::MAX_FREE) return fail(ctx, FHIP_ERR_UNSUPPORTED, "more than 64 free parameters");
    if (n_instances && ((n && !out) || (n_params && !values))) return fail(ctx, FHIP_ERR_BAD_VAR_SLICE, "missing values or output");
    for (uint32_t i = 0; i < n_constraints; i++)
        if (!constraints[i] || constraints[i]->t.n_outputs == 0) return fail(ctx, FHIP_ERR_BAD_TAPE, "a constraint has no output");
    if (n_instances == 0) return FHIP_OK;
    if (!max_iterations) max_iterations = fhsolve::DEFAULT_MAX_ITERATIONS;
    if (n_constraints == 0) {   // every residual (there are none) is 0: the start, after 0 iterations (lib.rs:234-236)
        for (uint32_t s = 0; s < n_instances; s++) {
            for (uint32_t k = 0; k < n; k++) out[(size_t)s * n + k] = values[(size_t)s * n_params + param_of[k]];
            if (err) err[s] = 0.0f;
            if (iterations) iterations[s] = 0;
            if (exit_reason) exit_reason[s] = fhsolve::EXIT_ZERO_RESIDUAL;
        }
        return FHIP_OK;
    }
    // ---- each constraint's input slots -> parameters (fhip_tape_axis_slot / fhip_tape_var_slot)
    std::vector<SolveTape> tapes(n_constraints);
    std::vector<int32_t> ints(free_of);
    ints.insert(ints.end(), param_of.begin(), param_of.end());
    uint32_t n_regs = 1;
    for (uint32_t i = 0; i < n_constraints; i++) {
        const fhip_tape* t = constraints[i];
        { fhip_status ts_ = tape_to_device(ctx, t); if (ts_) return ts_; }
        tapes[i].ops = (uint64_t)(uintptr_t)t->d_ops;
        tapes[i].len = (uint32_t)t->t.ops.size();
        tapes[i].slots = (uint32_t)ints.size();
        n_regs = std::max(n_regs, t->t.n_regs);
        ints.resize(ints.size() + std::max<uint32_t>(t->t.n_vars, 1), -1);
        for (uint32_t p = 0; p < n_params; p++) {
            const int slot = param_axis[p] < 3 ? fhip_tape_axis_slot(t, param_axis[p]) : fhip_tape_var_slot(t, param_index[p]);
            if (slot >= 0) ints[tapes[i].slots + slot] = (int32_t)p;
        }
    }
    // ---- launch shape: G lanes per instance; the instances' work arrays and, if it fits, the register file in LDS
    const uint32_t G = fhsolve::group_lanes(n), per_wave = WAVE / G;
    const size_t state_bytes = (((size_t)per_wave * fhsolve::Layout{n}.floats() * 4) + 15) & ~(size_t)15;
    const size_t file_bytes = (size_t)n_regs * WAVE * sizeof(GR);
    const bool slab = state_bytes + file_bytes > FH_LDS_MAX;
    const size_t lds = slab ? state_bytes : state_bytes + file_bytes;
    const uint32_t grid = (n_instances + per_wave - 1) / per_wave;
    // ---- device buffers: inputs in io_a, results in io_b, global register files in io_e
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_ints = al(n_constraints * sizeof(SolveTape)), o_vals = o_ints + al(ints.size() * 4),
                 in_bytes = o_vals + al((size_t)n_instances * std::max<uint32_t>(n_params, 1) * 4);
    const size_t n_out = (size_t)n_instances * n, res_bytes = (n_out + 3 * (size_t)n_instances) * 4;
    HIP_TRY(ctx, ctx->io_a.ensure(in_bytes));
    HIP_TRY(ctx, ctx->io_b.ensure(res_bytes));
    if (slab) HIP_TRY(ctx, ctx->io_e.ensure(file_bytes * grid));
    char* din = (char*)ctx->io_a.p;
    float* dres = (float*)ctx->io_b.p;
    HIP_TRY(ctx, hipMemcpyAsync(din, tapes.data(), n_constraints * sizeof(SolveTape), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(din + o_ints, ints.data(), ints.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_params) HIP_TRY(ctx, hipMemcpyAsync(din + o_vals, values, (size_t)n_instances * n_params * 4, hipMemcpyHostToDevice, ctx->stream));
    SolveArgs a;
    a.tapes = (const SolveTape*)din;
    a.ints = (const int32_t*)(din + o_ints);
    a.values = (const float*)(din + o_vals);
    a.res = dres;
    a.gregs = slab ? (GR*)ctx->io_e.p : nullptr;
    a.n_regs = n_regs;
    a.n_constraints = n_constraints;
    a.n_params = n_params;
    a.n_free = n;
    a.n_inst = n_instances;
    a.group = G;
    a.max_iterations = max_iterations;
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, FH_LDS_MAX));
    hipLaunchKernelGGL(k_solve, dim3(grid), dim3(WAVE), lds, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    if (n) HIP_TRY(ctx, hipMemcpyAsync(out, dres, n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (err) HIP_TRY(ctx, hipMemcpyAsync(err, dres + n_out, (size_t)n_instances * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (iterations) HIP_TRY(ctx, hipMemcpyAsync(iterations, dres + n_out + n_instances, (size_t)n_instances * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (exit_reason) HIP_TRY(ctx, hipMemcpyAsync(exit_reason, dres + n_out + 2 * (size_t)n_instances, (size_t)n_instances * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FHIP_OK;
}
