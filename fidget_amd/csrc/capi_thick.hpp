// ---- the local thickness of a distance field ---------------------------------------------------------------------------------------------------
// fhip_distance_thickness (fidget_hip.h): the passes of thick.hip on a finished fhip_distance, all on the context's stream; the host waits
// once, at the end, for the summary.  The result is a fhip_distance again - its field is T - so fhip_distance_slices, _threshold, _dev
// and _free serve it as they are.  A fragment of the C ABI, included by capi_mesh.hpp after capi_edt.hpp, whose
// fhip_distance and distance_threshold it uses; uses capi_mesh_util.hpp.  FHIP_MESH_TIMES: the passes' wall times on stderr.
fhip_status fhip_distance_thickness(fhip_ctx* ctx, const void* distance, void** out) {
    if (out) *out = nullptr;
    const fhip_distance* const d = (const fhip_distance*)distance;
    if (!ctx || !d || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_distance_thickness: context, distance field and result");
    if (ctx->device != d->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance: computed on another device");
    if (d->thickness) return fail(ctx, FHIP_ERR_UNSUPPORTED, "thickness: of a distance field, not of a thickness");
    if (d->n_fg == 0) return fail(ctx, FHIP_ERR_UNSUPPORTED, "thickness: a field without foreground has no bounded ball");
    if (d->max_d2 > fhlt::MAX_F) return fail(ctx, FHIP_ERR_UNSUPPORTED, "thickness: a squared distance above 3 * 1023^2");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t depth = d->depth;
    PassTimes times(st, "fhip thickness depth %u", depth);
    std::unique_ptr<fhip_distance> R(new fhip_distance());
    R->depth = depth; R->complement = d->complement; R->device = ctx->device; R->thickness = 1;
    const uint32_t N = 4u << depth;
    const uint64_t n_voxels = (uint64_t)N * N * N, n_keep = n_voxels / 64;
    const uint32_t vmax = (uint32_t)std::max<uint64_t>(d->max_d2, 1), A = fhlt::isqrt(vmax - 1);
    HIP_TRY(ctx, hipMalloc((void**)&R->d_field, (size_t)n_voxels * 4));
    const uint32_t red_blocks = (uint32_t)std::min<uint64_t>((n_voxels / 4 + 255) / 256, fhm::FH_LT_REDUCE_BLOCKS);
    ScratchBuf tables, keep, parts;
    const size_t table_bytes = 3 * ((size_t)vmax + 1) * 4;
    HIP_TRY(ctx, tables.ensure(table_bytes));
    HIP_TRY(ctx, keep.ensure((size_t)n_keep * 8));
    HIP_TRY(ctx, parts.ensure(((size_t)red_blocks * 3 + 4) * 8));
    uint64_t* const d_parts = (uint64_t*)parts.p;
    uint64_t* const d_sum = d_parts + 3 * (size_t)red_blocks;          // {largest key, smallest key, voxels with T > 0, kept centres}
    HIP_TRY(ctx, hipMemsetAsync(tables.p, 0, table_bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, 32, st));
    HIP_TRY(ctx, hipMemsetAsync(R->d_field, 0, (size_t)n_voxels * 4, st));
    HIP_TRY(ctx, times.mark("allocate, zero"));
    const uint64_t pairs = ((uint64_t)A + 1) * (A + 1);
    hipLaunchKernelGGL(fhm::k_lt_shells, cc_grid(pairs), dim3(256), 0, st, vmax, A, (uint32_t*)tables.p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_lt_need, dim3(3), dim3(1024), 0, st, vmax, (uint32_t*)tables.p);
    HIP_TRY(ctx, times.mark("need"));
    hipLaunchKernelGGL(fhm::k_lt_ridge, cc_grid(n_voxels), dim3(256), 0, st, (const uint32_t*)d->d_field, depth, (const uint32_t*)tables.p, vmax, (uint64_t*)keep.p,
                       (unsigned long long*)(d_sum + 3));
    HIP_TRY(ctx, times.mark("k_lt_ridge"));
    // a large ball's rows in parts, so that the few words that hold such centres occupy more than a wave each
    const uint32_t side = 2 * A + 1;
    const uint32_t split = std::min<uint32_t>(std::max<uint32_t>(side * side / 512, 1), fhm::FH_LT_PAINT_SPLIT);
    const uint32_t paint_blocks = (uint32_t)std::min<uint64_t>((n_keep + 3) / 4, fhm::FH_LT_PAINT_BLOCKS);
    hipLaunchKernelGGL(fhm::k_lt_paint, dim3(paint_blocks, split), dim3(256), 0, st, (const uint32_t*)d->d_field, (const uint64_t*)keep.p, depth, R->d_field);
    HIP_TRY(ctx, times.mark("k_lt_paint"));
    hipLaunchKernelGGL(fhm::k_lt_reduce, dim3(red_blocks), dim3(256), 0, st, (const uint32_t*)R->d_field, depth, d_parts);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_lt_reduce_sum, dim3(1), dim3(256), 0, st, (const uint64_t*)d_parts, red_blocks, d_sum);
    HIP_TRY(ctx, times.mark("k_lt_reduce"));
    uint64_t sum[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(sum, d_sum, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (times.on) {          // (otherwise they go with the scope)
        tables.release(); keep.release(); parts.release();
        HIP_TRY(ctx, times.mark("release"));
        fprintf(stderr, "fhip thickness depth %u: %llu centres, %llu balls painted, largest squared radius %llu\n", depth, (unsigned long long)(n_voxels - d->n_fg),
                (unsigned long long)sum[3], (unsigned long long)(sum[0] >> 32));
    }
    R->n_positive = sum[2];
    R->n_fg = n_voxels - sum[2];          // the zeros of T
    R->n_centres = n_voxels - d->n_fg;
    R->n_balls = sum[3];
    R->arg = 0;                           // (all zeros: 0 at index 0, as a distance field of foreground alone)
    if (sum[0] != 0) { R->max_d2 = sum[0] >> 32; R->arg = 0xFFFFFFFFull - (sum[0] & 0xFFFFFFFFull); }
    if (sum[1] != ~(uint64_t)0) { R->min_d2 = sum[1] >> 32; R->arg_min = sum[1] & 0xFFFFFFFFull; }
    *out = R.release();
    return FHIP_OK;
}
void fhip_thickness_info(const void* h, uint64_t out[8]) {
    const fhip_distance* const d = (const fhip_distance*)h;
    out[0] = d ? d->max_d2 : 0; out[1] = d ? d->arg : ~(uint64_t)0; out[2] = d ? d->min_d2 : 0; out[3] = d ? d->arg_min : ~(uint64_t)0;
    out[4] = d ? d->n_positive : 0; out[5] = d ? d->depth : 0; out[6] = d ? d->n_centres : 0; out[7] = d ? d->n_balls : 0;
}
fhip_status fhip_thickness_thin(fhip_ctx* ctx, const void* h, uint32_t t, uint64_t* out_bricks, int out_on_device) {
    return distance_threshold(ctx, h, t, 2u, out_bricks, out_on_device);
}
fhip_status fhip_thickness_histogram(fhip_ctx* ctx, const void* h, const uint32_t* edges, uint32_t n_edges, uint64_t* counts, int on_device) {
    const fhip_distance* const d = (const fhip_distance*)h;
    if (!ctx || !d) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_thickness_histogram: context and field");
    if (ctx->device != d->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance: computed on another device");
    if (!edges || !counts) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_thickness_histogram: edges and counts");
    if (n_edges < 2 || n_edges > fhm::FH_LT_MAX_EDGES) return fail(ctx, FHIP_ERR_UNSUPPORTED, "histogram: 2 to 1024 edges");
    if (on_device && (((uintptr_t)edges & 3u) || ((uintptr_t)counts & 7u))) return fail(ctx, FHIP_ERR_UNSUPPORTED, "histogram on the device: edges 4-byte, counts 8-byte aligned");
    if (!on_device)
        for (uint32_t e = 1; e < n_edges; e++)
            if (edges[e] < edges[e - 1]) return fail(ctx, FHIP_ERR_UNSUPPORTED, "histogram: the edges ascend");
    (void)hipSetDevice(ctx->device);
    FxStage st{ctx, on_device, {}};
    hipError_t e = hipSuccess;
    const uint32_t* const d_edges = (const uint32_t*)st.in(ctx->io_a, edges, (size_t)n_edges * 4, e); HIP_TRY(ctx, e);
    uint64_t* const d_counts = (uint64_t*)st.out(ctx->io_b, counts, (size_t)(n_edges - 1) * 8, e); HIP_TRY(ctx, e);
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)(n_edges - 1) * 8, ctx->stream));
    const uint32_t N = 4u << d->depth;
    const uint64_t n = (uint64_t)N * N * N;
    const uint32_t nb = (uint32_t)std::min<uint64_t>((n + 255) / 256, fhm::FH_LT_HIST_BLOCKS);
    hipLaunchKernelGGL(fhm::k_lt_hist, dim3(nb), dim3(256), 0, ctx->stream, (const uint32_t*)d->d_field, n, d_edges, n_edges, (unsigned long long*)d_counts);
    return st.finish();
}
