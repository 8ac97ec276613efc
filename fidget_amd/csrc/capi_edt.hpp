// ---- the distance transform of a voxel bitmap -----------------------------------------------------------------------------------------------
// fhip_voxels_distance (fidget_hip.h; the handle it declares void* is a fhip_distance): the three passes of edt.hip and the summary, all on
// the context's stream; the host waits once, at the end, for the summary.  A fragment of the C ABI, included by capi_mesh.hpp; uses
// capi_mesh_util.hpp.  FHIP_MESH_TIMES: the passes' wall times on stderr.
struct fhip_distance {
    uint64_t max_d2 = 0, arg = ~(uint64_t)0, n_fg = 0;       // arg: the smallest index with max_d2, all ones for "none"
    uint32_t depth = 0;
    int complement = 0, device = 0;
    uint32_t* d_field = nullptr;          // [N][N][N], [k][j][i]
    // a local thickness (capi_thick.hpp) is a field like this one - max_d2, arg and n_fg its largest value, where, and its zeros - with more to say
    int thickness = 0;
    uint64_t min_d2 = 0, arg_min = ~(uint64_t)0, n_positive = 0, n_centres = 0, n_balls = 0;
    ~fhip_distance() { if (d_field) (void)hipFree(d_field); }
};
fhip_status fhip_voxels_distance(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, int complement, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_distance: context and result");
    if (depth > fhedt::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance: voxel depth above 8 - the field of a grid of more than 1024^3 voxels exceeds 4 GiB");
    if (!bricks) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_voxels_distance: the bitmap");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    FxStage stage{ctx, on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, stage, bricks, depth, d_bricks); if (s) return s; }
    PassTimes times(st, "fhip distance depth %u%s", depth, complement ? " complement" : "");
    std::unique_ptr<fhip_distance> R(new fhip_distance());
    R->depth = depth; R->complement = complement ? 1 : 0; R->device = ctx->device;
    const uint32_t B = 1u << depth, N = 4u << depth;
    const uint64_t n_voxels = (uint64_t)N * N * N;
    HIP_TRY(ctx, hipMalloc((void**)&R->d_field, (size_t)n_voxels * 4));
    // the columns' stacks where they do not fit LDS, and the partials of the summary
    const uint32_t n_groups = (N * N + fhm::FH_EDT_LANES - 1) / fhm::FH_EDT_LANES;
    const bool in_lds = N <= fhm::FH_EDT_LDS_MAX_N;
    const uint32_t col_blocks = in_lds ? n_groups : std::min(n_groups, fhm::FH_EDT_COL_BLOCKS);
    const size_t lds_bytes = in_lds ? (size_t)N * fhm::FH_EDT_LANES * sizeof(fhedt::Entry) : 0;
    const uint32_t red_blocks = (uint32_t)std::min<uint64_t>((n_voxels / 4 + 255) / 256, fhm::FH_EDT_REDUCE_BLOCKS);
    ScratchBuf work, parts;
    if (!in_lds) HIP_TRY(ctx, work.ensure((size_t)col_blocks * N * fhm::FH_EDT_LANES * sizeof(fhedt::Entry)));
    HIP_TRY(ctx, parts.ensure(((size_t)red_blocks + 1) * 16));
    uint64_t* const d_parts = (uint64_t*)parts.p;
    uint64_t* const d_sum = d_parts + 2 * (size_t)red_blocks;
    HIP_TRY(ctx, times.mark("allocate"));
    hipLaunchKernelGGL(fhm::k_edt_rows, dim3(B * B), dim3(256), 0, st, d_bricks, depth, complement ? ~(uint64_t)0 : (uint64_t)0, R->d_field);
    HIP_TRY(ctx, times.mark("k_edt_rows"));
    for (uint32_t axis = 1; axis <= 2; axis++) {
        if (in_lds) hipLaunchKernelGGL(fhm::k_edt_cols<true>, dim3(col_blocks), dim3(fhm::FH_EDT_LANES), lds_bytes, st, R->d_field, depth, axis, (fhedt::Entry*)nullptr);
        else hipLaunchKernelGGL(fhm::k_edt_cols<false>, dim3(col_blocks), dim3(fhm::FH_EDT_LANES), 0, st, R->d_field, depth, axis, (fhedt::Entry*)work.p);
        HIP_TRY(ctx, times.mark(axis == 1 ? "k_edt_cols j" : "k_edt_cols k"));
    }
    hipLaunchKernelGGL(fhm::k_edt_reduce, dim3(red_blocks), dim3(256), 0, st, (const uint32_t*)R->d_field, depth, d_parts);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_edt_reduce_sum, dim3(1), dim3(256), 0, st, (const uint64_t*)d_parts, red_blocks, d_sum);
    HIP_TRY(ctx, times.mark("k_edt_reduce"));
    uint64_t sum[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(sum, d_sum, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (times.on) {          // (otherwise the two go with the scope)
        work.release(); parts.release();
        HIP_TRY(ctx, times.mark("release"));
    }
    R->n_fg = sum[1];
    if (sum[0] != 0) { R->max_d2 = sum[0] >> 32; R->arg = 0xFFFFFFFFull - (sum[0] & 0xFFFFFFFFull); }
    *out = R.release();
    return FHIP_OK;
}
void fhip_distance_info(const void* h, uint64_t out[4]) {
    const fhip_distance* const d = (const fhip_distance*)h;
    out[0] = d ? d->max_d2 : 0; out[1] = d ? d->arg : ~(uint64_t)0; out[2] = d ? d->n_fg : 0; out[3] = d ? d->depth : 0;
}
const uint32_t* fhip_distance_dev(const void* h) { return HANDLE_GET(fhip_distance, h, d_field); }
fhip_status fhip_distance_slices(fhip_ctx* ctx, const void* h, uint32_t k0, uint32_t k1, uint32_t* out, int out_on_device) {
    const fhip_distance* const d = (const fhip_distance*)h;
    if (!ctx || !d) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_distance_slices: context and distance field");
    if (ctx->device != d->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance: computed on another device");
    const uint32_t N = 4u << d->depth;
    if (k0 > k1 || k1 > N) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance slices: layers k0 <= k1 <= 4 << depth");
    if (k0 == k1) return FHIP_OK;
    if (!out) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_distance_slices: output buffer");
    if (out_on_device && ((uintptr_t)out & 15u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance slices to the device: the buffer must be 16-byte aligned");
    (void)hipSetDevice(ctx->device);
    const uint32_t* const src = d->d_field + (size_t)k0 * N * N;
    const size_t n = (size_t)(k1 - k0) * N * N;
    if (!out_on_device) {          // the layers asked for, straight from the field
        HIP_TRY(ctx, hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FHIP_OK;
    }
    const uint32_t nb = (uint32_t)std::min<uint64_t>((n / 4 + 255) / 256, fhm::FH_EDT_COPY_BLOCKS);
    hipLaunchKernelGGL(fhm::k_edt_copy, dim3(nb), dim3(256), 0, ctx->stream, (const uint4*)src, (uint64_t)(n / 4), (uint4*)out);
    HIP_TRY(ctx, hipGetLastError());
    return FHIP_OK;
}
// mode: k_edt_threshold's - 0 within, 1 beyond, 2 thin (fhip_thickness_thin)
static fhip_status distance_threshold(fhip_ctx* ctx, const void* h, uint32_t t, uint32_t mode, uint64_t* out_bricks, int out_on_device) {
    const fhip_distance* const d = (const fhip_distance*)h;
    if (!ctx || !d) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_distance_threshold: context and distance field");
    if (ctx->device != d->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance: computed on another device");
    if (t == fhedt::NONE) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance threshold: t at most 0xFFFFFFFE (0xFFFFFFFF stands for no distance)");
    if (!out_bricks) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_distance_threshold: output buffer");
    if (out_on_device && ((uintptr_t)out_bricks & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "distance threshold to the device: the bitmap must be 8-byte aligned");
    (void)hipSetDevice(ctx->device);
    FxStage st{ctx, out_on_device, {}};
    const uint64_t n_words = fhvox::n_words(d->depth);
    hipError_t e = hipSuccess;
    uint64_t* const d_out = (uint64_t*)st.out(ctx->io_b, out_bricks, (size_t)n_words * 8, e); HIP_TRY(ctx, e);
    hipLaunchKernelGGL(fhm::k_edt_threshold, cc_grid(n_words), dim3(256), 0, ctx->stream, (const uint32_t*)d->d_field, d->depth, t, mode, d_out);
    return st.finish();
}
fhip_status fhip_distance_threshold(fhip_ctx* ctx, const void* h, uint32_t t, int beyond, uint64_t* out_bricks, int out_on_device) {
    return distance_threshold(ctx, h, t, beyond ? 1u : 0u, out_bricks, out_on_device);
}
void fhip_distance_free(void* h) { delete (fhip_distance*)h; }
