// ---- the voxel bitmap ---------------------------------------------------------------------------------------------------------------------
// The voxel bitmap (fidget_hip.h): occupancy's level loop with the bitmap kernels of mesh.hip; a host `out` is filled from the context's
// buffer through the pinned landing area.  fhip_voxels_slices and fhip_voxels_layer_counts (k_vox_slices, k_vox_layer_counts) follow the
// effects' convention - device pointers and asynchronous, or host buffers.  A fragment of the C ABI, included by capi_mesh.hpp after the
// mesher, whose mesh_run makes the bitmap; uses capi_mesh_util.hpp.
uint64_t fhip_voxels_words(uint32_t depth) { return fhvox::n_words(depth); }
fhip_status fhip_shape_voxels(fhip_ctx* ctx, const fhip_tape* tape, uint32_t depth, const float* world_to_model, const int32_t* axis_slots,
                              const uint64_t* var_keys, const float* var_values, uint32_t n_vars, uint64_t* out, int out_is_device, uint64_t cells[4]) {
    if (!ctx || !tape || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_shape_voxels: context, tape and output buffer");
    if (depth > fhvox::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel depth above 10: the bitmap of a grid of more than 4096^3 voxels exceeds 8 GiB");
    const size_t bytes = (size_t)fhvox::n_words(depth) * 8;
    VoxTarget vt{out, cells};
    if (out_is_device) {
        if ((uintptr_t)out & 7u) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxels to the device: the buffer must be 8-byte aligned");
    } else {
        (void)hipSetDevice(ctx->device);
        HIP_TRY(ctx, ctx->io_d.ensure(bytes));
        vt.d_out = (uint64_t*)ctx->io_d.p;
    }
    fhip_mesh* m = nullptr;
    const fhip_status st = mesh_run(ctx, tape, depth, world_to_model, axis_slots, var_keys, var_values, n_vars, MESH_VOX, 0, 1, &m, nullptr, &vt);
    delete m;
    if (st || out_is_device) return st;
    return mesh_to_host(ctx, out, vt.d_out, bytes);
}
fhip_status fhip_voxels_slices(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, uint32_t k0, uint32_t k1, uint8_t* out, int on_device) {
    if (!ctx) return FHIP_ERR_BAD_TAPE;
    if (depth > fhvox::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel depth above 10");
    const uint32_t N = 4u << depth;
    if (k0 > k1 || k1 > N) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel slices: layers k0 <= k1 <= 4 << depth");
    if (k0 == k1) return FHIP_OK;
    if (!bricks || !out) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_voxels_slices: bitmap and output buffer");
    if (on_device && ((uintptr_t)out & 15u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel slices to the device: the buffer must be 16-byte aligned");
    (void)hipSetDevice(ctx->device);
    FxStage st{ctx, on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, st, bricks, depth, d_bricks); if (s) return s; }
    hipError_t e = hipSuccess;
    uint8_t* const d_out = (uint8_t*)st.out(ctx->io_b, out, (size_t)(k1 - k0) * N * N, e); HIP_TRY(ctx, e);
    const uint64_t runs = ((uint64_t)(k1 - k0) * N) << (depth < 2 ? 0 : depth - 2);
    const uint32_t nb = (uint32_t)std::min<uint64_t>((runs + 255) / 256, fhm::FH_VOX_SLICE_BLOCKS);
    hipLaunchKernelGGL(fhm::k_vox_slices, dim3(nb), dim3(256), 0, ctx->stream, d_bricks, depth, k0, k1, d_out);
    return st.finish();
}
fhip_status fhip_voxels_layer_counts(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, uint64_t* out, int on_device) {
    if (!ctx) return FHIP_ERR_BAD_TAPE;
    if (depth > fhvox::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel depth above 10");
    if (!bricks || !out) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_voxels_layer_counts: bitmap and output buffer");
    if (on_device && ((uintptr_t)out & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "layer counts to the device: the buffer must be 8-byte aligned");
    (void)hipSetDevice(ctx->device);
    FxStage st{ctx, on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, st, bricks, depth, d_bricks); if (s) return s; }
    const uint32_t B = 1u << depth, N = 4u << depth;
    const uint32_t n_parts = (uint32_t)std::min<uint64_t>((((uint64_t)B * B) + 255) / 256, fhm::FH_VOX_COUNT_PARTS);
    hipError_t e = hipSuccess;
    uint64_t* const d_out = (uint64_t*)st.out(ctx->io_b, out, (size_t)N * 8, e); HIP_TRY(ctx, e);
    HIP_TRY(ctx, ctx->io_c.ensure((size_t)B * n_parts * 4 * 8));
    hipLaunchKernelGGL(fhm::k_vox_layer_counts, dim3(n_parts, B), dim3(256), 0, ctx->stream, d_bricks, depth, (uint64_t*)ctx->io_c.p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_vox_layer_sum, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, (const uint64_t*)ctx->io_c.p, n_parts, N, d_out);
    return st.finish();
}
