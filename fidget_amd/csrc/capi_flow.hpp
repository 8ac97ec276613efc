// ---- a voxel bitmap along a direction ----------------------------------------------------------------------------------------------------------
// fhip_voxels_flow, fhip_voxels_overhangs and fhip_voxels_heights (fidget_hip.h): one launch of flow.hip each, on the context's stream.
// The effects' convention, as fhip_voxels_slices has it: device pointers are worked on in place and asynchronously; host arrays go
// through the context's staging buffers (seeds or bricks io_a, blockers io_c, the result io_b) and the call waits for the result.  A
// fragment of the C ABI, included by capi_mesh.hpp; uses capi_mesh_util.hpp.
fhip_status fhip_voxels_flow(fhip_ctx* ctx, const uint64_t* seeds, const uint64_t* blockers, uint32_t depth, int on_device, uint32_t dir, uint32_t flags,
                             uint64_t* out, int out_on_device) {
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_flow: context and result");
    { const fhip_status s = bitmap_args(ctx, "fhip_voxels_flow: the seeds", depth, seeds, blockers, out, out_on_device); if (s) return s; }
    if (dir > 5) return fail(ctx, FHIP_ERR_UNSUPPORTED, "flow: a direction is 0 .. 5 = -x, +x, -y, +y, -z, +z");
    if (flags & ~fhfl::FLOW_WITH_SEEDS) return fail(ctx, FHIP_ERR_UNSUPPORTED, "flow: unknown flag bits");
    if (on_device && ((uintptr_t)blockers & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "a voxel bitmap on the device must be 8-byte aligned");
    (void)hipSetDevice(ctx->device);
    FxStage in{ctx, on_device, {}}, st{ctx, out_on_device, {}};
    const uint64_t* d_seeds = nullptr;
    { const fhip_status s = voxels_in(ctx, in, seeds, depth, d_seeds); if (s) return s; }
    const uint64_t n_words = fhvox::n_words(depth);
    hipError_t e = hipSuccess;
    const uint64_t* const d_blockers = (const uint64_t*)in.in(ctx->io_c, blockers, (size_t)n_words * 8, e); HIP_TRY(ctx, e);
    uint64_t* const d_out = (uint64_t*)st.out(ctx->io_b, out, (size_t)n_words * 8, e); HIP_TRY(ctx, e);
    const uint32_t B = 1u << depth, with_seeds = flags & fhfl::FLOW_WITH_SEEDS;
    if (dir < 2) {          // a wave per 64 bricks of a row, or per row where it is longer
        const uint64_t waves = depth < 6 ? (n_words + 63) / 64 : (uint64_t)B * B;
        hipLaunchKernelGGL(fhm::k_flow_x, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, d_seeds, d_blockers, depth, dir, with_seeds, d_out);
    } else {
        hipLaunchKernelGGL(fhm::k_flow_yz, dim3((B * B + 63) / 64), dim3(64), 0, ctx->stream, d_seeds, d_blockers, depth, dir, with_seeds, d_out);
    }
    return st.finish();
}
fhip_status fhip_voxels_overhangs(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t up, uint32_t reach2, int bed, uint64_t* out,
                                  int out_on_device) {
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_overhangs: context and result");
    { const fhip_status s = bitmap_args(ctx, "fhip_voxels_overhangs: the bitmap", depth, bricks, nullptr, out, out_on_device); if (s) return s; }
    if (up > 5) return fail(ctx, FHIP_ERR_UNSUPPORTED, "overhangs: a direction is 0 .. 5 = -x, +x, -y, +y, -z, +z");
    if (reach2 > fhfl::MAX_REACH2) return fail(ctx, FHIP_ERR_UNSUPPORTED, "overhangs: reach2 at most 16 - a supporter lies in the brick or in one next to it");
    (void)hipSetDevice(ctx->device);
    FxStage in{ctx, on_device, {}}, st{ctx, out_on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, in, bricks, depth, d_bricks); if (s) return s; }
    const uint64_t n_words = fhvox::n_words(depth);
    hipError_t e = hipSuccess;
    uint64_t* const d_out = (uint64_t*)st.out(ctx->io_b, out, (size_t)n_words * 8, e); HIP_TRY(ctx, e);
    hipLaunchKernelGGL(fhm::k_overhangs, cc_grid(n_words), dim3(256), 0, ctx->stream, d_bricks, depth, up, reach2, bed ? 1u : 0u, d_out);
    return st.finish();
}
fhip_status fhip_voxels_heights(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t axis, int32_t* out, int out_on_device) {
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_heights: context and result");
    { const fhip_status s = bitmap_args(ctx, "fhip_voxels_heights: the bitmap", depth, bricks); if (s) return s; }
    if (axis > 2) return fail(ctx, FHIP_ERR_UNSUPPORTED, "heights: an axis is 0, 1, 2 = x, y, z");
    if ((const void*)out == (const void*)bricks) return fail(ctx, FHIP_ERR_UNSUPPORTED, "a voxel bitmap along a direction: the result must not be an input");
    if (out_on_device && ((uintptr_t)out & 3u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "heights to the device: the buffer must be 4-byte aligned");
    (void)hipSetDevice(ctx->device);
    FxStage in{ctx, on_device, {}}, st{ctx, out_on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, in, bricks, depth, d_bricks); if (s) return s; }
    const uint32_t B = 1u << depth, N = 4u << depth;
    hipError_t e = hipSuccess;
    int32_t* const d_out = (int32_t*)st.out(ctx->io_b, out, (size_t)3 * N * N * 4, e); HIP_TRY(ctx, e);
    if (axis == 0 && depth >= 6) hipLaunchKernelGGL(fhm::k_heights_x, dim3(B * B / 4), dim3(256), 0, ctx->stream, d_bricks, depth, d_out);
    else hipLaunchKernelGGL(fhm::k_heights, dim3((N * N + 255) / 256), dim3(256), 0, ctx->stream, d_bricks, depth, axis, d_out);
    return st.finish();
}
