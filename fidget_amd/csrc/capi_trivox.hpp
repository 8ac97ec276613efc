// ---- a triangle mesh to a voxel bitmap ---------------------------------------------------------------------------------------------------------
// fhip_triangles_voxels and fhip_mesh_voxels (fidget_hip.h): the passes of trivox.hip on the context's stream - the bitmap, the exit
// plane and the counters cleared; k_tv_setup; the prefix sums of the column counts (ctr_scan twice: the low words, and from where they
// wrapped the high words); k_tv_cross over the W items; k_tv_fill.  The host waits once for W - it decides an overflow and sizes the
// launch - and once at the end for the counters, which go to the caller's host array: the call blocks, also with device pointers.
// Host input arrays may be far larger than a bitmap: they get device memory of their own for the call, released with it.  The call's
// scratch - the exit plane and the counters, then per triangle the record and four 32-bit words, 64 bytes and the scans' block totals -
// is carved from ctx->mesh_leaves, the buffer the mesher keeps its leaf records in between builds: it only grows, stays with the
// context after the call, and fhip_ctx_trim (or a frame that needs the room, or fhip_ctx_destroy) gives it back.  Neither use needs
// its contents after its own call.  Why it is kept: allocating and releasing some gigabytes in every call of a row of calls took,
// in some runs, thirty times what the passes take (profiles/mesh_voxels/README.md).  A host `out` goes through the staging buffer
// io_b, a bitmap's size, as the other bitmap calls' results do; like theirs it stays until fhip_ctx_destroy.  A fragment of the C ABI,
// included by capi_mesh.hpp; uses capi_mesh_util.hpp.  FHIP_MESH_TIMES: the passes' wall times on stderr.
fhip_status fhip_triangles_voxels(fhip_ctx* ctx, const float* vertices, uint64_t n_vertices, const uint64_t* triangles, uint64_t n_triangles, int on_device,
                                  const double* mesh_to_world, uint32_t depth, uint64_t* out, int out_on_device, uint64_t info[8]) {
    if (!ctx || !out || !info) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_triangles_voxels: context, result and info");
    if (depth > fhvox::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel depth above 10");
    if (n_triangles >= (1ull << 32)) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh to voxels: 2^32 triangles and more");
    if (n_triangles && !vertices) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_triangles_voxels: the vertices");
    if (n_vertices > (1ull << 60)) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh to voxels: more than 2^60 vertices");
    if (on_device && (((uintptr_t)vertices & 3u) || ((uintptr_t)triangles & 7u)))
        return fail(ctx, FHIP_ERR_UNSUPPORTED, "a mesh on the device: vertices 4-byte aligned, triangles 8-byte aligned");
    if (out_on_device && ((uintptr_t)out & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "a voxel bitmap on the device must be 8-byte aligned");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    PassTimes times(st, "fhip mesh to voxels depth %u", depth);
    const uint32_t T = (uint32_t)n_triangles, B = 1u << depth;
    const uint64_t n_words = fhvox::n_words(depth), n_exit = fhtv::exit_words(depth);
    FxStage stage{ctx, out_on_device, {}};
    ScratchBuf in_v, in_t;
    const float* d_vertices = vertices;
    const uint64_t* d_triangles = triangles;
    if (!on_device && T) {
        const uint64_t used = triangles ? n_vertices : std::min<uint64_t>(n_vertices, (uint64_t)3 * T);          // (a soup reads its first 3 T vertices)
        HIP_TRY(ctx, in_v.ensure(std::max<size_t>((size_t)used * 12, 4)));
        HIP_TRY(ctx, hipMemcpyAsync(in_v.p, vertices, (size_t)used * 12, hipMemcpyHostToDevice, st));
        d_vertices = (const float*)in_v.p;
        if (triangles) {
            HIP_TRY(ctx, in_t.ensure((size_t)T * 24));
            HIP_TRY(ctx, hipMemcpyAsync(in_t.p, triangles, (size_t)T * 24, hipMemcpyHostToDevice, st));
            d_triangles = (const uint64_t*)in_t.p;
        }
    }
    hipError_t e = hipSuccess;
    uint64_t* const d_out = (uint64_t*)stage.out(ctx->io_b, out, (size_t)n_words * 8, e); HIP_TRY(ctx, e);
    // one buffer: the exit plane and the counters; the records (16-byte aligned); the column counts, their two rows of sums, the wrap
    // flags and the scans' block totals
    const size_t n_counters = (size_t)fhm::FH_TV_SLOTS * fhm::FH_TV_COUNTERS;          // rows of counters, summed below
    const size_t head_bytes = ((size_t)(n_exit + n_counters) * 8 + 15) / 16 * 16, record_bytes = (size_t)T * sizeof(fhtv::Tri);
    const size_t sum_bytes = T ? (((size_t)T + 1) * 4 + ctr_scan_words(T) + 1) * 4 : 0;
    HIP_TRY(ctx, ctx->mesh_leaves.ensure(head_bytes + record_bytes + sum_bytes));
    uint64_t* const d_exit = (uint64_t*)ctx->mesh_leaves.p;
    uint64_t* const d_counters = d_exit + n_exit;
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, (size_t)n_words * 8, st));
    HIP_TRY(ctx, hipMemsetAsync(d_exit, 0, (size_t)(n_exit + n_counters) * 8, st));
    HIP_TRY(ctx, times.mark("clear"));
    uint64_t W = 0;
    if (T) {
        fhtv::Tri* const records = (fhtv::Tri*)((char*)ctx->mesh_leaves.p + head_bytes);
        uint32_t* const columns = (uint32_t*)((char*)ctx->mesh_leaves.p + head_bytes + record_bytes);
        uint32_t* const low = columns + (size_t)T + 1;
        uint32_t* const high = low + (size_t)T + 1;
        uint32_t* const wrapped = high + (size_t)T + 1;
        uint32_t* const scan_tmp = wrapped + (size_t)T + 1;
        fhm::FhTvTransform M;
        memset(&M, 0, sizeof(M));
        if (mesh_to_world) { memcpy(M.m, mesh_to_world, sizeof(M.m)); M.present = 1; }
        hipLaunchKernelGGL(fhm::k_tv_setup, dim3((unsigned)(((uint64_t)T + 255) / 256)), dim3(256), 0, st, d_vertices, n_vertices, d_triangles, T, M, depth,
                           records, columns, d_counters);
        HIP_TRY(ctx, times.mark("k_tv_setup"));
        HIP_TRY(ctx, ctr_scan(st, columns, T, low, scan_tmp));
        hipLaunchKernelGGL(fhm::k_tv_wraps, dim3((unsigned)(((uint64_t)T + 255) / 256)), dim3(256), 0, st, (const uint32_t*)low, T, wrapped);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, ctr_scan(st, (const uint32_t*)wrapped, T, high, scan_tmp));          // (the same block totals' room: the stream keeps the two in order)
        HIP_TRY(ctx, times.mark("scans"));
        uint32_t w_low = 0, w_high = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&w_low, low + T, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&w_high, high + T, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        W = ((uint64_t)w_high << 32) | w_low;
        if (W >= (1ull << 40)) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh to voxels: 2^40 columns under the triangles' boxes and more");
        if (W) {
            // equal shares of whole 64 items to the waves of at most FH_TV_CROSS_BLOCKS blocks; no block without an item
            const uint64_t waves = std::min<uint64_t>((W + 63) / 64, (uint64_t)4 * fhm::FH_TV_CROSS_BLOCKS);
            const uint64_t per_wave = ((W + waves - 1) / waves + 63) / 64 * 64;
            const uint32_t nb = (uint32_t)(((W + per_wave - 1) / per_wave + 3) / 4);
            hipLaunchKernelGGL(fhm::k_tv_cross, dim3(nb), dim3(256), 0, st, (const fhtv::Tri*)records, (const uint32_t*)low, (const uint32_t*)high, T, W, per_wave, depth,
                               d_out, d_exit, d_counters);
            HIP_TRY(ctx, times.mark("k_tv_cross"));
        }
        // (an empty bitmap is its own prefix XOR, but the open rows of crossings that were all clipped are still counted)
        const uint64_t waves = depth < 6 ? (n_words + 63) / 64 : (uint64_t)B * B;
        hipLaunchKernelGGL(fhm::k_tv_fill, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, d_out, (const uint64_t*)d_exit, depth, d_counters);
        HIP_TRY(ctx, times.mark("k_tv_fill"));
    }
    std::vector<uint64_t> rows(n_counters);
    HIP_TRY(ctx, hipMemcpyAsync(rows.data(), d_counters, n_counters * 8, hipMemcpyDeviceToHost, st));
    { const fhip_status s = stage.finish(); if (s) return s; }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    uint64_t c[fhm::FH_TV_COUNTERS] = {};
    for (size_t r = 0; r < n_counters; r++) c[r % fhm::FH_TV_COUNTERS] += rows[r];
    info[0] = T; info[1] = c[fhm::FH_TV_REJECTED]; info[2] = c[fhm::FH_TV_FLAT]; info[3] = c[fhm::FH_TV_CROSSINGS]; info[4] = c[fhm::FH_TV_CLIPPED];
    info[5] = c[fhm::FH_TV_OPEN]; info[6] = c[fhm::FH_TV_SET]; info[7] = W;
    return FHIP_OK;
}
fhip_status fhip_mesh_voxels(fhip_ctx* ctx, const fhip_mesh* mesh, const double* mesh_to_world, uint32_t depth, uint64_t* out, int out_on_device, uint64_t info[8]) {
    if (!ctx || !mesh) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_mesh_voxels: context and mesh");
    const uint64_t nv = mesh->vertices.size(), nt = mesh->triangles.size();
    if (mesh->d_vertices && mesh->d_triangles)          // resident (fhip_mesh_vertices_dev): read where they are
        return fhip_triangles_voxels(ctx, (const float*)mesh->d_vertices, nv, mesh->d_triangles, nt, 1, mesh_to_world, depth, out, out_on_device, info);
    return fhip_triangles_voxels(ctx, (const float*)mesh->vertices.data(), nv, (const uint64_t*)mesh->triangles.data(), nt, 0, mesh_to_world, depth, out, out_on_device, info);
}
