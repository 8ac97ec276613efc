// ---- the boundary mesh of a voxel bitmap ------------------------------------------------------------------------------------------------------
// fhip_voxels_surface and fhip_voxels_mesh (fidget_hip.h): the counting pass of vmesh.hip and its sums; for the mesh, the two prefix sums
// (ctr_scan) and the two emitting passes, all on the context's stream.  The host waits once for the totals - they decide an overflow and
// size the arrays - and once at the end, for the arrays on their way to the host.  A fragment of the C ABI, included by
// capi_mesh.hpp; uses capi_mesh_util.hpp.  FHIP_MESH_TIMES: the passes' wall times on stderr.
static fhip_status vmesh_run(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint64_t sums[fhm::FH_VM_SUMS], fhip_mesh** mesh) {
    { const fhip_status s = bitmap_args(ctx, "the boundary of a voxel bitmap: the bitmap", depth, bricks); if (s) return s; }
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    FxStage stage{ctx, on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, stage, bricks, depth, d_bricks); if (s) return s; }
    PassTimes times(st, "fhip voxel %s depth %u", mesh ? "mesh" : "surface", depth);
    const uint64_t n_words = fhvox::n_words(depth);
    const uint32_t n_corner = (uint32_t)fhvm::n_corner_bricks(depth);
    const uint32_t count_blocks = std::min((n_corner + 255) / 256, fhm::FH_VM_COUNT_BLOCKS);
    // the partial sums and the totals; for the mesh the bricks' face counts and their sums, the corner bricks' flags, vertex counts and sums
    ScratchBuf parts, face_buf, corner_buf, flag_buf, scan_tmp;
    HIP_TRY(ctx, parts.ensure(((size_t)count_blocks + 1) * fhm::FH_VM_SUMS * 8));
    uint64_t* const d_parts = (uint64_t*)parts.p;
    uint64_t* const d_sums = d_parts + (size_t)count_blocks * fhm::FH_VM_SUMS;
    uint32_t *face_count = nullptr, *face_base = nullptr, *vertex_count = nullptr, *vertex_base = nullptr;
    if (mesh) {
        HIP_TRY(ctx, face_buf.ensure(((size_t)2 * n_words + 1) * 4));
        HIP_TRY(ctx, corner_buf.ensure(((size_t)2 * n_corner + 1) * 4));
        HIP_TRY(ctx, flag_buf.ensure((size_t)n_corner * 8));
        HIP_TRY(ctx, scan_tmp.ensure((std::max(ctr_scan_words((uint32_t)n_words), ctr_scan_words(n_corner)) + 1) * 4));
        face_count = (uint32_t*)face_buf.p; face_base = face_count + n_words;
        vertex_count = (uint32_t*)corner_buf.p; vertex_base = vertex_count + n_corner;
    }
    HIP_TRY(ctx, times.mark("allocate"));
    hipLaunchKernelGGL(fhm::k_vm_count, dim3(count_blocks), dim3(256), 0, st, d_bricks, depth, face_count, (uint64_t*)flag_buf.p, vertex_count, d_parts);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_vm_sum, dim3(fhm::FH_VM_SUMS), dim3(256), 0, st, (const uint64_t*)d_parts, count_blocks, d_sums);
    HIP_TRY(ctx, times.mark("k_vm_count"));
    HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, fhm::FH_VM_SUMS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (!mesh) return FHIP_OK;
    const uint64_t n_faces = sums[0] + sums[1] + sums[2] + sums[3] + sums[4] + sums[5], n_verts = sums[6];
    if (2 * n_faces >= (1ull << 32) || n_verts >= (1ull << 32))          // (the prefix sums below are 32-bit and would wrap)
        return fail(ctx, FHIP_ERR_OVERFLOW, "voxel mesh: 2^32 triangles or vertices and more");
    std::unique_ptr<fhip_mesh> M(new fhip_mesh());
    M->depth = depth;
    if (n_faces == 0) { *mesh = M.release(); return FHIP_OK; }
    HIP_TRY(ctx, ctr_scan(st, face_count, (uint32_t)n_words, face_base, (uint32_t*)scan_tmp.p));
    HIP_TRY(ctx, ctr_scan(st, vertex_count, n_corner, vertex_base, (uint32_t*)scan_tmp.p));          // (the same block totals' room: the stream keeps the two in order)
    HIP_TRY(ctx, times.mark("scans"));
    HIP_TRY(ctx, hipMalloc((void**)&M->d_vertices, (size_t)n_verts * sizeof(fhmesh::V3)));
    HIP_TRY(ctx, hipMalloc((void**)&M->d_triangles, (size_t)n_faces * 48));
    HIP_TRY(ctx, times.mark("allocate arrays"));
    hipLaunchKernelGGL(fhm::k_vm_vertices, dim3((n_corner + fhm::FH_VM_PER_BLOCK - 1) / fhm::FH_VM_PER_BLOCK), dim3(256), 0, st, (const uint64_t*)flag_buf.p,
                       (const uint32_t*)vertex_base, depth, M->d_vertices);
    HIP_TRY(ctx, times.mark("k_vm_vertices"));
    hipLaunchKernelGGL(fhm::k_vm_faces, dim3((unsigned)((n_words + fhm::FH_VM_PER_BLOCK - 1) / fhm::FH_VM_PER_BLOCK)), dim3(256), 0, st, d_bricks, depth,
                       (const uint32_t*)face_base, (const uint64_t*)flag_buf.p, (const uint32_t*)vertex_base, M->d_triangles);
    HIP_TRY(ctx, times.mark("k_vm_faces"));
    M->vertices.resize((size_t)n_verts);
    M->triangles.resize((size_t)(2 * n_faces));
    { const fhip_status s = mesh_to_host(ctx, M->vertices.data(), M->d_vertices, (size_t)n_verts * sizeof(fhmesh::V3)); if (s) return s; }
    { const fhip_status s = mesh_to_host(ctx, M->triangles.data(), M->d_triangles, (size_t)n_faces * 48); if (s) return s; }
    HIP_TRY(ctx, times.mark("to the host"));
    *mesh = M.release();
    return FHIP_OK;
}
fhip_status fhip_voxels_surface(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint64_t out[10]) {
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_surface: context and result");
    uint64_t sums[fhm::FH_VM_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const fhip_status s = vmesh_run(ctx, bricks, depth, on_device, sums, nullptr);
    if (s) return s;
    for (uint32_t d = 0; d < 8; d++) out[d] = sums[d];          // faces[6], V, E
    out[8] = sums[0] + sums[1] + sums[2] + sums[3] + sums[4] + sums[5];
    out[9] = sums[8];
    return FHIP_OK;
}
fhip_status fhip_voxels_mesh(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, fhip_mesh** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_mesh: context and result");
    uint64_t sums[fhm::FH_VM_SUMS];
    return vmesh_run(ctx, bricks, depth, on_device, sums, out);
}
