// ---- connected components of a voxel bitmap --------------------------------------------------------------------------------------------------
// fhip_voxels_components (fidget_hip.h; the handle it declares void* is a fhip_components): the k_cc_* passes of mesh.hip with the prefix sums
// of the contours between them, all on the context's stream.  The host waits twice on the way - for the number of nodes, which sizes their
// arrays, and for the number of components, which sizes the table - and once at the end.  FHIP_MESH_TIMES: the passes' wall times on stderr.
// A fragment of the C ABI, included by capi_mesh.hpp; uses capi_mesh_util.hpp.
struct fhip_components {
    uint64_t n_comps = 0, n_nodes = 0, n_voxels = 0;
    uint32_t depth = 0, conn = 6;
    int complement = 0, device = 0;
    uint32_t* d_base = nullptr;          // [B^3 + 1]: a brick's first node
    uint32_t* d_comp = nullptr;          // [n_nodes]: a node's component
    std::vector<uint64_t> size;          // the table, on the host
    std::vector<uint32_t> seed, lo, hi;
    std::vector<uint8_t> border;
    ~fhip_components() {
        if (d_base) (void)hipFree(d_base);
        if (d_comp) (void)hipFree(d_comp);
    }
};
fhip_status fhip_voxels_components(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t connectivity, int complement, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_components: context and result");
    if (!fhcc::conn_ok(connectivity)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "components: connectivity 6 or 26");
    { const fhip_status s = bitmap_args(ctx, "fhip_voxels_components: the bitmap", depth, bricks); if (s) return s; }
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    FxStage stage{ctx, on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, stage, bricks, depth, d_bricks); if (s) return s; }
    PassTimes times(st, "fhip components depth %u conn %u%s", depth, connectivity, complement ? " complement" : "");
    std::unique_ptr<fhip_components> R(new fhip_components());
    R->depth = depth; R->conn = connectivity; R->complement = complement ? 1 : 0; R->device = ctx->device;
    const uint64_t n_words = fhvox::n_words(depth), flip = complement ? ~(uint64_t)0 : 0;
    HIP_TRY(ctx, hipMalloc((void**)&R->d_base, (size_t)(n_words + 1) * 4));
    ScratchBuf counts, node_tmp, scan_tmp, scan_tmp2;
    HIP_TRY(ctx, counts.ensure((size_t)n_words * 4 + 24));          // the bricks' node counts, then the two totals
    HIP_TRY(ctx, scan_tmp.ensure((ctr_scan_words((uint32_t)n_words) + 1) * 4));
    uint32_t* const cnt = (uint32_t*)counts.p;
    unsigned long long* const totals = (unsigned long long*)((char*)counts.p + (((size_t)n_words * 4 + 7) & ~(size_t)7));
    HIP_TRY(ctx, hipMemsetAsync(totals, 0, 16, st));
    HIP_TRY(ctx, times.mark(nullptr));
    hipLaunchKernelGGL(fhm::k_cc_count, cc_grid(n_words), dim3(256), 0, st, d_bricks, n_words, flip, connectivity, cnt, totals);
    HIP_TRY(ctx, times.mark("k_cc_count"));
    uint64_t tot[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(tot, totals, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (tot[0] > 0xFFFFFFFEull) return fail(ctx, FHIP_ERR_OVERFLOW, "components: more than 2^32 - 2 nodes (the bricks' own components)");
    const uint64_t n_nodes = tot[0];
    R->n_nodes = n_nodes; R->n_voxels = tot[1];
    HIP_TRY(ctx, ctr_scan(st, cnt, (uint32_t)n_words, R->d_base, (uint32_t*)scan_tmp.p));
    HIP_TRY(ctx, times.mark("scan (base)"));
    if (n_nodes == 0) {         // an empty foreground: no components, and the later calls find no set bit to look up
        HIP_TRY(ctx, hipStreamSynchronize(st));
        *out = R.release();
        return FHIP_OK;
    }
    // parent [n_nodes], the roots' ranks [n_nodes + 1]; the flags, and then the components in their place, are the handle's array
    HIP_TRY(ctx, hipMalloc((void**)&R->d_comp, (size_t)n_nodes * 4));
    HIP_TRY(ctx, node_tmp.ensure(((size_t)2 * n_nodes + 1) * 4));
    HIP_TRY(ctx, scan_tmp2.ensure((ctr_scan_words((uint32_t)n_nodes) + 1) * 4));
    uint32_t* const parent = (uint32_t*)node_tmp.p;
    uint32_t* const rank = parent + n_nodes;
    hipLaunchKernelGGL(fhm::k_cc_init, cc_grid(n_nodes), dim3(256), 0, st, parent, n_nodes);
    HIP_TRY(ctx, times.mark("k_cc_init"));
    hipLaunchKernelGGL(fhm::k_cc_merge, cc_grid(n_words), dim3(256), 0, st, d_bricks, depth, flip, connectivity, (const uint32_t*)R->d_base, parent);
    HIP_TRY(ctx, times.mark("k_cc_merge"));
    hipLaunchKernelGGL(fhm::k_cc_flatten, cc_grid(n_nodes), dim3(256), 0, st, parent, n_nodes);
    HIP_TRY(ctx, times.mark("k_cc_flatten"));
    hipLaunchKernelGGL(fhm::k_cc_roots, cc_grid(n_nodes), dim3(256), 0, st, (const uint32_t*)parent, n_nodes, R->d_comp);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctr_scan(st, R->d_comp, (uint32_t)n_nodes, rank, (uint32_t*)scan_tmp2.p));
    hipLaunchKernelGGL(fhm::k_cc_number, cc_grid(n_nodes), dim3(256), 0, st, (const uint32_t*)parent, (const uint32_t*)rank, n_nodes, R->d_comp);
    HIP_TRY(ctx, times.mark("roots+scan+number"));
    uint32_t n_comps = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_comps, rank + n_nodes, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    R->n_comps = n_comps;
    // the table on the device: size u64 [c], then lo, hi, seed u32 [c][3] and border u32 [c]
    ScratchBuf table;
    const size_t c = n_comps, table_bytes = c * 8 + c * 10 * 4;
    HIP_TRY(ctx, table.ensure(table_bytes));
    unsigned long long* const d_size = (unsigned long long*)table.p;
    uint32_t* const d_lo = (uint32_t*)(d_size + c);
    uint32_t* const d_hi = d_lo + 3 * c;
    uint32_t* const d_seed = d_hi + 3 * c;
    uint32_t* const d_border = d_seed + 3 * c;
    HIP_TRY(ctx, hipMemsetAsync(table.p, 0, table_bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(d_lo, 0xFF, 3 * c * 4, st));
    HIP_TRY(ctx, times.mark(nullptr));
    hipLaunchKernelGGL(fhm::k_cc_table, cc_grid(n_words), dim3(256), 0, st, d_bricks, depth, flip, connectivity, (const uint32_t*)R->d_base, (const uint32_t*)R->d_comp,
                       (const uint32_t*)parent, d_size, d_lo, d_hi, d_border, d_seed);
    HIP_TRY(ctx, times.mark("k_cc_table"));
    std::vector<uint8_t> host(table_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), table.p, table_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    R->size.resize(c); R->lo.resize(3 * c); R->hi.resize(3 * c); R->seed.resize(3 * c); R->border.resize(c);
    memcpy(R->size.data(), host.data(), c * 8);
    memcpy(R->lo.data(), host.data() + c * 8, 3 * c * 4);
    memcpy(R->hi.data(), host.data() + c * 8 + 3 * c * 4, 3 * c * 4);
    memcpy(R->seed.data(), host.data() + c * 8 + 6 * c * 4, 3 * c * 4);
    const uint32_t* const hb = (const uint32_t*)(host.data() + c * 8 + 9 * c * 4);
    for (size_t k = 0; k < c; k++) R->border[k] = hb[k] ? 1 : 0;
    *out = R.release();
    return FHIP_OK;
}
void fhip_components_counts(const void* h, uint64_t out[4]) {
    const fhip_components* const c = (const fhip_components*)h;
    out[0] = c ? c->n_comps : 0; out[1] = c ? c->n_nodes : 0; out[2] = c ? c->n_voxels : 0; out[3] = c ? c->depth : 0;
}
fhip_status fhip_components_table(const void* h, uint64_t* size, uint32_t* seed, uint32_t* lo, uint32_t* hi, uint8_t* border) {
    const fhip_components* const c = (const fhip_components*)h;
    if (!c) return FHIP_ERR_BAD_TAPE;
    const size_t n = (size_t)c->n_comps;
    if (n == 0) return FHIP_OK;
    if (size) memcpy(size, c->size.data(), n * 8);
    if (seed) memcpy(seed, c->seed.data(), 3 * n * 4);
    if (lo) memcpy(lo, c->lo.data(), 3 * n * 4);
    if (hi) memcpy(hi, c->hi.data(), 3 * n * 4);
    if (border) memcpy(border, c->border.data(), n);
    return FHIP_OK;
}
fhip_status fhip_components_label_slices(fhip_ctx* ctx, const void* h, const uint64_t* bricks, int bricks_on_device, uint32_t k0, uint32_t k1, int32_t* out, int out_on_device) {
    const fhip_components* const c = (const fhip_components*)h;
    if (!ctx || !c) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_components_label_slices: context and components");
    if (ctx->device != c->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "components: labelled on another device");
    const uint32_t N = 4u << c->depth;
    if (k0 > k1 || k1 > N) return fail(ctx, FHIP_ERR_UNSUPPORTED, "label slices: layers k0 <= k1 <= 4 << depth");
    if (c->n_comps > 0x7FFFFFFFull) return fail(ctx, FHIP_ERR_UNSUPPORTED, "label slices: more than 2^31 - 1 components do not fit an int32 image");
    if (k0 == k1) return FHIP_OK;
    if (!bricks || !out) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_components_label_slices: bitmap and output buffer");
    if (out_on_device && ((uintptr_t)out & 15u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "label slices to the device: the buffer must be 16-byte aligned");
    (void)hipSetDevice(ctx->device);
    FxStage in{ctx, bricks_on_device, {}}, st{ctx, out_on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, in, bricks, c->depth, d_bricks); if (s) return s; }
    hipError_t e = hipSuccess;
    int32_t* const d_out = (int32_t*)st.out(ctx->io_b, out, (size_t)(k1 - k0) * N * N * 4, e); HIP_TRY(ctx, e);
    const uint64_t runs = ((uint64_t)(k1 - k0) * N) << (c->depth < 2 ? 0 : c->depth - 2);
    const uint32_t nb = (uint32_t)std::min<uint64_t>((runs + 255) / 256, fhm::FH_VOX_SLICE_BLOCKS);
    hipLaunchKernelGGL(fhm::k_cc_label_slices, dim3(nb), dim3(256), 0, ctx->stream, d_bricks, c->depth, c->complement ? ~(uint64_t)0 : (uint64_t)0, c->conn,
                       (const uint32_t*)c->d_base, (const uint32_t*)c->d_comp, k0, k1, d_out);
    return st.finish();
}
fhip_status fhip_components_extract(fhip_ctx* ctx, const void* h, const uint64_t* bricks, int bricks_on_device, const uint32_t* ids, uint64_t n_ids, uint64_t* out, int out_on_device) {
    const fhip_components* const c = (const fhip_components*)h;
    if (!ctx || !c) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_components_extract: context and components");
    if (ctx->device != c->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "components: labelled on another device");
    if (!bricks || !out || (n_ids && !ids)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_components_extract: bitmap, ids and output buffer");
    if (out_on_device && ((uintptr_t)out & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "extract to the device: the buffer must be 8-byte aligned");
    std::vector<uint8_t> chosen((size_t)c->n_comps + 1, 0);
    for (uint64_t k = 0; k < n_ids; k++) {
        if (ids[k] >= c->n_comps) return fail(ctx, FHIP_ERR_UNSUPPORTED, "extract: a component id beyond the number of components");
        chosen[ids[k]] = 1;
    }
    (void)hipSetDevice(ctx->device);
    FxStage in{ctx, bricks_on_device, {}}, st{ctx, out_on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, in, bricks, c->depth, d_bricks); if (s) return s; }
    const uint64_t n_words = fhvox::n_words(c->depth);
    hipError_t e = hipSuccess;
    uint64_t* const d_out = (uint64_t*)st.out(ctx->io_b, out, (size_t)n_words * 8, e); HIP_TRY(ctx, e);
    HIP_TRY(ctx, ctx->io_c.ensure(chosen.size()));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->io_c.p, chosen.data(), chosen.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (`chosen` is pageable and leaves with this call)
    hipLaunchKernelGGL(fhm::k_cc_extract, cc_grid(n_words), dim3(256), 0, ctx->stream, d_bricks, n_words, c->complement ? ~(uint64_t)0 : (uint64_t)0, c->conn,
                       (const uint32_t*)c->d_base, (const uint32_t*)c->d_comp, (const uint8_t*)ctx->io_c.p, d_out);
    return st.finish();
}
void fhip_components_free(void* h) { delete (fhip_components*)h; }
