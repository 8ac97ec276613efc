// ---- the outlines of a voxel bitmap's layers -----------------------------------------------------------------------------------------------
// fhip_voxels_outlines (fidget_hip.h; the handle it declares void* is a fhip_outlines): the passes of outline.hip on the context's stream
// with the prefix sums of the contours (ctr_scan) between them.  Bricks on the host go through the staging buffer io_a, bricks on the
// device are read in place.  The host waits for the layers' vertex counts - they size the arrays, and 2^32 vertices or more end the
// call there, before anything is written - for the number of loops, which sizes their table, and at the end: the call blocks, as
// fhip_contour2d does.  The vertices' arrays - xy, next, loop_of - are the handle's own device arrays; the loops' table and the layers'
// ranges and sums are on the host.  A fragment of the C ABI, included by capi_mesh.hpp; uses capi_mesh_util.hpp.
struct fhip_outlines {
    int device = 0;
    uint32_t N = 0, k0 = 0, conn = 0;
    uint64_t n_vertices = 0, n_loops = 0, n_layers = 0;
    uint32_t *d_xy = nullptr, *d_next = nullptr, *d_loop = nullptr;
    std::vector<uint64_t> vertex_start{0}, loop_start{0}, layer_perimeter, loop_perimeter;
    std::vector<int64_t> layer_area2, loop_area2;
    std::vector<uint32_t> loop_leader, loop_n;
    std::vector<uint16_t> loop_lo, loop_hi;
    ~fhip_outlines() {
        if (d_xy) (void)hipFree(d_xy);
        if (d_next) (void)hipFree(d_next);
        if (d_loop) (void)hipFree(d_loop);
    }
};
fhip_status fhip_voxels_outlines(fhip_ctx* ctx, const uint64_t* bricks, uint32_t depth, int on_device, uint32_t k0, uint32_t k1, uint32_t connectivity, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_voxels_outlines: context and result");
    if (depth > fhvox::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel depth above 10");
    const uint32_t N = 4u << depth;
    if (k0 > k1 || k1 > N) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel outlines: layers k0 <= k1 <= 4 << depth");
    if (!fhol::conn_ok(connectivity)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel outlines: connectivity 4 or 8");
    std::unique_ptr<fhip_outlines> R(new fhip_outlines());
    R->device = ctx->device; R->N = N; R->k0 = k0; R->conn = connectivity;
    const uint32_t K = k1 - k0;
    if (K == 0) { *out = R.release(); return FHIP_OK; }
    if (!bricks) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_voxels_outlines: the bitmap");
    R->n_layers = K;
    R->vertex_start.assign((size_t)K + 1, 0); R->loop_start.assign((size_t)K + 1, 0);
    R->layer_area2.assign(K, 0); R->layer_perimeter.assign(K, 0);
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    FxStage stage{ctx, on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, stage, bricks, depth, d_bricks); if (s) return s; }
    const uint64_t n_entries = (uint64_t)K * (N + 1) * fhol::n_chunks(depth);          // (at most 4096 * 4097 * 129 < 2^32)
    ScratchBuf counts, bases, per_layer, scan_tmp;
    HIP_TRY(ctx, counts.ensure((size_t)n_entries * 4));
    HIP_TRY(ctx, bases.ensure(((size_t)n_entries + 1) * 4));
    HIP_TRY(ctx, per_layer.ensure((size_t)K * 8));
    HIP_TRY(ctx, scan_tmp.ensure((ctr_scan_words((uint32_t)n_entries) + 1) * 4));
    uint32_t* const cnt = (uint32_t*)counts.p;
    uint32_t* const base = (uint32_t*)bases.p;
    hipLaunchKernelGGL(fhm::k_ol_count, cc_grid(n_entries), dim3(256), 0, st, d_bricks, depth, k0, K, cnt);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_ol_layers, dim3(K), dim3(256), 0, st, (const uint32_t*)cnt, depth, (unsigned long long*)per_layer.p);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint64_t> layer_n(K);
    HIP_TRY(ctx, hipMemcpyAsync(layer_n.data(), per_layer.p, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (uint32_t l = 0; l < K; l++) R->vertex_start[l + 1] = R->vertex_start[l] + layer_n[l];
    const uint64_t n = R->vertex_start[K];
    if (n > fhol::MAX_VERTICES) return fail(ctx, FHIP_ERR_OVERFLOW, "voxel outlines: 2^32 vertices or more");
    R->n_vertices = n;
    if (n == 0) { *out = R.release(); return FHIP_OK; }          // empty layers: no arrays
    HIP_TRY(ctx, ctr_scan(st, cnt, (uint32_t)n_entries, base, (uint32_t*)scan_tmp.p));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_xy, (size_t)n * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_next, (size_t)n * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_loop, (size_t)n * 4));
    hipLaunchKernelGGL(fhm::k_ol_emit, cc_grid(n_entries), dim3(256), 0, st, d_bricks, depth, k0, K, connectivity, (const uint32_t*)base, R->d_xy, R->d_next);
    HIP_TRY(ctx, hipGetLastError());
    // the loops: parent [n], the roots' ranks [n + 1]; the flags, and then the loops in their place, are the handle's array
    ScratchBuf node_tmp, scan_tmp2;
    HIP_TRY(ctx, node_tmp.ensure(((size_t)2 * n + 1) * 4));
    HIP_TRY(ctx, scan_tmp2.ensure((ctr_scan_words((uint32_t)n) + 1) * 4));
    uint32_t* const parent = (uint32_t*)node_tmp.p;
    uint32_t* const rank = parent + n;
    hipLaunchKernelGGL(fhm::k_cc_init, cc_grid(n), dim3(256), 0, st, parent, n);
    hipLaunchKernelGGL(fhm::k_ol_unite, cc_grid(n), dim3(256), 0, st, (const uint32_t*)R->d_next, (uint32_t)n, parent);
    hipLaunchKernelGGL(fhm::k_cc_flatten, cc_grid(n), dim3(256), 0, st, parent, n);
    hipLaunchKernelGGL(fhm::k_cc_roots, cc_grid(n), dim3(256), 0, st, (const uint32_t*)parent, n, R->d_loop);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctr_scan(st, R->d_loop, (uint32_t)n, rank, (uint32_t*)scan_tmp2.p));
    hipLaunchKernelGGL(fhm::k_cc_number, cc_grid(n), dim3(256), 0, st, (const uint32_t*)parent, (const uint32_t*)rank, n, R->d_loop);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t n_loops = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_loops, rank + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    R->n_loops = n_loops;
    // the loops' table on the device: area2, perimeter u64 [s]; n_vertices, leader u32 [s]; lo, hi u32 [s][2]
    ScratchBuf table;
    const size_t S = n_loops, table_bytes = S * (2 * 8 + 6 * 4);
    HIP_TRY(ctx, table.ensure(table_bytes));
    fhm::OlLoopTable tab;
    tab.area2 = (unsigned long long*)table.p;
    tab.perimeter = tab.area2 + S;
    tab.n_vertices = (uint32_t*)(tab.perimeter + S);
    tab.leader = tab.n_vertices + S;
    tab.lo = tab.leader + S;
    tab.hi = tab.lo + 2 * S;
    HIP_TRY(ctx, hipMemsetAsync(table.p, 0, table_bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(tab.lo, 0xFF, 2 * S * 4, st));
    hipLaunchKernelGGL(fhm::k_ol_measure, cc_grid(n), dim3(256), 0, st, (const uint32_t*)R->d_xy, (const uint32_t*)R->d_next, (const uint32_t*)parent,
                       (const uint32_t*)R->d_loop, (uint32_t)n, tab);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint8_t> host(table_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), table.p, table_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    R->loop_area2.resize(S); R->loop_perimeter.resize(S); R->loop_n.resize(S); R->loop_leader.resize(S); R->loop_lo.resize(2 * S); R->loop_hi.resize(2 * S);
    memcpy(R->loop_area2.data(), host.data(), S * 8);
    memcpy(R->loop_perimeter.data(), host.data() + S * 8, S * 8);
    memcpy(R->loop_n.data(), host.data() + S * 16, S * 4);
    memcpy(R->loop_leader.data(), host.data() + S * 20, S * 4);
    const uint32_t* const lo = (const uint32_t*)(host.data() + S * 24);
    const uint32_t* const hi = lo + 2 * S;
    for (size_t q = 0; q < 2 * S; q++) { R->loop_lo[q] = (uint16_t)lo[q]; R->loop_hi[q] = (uint16_t)hi[q]; }
    // a layer's loops: those whose leaders are its vertices - leaders ascend with the loops
    for (uint32_t l = 0; l <= K; l++)
        R->loop_start[l] = (uint64_t)(std::lower_bound(R->loop_leader.begin(), R->loop_leader.end(), R->vertex_start[l], [](uint32_t a, uint64_t b) { return a < b; }) - R->loop_leader.begin());
    for (uint32_t l = 0; l < K; l++)
        for (uint64_t q = R->loop_start[l]; q < R->loop_start[l + 1]; q++) { R->layer_area2[l] += R->loop_area2[q]; R->layer_perimeter[l] += R->loop_perimeter[q]; }
    *out = R.release();
    return FHIP_OK;
}
void fhip_outlines_counts(const void* h, uint64_t out[8]) {
    const fhip_outlines* const o = (const fhip_outlines*)h;
    const uint64_t c[8] = {o ? o->n_vertices : 0, o ? o->n_loops : 0, o ? o->n_layers : 0, o ? o->N : 0, o ? o->k0 : 0, o ? o->conn : 0, 0, 0};
    for (int k = 0; k < 8; k++) out[k] = c[k];
}
fhip_status fhip_outlines_layers(const void* h, uint64_t* vertex_start, uint64_t* loop_start, int64_t* area2, uint64_t* perimeter) {
    const fhip_outlines* const o = (const fhip_outlines*)h;
    if (!o) return FHIP_ERR_BAD_TAPE;
    const size_t K = (size_t)o->n_layers;
    if (vertex_start) memcpy(vertex_start, o->vertex_start.data(), (K + 1) * 8);
    if (loop_start) memcpy(loop_start, o->loop_start.data(), (K + 1) * 8);
    if (area2 && K) memcpy(area2, o->layer_area2.data(), K * 8);
    if (perimeter && K) memcpy(perimeter, o->layer_perimeter.data(), K * 8);
    return FHIP_OK;
}
fhip_status fhip_outlines_vertices(const void* h, uint64_t first, uint64_t count, uint16_t* xy, uint32_t* next, uint32_t* loop_of) {
    const fhip_outlines* const o = (const fhip_outlines*)h;
    if (!o) return FHIP_ERR_BAD_TAPE;
    if (first > o->n_vertices || count > o->n_vertices - first) return FHIP_ERR_UNSUPPORTED;
    const size_t bytes = (size_t)count * 4;
    if (xy && handle_to_host(o->device, xy, o->d_xy + first, bytes)) return FHIP_ERR_HIP;
    if (next && handle_to_host(o->device, next, o->d_next + first, bytes)) return FHIP_ERR_HIP;
    if (loop_of && handle_to_host(o->device, loop_of, o->d_loop + first, bytes)) return FHIP_ERR_HIP;
    return FHIP_OK;
}
fhip_status fhip_outlines_loops(const void* h, uint64_t first, uint64_t count, uint32_t* leader, uint32_t* n_vertices, int64_t* area2, uint64_t* perimeter, uint16_t* lo,
                                uint16_t* hi) {
    const fhip_outlines* const o = (const fhip_outlines*)h;
    if (!o) return FHIP_ERR_BAD_TAPE;
    if (first > o->n_loops || count > o->n_loops - first) return FHIP_ERR_UNSUPPORTED;
    if (count == 0) return FHIP_OK;
    const size_t f = (size_t)first, c = (size_t)count;
    if (leader) memcpy(leader, o->loop_leader.data() + f, c * 4);
    if (n_vertices) memcpy(n_vertices, o->loop_n.data() + f, c * 4);
    if (area2) memcpy(area2, o->loop_area2.data() + f, c * 8);
    if (perimeter) memcpy(perimeter, o->loop_perimeter.data() + f, c * 8);
    if (lo) memcpy(lo, o->loop_lo.data() + 2 * f, 2 * c * 2);
    if (hi) memcpy(hi, o->loop_hi.data() + 2 * f, 2 * c * 2);
    return FHIP_OK;
}
const uint16_t* fhip_outlines_xy_dev(const void* h) { return (const uint16_t*)HANDLE_GET(fhip_outlines, h, d_xy); }
const uint32_t* fhip_outlines_next_dev(const void* h) { return HANDLE_GET(fhip_outlines, h, d_next); }
const uint32_t* fhip_outlines_loop_dev(const void* h) { return HANDLE_GET(fhip_outlines, h, d_loop); }
void fhip_outlines_free(void* h) { delete (fhip_outlines*)h; }
