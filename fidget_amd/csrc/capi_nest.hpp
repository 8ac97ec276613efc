// ---- the nesting of a voxel bitmap's outlines -----------------------------------------------------------------------------------------------
// fhip_outlines_nesting (fidget_hip.h; the handle it declares void* is a fhip_nesting): the passes of nest.hip on the context's stream over
// the arrays of a fhip_outlines (capi_outline.hpp) - xy and loop_of where they are on the device, the loops' leaders and area2 and the
// layers' ranges sent up from the handle's host tables - and the bitmap that was outlined, by voxels_in's convention.  The number of
// doubling rounds comes from loop_start alone, so the host waits once, at the end: the call blocks, as fhip_voxels_outlines does.
// parent and depth stay on the device with the handle; everything is also on the host.  fhip_nesting_children is host code alone.
// A fragment of the C ABI, included by capi_mesh.hpp after capi_outline.hpp; uses capi_mesh_util.hpp.
struct fhip_nesting {
    int device = 0;
    uint32_t k0 = 0, conn = 0;
    uint64_t n_loops = 0, n_layers = 0, n_outer = 0, n_top = 0, max_depth = 0;
    uint32_t *d_parent = nullptr, *d_depth = nullptr;
    std::vector<uint32_t> left, parent, depth, n_children, layer_max_depth;
    std::vector<int64_t> region_area2;
    std::vector<uint64_t> layer_outer, layer_top;
    ~fhip_nesting() {
        if (d_parent) (void)hipFree(d_parent);
        if (d_depth) (void)hipFree(d_depth);
    }
};
fhip_status fhip_outlines_nesting(fhip_ctx* ctx, const void* outlines, const uint64_t* bricks, int bricks_on_device, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !out || !outlines) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_outlines_nesting: context, outlines and result");
    if (!bricks) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_outlines_nesting: the bitmap");
    const fhip_outlines* const o = (const fhip_outlines*)outlines;
    if (o->device != ctx->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_outlines_nesting: the outlines are another device's");
    uint32_t depth = 0;
    while ((4u << depth) < o->N) depth++;
    std::unique_ptr<fhip_nesting> R(new fhip_nesting());
    R->device = ctx->device; R->k0 = o->k0; R->conn = o->conn;
    const uint32_t K = (uint32_t)o->n_layers, n = (uint32_t)o->n_loops;
    R->n_layers = K; R->n_loops = n;
    R->layer_outer.assign(K, 0); R->layer_top.assign(K, 0); R->layer_max_depth.assign(K, 0);
    if (n == 0) { *out = R.release(); return FHIP_OK; }          // no layers, or empty ones: no arrays
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    FxStage stage{ctx, bricks_on_device, {}};
    const uint64_t* d_bricks = nullptr;
    { const fhip_status s = voxels_in(ctx, stage, bricks, depth, d_bricks); if (s) return s; }
    // what goes up, in one piece: area2 i64 [n]; leader u32 [n]; loop_start, vertex_start u32 [K + 1] (ids are below 2^32)
    uint64_t largest = 0;
    for (uint32_t l = 0; l < K; l++) largest = std::max(largest, o->loop_start[l + 1] - o->loop_start[l]);
    const uint32_t rounds = fhnest::rounds(largest);
    const size_t S = n, in_bytes = S * 12 + 2 * ((size_t)K + 1) * 4;
    std::vector<uint8_t> up(in_bytes);
    memcpy(up.data(), o->loop_area2.data(), S * 8);
    memcpy(up.data() + S * 8, o->loop_leader.data(), S * 4);
    uint32_t* const starts = (uint32_t*)(up.data() + S * 12);
    for (uint32_t l = 0; l <= K; l++) { starts[l] = (uint32_t)o->loop_start[l]; starts[(size_t)K + 1 + l] = (uint32_t)o->vertex_start[l]; }
    // the work: the input; left, the second buffer of the links and of the hops, the ancestors' two, u32 [n] each; then what k_on_sums adds up,
    // cleared as one piece: region_area2 i64 [n], outer, top u64 [K], n_children u32 [n], max_depth u32 [K]
    const size_t sums_bytes = S * 8 + (size_t)K * 16 + S * 4 + (size_t)K * 4, work_at = (in_bytes + 7) / 8 * 8, sums_at = (work_at + 5 * S * 4 + 7) / 8 * 8;
    ScratchBuf work;
    HIP_TRY(ctx, work.ensure(sums_at + sums_bytes));
    uint8_t* const w = (uint8_t*)work.p;
    HIP_TRY(ctx, hipMemcpyAsync(w, up.data(), in_bytes, hipMemcpyHostToDevice, st));
    fhm::OnLoops L;
    L.area2 = (const int64_t*)w;
    L.leader = (const uint32_t*)(w + S * 8);
    L.loop_start = L.leader + S;
    L.vertex_start = L.loop_start + K + 1;
    L.n = n; L.K = K; L.k0 = o->k0;
    uint32_t* const d_left = (uint32_t*)(w + work_at);
    uint32_t* const other_link = d_left + S;
    uint32_t* const other_hops = other_link + S;
    uint32_t* anc[2] = {other_hops + S, other_hops + 2 * S};
    uint8_t* const sums = w + sums_at;
    fhm::OnSums T;
    T.region_area2 = (unsigned long long*)sums;
    T.outer = T.region_area2 + S;
    T.top = T.outer + K;
    T.n_children = (uint32_t*)(T.top + K);
    T.max_depth = T.n_children + S;
    HIP_TRY(ctx, hipMemsetAsync(sums, 0, sums_bytes, st));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_parent, S * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_depth, S * 4));
    // a doubling round reads one buffer and writes the other; the buffers are ordered so that the last round writes the handle's array
    uint32_t* link[2] = {(rounds & 1u) ? other_link : R->d_parent, (rounds & 1u) ? R->d_parent : other_link};
    uint32_t* hops[2] = {(rounds & 1u) ? other_hops : R->d_depth, (rounds & 1u) ? R->d_depth : other_hops};
    hipLaunchKernelGGL(fhm::k_on_left, cc_grid(n), dim3(256), 0, st, d_bricks, depth, (const uint32_t*)o->d_xy, (const uint32_t*)o->d_loop, L, d_left, link[0]);
    HIP_TRY(ctx, hipGetLastError());
    for (uint32_t r = 0; r < rounds; r++)
        hipLaunchKernelGGL(fhm::k_on_resolve, cc_grid(n), dim3(256), 0, st, (const uint32_t*)link[r & 1u], L.area2, n, link[(r + 1) & 1u]);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_on_depth0, cc_grid(n), dim3(256), 0, st, (const uint32_t*)R->d_parent, n, anc[0], hops[0]);
    for (uint32_t r = 0; r < rounds; r++)
        hipLaunchKernelGGL(fhm::k_on_depth, cc_grid(n), dim3(256), 0, st, (const uint32_t*)anc[r & 1u], (const uint32_t*)hops[r & 1u], n, anc[(r + 1) & 1u], hops[(r + 1) & 1u]);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fhm::k_on_sums, cc_grid(n), dim3(256), 0, st, L, (const uint32_t*)R->d_parent, (const uint32_t*)R->d_depth, T);
    HIP_TRY(ctx, hipGetLastError());
    R->left.resize(S); R->parent.resize(S); R->depth.resize(S); R->n_children.resize(S); R->region_area2.resize(S);
    std::vector<uint8_t> host(sums_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(R->left.data(), d_left, S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(R->parent.data(), R->d_parent, S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(R->depth.data(), R->d_depth, S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), sums, sums_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    memcpy(R->region_area2.data(), host.data(), S * 8);
    memcpy(R->layer_outer.data(), host.data() + S * 8, (size_t)K * 8);
    memcpy(R->layer_top.data(), host.data() + S * 8 + (size_t)K * 8, (size_t)K * 8);
    memcpy(R->n_children.data(), host.data() + S * 8 + (size_t)K * 16, S * 4);
    memcpy(R->layer_max_depth.data(), host.data() + S * 8 + (size_t)K * 16 + S * 4, (size_t)K * 4);
    for (uint32_t l = 0; l < K; l++) {
        R->n_outer += R->layer_outer[l];
        R->n_top += R->layer_top[l];
        R->max_depth = std::max<uint64_t>(R->max_depth, R->layer_max_depth[l]);
    }
    *out = R.release();
    return FHIP_OK;
}
void fhip_nesting_counts(const void* h, uint64_t out[8]) {
    const fhip_nesting* const t = (const fhip_nesting*)h;
    const uint64_t c[8] = {t ? t->n_loops : 0, t ? t->n_outer : 0, t ? t->n_top : 0, t ? t->max_depth : 0, t ? t->n_layers : 0, t ? t->k0 : 0, t ? t->conn : 0, 0};
    for (int k = 0; k < 8; k++) out[k] = c[k];
}
fhip_status fhip_nesting_layers(const void* h, uint64_t* outer, uint64_t* top, uint32_t* max_depth) {
    const fhip_nesting* const t = (const fhip_nesting*)h;
    if (!t) return FHIP_ERR_BAD_TAPE;
    const size_t K = (size_t)t->n_layers;
    if (outer && K) memcpy(outer, t->layer_outer.data(), K * 8);
    if (top && K) memcpy(top, t->layer_top.data(), K * 8);
    if (max_depth && K) memcpy(max_depth, t->layer_max_depth.data(), K * 4);
    return FHIP_OK;
}
fhip_status fhip_nesting_loops(const void* h, uint64_t first, uint64_t count, uint32_t* left, uint32_t* parent, uint32_t* depth, uint32_t* n_children,
                               int64_t* region_area2) {
    const fhip_nesting* const t = (const fhip_nesting*)h;
    if (!t) return FHIP_ERR_BAD_TAPE;
    if (first > t->n_loops || count > t->n_loops - first) return FHIP_ERR_UNSUPPORTED;
    if (count == 0) return FHIP_OK;
    const size_t f = (size_t)first, c = (size_t)count;
    if (left) memcpy(left, t->left.data() + f, c * 4);
    if (parent) memcpy(parent, t->parent.data() + f, c * 4);
    if (depth) memcpy(depth, t->depth.data() + f, c * 4);
    if (n_children) memcpy(n_children, t->n_children.data() + f, c * 4);
    if (region_area2) memcpy(region_area2, t->region_area2.data() + f, c * 8);
    return FHIP_OK;
}
const uint32_t* fhip_nesting_parent_dev(const void* h) { return HANDLE_GET(fhip_nesting, h, d_parent); }
const uint32_t* fhip_nesting_depth_dev(const void* h) { return HANDLE_GET(fhip_nesting, h, d_depth); }
// the loops by parent as CSR, a counting sort: children[child_start[p] .. child_start[p + 1]) ascend; loops without a parent are in no list
fhip_status fhip_nesting_children(const uint32_t* parent, uint64_t n, uint64_t* child_start, uint32_t* children) {
    if (!child_start || (n && !parent)) return FHIP_ERR_BAD_TAPE;
    for (uint64_t l = 0; l <= n; l++) child_start[l] = 0;
    for (uint64_t l = 0; l < n; l++) {
        if (parent[l] == fhnest::NONE) continue;
        if (parent[l] >= n) return FHIP_ERR_UNSUPPORTED;
        child_start[(size_t)parent[l] + 1]++;
    }
    for (uint64_t l = 0; l < n; l++) child_start[l + 1] += child_start[l];
    if (!children) return child_start[n] ? FHIP_ERR_BAD_TAPE : FHIP_OK;
    std::vector<uint64_t> at(child_start, child_start + n);
    for (uint64_t l = 0; l < n; l++)
        if (parent[l] != fhnest::NONE) children[at[parent[l]]++] = (uint32_t)l;
    return FHIP_OK;
}
void fhip_nesting_free(void* h) { delete (fhip_nesting*)h; }
