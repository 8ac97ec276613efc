// ---- the slices of a triangle mesh: contour loops per plane -------------------------------------------------------------------------------------
// fhip_topology_slices (fidget_hip.h; the handle it declares void* is a fhip_slices, the topology a fhip_topology of capi_topo.hpp): the
// passes of slice.hip on the context's stream with the prefix sums of the contours (ctr_scan) between them.  The planes are checked on
// the host before anything is launched.  The host waits for the counts of crossing corners and of segments - the first sizes the edge
// table, which a topology does not keep - for the table's verdict and the number of crossings, which sizes the handle's arrays, for the
// number of loops, which sizes their table, and at the end: the call blocks, as fhip_triangles_topology does.  The scratch is carved
// from ctx->mesh_leaves as capi_topo.hpp does, and stays with the context until fhip_ctx_trim: first what the mesh and the planes
// size - the counters, the planes, a level per vertex, per corner a slot and a count with its prefix sum, per triangle the same - then,
// appended as the counts come in, the table and the segments' ends, per crossing a parent, a rank and the words of its successor and
// its degree, and the loops' table; where the buffer has to grow for that, what it holds moves along (SliceScratch::grow).  The
// crossings' arrays are the handle's own device arrays; the loops' table and the planes' counts are on the host.  A fragment of the C
// ABI, included by capi_mesh.hpp; uses capi_mesh_util.hpp and capi_topo.hpp (fhip_topology, TopoCarve).  FHIP_MESH_TIMES: the passes'
// times on stderr (PassTimes).
struct fhip_slices {
    int device = 0;
    uint64_t n_planes = 0, n_crossings = 0, n_segments = 0, n_loops = 0, n_irregular = 0, edge_slots = 0;
    float* d_xy = nullptr;
    uint32_t *d_plane = nullptr, *d_edge = nullptr, *d_next = nullptr, *d_loop = nullptr;
    uint8_t* d_degree = nullptr;
    std::vector<float> zs, loop_lo, loop_hi;
    std::vector<uint64_t> plane_crossings, plane_segments, plane_loops;
    std::vector<uint32_t> loop_leader, loop_plane, loop_crossings, loop_segments, loop_irregular;
    std::vector<double> loop_area2;
    ~fhip_slices() {
        for (void* p : {(void*)d_xy, (void*)d_plane, (void*)d_edge, (void*)d_next, (void*)d_loop, (void*)d_degree})
            if (p) (void)hipFree(p);
    }
};
// The call's pieces of ctx->mesh_leaves, in the order in which their sizes become known; every later piece lies behind the earlier ones
struct SliceScratch {
    uint64_t *counters = nullptr, *table = nullptr, *next_words = nullptr, *degree = nullptr;
    float* zs = nullptr;
    uint32_t *level = nullptr, *corner_slot = nullptr, *count = nullptr, *base = nullptr, *seg_count = nullptr, *seg_base = nullptr, *scan_tmp = nullptr, *segments = nullptr,
             *parent = nullptr, *rank = nullptr, *scan_tmp2 = nullptr;
    char* loops = nullptr;
    size_t bytes = 0;
    void walk(char* p, size_t n_counters, uint32_t P, uint64_t n_rows, uint32_t T, size_t slots, uint64_t m, uint64_t n, size_t loop_bytes) {
        TopoCarve cv;
        cv.p = p;
        const uint32_t C = 3 * T;
        counters = cv.u64(n_counters);
        zs = (float*)cv.u32(P);
        level = cv.u32((size_t)n_rows);
        corner_slot = cv.u32(C);
        count = cv.u32(C);
        base = cv.u32((size_t)C + 1);
        seg_count = cv.u32(T);
        seg_base = cv.u32((size_t)T + 1);
        scan_tmp = cv.u32(ctr_scan_words(C) + 1);
        table = cv.u64(fhtopo::EDGE_SLOT_WORDS * slots);
        segments = cv.u32(2 * (size_t)m);
        next_words = cv.u64((size_t)n);
        degree = cv.u64((size_t)n);
        parent = cv.u32((size_t)n);
        rank = cv.u32((size_t)n + 1);
        scan_tmp2 = cv.u32(ctr_scan_words((uint32_t)n) + 1);
        loops = (char*)cv.take(loop_bytes);
        bytes = cv.at;
    }
    // ctx->mesh_leaves of at least `want` bytes, its first `keep` bytes as they were
    static hipError_t grow(fhip_ctx* ctx, size_t want, size_t keep) {
        DevBuf& b = ctx->mesh_leaves;
        if (want <= b.cap) return hipSuccess;
        if (!keep || !b.p) return b.ensure(want);
        void* fresh = nullptr;
        hipError_t e = hipMalloc(&fresh, want);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(fresh, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipFree(fresh); return e; }
        (void)hipFree(b.p);
        b.p = fresh; b.cap = want;
        return hipSuccess;
    }
};
fhip_status fhip_topology_slices(fhip_ctx* ctx, const void* topology, const float* zs, uint32_t n_planes, uint32_t table_log2, void** out) {
    if (out) *out = nullptr;
    const fhip_topology* const topo = (const fhip_topology*)topology;
    if (!ctx || !topo || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_topology_slices: context, topology and result");
    if (ctx->device != topo->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "topology: made on another device");
    if (topo->counts[TOPO_REJECTED]) return fail(ctx, FHIP_ERR_UNSUPPORTED, "mesh slices: the topology rejected triangles and holds no mesh");
    if (table_log2 > fhtopo::MAX_LOG2) return fail(ctx, FHIP_ERR_UNSUPPORTED, "mesh slices: table_log2 above 32");
    if (n_planes > fhslice::MAX_PLANES) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh slices: more than 2^32 - 2 planes");
    if (n_planes && !zs) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_topology_slices: the planes");
    if (!fhslice::planes_ok(zs, n_planes)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "mesh slices: the planes must be finite and strictly ascending");
    std::unique_ptr<fhip_slices> R(new fhip_slices());
    R->device = ctx->device;
    R->n_planes = n_planes;
    const uint32_t P = n_planes, T = (uint32_t)topo->counts[TOPO_TRIANGLES], C = 3 * T;
    if (P) R->zs.assign(zs, zs + P);
    R->plane_crossings.assign(P, 0); R->plane_segments.assign(P, 0); R->plane_loops.assign(P, 0);
    if (!P || !T || !topo->d_triangles || !topo->d_vertices) { *out = R.release(); return FHIP_OK; }          // (no plane, no triangle: nothing crosses)
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    PassTimes times(st, "fhip mesh slices (%u triangles, %u planes)", T, P);
    const float* const vertices = topo->d_vertices;
    const uint64_t* const triangles = topo->d_triangles;
    const uint64_t n_rows = topo->n_vertex_rows;
    const size_t n_counters = (size_t)fhm::FH_MT_ROWS * fhm::FH_MT_COUNTERS;
    SliceScratch S;
    size_t slots = 0, loop_bytes = 0;
    uint64_t n = 0, m = 0;
    const auto carve = [&]() -> hipError_t {          // the pieces known so far; what the buffer holds stays
        const size_t keep = S.bytes;
        S.walk(nullptr, n_counters, P, n_rows, T, slots, m, n, loop_bytes);
        const hipError_t e = SliceScratch::grow(ctx, S.bytes, keep);
        if (e == hipSuccess) S.walk((char*)ctx->mesh_leaves.p, n_counters, P, n_rows, T, slots, m, n, loop_bytes);
        return e;
    };
    std::vector<uint64_t> rows(n_counters);
    uint64_t c[fhm::FH_MT_COUNTERS];
    const auto read_counters = [&]() -> hipError_t {          // waits for everything so far
        hipError_t e = hipMemcpyAsync(rows.data(), S.counters, n_counters * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        for (uint64_t& x : c) x = 0;
        for (size_t r = 0; r < n_counters; r++) c[r % fhm::FH_MT_COUNTERS] += rows[r];
        return e;
    };
    HIP_TRY(ctx, carve());
    HIP_TRY(ctx, hipMemsetAsync(S.counters, 0, n_counters * 8, st));
    HIP_TRY(ctx, hipMemcpyAsync(S.zs, R->zs.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, times.mark(nullptr));
    hipLaunchKernelGGL(fhm::k_ms_levels, cc_grid(n_rows), dim3(256), 0, st, vertices, n_rows, (const float*)S.zs, P, S.level);
    HIP_TRY(ctx, times.mark("k_ms_levels"));
    hipLaunchKernelGGL(fhm::k_ms_count, cc_grid(T), dim3(256), 0, st, triangles, (const uint32_t*)S.level, T, S.seg_count, S.counters);
    HIP_TRY(ctx, times.mark("k_ms_count"));
    HIP_TRY(ctx, read_counters());
    const uint64_t crossing_corners = c[fhm::FH_MS_CORNERS];
    m = c[fhm::FH_MS_SEGMENTS];
    if (m > fhslice::MAX_ITEMS) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh slices: 2^32 - 1 segments or more");
    if (m == 0) { *out = R.release(); return FHIP_OK; }          // (no triangle crosses a plane: no arrays)
    const uint32_t log2 = table_log2 ? table_log2 : fhslice::default_log2(crossing_corners);
    slots = (size_t)fhtopo::n_slots(log2);
    R->edge_slots = slots;
    R->n_segments = m;
    HIP_TRY(ctx, carve());
    HIP_TRY(ctx, hipMemsetAsync(S.table, 0, slots * fhtopo::EDGE_SLOT_WORDS * 8, st));
    HIP_TRY(ctx, times.mark("(wait) + clear"));
    hipLaunchKernelGGL(fhm::k_ms_insert, cc_grid(T), dim3(256), 0, st, triangles, (const uint32_t*)S.level, T, S.table, log2, S.corner_slot, S.counters);
    HIP_TRY(ctx, times.mark("k_ms_insert"));
    hipLaunchKernelGGL(fhm::k_ms_first, cc_grid(C), dim3(256), 0, st, (const uint64_t*)S.table, (const uint32_t*)S.corner_slot, (const uint32_t*)S.level, C, S.count, S.counters);
    HIP_TRY(ctx, times.mark("k_ms_first"));
    HIP_TRY(ctx, read_counters());
    if (c[fhm::FH_MS_OVERFLOW]) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh slices: the edge table is full");
    n = c[fhm::FH_MS_CROSSINGS];
    if (n > fhslice::MAX_ITEMS) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh slices: 2^32 - 1 crossings or more");
    R->n_crossings = n;
    HIP_TRY(ctx, carve());
    HIP_TRY(ctx, hipMalloc((void**)&R->d_xy, (size_t)n * 8));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_plane, (size_t)n * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_edge, (size_t)n * 8));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_next, (size_t)n * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_loop, (size_t)n * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_degree, (size_t)n));
    HIP_TRY(ctx, hipMemsetAsync(S.next_words, 0, (size_t)n * 8, st));
    HIP_TRY(ctx, hipMemsetAsync(S.degree, 0, (size_t)n * 8, st));
    HIP_TRY(ctx, times.mark("(wait) + arrays + clear"));
    HIP_TRY(ctx, ctr_scan(st, S.count, C, S.base, S.scan_tmp));
    hipLaunchKernelGGL(fhm::k_ms_ids, cc_grid(C), dim3(256), 0, st, (const uint64_t*)S.table, (const uint32_t*)S.base, C, S.corner_slot);
    HIP_TRY(ctx, times.mark("scan + k_ms_ids"));
    hipLaunchKernelGGL(fhm::k_ms_emit, cc_grid(n), dim3(256), 0, st, vertices, triangles, (const uint32_t*)S.level, (const float*)S.zs, (const uint32_t*)S.base, C, (uint32_t)n,
                       (float2*)R->d_xy, R->d_plane, (uint2*)R->d_edge);
    HIP_TRY(ctx, times.mark("k_ms_emit"));
    HIP_TRY(ctx, ctr_scan(st, S.seg_count, T, S.seg_base, S.scan_tmp));
    hipLaunchKernelGGL(fhm::k_cc_init, cc_grid(n), dim3(256), 0, st, S.parent, n);
    HIP_TRY(ctx, times.mark("scan + k_cc_init"));
    hipLaunchKernelGGL(fhm::k_ms_segments, cc_grid(m), dim3(256), 0, st, triangles, (const uint32_t*)S.level, (const uint32_t*)S.seg_base, T, (uint32_t)m,
                       (const uint32_t*)S.corner_slot, (uint32_t)n, (uint2*)S.segments, S.next_words, S.degree, S.parent);
    HIP_TRY(ctx, times.mark("k_ms_segments"));
    hipLaunchKernelGGL(fhm::k_cc_flatten, cc_grid(n), dim3(256), 0, st, S.parent, n);
    hipLaunchKernelGGL(fhm::k_cc_roots, cc_grid(n), dim3(256), 0, st, (const uint32_t*)S.parent, n, R->d_loop);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctr_scan(st, R->d_loop, (uint32_t)n, S.rank, S.scan_tmp2));
    hipLaunchKernelGGL(fhm::k_cc_number, cc_grid(n), dim3(256), 0, st, (const uint32_t*)S.parent, (const uint32_t*)S.rank, n, R->d_loop);
    HIP_TRY(ctx, times.mark("flatten + roots + scan + number"));
    uint32_t n_loops = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_loops, S.rank + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    R->n_loops = n_loops;
    // the loops' table on the device: area2 f64 [L]; leader, plane, crossings, segments, irregular u32 [L]; lo, hi u32 [L][2]
    const size_t L = n_loops;
    loop_bytes = L * (8 + 9 * 4);
    HIP_TRY(ctx, carve());
    fhm::MsLoopTable tab;
    tab.area2 = (double*)S.loops;
    tab.leader = (uint32_t*)(tab.area2 + L);
    tab.plane = tab.leader + L;
    tab.crossings = tab.plane + L;
    tab.segments = tab.crossings + L;
    tab.irregular = tab.segments + L;
    tab.lo = tab.irregular + L;
    tab.hi = tab.lo + 2 * L;
    HIP_TRY(ctx, hipMemsetAsync(S.loops, 0, loop_bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(tab.lo, 0xFF, 2 * L * 4, st));
    HIP_TRY(ctx, times.mark("(wait) + clear"));
    hipLaunchKernelGGL(fhm::k_ms_measure_x, cc_grid(n), dim3(256), 0, st, (const float2*)R->d_xy, (const uint32_t*)R->d_plane, (const uint32_t*)S.parent,
                       (const uint32_t*)R->d_loop, (const uint64_t*)S.next_words, (const uint64_t*)S.degree, (uint32_t)n, R->d_next, R->d_degree, tab);
    HIP_TRY(ctx, times.mark("k_ms_measure_x"));
    hipLaunchKernelGGL(fhm::k_ms_measure_s, cc_grid(m), dim3(256), 0, st, (const float2*)R->d_xy, (const uint2*)S.segments, (const uint32_t*)R->d_loop, (uint32_t)m, tab);
    HIP_TRY(ctx, times.mark("k_ms_measure_s"));
    // through the context's pinned landing area, and from there straight into the handle's columns: millions of loops are hundreds of MB
    HIP_TRY(ctx, pinned_ensure(ctx, loop_bytes));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->mesh_pinned, S.loops, loop_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const uint8_t* const host = (const uint8_t*)ctx->mesh_pinned;
    HIP_TRY(ctx, times.mark("the loops' table"));
    R->loop_area2.resize(L); R->loop_leader.resize(L); R->loop_plane.resize(L); R->loop_crossings.resize(L); R->loop_segments.resize(L); R->loop_irregular.resize(L);
    R->loop_lo.resize(2 * L); R->loop_hi.resize(2 * L);
    memcpy(R->loop_area2.data(), host, L * 8);
    const uint32_t* const cols = (const uint32_t*)(host + L * 8);
    memcpy(R->loop_leader.data(), cols, L * 4);
    memcpy(R->loop_plane.data(), cols + L, L * 4);
    memcpy(R->loop_crossings.data(), cols + 2 * L, L * 4);
    memcpy(R->loop_segments.data(), cols + 3 * L, L * 4);
    memcpy(R->loop_irregular.data(), cols + 4 * L, L * 4);
    for (size_t k = 0; k < 2 * L; k++) {
        R->loop_lo[k] = fhtopo::bits_float(fhtopo::unordered(cols[5 * L + k]));
        R->loop_hi[k] = fhtopo::bits_float(fhtopo::unordered(cols[7 * L + k]));
    }
    // the planes' counts: a loop lies in one plane, so they are sums over the loops' rows (no pass over the crossings, no atomics)
    for (size_t l = 0; l < L; l++) {
        const uint32_t p = R->loop_plane[l];
        if (p >= P) return fail(ctx, FHIP_ERR_HIP, "mesh slices: a loop in no plane");
        R->plane_crossings[p] += R->loop_crossings[l];
        R->plane_segments[p] += R->loop_segments[l];
        R->plane_loops[p]++;
        R->n_irregular += R->loop_irregular[l];
    }
    *out = R.release();
    return FHIP_OK;
}
// {planes, crossings, segments, loops, irregular crossings, edge-table slots, 0, 0}
void fhip_slices_counts(const void* h, uint64_t out[8]) {
    const fhip_slices* const s = (const fhip_slices*)h;
    const uint64_t c[8] = {s ? s->n_planes : 0, s ? s->n_crossings : 0, s ? s->n_segments : 0, s ? s->n_loops : 0, s ? s->n_irregular : 0, s ? s->edge_slots : 0, 0, 0};
    for (int k = 0; k < 8; k++) out[k] = c[k];
}
fhip_status fhip_slices_planes(const void* h, float* zs, uint64_t* crossings, uint64_t* segments, uint64_t* loops) {
    const fhip_slices* const s = (const fhip_slices*)h;
    if (!s) return FHIP_ERR_BAD_TAPE;
    const size_t P = (size_t)s->n_planes;
    if (P == 0) return FHIP_OK;
    if (zs) memcpy(zs, s->zs.data(), P * 4);
    if (crossings) memcpy(crossings, s->plane_crossings.data(), P * 8);
    if (segments) memcpy(segments, s->plane_segments.data(), P * 8);
    if (loops) memcpy(loops, s->plane_loops.data(), P * 8);
    return FHIP_OK;
}
fhip_status fhip_slices_loops(const void* h, uint32_t* leader, uint32_t* plane, uint32_t* crossings, uint32_t* segments, uint32_t* irregular, double* area2, float* lo, float* hi) {
    const fhip_slices* const s = (const fhip_slices*)h;
    if (!s) return FHIP_ERR_BAD_TAPE;
    const size_t L = (size_t)s->n_loops;
    if (L == 0) return FHIP_OK;
    if (leader) memcpy(leader, s->loop_leader.data(), L * 4);
    if (plane) memcpy(plane, s->loop_plane.data(), L * 4);
    if (crossings) memcpy(crossings, s->loop_crossings.data(), L * 4);
    if (segments) memcpy(segments, s->loop_segments.data(), L * 4);
    if (irregular) memcpy(irregular, s->loop_irregular.data(), L * 4);
    if (area2) memcpy(area2, s->loop_area2.data(), L * 8);
    if (lo) memcpy(lo, s->loop_lo.data(), 2 * L * 4);
    if (hi) memcpy(hi, s->loop_hi.data(), 2 * L * 4);
    return FHIP_OK;
}
fhip_status fhip_slices_vertices(const void* h, float* xy, uint32_t* plane, uint32_t* edge, uint32_t* next, uint32_t* loop_of, uint8_t* degree) {
    const fhip_slices* const s = (const fhip_slices*)h;
    if (!s) return FHIP_ERR_BAD_TAPE;
    const size_t n = (size_t)s->n_crossings;
    if (xy && handle_to_host(s->device, xy, s->d_xy, n * 8)) return FHIP_ERR_HIP;
    if (plane && handle_to_host(s->device, plane, s->d_plane, n * 4)) return FHIP_ERR_HIP;
    if (edge && handle_to_host(s->device, edge, s->d_edge, n * 8)) return FHIP_ERR_HIP;
    if (next && handle_to_host(s->device, next, s->d_next, n * 4)) return FHIP_ERR_HIP;
    if (loop_of && handle_to_host(s->device, loop_of, s->d_loop, n * 4)) return FHIP_ERR_HIP;
    if (degree && handle_to_host(s->device, degree, s->d_degree, n)) return FHIP_ERR_HIP;
    return FHIP_OK;
}
const float* fhip_slices_xy_dev(const void* h) { return HANDLE_GET(fhip_slices, h, d_xy); }
const uint32_t* fhip_slices_next_dev(const void* h) { return HANDLE_GET(fhip_slices, h, d_next); }
const uint32_t* fhip_slices_loop_dev(const void* h) { return HANDLE_GET(fhip_slices, h, d_loop); }
const uint32_t* fhip_slices_plane_dev(const void* h) { return HANDLE_GET(fhip_slices, h, d_plane); }
void fhip_slices_free(void* h) { delete (fhip_slices*)h; }
