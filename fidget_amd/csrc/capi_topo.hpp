// ---- the check of a triangle mesh: weld, edges, shells, volume ---------------------------------------------------------------------------------
// fhip_triangles_topology and fhip_mesh_topology (fidget_hip.h; the handle it declares void* is a fhip_topology): the passes of topo.hip on
// the context's stream with the prefix sums of the contours (ctr_scan) between them.  The host waits for the rejected triangles - any,
// and the call ends there with the count alone - for the number of welded vertices and whether the vertex table held them, for the
// edge table likewise, for the number of shells, which sizes their table, and at the end: the call blocks, also with device pointers.
// Host input arrays get device memory of their own for the call.  The scratch - the counters, the two tables, per corner a slot, a
// vertex id, a flag and a rank, per triangle a parent, a flag and a rank, the scans' block totals - is carved from ctx->mesh_leaves as
// capi_trivox.hpp does: it stays with the context and fhip_ctx_trim gives it back.  The results - the vertices, the triangles, a shell per
// triangle and a byte per corner, from which fhip_topology_edges makes its lists - are the handle's own device arrays; the shells'
// columns and the counts are on the host.  A fragment of the C ABI, included by capi_mesh.hpp; uses capi_mesh_util.hpp.
// FHIP_MESH_TIMES: the passes' times between events on the stream, on stderr.
struct fhip_topology {
    int device = 0;
    uint64_t counts[16] = {};
    uint64_t n_vertex_rows = 0;          // the rows of d_vertices: the welded vertices, or the vertices as given
    float* d_vertices = nullptr;
    uint64_t* d_triangles = nullptr;
    uint32_t* d_shell = nullptr;
    uint8_t* d_corner_class = nullptr;
    std::vector<uint64_t> shell_triangles, shell_unbalanced;
    std::vector<uint32_t> shell_first;
    std::vector<float> shell_lo, shell_hi;
    std::vector<double> shell_volume6, shell_area2;
    ~fhip_topology() {
        if (d_vertices) (void)hipFree(d_vertices);
        if (d_triangles) (void)hipFree(d_triangles);
        if (d_shell) (void)hipFree(d_shell);
        if (d_corner_class) (void)hipFree(d_corner_class);
    }
};
enum { TOPO_TRIANGLES = 0, TOPO_REJECTED, TOPO_DEGENERATE, TOPO_VERTICES, TOPO_EDGES, TOPO_BOUNDARY, TOPO_FLIPPED, TOPO_NONMANIFOLD, TOPO_UNBALANCED, TOPO_SHELLS,
       TOPO_VERTEX_SLOTS, TOPO_EDGE_SLOTS };
struct TopoTimes {          // FHIP_MESH_TIMES: an event after every pass, and after every wait of the host, on the stream; the times between them at the end
    bool on;
    hipStream_t st;
    std::vector<std::pair<const char*, hipEvent_t>> events;
    hipError_t mark(const char* what) {
        if (!on) return hipSuccess;
        hipEvent_t ev;
        const hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) return e;
        events.push_back({what, ev});
        return hipEventRecord(ev, st);
    }
    void report() {
        if (!on || events.empty() || hipEventSynchronize(events.back().second) != hipSuccess) return;
        for (size_t k = 1; k < events.size(); k++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, events[k - 1].second, events[k].second) == hipSuccess) fprintf(stderr, "fhip mesh topology: %-28s %10.4f ms\n", events[k].first, ms);
        }
    }
    ~TopoTimes() { for (auto& e : events) (void)hipEventDestroy(e.second); }
};
struct TopoCarve {          // pieces of one buffer, each 16-byte aligned: sized in a first walk (p == nullptr), handed out in a second
    char* p = nullptr;
    size_t at = 0;
    void* take(size_t bytes) {
        void* const r = p ? p + at : nullptr;
        at += (bytes + 15) / 16 * 16;
        return r;
    }
    uint32_t* u32(size_t n) { return (uint32_t*)take(n * 4); }
    uint64_t* u64(size_t n) { return (uint64_t*)take(n * 8); }
};
fhip_status fhip_triangles_topology(fhip_ctx* ctx, const float* vertices, uint64_t n_vertices, const uint64_t* triangles, uint64_t n_triangles, int on_device, int weld,
                                    uint32_t table_log2, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_triangles_topology: context and result");
    if (n_triangles > fhtopo::MAX_CORNERS / 3) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh topology: more than 2^32 - 2 corners");
    if (triangles && n_vertices > fhtopo::MAX_CORNERS) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh topology: more than 2^32 - 2 vertices");
    if (!triangles && !weld) return fail(ctx, FHIP_ERR_UNSUPPORTED, "mesh topology: a soup has no vertices until it is welded");
    if (table_log2 > fhtopo::MAX_LOG2) return fail(ctx, FHIP_ERR_UNSUPPORTED, "mesh topology: table_log2 above 32");
    if (n_triangles && !vertices) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_triangles_topology: the vertices");
    if (on_device && (((uintptr_t)vertices & 3u) || ((uintptr_t)triangles & 7u)))
        return fail(ctx, FHIP_ERR_UNSUPPORTED, "a mesh on the device: vertices 4-byte aligned, triangles 8-byte aligned");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    TopoTimes tt{getenv("FHIP_MESH_TIMES") != nullptr, st, {}};
    const auto mark = [&tt](const char* what) -> hipError_t {          // a launch's error, or the event after the pass
        const hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : tt.mark(what);
    };
    const uint32_t T = (uint32_t)n_triangles, C = 3 * T;
    const bool welded = weld != 0;
    if (!triangles) n_vertices = std::min<uint64_t>(n_vertices, (uint64_t)C);          // (a soup reads its first 3 T vertices)
    std::unique_ptr<fhip_topology> R(new fhip_topology());
    R->device = ctx->device;
    R->counts[TOPO_TRIANGLES] = T;
    ScratchBuf in_v, in_t;
    const float* d_vertices = vertices;
    const uint64_t* d_triangles = triangles;
    if (!on_device && T) {
        HIP_TRY(ctx, in_v.ensure(std::max<size_t>((size_t)n_vertices * 12, 4)));
        HIP_TRY(ctx, hipMemcpyAsync(in_v.p, vertices, (size_t)n_vertices * 12, hipMemcpyHostToDevice, st));
        d_vertices = (const float*)in_v.p;
        if (triangles) {
            HIP_TRY(ctx, in_t.ensure((size_t)T * 24));
            HIP_TRY(ctx, hipMemcpyAsync(in_t.p, triangles, (size_t)T * 24, hipMemcpyHostToDevice, st));
            d_triangles = (const uint64_t*)in_t.p;
        }
    }
    const uint32_t log2_v = welded ? (table_log2 ? table_log2 : fhtopo::default_log2(T)) : 0, log2_e = table_log2 ? table_log2 : fhtopo::default_log2(T);
    const size_t slots_v = welded ? (size_t)fhtopo::n_slots(log2_v) : 0, slots_e = (size_t)fhtopo::n_slots(log2_e);
    const size_t n_counters = (size_t)fhm::FH_MT_ROWS * fhm::FH_MT_COUNTERS, used_words = welded ? 0 : (size_t)((n_vertices + 3) / 4);          // a byte per vertex
    TopoCarve cv;
    uint64_t *d_counters = nullptr, *e_table = nullptr;
    uint32_t *v_table = nullptr, *used = nullptr, *corner_slot = nullptr, *vid = nullptr, *flag = nullptr, *rank = nullptr, *parent = nullptr,
             *scan_tmp = nullptr;
    for (int pass = 0; pass < 2; pass++) {
        cv.at = 0;
        d_counters = cv.u64(n_counters);
        e_table = cv.u64(fhtopo::EDGE_SLOT_WORDS * slots_e);
        v_table = cv.u32(fhtopo::VERTEX_SLOT_WORDS * slots_v);
        used = cv.u32(used_words);
        corner_slot = cv.u32(C);          // the corner's vertex slot, then its edge slot
        vid = cv.u32(C);
        flag = cv.u32((size_t)C + 1);          // the corners' flags and ranks, then the triangles'
        rank = cv.u32((size_t)C + 1);
        parent = cv.u32(T);
        scan_tmp = cv.u32(ctr_scan_words(C) + 1);
        if (pass == 0) {
            if (!T) break;          // (no triangles: no scratch, no arrays, all zeros)
            HIP_TRY(ctx, ctx->mesh_leaves.ensure(cv.at));
            cv.p = (char*)ctx->mesh_leaves.p;
        }
    }
    if (!T) { *out = R.release(); return FHIP_OK; }
    std::vector<uint64_t> rows(n_counters);
    uint64_t c[fhm::FH_MT_COUNTERS];
    auto read_counters = [&]() -> hipError_t {          // waits for everything so far
        hipError_t e = hipMemcpyAsync(rows.data(), d_counters, n_counters * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        for (uint64_t& x : c) x = 0;
        for (size_t r = 0; r < n_counters; r++) c[r % fhm::FH_MT_COUNTERS] += rows[r];
        return e;
    };
    HIP_TRY(ctx, hipMemsetAsync(d_counters, 0, n_counters * 8, st));
    HIP_TRY(ctx, mark("start"));
    hipLaunchKernelGGL(fhm::k_mt_check, cc_grid(T), dim3(256), 0, st, d_vertices, n_vertices, d_triangles, T, d_counters);
    HIP_TRY(ctx, mark("k_mt_check"));
    HIP_TRY(ctx, read_counters());
    HIP_TRY(ctx, mark("(the host reads the counters)"));
    R->counts[TOPO_REJECTED] = c[fhm::FH_MT_REJECTED];
    if (c[fhm::FH_MT_REJECTED]) { *out = R.release(); return FHIP_OK; }          // the count alone: no arrays

    // the handle's arrays, all but the welded vertices, whose number is not known yet
    HIP_TRY(ctx, hipMalloc((void**)&R->d_triangles, (size_t)T * 24));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_shell, (size_t)T * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_corner_class, (size_t)C));
    if (!welded) HIP_TRY(ctx, hipMalloc((void**)&R->d_vertices, std::max<size_t>((size_t)n_vertices * 12, 4)));
    HIP_TRY(ctx, mark("(the handle's arrays)"));
    HIP_TRY(ctx, hipMemsetAsync(e_table, 0, slots_e * fhtopo::EDGE_SLOT_WORDS * 8, st));
    uint64_t n_rows = 0;
    if (welded) {
        HIP_TRY(ctx, hipMemsetAsync(v_table, 0xFF, slots_v * fhtopo::VERTEX_SLOT_WORDS * 4, st));
        HIP_TRY(ctx, mark("clear"));
        const fhtopo::Corners in{d_vertices, d_triangles};
        hipLaunchKernelGGL(fhm::k_mt_weld, cc_grid(C), dim3(256), 0, st, in, C, v_table, log2_v, corner_slot, d_counters);
        HIP_TRY(ctx, mark("k_mt_weld"));
        HIP_TRY(ctx, read_counters());
        if (c[fhm::FH_MT_OVERFLOW]) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh topology: the vertex table is full");
        hipLaunchKernelGGL(fhm::k_mt_vflag, cc_grid(C), dim3(256), 0, st, (const uint32_t*)corner_slot, (const uint32_t*)v_table, C, flag);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, ctr_scan(st, flag, C, rank, scan_tmp));
        uint32_t n_welded = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&n_welded, rank + C, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, mark("k_mt_vflag + scan + wait"));
        n_rows = n_welded;
        R->counts[TOPO_VERTICES] = n_welded;
        HIP_TRY(ctx, hipMalloc((void**)&R->d_vertices, std::max<size_t>((size_t)n_rows * 12, 4)));
        HIP_TRY(ctx, mark("(the handle's vertices)"));
        hipLaunchKernelGGL(fhm::k_mt_vemit, cc_grid(C), dim3(256), 0, st, in, (const uint32_t*)corner_slot, (const uint32_t*)v_table, (const uint32_t*)rank, C, R->d_vertices, vid);
        HIP_TRY(ctx, mark("k_mt_vemit"));
    } else {
        n_rows = n_vertices;
        HIP_TRY(ctx, hipMemsetAsync(used, 0, used_words * 4, st));
        HIP_TRY(ctx, mark("clear"));
        HIP_TRY(ctx, hipMemcpyAsync(R->d_vertices, d_vertices, (size_t)n_rows * 12, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(fhm::k_mt_ids, cc_grid(C), dim3(256), 0, st, d_triangles, C, vid, (uint8_t*)used);
        hipLaunchKernelGGL(fhm::k_mt_used, cc_grid(used_words), dim3(256), 0, st, (const uint32_t*)used, (uint32_t)used_words, d_counters);
        HIP_TRY(ctx, mark("copy + k_mt_ids + k_mt_used"));
    }
    R->n_vertex_rows = n_rows;
    R->counts[TOPO_VERTEX_SLOTS] = slots_v;
    R->counts[TOPO_EDGE_SLOTS] = slots_e;
    hipLaunchKernelGGL(fhm::k_mt_edges, cc_grid(T), dim3(256), 0, st, (const uint32_t*)vid, T, e_table, log2_e, R->d_triangles, parent, corner_slot, d_counters);
    HIP_TRY(ctx, mark("k_mt_edges"));
    HIP_TRY(ctx, read_counters());
    HIP_TRY(ctx, mark("(the host reads the counters)"));
    if (c[fhm::FH_MT_OVERFLOW]) return fail(ctx, FHIP_ERR_OVERFLOW, "mesh topology: the edge table is full");
    hipLaunchKernelGGL(fhm::k_mt_link, cc_grid(T), dim3(256), 0, st, (const uint64_t*)R->d_triangles, T, (const uint64_t*)e_table,
                       (const uint32_t*)corner_slot, R->d_corner_class, parent, d_counters);
    HIP_TRY(ctx, mark("k_mt_link"));
    hipLaunchKernelGGL(fhm::k_cc_flatten, cc_grid(T), dim3(256), 0, st, parent, (uint64_t)T);
    hipLaunchKernelGGL(fhm::k_mt_roots, cc_grid(T), dim3(256), 0, st, (const uint32_t*)parent, (const uint64_t*)R->d_triangles, T, flag);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctr_scan(st, flag, T, rank, scan_tmp));
    HIP_TRY(ctx, mark("flatten + roots + scan"));
    HIP_TRY(ctx, read_counters());
    uint32_t n_shells = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_shells, rank + T, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (!welded) R->counts[TOPO_VERTICES] = c[fhm::FH_MT_USED];
    R->counts[TOPO_DEGENERATE] = c[fhm::FH_MT_DEGENERATE];
    R->counts[TOPO_EDGES] = c[fhm::FH_MT_EDGES];
    R->counts[TOPO_BOUNDARY] = c[fhm::FH_MT_BOUNDARY];
    R->counts[TOPO_FLIPPED] = c[fhm::FH_MT_FLIPPED];
    R->counts[TOPO_NONMANIFOLD] = c[fhm::FH_MT_NONMANIFOLD];
    R->counts[TOPO_UNBALANCED] = c[fhm::FH_MT_UNBALANCED];
    R->counts[TOPO_SHELLS] = n_shells;
    // the shells' table on the device: triangles, unbalanced u64 [s]; volume6, area2 f64 [s]; first u32 [s]; lo, hi u32 [s][3]
    ScratchBuf table;
    const size_t S = n_shells, table_bytes = S * (4 * 8 + 7 * 4);
    HIP_TRY(ctx, table.ensure(std::max<size_t>(table_bytes, 4)));
    fhm::MtShellTable tab;
    tab.triangles = (unsigned long long*)table.p;
    tab.unbalanced = tab.triangles + S;
    tab.volume6 = (double*)(tab.unbalanced + S);
    tab.area2 = tab.volume6 + S;
    uint32_t* const d_first = (uint32_t*)(tab.area2 + S);
    tab.lo = d_first + S;
    tab.hi = tab.lo + 3 * S;
    if (S) {          // (none: every triangle degenerate)
        HIP_TRY(ctx, hipMemsetAsync(table.p, 0, table_bytes, st));
        HIP_TRY(ctx, hipMemsetAsync(tab.lo, 0xFF, 3 * S * 4, st));
    }
    hipLaunchKernelGGL(fhm::k_mt_number, cc_grid(T), dim3(256), 0, st, (const uint32_t*)parent, (const uint32_t*)rank, (const uint32_t*)flag, T, R->d_shell, d_first);
    HIP_TRY(ctx, mark("(wait) + clear + k_mt_number"));
    {   // equal shares of whole 64 triangles to the waves of at most FH_MT_TABLE_BLOCKS blocks; no block without a triangle
        const uint64_t waves = std::min<uint64_t>(((uint64_t)T + 63) / 64, (uint64_t)4 * fhm::FH_MT_TABLE_BLOCKS);
        const uint64_t per_wave = ((T + waves - 1) / waves + 63) / 64 * 64;
        const uint32_t nb = (uint32_t)(((T + per_wave - 1) / per_wave + 3) / 4);
        hipLaunchKernelGGL(fhm::k_mt_table, dim3(nb), dim3(256), 0, st, (const float*)R->d_vertices, (const uint64_t*)R->d_triangles, (const uint32_t*)R->d_shell,
                           (const uint8_t*)R->d_corner_class, T, per_wave, tab);
    }
    HIP_TRY(ctx, mark("k_mt_table"));
    std::vector<uint8_t> host(table_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), table.p, table_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    tt.report();
    R->shell_triangles.resize(S); R->shell_unbalanced.resize(S); R->shell_volume6.resize(S); R->shell_area2.resize(S); R->shell_first.resize(S);
    R->shell_lo.resize(3 * S); R->shell_hi.resize(3 * S);
    if (S) {
        memcpy(R->shell_triangles.data(), host.data(), S * 8);
        memcpy(R->shell_unbalanced.data(), host.data() + S * 8, S * 8);
        memcpy(R->shell_volume6.data(), host.data() + S * 16, S * 8);
        memcpy(R->shell_area2.data(), host.data() + S * 24, S * 8);
        memcpy(R->shell_first.data(), host.data() + S * 32, S * 4);
        const uint32_t* const lo = (const uint32_t*)(host.data() + S * 36);
        const uint32_t* const hi = lo + 3 * S;
        for (size_t k = 0; k < 3 * S; k++) {
            R->shell_lo[k] = fhtopo::bits_float(fhtopo::unordered(lo[k]));
            R->shell_hi[k] = fhtopo::bits_float(fhtopo::unordered(hi[k]));
        }
    }
    *out = R.release();
    return FHIP_OK;
}
fhip_status fhip_mesh_topology(fhip_ctx* ctx, const fhip_mesh* mesh, int weld, uint32_t table_log2, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !mesh) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_mesh_topology: context and mesh");
    const uint64_t nv = mesh->vertices.size(), nt = mesh->triangles.size();
    if (mesh->d_vertices && mesh->d_triangles)          // resident (fhip_mesh_vertices_dev): read where they are
        return fhip_triangles_topology(ctx, (const float*)mesh->d_vertices, nv, mesh->d_triangles, nt, 1, weld, table_log2, out);
    return fhip_triangles_topology(ctx, (const float*)mesh->vertices.data(), nv, (const uint64_t*)mesh->triangles.data(), nt, 0, weld, table_log2, out);
}
void fhip_topology_counts(const void* h, uint64_t out[16]) {
    const fhip_topology* const t = (const fhip_topology*)h;
    for (int k = 0; k < 16; k++) out[k] = t ? t->counts[k] : 0;
}
uint64_t fhip_topology_vertex_rows(const void* h) { return HANDLE_GET(fhip_topology, h, n_vertex_rows); }
// the arrays to the host: refused without a handle, and without a destination for rows that the handle has; an array it has not is no rows
fhip_status fhip_topology_vertices(const void* h, float* out) {
    const fhip_topology* const t = (const fhip_topology*)h;
    if (!t || (t->n_vertex_rows && !out)) return FHIP_ERR_BAD_TAPE;
    return t->d_vertices ? handle_to_host(t->device, out, t->d_vertices, (size_t)t->n_vertex_rows * 12) : FHIP_OK;
}
fhip_status fhip_topology_triangles(const void* h, uint64_t* out) {
    const fhip_topology* const t = (const fhip_topology*)h;
    if (!t || (t->d_triangles && t->counts[TOPO_TRIANGLES] && !out)) return FHIP_ERR_BAD_TAPE;
    return t->d_triangles ? handle_to_host(t->device, out, t->d_triangles, (size_t)t->counts[TOPO_TRIANGLES] * 24) : FHIP_OK;
}
fhip_status fhip_topology_triangle_shells(const void* h, uint32_t* out) {
    const fhip_topology* const t = (const fhip_topology*)h;
    if (!t || (t->d_shell && t->counts[TOPO_TRIANGLES] && !out)) return FHIP_ERR_BAD_TAPE;
    return t->d_shell ? handle_to_host(t->device, out, t->d_shell, (size_t)t->counts[TOPO_TRIANGLES] * 4) : FHIP_OK;
}
const float* fhip_topology_vertices_dev(const void* h) { return HANDLE_GET(fhip_topology, h, d_vertices); }
const uint64_t* fhip_topology_triangles_dev(const void* h) { return HANDLE_GET(fhip_topology, h, d_triangles); }
const uint32_t* fhip_topology_triangle_shells_dev(const void* h) { return HANDLE_GET(fhip_topology, h, d_shell); }
fhip_status fhip_topology_shells(const void* h, uint64_t* triangles, uint32_t* first, uint64_t* unbalanced, float* lo, float* hi, double* volume6, double* area2) {
    const fhip_topology* const t = (const fhip_topology*)h;
    if (!t) return FHIP_ERR_BAD_TAPE;
    const size_t n = (size_t)t->counts[TOPO_SHELLS];
    if (n == 0) return FHIP_OK;
    if (triangles) memcpy(triangles, t->shell_triangles.data(), n * 8);
    if (first) memcpy(first, t->shell_first.data(), n * 4);
    if (unbalanced) memcpy(unbalanced, t->shell_unbalanced.data(), n * 8);
    if (lo) memcpy(lo, t->shell_lo.data(), 3 * n * 4);
    if (hi) memcpy(hi, t->shell_hi.data(), 3 * n * 4);
    if (volume6) memcpy(volume6, t->shell_volume6.data(), n * 8);
    if (area2) memcpy(area2, t->shell_area2.data(), n * 8);
    return FHIP_OK;
}
// kind 0 boundary, 1 flipped, 2 nonmanifold, 3 unbalanced: counts[5 + kind] pairs (a, b), in the order of the edges' first corners
fhip_status fhip_topology_edges(fhip_ctx* ctx, const void* h, uint32_t kind, uint32_t* out, int out_on_device) {
    const fhip_topology* const t = (const fhip_topology*)h;
    if (!ctx || !t) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_topology_edges: context and topology");
    if (ctx->device != t->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "topology: made on another device");
    if (kind >= fhtopo::N_KINDS) return fail(ctx, FHIP_ERR_UNSUPPORTED, "topology edges: kind 0 boundary, 1 flipped, 2 nonmanifold, 3 unbalanced");
    const uint64_t n = t->counts[TOPO_BOUNDARY + kind];
    if (n == 0) return FHIP_OK;
    if (!out) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_topology_edges: the output buffer");
    if (out_on_device && ((uintptr_t)out & 3u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "topology edges to the device: the buffer must be 4-byte aligned");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t C = 3 * (uint32_t)t->counts[TOPO_TRIANGLES];
    TopoCarve cv;
    uint32_t *flag = nullptr, *rank = nullptr, *scan_tmp = nullptr, *pairs = nullptr;
    for (int pass = 0; pass < 2; pass++) {
        cv.at = 0;
        flag = cv.u32((size_t)C + 1);
        rank = cv.u32((size_t)C + 1);
        scan_tmp = cv.u32(ctr_scan_words(C) + 1);
        pairs = cv.u32(out_on_device ? 0 : (size_t)n * 2);
        if (pass == 0) {
            HIP_TRY(ctx, ctx->mesh_leaves.ensure(cv.at));
            cv.p = (char*)ctx->mesh_leaves.p;
        }
    }
    uint32_t* const d_out = out_on_device ? out : pairs;
    hipLaunchKernelGGL(fhm::k_mt_eflag, cc_grid(C), dim3(256), 0, st, (const uint8_t*)t->d_corner_class, C, 1u << kind, flag);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctr_scan(st, flag, C, rank, scan_tmp));
    hipLaunchKernelGGL(fhm::k_mt_eemit, cc_grid(C), dim3(256), 0, st, (const uint64_t*)t->d_triangles, (const uint32_t*)flag, (const uint32_t*)rank, C, d_out);
    HIP_TRY(ctx, hipGetLastError());
    if (!out_on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(out, pairs, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return FHIP_OK;
}
void fhip_topology_free(void* h) { delete (fhip_topology*)h; }
