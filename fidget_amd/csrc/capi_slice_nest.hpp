// ---- the nesting of a mesh's slices: polygons with holes per plane ---------------------------------------------------------------------------
// fhip_slices_nesting (fidget_hip.h; the handle it declares void* is a fhip_slice_nesting, the slices a fhip_slices of capi_slice.hpp): the
// passes of slice_nest.hip on the context's stream over the crossings' arrays where the slices call left them on the device, with what
// the kernels need of the loops' table - leader, plane, and two flags: irregular, area2 > 0 - and the planes' bands sent up from the
// handle's host tables.  THE BANDS.  bands == 0: a plane gets fhsn::default_bands of its regular segments, its y-extent is that of its
// regular loops' lo / hi.  The count pass gives the entries' 64-bit total; where that is above fhsn::ENTRY_MULTIPLE times the regular
// segments and a plane still has more than one band, every plane's number is halved and the count repeated - at most log2 of the
// largest number of times, and only under the host's rule: a caller's `bands` is used as it is.  The host waits for that total, for the
// hits' total, which sizes the two hit arrays, and at the end: the call blocks, as fhip_topology_slices does.  The scratch is carved
// from ctx->mesh_leaves in the order in which the sizes become known (SliceScratch::grow keeps what is there) and stays with the context
// until fhip_ctx_trim.  parent and depth are the handle's own device arrays; everything is also on the host, region_area2 added there
// in ascending child id.  A fragment of the C ABI, included by capi_mesh.hpp after capi_slice.hpp and capi_nest.hpp; children lists are
// fhip_nesting_children's.  FHIP_MESH_TIMES: the passes' times on stderr (PassTimes).
struct fhip_slice_nesting {
    int device = 0;
    uint64_t n_loops = 0, n_planes = 0, n_regular = 0, n_outer = 0, n_top = 0, max_depth = 0, n_improper = 0, n_misoriented = 0, n_bands = 0, n_entries = 0, n_hits = 0;
    uint32_t *d_parent = nullptr, *d_depth = nullptr;
    std::vector<uint32_t> parent, depth, n_children, plane_bands;
    std::vector<double> region_area2;
    std::vector<uint64_t> plane_counts[fhm::FH_SN_PLANE_WORDS];
    ~fhip_slice_nesting() {
        if (d_parent) (void)hipFree(d_parent);
        if (d_depth) (void)hipFree(d_depth);
    }
};
struct SliceNestScratch {
    uint64_t* counters = nullptr;
    uint32_t *loops = nullptr, *band_count = nullptr, *band_start = nullptr, *hit_count = nullptr, *hit_base = nullptr, *n_children = nullptr, *plane_counts = nullptr,
             *scan_tmp = nullptr, *entry_loop = nullptr, *hits = nullptr, *contain = nullptr;
    float4* entry_ends = nullptr;
    fhsn::Band* bands = nullptr;
    size_t bytes = 0;
    void walk(char* p, size_t n_counters, uint32_t P, uint32_t L, uint32_t n_bands, uint64_t n_entries, uint64_t n_hits) {
        TopoCarve cv;
        cv.p = p;
        counters = cv.u64(n_counters);
        loops = cv.u32(3 * (size_t)L);
        bands = (fhsn::Band*)cv.take((size_t)P * sizeof(fhsn::Band));
        band_count = cv.u32((size_t)n_bands + 1);
        band_start = cv.u32((size_t)n_bands + 1);
        hit_count = cv.u32((size_t)L + 1);
        hit_base = cv.u32((size_t)L + 1);
        n_children = cv.u32((size_t)L + (size_t)fhm::FH_SN_PLANE_WORDS * P);          // (cleared as one piece with the planes' counts)
        plane_counts = n_children + L;
        scan_tmp = cv.u32(std::max(ctr_scan_words(n_bands), ctr_scan_words(L)) + 1);
        entry_ends = (float4*)cv.take((size_t)n_entries * sizeof(float4));
        entry_loop = cv.u32((size_t)n_entries);
        hits = cv.u32((size_t)n_hits);
        contain = cv.u32((size_t)n_hits);
        bytes = cv.at;
    }
};
fhip_status fhip_slices_nesting(fhip_ctx* ctx, const void* slices, uint32_t bands, void** out) {
    if (out) *out = nullptr;
    const fhip_slices* const s = (const fhip_slices*)slices;
    if (!ctx || !s || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_slices_nesting: context, slices and result");
    if (ctx->device != s->device) return fail(ctx, FHIP_ERR_UNSUPPORTED, "fhip_slices_nesting: the slices are another device's");
    std::unique_ptr<fhip_slice_nesting> R(new fhip_slice_nesting());
    R->device = ctx->device;
    const uint32_t P = (uint32_t)s->n_planes, L = (uint32_t)s->n_loops, n = (uint32_t)s->n_crossings;
    R->n_planes = P; R->n_loops = L;
    for (auto& col : R->plane_counts) col.assign(P, 0);
    R->plane_bands.assign(P, 0);
    // what goes up of the loops' table, and per plane the regular segments and the y-extent of the regular loops
    // (through the context's pinned landing area, both ways: millions of loops are tens of MB)
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, pinned_ensure(ctx, std::max<size_t>(3 * (size_t)L * 4, 16)));
    uint32_t* const up = (uint32_t*)ctx->mesh_pinned;
    std::vector<uint64_t> plane_regular(P, 0);
    std::vector<float> y0(P, 0.0f), y1(P, 0.0f);
    uint64_t n_regular = 0, regular_segments = 0;
    for (size_t l = 0; l < L; l++) {
        const uint32_t p = s->loop_plane[l];
        const bool regular = s->loop_irregular[l] == 0 && p < P;
        up[l] = s->loop_leader[l];
        up[(size_t)L + l] = p;
        up[2 * (size_t)L + l] = (regular ? 0u : fhsn::IRREGULAR) | (s->loop_area2[l] > 0 ? fhsn::POSITIVE : 0u);
        if (!regular) continue;
        const float lo = s->loop_lo[2 * l + 1], hi = s->loop_hi[2 * l + 1];
        if (!plane_regular[p] || lo < y0[p]) y0[p] = lo;
        if (!plane_regular[p] || hi > y1[p]) y1[p] = hi;
        plane_regular[p] += s->loop_crossings[l];          // (a regular loop has a segment per crossing)
        regular_segments += s->loop_crossings[l];
        n_regular++;
    }
    if (!P || !n_regular || !n || !s->d_xy) { *out = R.release(); return FHIP_OK; }          // (no plane, no loop, irregular loops alone: no arrays)
    for (uint32_t p = 0; p < P; p++) R->plane_bands[p] = bands ? bands : fhsn::default_bands(plane_regular[p]);
    hipStream_t st = ctx->stream;
    PassTimes times(st, "fhip slices nesting (%u loops, %u planes)", L, P);
    const size_t n_counters = (size_t)fhm::FH_MT_ROWS * fhm::FH_MT_COUNTERS;
    SliceNestScratch S;
    uint32_t n_bands = 0;
    uint64_t n_entries = 0, n_hits = 0;
    fhm::SnIn I;
    I.xy = (const float2*)s->d_xy; I.plane = s->d_plane; I.next = s->d_next; I.loop_of = s->d_loop; I.n = n;
    I.L = L; I.P = P;
    // the pieces known so far; what the buffer holds stays, but where it has to grow it MOVES: the kernels' pointers into it are set here
    const auto carve = [&]() -> hipError_t {
        const size_t keep = S.bytes;
        S.walk(nullptr, n_counters, P, L, n_bands, n_entries, n_hits);
        const hipError_t e = SliceScratch::grow(ctx, S.bytes, keep);
        if (e != hipSuccess) return e;
        S.walk((char*)ctx->mesh_leaves.p, n_counters, P, L, n_bands, n_entries, n_hits);
        I.leader = S.loops; I.loop_plane = S.loops + L; I.flags = S.loops + 2 * (size_t)L;
        I.bands = S.bands;
        return hipSuccess;
    };
    std::vector<uint64_t> rows(n_counters);
    const auto read_counter = [&](uint32_t which, uint64_t& total) -> hipError_t {          // waits for everything so far
        hipError_t e = hipMemcpyAsync(rows.data(), S.counters, n_counters * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        total = 0;
        for (size_t r = which; r < n_counters; r += fhm::FH_MT_COUNTERS) total += rows[r];
        return e;
    };
    std::vector<fhsn::Band> table(P);
    const auto lay_out = [&]() -> bool {          // the planes' bands one after the other; false: 2^32 - 1 of them or more
        uint64_t base = 0;
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t nb = R->plane_bands[p];
            table[p] = fhsn::Band{y0[p], fhsn::band_scale(y0[p], y1[p], nb), nb, (uint32_t)base};
            base += nb;
            if (base > fhsn::MAX_ENTRIES) return false;
        }
        n_bands = (uint32_t)base;
        return true;
    };
    if (!lay_out()) return fail(ctx, FHIP_ERR_OVERFLOW, "slices nesting: 2^32 - 1 bands or more");
    HIP_TRY(ctx, carve());          // (the first lay-out is the largest: halving only shrinks it)
    HIP_TRY(ctx, hipMemcpyAsync(S.loops, up, 3 * (size_t)L * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, times.mark(nullptr));
    for (;;) {
        I.n_bands = n_bands;
        HIP_TRY(ctx, hipMemcpyAsync(S.bands, table.data(), (size_t)P * sizeof(fhsn::Band), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(S.counters, 0, n_counters * 8, st));
        HIP_TRY(ctx, hipMemsetAsync(S.band_count, 0, ((size_t)n_bands + 1) * 4, st));
        hipLaunchKernelGGL(fhm::k_sn_count, cc_grid(n), dim3(256), 0, st, I, S.band_count, S.counters);
        HIP_TRY(ctx, times.mark("k_sn_count"));
        HIP_TRY(ctx, read_counter(fhm::FH_SN_ENTRIES, n_entries));
        bool halved = false;
        if (!bands && n_entries > (uint64_t)fhsn::ENTRY_MULTIPLE * regular_segments)
            for (uint32_t& nb : R->plane_bands)
                if (nb > 1) { nb /= 2; halved = true; }
        if (!halved) break;
        (void)lay_out();
    }
    if (n_entries > fhsn::MAX_ENTRIES) return fail(ctx, FHIP_ERR_OVERFLOW, "slices nesting: 2^32 - 1 band entries or more");
    R->n_bands = n_bands; R->n_entries = n_entries;
    HIP_TRY(ctx, carve());
    HIP_TRY(ctx, ctr_scan(st, S.band_count, n_bands, S.band_start, S.scan_tmp));
    HIP_TRY(ctx, hipMemcpyAsync(S.band_count, S.band_start, (size_t)n_bands * 4, hipMemcpyDeviceToDevice, st));          // the cursors
    hipLaunchKernelGGL(fhm::k_sn_fill, cc_grid(n), dim3(256), 0, st, I, S.band_count, (uint32_t)n_entries, S.entry_ends, S.entry_loop);
    HIP_TRY(ctx, times.mark("scan + k_sn_fill"));
    const dim3 waves((unsigned)(((uint64_t)L + 3) / 4));
    hipLaunchKernelGGL(fhm::k_sn_hits<false>, waves, dim3(256), 0, st, I, (const uint32_t*)S.band_start, (const float4*)S.entry_ends, (const uint32_t*)S.entry_loop,
                       (uint32_t)n_entries, S.hit_count, (const uint32_t*)nullptr, 0u, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, S.counters);
    HIP_TRY(ctx, times.mark("k_sn_hits count"));
    HIP_TRY(ctx, read_counter(fhm::FH_SN_HITS, n_hits));
    uint64_t n_long = 0;          // (the lists too long for LDS; from the copy of the counters just read)
    for (size_t r = fhm::FH_SN_LONG; r < n_counters; r += fhm::FH_MT_COUNTERS) n_long += rows[r];
    if (n_hits > fhsn::MAX_ENTRIES) return fail(ctx, FHIP_ERR_OVERFLOW, "slices nesting: 2^32 - 1 hits or more");
    R->n_hits = n_hits;
    HIP_TRY(ctx, carve());
    HIP_TRY(ctx, hipMalloc((void**)&R->d_parent, (size_t)L * 4));
    HIP_TRY(ctx, hipMalloc((void**)&R->d_depth, (size_t)L * 4));
    HIP_TRY(ctx, hipMemsetAsync(S.n_children, 0, ((size_t)L + (size_t)fhm::FH_SN_PLANE_WORDS * P) * 4, st));
    HIP_TRY(ctx, ctr_scan(st, S.hit_count, L, S.hit_base, S.scan_tmp));
    hipLaunchKernelGGL(fhm::k_sn_hits<true>, waves, dim3(256), 0, st, I, (const uint32_t*)S.band_start, (const float4*)S.entry_ends, (const uint32_t*)S.entry_loop,
                       (uint32_t)n_entries, (uint32_t*)nullptr, (const uint32_t*)S.hit_base, (uint32_t)n_hits, S.hits, S.contain, R->d_depth, S.counters);
    HIP_TRY(ctx, times.mark("scan + k_sn_hits"));
    if (n_long) {
        hipLaunchKernelGGL(fhm::k_sn_contain, waves, dim3(256), 0, st, I.flags, L, (const uint32_t*)S.hit_base, (uint32_t)n_hits, (const uint32_t*)S.hits, S.contain, R->d_depth);
        HIP_TRY(ctx, times.mark("k_sn_contain"));
    }
    hipLaunchKernelGGL(fhm::k_sn_parent, cc_grid(L), dim3(256), 0, st, I, (const uint32_t*)S.hit_base, (uint32_t)n_hits, (const uint32_t*)S.contain,
                       (const uint32_t*)R->d_depth, R->d_parent, S.n_children, S.plane_counts);
    HIP_TRY(ctx, times.mark("k_sn_parent"));
    R->parent.resize(L); R->depth.resize(L); R->n_children.resize(L); R->region_area2.resize(L);
    const size_t n_counts = (size_t)fhm::FH_SN_PLANE_WORDS * P, down_bytes = (3 * (size_t)L + n_counts) * 4;
    HIP_TRY(ctx, pinned_ensure(ctx, down_bytes));
    uint32_t* const down = (uint32_t*)ctx->mesh_pinned;          // parent, depth [L]; then n_children [L] and the planes' counts, one piece on the device too
    HIP_TRY(ctx, hipMemcpyAsync(down, R->d_parent, (size_t)L * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(down + L, R->d_depth, (size_t)L * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(down + 2 * (size_t)L, S.n_children, ((size_t)L + n_counts) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    memcpy(R->parent.data(), down, (size_t)L * 4);
    memcpy(R->depth.data(), down + L, (size_t)L * 4);
    memcpy(R->n_children.data(), down + 2 * (size_t)L, (size_t)L * 4);
    const uint32_t* const counts = down + 3 * (size_t)L;
    HIP_TRY(ctx, times.mark("the loops' arrays"));
    for (uint32_t p = 0; p < P; p++) {
        for (uint32_t k = 0; k < fhm::FH_SN_PLANE_WORDS; k++) R->plane_counts[k][p] = counts[(size_t)fhm::FH_SN_PLANE_WORDS * p + k];
        R->n_regular += R->plane_counts[fhm::FH_SN_REGULAR][p];
        R->n_outer += R->plane_counts[fhm::FH_SN_OUTER][p];
        R->n_top += R->plane_counts[fhm::FH_SN_TOP][p];
        R->max_depth = std::max(R->max_depth, R->plane_counts[fhm::FH_SN_MAX_DEPTH][p]);
        R->n_improper += R->plane_counts[fhm::FH_SN_IMPROPER][p];
        R->n_misoriented += R->plane_counts[fhm::FH_SN_MISORIENTED][p];
    }
    // a loop's own area2, then its children's in ascending id: the loops in ascending order, each into its parent's sum
    // (an irregular loop is no one's child and has none: 0)
    for (size_t l = 0; l < L; l++) R->region_area2[l] = R->depth[l] == fhsn::NONE ? 0.0 : s->loop_area2[l];
    for (size_t l = 0; l < L; l++)
        if (R->parent[l] != fhsn::NONE && R->parent[l] < L) R->region_area2[R->parent[l]] += s->loop_area2[l];
    *out = R.release();
    return FHIP_OK;
}
// {loops, regular, outer, top, max_depth, improper, misoriented, planes, bands, band entries, hits, 0 ..}
void fhip_slice_nesting_counts(const void* h, uint64_t out[16]) {
    const fhip_slice_nesting* const t = (const fhip_slice_nesting*)h;
    for (int k = 0; k < 16; k++) out[k] = 0;
    if (!t) return;
    const uint64_t c[11] = {t->n_loops, t->n_regular, t->n_outer, t->n_top, t->max_depth, t->n_improper, t->n_misoriented, t->n_planes, t->n_bands, t->n_entries, t->n_hits};
    for (int k = 0; k < 11; k++) out[k] = c[k];
}
fhip_status fhip_slice_nesting_planes(const void* h, uint64_t* regular, uint64_t* outer, uint64_t* top, uint64_t* max_depth, uint64_t* improper, uint64_t* misoriented,
                                      uint32_t* bands) {
    const fhip_slice_nesting* const t = (const fhip_slice_nesting*)h;
    if (!t) return FHIP_ERR_BAD_TAPE;
    const size_t P = (size_t)t->n_planes;
    if (P == 0) return FHIP_OK;
    uint64_t* const cols[fhm::FH_SN_PLANE_WORDS] = {regular, outer, top, max_depth, improper, misoriented};
    for (uint32_t k = 0; k < fhm::FH_SN_PLANE_WORDS; k++)
        if (cols[k]) memcpy(cols[k], t->plane_counts[k].data(), P * 8);
    if (bands) memcpy(bands, t->plane_bands.data(), P * 4);
    return FHIP_OK;
}
fhip_status fhip_slice_nesting_loops(const void* h, uint32_t* parent, uint32_t* depth, uint32_t* n_children, double* region_area2) {
    const fhip_slice_nesting* const t = (const fhip_slice_nesting*)h;
    if (!t) return FHIP_ERR_BAD_TAPE;
    const size_t L = (size_t)t->n_loops;
    if (L == 0) return FHIP_OK;
    if (t->parent.empty()) {          // (an empty result has no arrays: every loop is irregular, or there is no plane)
        for (size_t l = 0; l < L; l++) {
            if (parent) parent[l] = fhsn::NONE;
            if (depth) depth[l] = fhsn::NONE;
            if (n_children) n_children[l] = 0;
            if (region_area2) region_area2[l] = 0;
        }
        return FHIP_OK;
    }
    if (parent) memcpy(parent, t->parent.data(), L * 4);
    if (depth) memcpy(depth, t->depth.data(), L * 4);
    if (n_children) memcpy(n_children, t->n_children.data(), L * 4);
    if (region_area2) memcpy(region_area2, t->region_area2.data(), L * 8);
    return FHIP_OK;
}
const uint32_t* fhip_slice_nesting_parent_dev(const void* h) { return HANDLE_GET(fhip_slice_nesting, h, d_parent); }
const uint32_t* fhip_slice_nesting_depth_dev(const void* h) { return HANDLE_GET(fhip_slice_nesting, h, d_depth); }
void fhip_slice_nesting_free(void* h) { delete (fhip_slice_nesting*)h; }
