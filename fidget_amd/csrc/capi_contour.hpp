// ---- contours of a 2D slice -----------------------------------------------------------------------------------------------------------------
// fhip_contour2d (fidget_hip.h; the handle it declares void* is a fhip_contours): the pixel-perfect render2d frame into the context's buffer, then the four k_ctr_* passes of mesh.hip with
// the two prefix sums between them, all on the context's stream.  The host waits once in the middle - for the two totals, which size the
// arrays of the result - and once at the end.  A fragment of the C ABI, included by capi_mesh.hpp; uses capi_mesh_util.hpp.
struct fhip_contours {
    uint64_t n_vertices = 0, n_segments = 0;
    uint32_t width = 0, height = 0;
    int device = 0;
    float2* d_vertices = nullptr;
    uint2* d_segments = nullptr;
    uint32_t* d_next = nullptr;
    ~fhip_contours() {
        if (d_vertices) (void)hipFree(d_vertices);
        if (d_segments) (void)hipFree(d_segments);
        if (d_next) (void)hipFree(d_next);
    }
};
fhip_status fhip_contour2d(fhip_ctx* ctx, const fhip_tape* tape, const fhip_render2d_config* cfg, void** out) {
    if (out) *out = nullptr;
    if (!ctx || !tape || !cfg || !out) return fail(ctx, FHIP_ERR_BAD_TAPE, "fhip_contour2d: context, tape, configuration and result");
    const uint32_t W = cfg->width, H = cfg->height;
    if (!fhctr::size_ok(W, H)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "contours: 2^32 pixels or lattice edges and more");
    (void)hipSetDevice(ctx->device);
    std::unique_ptr<fhip_contours> R(new fhip_contours());
    R->width = W; R->height = H; R->device = ctx->device;
    if (W == 0 || H == 0) { *out = R.release(); return FHIP_OK; }
    fhip_render2d_config c = *cfg;
    c.pixel_perfect = 1;        // a true value at every pixel, no fills
    std::shared_ptr<const fhip_tape> bound;     // (as fhip_render2d)
    if (tape->t.n_vars > FH_MAX_INPUTS) {
        const fhip_status bs = bound_tape(ctx, tape, c.axis_slots, c.var_keys, c.var_values, c.n_vars, bound);
        if (bs) return bs;
        tape = bound.get();
        c.axis_slots = BOUND_AXES; c.var_keys = nullptr; c.var_values = nullptr; c.n_vars = 0;
    }
    ctx->tune_cur = -1;
    ctx->tune_last_key = 0;
    const size_t npix = (size_t)W * H;
    HIP_TRY(ctx, ctx->io_a.ensure(npix * 4));
    const float* const img = (const float*)ctx->io_a.p;
    { const fhip_status st = render2d_frame(ctx, tape, &c, (float*)ctx->io_a.p, 1); if (st) return st; }
    // what the passes hand to each other, in one buffer: the edges' ballot words, the block counts and their sums, the scans' block totals
    const uint32_t eb = (uint32_t)((fhctr::n_edges(W, H) + 255) / 256), cb = (uint32_t)((fhctr::n_cells(W, H) + 255) / 256);
    const size_t scan_words = std::max(ctr_scan_words(eb), ctr_scan_words(cb));
    HIP_TRY(ctx, ctx->io_b.ensure((size_t)eb * 32 + ((size_t)2 * eb + 2 * (size_t)cb + 2 + scan_words) * 4 + 16));
    uint64_t* const bits = (uint64_t*)ctx->io_b.p;
    uint32_t* const e_cnt = (uint32_t*)(bits + (size_t)eb * 4);
    uint32_t* const e_off = e_cnt + eb;          // eb + 1
    uint32_t* const c_cnt = e_off + eb + 1;
    uint32_t* const c_off = c_cnt + cb;          // cb + 1
    uint32_t* const scan_tmp = c_off + cb + 1;
    hipStream_t st = ctx->stream;
    auto grid = [](uint32_t nb) { return dim3(std::max(1u, std::min(nb, fhm::FH_CTR_BLOCKS))); };
    if (eb) {
        hipLaunchKernelGGL(fhm::k_ctr_edges, grid(eb), dim3(256), 0, st, img, W, H, bits, e_cnt);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, ctr_scan(st, e_cnt, eb, e_off, scan_tmp));
    if (cb) {
        hipLaunchKernelGGL(fhm::k_ctr_cells, grid(cb), dim3(256), 0, st, img, W, H, c_cnt);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, ctr_scan(st, c_cnt, cb, c_off, scan_tmp));      // (the same block totals' room: the stream keeps the two scans in order)
    uint32_t totals[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&totals[0], e_off + eb, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&totals[1], c_off + cb, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    R->n_vertices = totals[0]; R->n_segments = totals[1];
    if (totals[0]) {
        HIP_TRY(ctx, hipMalloc((void**)&R->d_vertices, (size_t)totals[0] * 8));
        HIP_TRY(ctx, hipMalloc((void**)&R->d_next, (size_t)totals[0] * 4));
        hipLaunchKernelGGL(fhm::k_ctr_vertices, grid(eb), dim3(256), 0, st, img, W, H, (const uint64_t*)bits, (const uint32_t*)e_off, R->d_vertices, R->d_next);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (totals[1]) {       // (a segment joins two vertices: there are some)
        HIP_TRY(ctx, hipMalloc((void**)&R->d_segments, (size_t)totals[1] * 8));
        hipLaunchKernelGGL(fhm::k_ctr_segments, grid(cb), dim3(256), 0, st, img, W, H, (const uint64_t*)bits, (const uint32_t*)e_off, (const uint32_t*)c_off, R->d_segments, R->d_next);
        HIP_TRY(ctx, hipGetLastError());
    }
    { const fhip_status fs = finish_render(ctx); if (fs) return fs; }      // waits for the stream; the frame's own checks
    *out = R.release();
    return FHIP_OK;
}
void fhip_contours_counts(const void* h, uint64_t out[4]) {
    const fhip_contours* const c = (const fhip_contours*)h;
    out[0] = c ? c->n_vertices : 0; out[1] = c ? c->n_segments : 0; out[2] = c ? c->width : 0; out[3] = c ? c->height : 0;
}
// the arrays to the host: refused without a handle, and without a destination for an array that is not empty
fhip_status fhip_contours_vertices(const void* h, float* out) {
    const fhip_contours* const c = (const fhip_contours*)h;
    if (!c || (c->n_vertices && !out)) return FHIP_ERR_BAD_TAPE;
    return handle_to_host(c->device, out, c->d_vertices, (size_t)c->n_vertices * 8);
}
fhip_status fhip_contours_segments(const void* h, uint32_t* out) {
    const fhip_contours* const c = (const fhip_contours*)h;
    if (!c || (c->n_segments && !out)) return FHIP_ERR_BAD_TAPE;
    return handle_to_host(c->device, out, c->d_segments, (size_t)c->n_segments * 8);
}
fhip_status fhip_contours_next(const void* h, uint32_t* out) {
    const fhip_contours* const c = (const fhip_contours*)h;
    if (!c || (c->n_vertices && !out)) return FHIP_ERR_BAD_TAPE;
    return handle_to_host(c->device, out, c->d_next, (size_t)c->n_vertices * 4);
}
const float* fhip_contours_vertices_dev(const void* h) { return (const float*)HANDLE_GET(fhip_contours, h, d_vertices); }
const uint32_t* fhip_contours_segments_dev(const void* h) { return (const uint32_t*)HANDLE_GET(fhip_contours, h, d_segments); }
void fhip_contours_free(void* h) { delete (fhip_contours*)h; }
fhip_status fhip_contour_loops(const uint32_t* next, uint64_t n, uint32_t* order, uint64_t* loop_start, uint8_t* closed, uint64_t* n_loops) {
    if (n_loops) *n_loops = 0;
    if (n >= fhctr::NONE || (n && !next)) return FHIP_ERR_UNSUPPORTED;
    return fhctr::follow_loops(next, n, order, loop_start, closed, n_loops) ? FHIP_OK : FHIP_ERR_UNSUPPORTED;
}
