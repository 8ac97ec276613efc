// Fragment of capi.hip: what more than one fragment of the mesh path uses - the pinned landing area and the copies through it, scoped
// device buffers, the prefix sum, the grid of a pass over n items, a bitmap's way in and the checks of its arguments, the pass timer,
// a handle's arrays to the host.  Included once, at the top of capi_mesh.hpp, so every fragment in that file's list may use all of it;
// it uses capi_core.hpp (fhip_ctx, DevBuf, fail, HIP_TRY), capi_effects.hpp (FxStage) and the kernels of mesh.hip.
#include <stdarg.h>
// The context's pinned landing area (leaf records, octree cells and finished meshes on their way to the host), kept between calls - pinning
// 17 GB takes over a second: at least `bytes`, and an eighth more where it has to grow
static hipError_t pinned_ensure(fhip_ctx* ctx, size_t bytes) {
    if (ctx->mesh_pinned_cap >= bytes) return hipSuccess;
    if (ctx->mesh_pinned) (void)hipHostFree(ctx->mesh_pinned);
    ctx->mesh_pinned = nullptr; ctx->mesh_pinned_cap = 0;
    const hipError_t e = hipHostMalloc(&ctx->mesh_pinned, bytes + bytes / 8, hipHostMallocDefault);
    if (e == hipSuccess) ctx->mesh_pinned_cap = bytes + bytes / 8;
    return e;
}
static double mesh_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct ScratchBuf : DevBuf {       // a device buffer that goes with its scope (movable for std::vector, not copyable)
    ScratchBuf() = default;
    ScratchBuf(ScratchBuf&& o) noexcept { p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    ~ScratchBuf() { release(); }
};
// `bytes` from device memory to a host buffer of the caller's through the context's pinned landing area, as a built mesh travels
static fhip_status mesh_to_host(fhip_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
    if (!bytes) return FHIP_OK;
    HIP_TRY(ctx, pinned_ensure(ctx, bytes));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->mesh_pinned, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t CH = (size_t)4 << 20;
    fhmesh::parallel_for((bytes + CH - 1) / CH, [&](size_t i) { memcpy((char*)dst + i * CH, (const char*)ctx->mesh_pinned + i * CH, std::min(CH, bytes - i * CH)); });
    return FHIP_OK;
}
// host arrays to the context's buffer `b`; waits, so that the caller's arrays are free again when the call returns
static fhip_status mesh_upload(fhip_ctx* ctx, DevBuf& b, const void* src, size_t bytes) {
    HIP_TRY(ctx, b.ensure(std::max<size_t>(bytes, 4)));
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FHIP_OK;
}
// k_scan_block / k_scan_add over `n` counts (WalkDevX::scan) with the block totals of every level in `tmp`, ctr_scan_words(n) words of it
static size_t ctr_scan_words(uint32_t n) {
    size_t t = 0;
    for (uint32_t nb = (uint32_t)(((uint64_t)n + fhm::FH_SCAN_PER_BLOCK) / fhm::FH_SCAN_PER_BLOCK); nb > 1; nb = (nb + fhm::FH_SCAN_PER_BLOCK) / fhm::FH_SCAN_PER_BLOCK) t += 2 * (size_t)nb + 1;       // (64 bits: n up to 2^32 - 2, the nodes of fhip_voxels_components)
    return t;
}
static hipError_t ctr_scan(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* tmp) {
    const uint32_t nb = (uint32_t)(((uint64_t)n + fhm::FH_SCAN_PER_BLOCK) / fhm::FH_SCAN_PER_BLOCK);       // blocks over the n + 1 sums
    if (nb == 1) {
        hipLaunchKernelGGL(fhm::k_scan_block, dim3(1), dim3(256), 0, st, in, n, out, (uint32_t*)nullptr);
        return hipGetLastError();
    }
    uint32_t* const sums = tmp;
    uint32_t* const sums_off = tmp + nb;
    hipLaunchKernelGGL(fhm::k_scan_block, dim3(nb), dim3(256), 0, st, in, n, out, sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = ctr_scan(st, sums, nb, sums_off, tmp + 2 * (size_t)nb + 1);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fhm::k_scan_add, dim3((unsigned)(((uint64_t)n + 1 + 255) / 256)), dim3(256), 0, st, out, n, (const uint32_t*)sums_off);
    return hipGetLastError();
}
// the grid of a pass of 256-thread blocks over n items: one block at the least
static dim3 cc_grid(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, (n + 255) / 256)); }
// a bitmap's way in, by the effects' convention: a device pointer is used where it is, a host array goes up through io_a
static fhip_status voxels_in(fhip_ctx* ctx, FxStage& st, const uint64_t* bricks, uint32_t depth, const uint64_t*& d_bricks) {
    if (st.on_device && ((uintptr_t)bricks & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "a voxel bitmap on the device must be 8-byte aligned");
    hipError_t e = hipSuccess;
    d_bricks = (const uint64_t*)st.in(ctx->io_a, bricks, (size_t)fhvox::n_words(depth) * 8, e);
    HIP_TRY(ctx, e);
    return FHIP_OK;
}
// The argument checks of a call on a voxel bitmap, in this order: the depth, the bitmap `a` present (`missing`: the entry point's words
// for it), and with a result bitmap `out`: not one of the inputs `a`, `b`; 8-byte aligned where it is on the device
static fhip_status bitmap_args(fhip_ctx* ctx, const char* missing, uint32_t depth, const uint64_t* a, const uint64_t* b = nullptr, const uint64_t* out = nullptr,
                               int out_on_device = 0) {
    if (depth > fhvox::MAX_DEPTH) return fail(ctx, FHIP_ERR_UNSUPPORTED, "voxel depth above 10");
    if (!a) return fail(ctx, FHIP_ERR_UNSUPPORTED, missing);
    if (out && (out == a || out == b)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "a voxel bitmap along a direction: the result must not be an input");
    if (out && out_on_device && ((uintptr_t)out & 7u)) return fail(ctx, FHIP_ERR_UNSUPPORTED, "a voxel bitmap on the device must be 8-byte aligned");
    return FHIP_OK;
}
// FHIP_MESH_TIMES: the wall time of every pass of a call on stderr, "<prefix>: <pass> <seconds> s".  mark() after a pass gives the launch's
// error; with the variable set it then waits for the stream, prints the time since the last mark (`what` null: prints nothing) and
// starts the clock again.  The prefix is printf's, formatted once and only when timing.
namespace {          // (its members are no symbols of the library)
struct PassTimes {
    hipStream_t st;
    bool on;
    double t_last = 0;
    char prefix[96] = "";
    __attribute__((format(printf, 3, 4))) PassTimes(hipStream_t stream, const char* fmt, ...) : st(stream), on(getenv("FHIP_MESH_TIMES") != nullptr) {
        if (!on) return;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(prefix, sizeof(prefix), fmt, ap);
        va_end(ap);
        t_last = mesh_now();
    }
    hipError_t mark(const char* what) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || !on) return e;
        const hipError_t es = hipStreamSynchronize(st);
        if (what) fprintf(stderr, "%s: %-16s %.6f s\n", prefix, what, mesh_now() - t_last);
        t_last = mesh_now();
        return es;
    }
};
}
// `bytes` of a handle's device array to the caller's host array; the handle's own checks - no handle, no destination, no array - are the caller's
static fhip_status handle_to_host(int device, void* dst, const void* d_src, size_t bytes) {
    if (!bytes) return FHIP_OK;
    (void)hipSetDevice(device);
    return hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? FHIP_OK : FHIP_ERR_HIP;
}
// a handle's getter: the member of the T that `h` points to, or nothing (null, 0) for no handle
#define HANDLE_GET(T, h, member) ((h) ? ((const T*)(h))->member : decltype(((const T*)(h))->member){})
