"""The device context: `HipContext` (fhip_ctx: one device + stream, its options, counters and diagnostics) and the process's default
one.  `_default_ctx` is this module's state: read it through `default_context()`."""
import ctypes as C
import os

import numpy as np

from ._abi import FidgetHipError, _p, lib


class HipContext:
    """fhip_ctx: one device + stream.  `stream` may be a raw hipStream_t (e.g. torch's)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        st = lib().fhip_ctx_create(device, C.c_void_p(stream or 0), C.byref(h))
        if st != 0:
            raise FidgetHipError(st, "no usable HIP device: fidget_amd has no CPU fallback")
        self._h = h

    def __del__(self):
        try:
            lib().fhip_ctx_destroy(self._h)
        except Exception:
            pass

    def check(self, st):
        if st != 0:
            raise FidgetHipError(st, (lib().fhip_last_error(self._h) or b"").decode())

    def sync(self):
        self.check(lib().fhip_ctx_sync(self._h))

    def trim(self):
        """fhip_ctx_trim: memory kept between calls for speed alone (mesh leaf records and the scratch of `voxelize_mesh` in the same buffer, frame lanes) goes back to the device"""
        self.check(lib().fhip_ctx_trim(self._h))

    def reserve_arena(self, megabytes):
        """fhip_ctx_reserve_arena: every buffer set's tape arena at least this large from the next frame on"""
        self.check(lib().fhip_ctx_reserve_arena(self._h, int(megabytes)))

    def cancel(self):
        lib().fhip_cancel(self._h)

    def cancel_watch(self, flag):
        """fhip_cancel_watch: `flag` = a numpy uint8 array of one element the context reads beside its own flag (None: stop watching)"""
        self._watched = flag          # (kept alive while it is watched)
        lib().fhip_cancel_watch(self._h, None if flag is None else flag.ctypes.data_as(C.c_void_p))

    def cancel_reset(self):
        lib().fhip_cancel_reset(self._h)

    def lane_tune(self):
        """What the frame arrangement tuner knows about the kind of 3D frame queued last (fhip_debug_lane_tune): phase 0 .. 2 measuring
        (stage pipeline, lanes, stage pipeline again), 3 waiting, 4 decided, -1 none; ms per frame of the three windows; the decision."""
        ms, ln = (C.c_float * 3)(), C.c_int(0)
        ph = lib().fhip_debug_lane_tune(self._h, ms, C.byref(ln))
        return {"phase": int(ph), "stage_pipeline_ms": [float(ms[0]), float(ms[2])], "frame_lanes_ms": float(ms[1]), "kept": "frame lanes" if ln.value else "stage pipeline"}

    def lane_frames(self):
        """Frames of this context that went to a frame lane so far (fhip_debug_lane_frames)"""
        return int(lib().fhip_debug_lane_frames(self._h))

    def rare_frames(self):
        """3D frames of this context rendered in rare mode so far - the launches for tapes beyond the assembly kernels' register files folded
        into the slab's other launches (fhip_debug_rare_frames; capi_render.hpp)"""
        return int(lib().fhip_debug_rare_frames(self._h))

    def rare_launches(self):
        """Launches this context's by-list frames made for nothing but rare mode's blocks so far: one per slab of such a frame
        (fhip_debug_rare_launches)"""
        return int(lib().fhip_debug_rare_launches(self._h))

    def set_option(self, name, value=1):
        """A behaviour switch of this context (fhip_ctx_set_option: "no_column_inv", "frame_lanes", ...).  The environment
        (FHIP_<NAME>) is read once, when the context is created; this is the only way to change a switch afterwards."""
        self.check(lib().fhip_ctx_set_option(self._h, name.encode(), int(value)))

    def option(self, name):
        v = C.c_int(0)
        self.check(lib().fhip_ctx_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def options(self, **kw):
        """Context manager: switches set for the duration of a block, then restored."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: self.option(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return scope()

    def profile(self, on):
        lib().fhip_profile_enable(self._h, int(on))

    def profile_read(self):
        ms = np.zeros(4, np.float64)
        n = np.zeros(4, np.uint32)
        self.check(lib().fhip_profile_read(self._h, _p(ms), _p(n)))
        names = ["tiles", "points", "normals", "other"]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def profile_read_kernels(self):
        """(ms, launches) of the last profiled frame per assembly kernel, every launch timed on its own."""
        ms = np.zeros(8, np.float64)
        n = np.zeros(8, np.uint32)
        self.check(lib().fhip_profile_read_kernels(self._h, _p(ms), _p(n)))
        # (fh_prune1: the root level's prune, i.e. k_prune2 with the scalar sweep behind it when option prune2 is on)
        names = ["fh_columns", "fh_float_eval_16x4", "fh_float_eval_32x2", "fh_tiles", "fh_prune1", "fh_tiles_v32", "fh_tiles_v64", "unused"]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def counters(self):
        c = np.zeros(8, np.uint64)
        self.check(lib().fhip_render_counters(self._h, _p(c)))
        return {"arena_ops": int(c[0]), "arena_overflow": int(c[1]), "leaves_last_slab": int(c[2]),
                "queue_overflow": int(c[3]), "groups_last_slab": [int(v) for v in c[4:6]], "hip_tile_stage_frames": int(c[6]), "substituted_tile_lists": int(c[7])}

    def last_leaves(self, cap=1 << 20):
        """Leaf records of the last slab of the last 3D frame: structured array (off, len, regs, choices, x, y, z)."""
        dt = np.dtype([("off", np.uint32), ("len", np.uint32), ("regs", np.uint16), ("choices", np.uint16),
                       ("x", np.uint32), ("y", np.uint32), ("z", np.uint32)])
        buf = np.zeros(cap, dt)
        n = lib().fhip_debug_leaves(self._h, _p(buf), cap)
        return buf[:n]

    def groups(self, kind, index, cap=1 << 20):
        """Work-queue entries the last 3D frame left behind (kind 0: tile level `index`; 1: parked z-slab `index`):
        (structured array (off, len, regs, choices, x, y, z, ...), (n_small_layout, n_other))."""
        dt = np.dtype([("off", np.uint32), ("len", np.uint32), ("regs", np.uint16), ("choices", np.uint16),
                       ("x", np.uint32), ("y", np.uint32), ("z", np.uint32), ("first", np.uint32), ("n", np.uint32), ("stride", np.uint32)])
        assert dt.itemsize == 36  # sizeof(FhGroup)
        buf = np.zeros(cap, dt)
        cnt = np.zeros(2, np.uint32)
        n = lib().fhip_debug_groups(self._h, kind, index, _p(buf), cap, _p(cnt))
        return buf[:n], (int(cnt[0]), int(cnt[1]))

    def arena_ops(self, off, n):
        """`n` device-format ops of the tape arena from op `off` (diagnostics; see last_leaves)."""
        buf = np.zeros(n, np.uint64)
        got = lib().fhip_debug_arena(self._h, int(off), int(n), _p(buf))
        return buf[:got]

    def leaf_stats(self):
        """Leaf-stage counters of the last profiled 3D frame (render_state.h leaf_stat)."""
        c = np.zeros(8, np.uint64)
        self.check(lib().fhip_debug_leaf_stats(self._h, _p(c)))
        return {"leaves": int(c[0]), "tape_ops": int(c[1]), "tape_words_read": int(c[2]), "lane_ops": int(c[3]),
                "prune2_phase_clocks_max": [int(v) for v in c[4:8]]}

    def wave_stats(self):
        """Per kernel kind: mean / max busy microseconds of the waves that found work, their
        number and the units of work they pulled (frame totals)."""
        c = np.zeros(64, np.uint64)
        self.check(lib().fhip_debug_stats(self._h, _p(c)))
        names = ["tiles_l0", "tiles_l1", "tiles_l2", "tiles_l3", "tiles_l4", "columns_c0", "columns_c12", "tiles_2d"]
        self.tile_v = {f"l{l}": {"slots": int(c[8 + l]), "fwd_clocks": int(c[16 + l]), "prune_clocks": int(c[24 + l]), "max_slot_clocks": int(c[l])}
                       for l in range(8) if c[8 + l]}
        self.tile_phases = {f"l{l}": {"fwd_us": int(c[32 + l]) / 100.0, "prune_us": int(c[40 + l]) / 100.0,
                                      "ops": int(c[48 + l]), "ops_written": int(c[56 + l]), "fwd_shader_clocks": int(c[16 + l])} for l in range(8) if c[48 + l]}
        return {k: {"busy_us_sum": int(c[4 * i]) / 100.0, "busy_us_max": int(c[4 * i + 1]) / 100.0,
                    "waves": int(c[4 * i + 2]), "units": int(c[4 * i + 3])} for i, k in enumerate(names) if c[4 * i + 2]}


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = HipContext(int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("FHIP_USE_LOCAL_RANK") else 0)
    return _default_ctx
