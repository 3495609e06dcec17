"""ctypes face of oracle/liboracle.so — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module; the
product package (magr_ray_tracer_amd) never does.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
S1, S0 = 1, 0

OrcConfig = np.dtype([(n, "<i4") for n in ("width", "height", "max_bounces", "shading", "sampling", "accel",
                                            "russian_roulette", "filter_fireflies", "schedule", "connect_order")])
OrcCounters = np.dtype([(n, "<u8") for n in ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests")])
OrcRayWork = np.dtype([(n, "<u4") for n in ("node_visits", "prim_tests", "tlas_visits", "inst_visits", "occluded")])
REFERENCE_ORDER, LATER_EXIT = 0, 1      # OrcConfig.connect_order


class _Scene(C.Structure):
    _fields_ = [("prims", C.c_void_p), ("nPrims", C.c_int32), ("mats", C.c_void_p), ("nMats", C.c_int32),
                ("tex", C.c_void_p), ("nTex", C.c_int32), ("lights", C.c_void_p), ("nLights", C.c_int32),
                ("bvh2", C.c_void_p), ("bvh4", C.c_void_p), ("nNodes", C.c_int32), ("primIdx", C.c_void_p), ("nIdx", C.c_int32),
                ("tlas", C.c_void_p), ("nTlas", C.c_int32), ("blas", C.c_void_p), ("nBlas", C.c_int32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "liboracle.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -m magr_ray_tracer_amd.build`")
        L = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int32
        L.orc_seed_stream.argtypes = [vp, C.c_int64, C.c_int64]
        L.orc_generate.argtypes = [vp, i32, i32, vp, vp, i32, vp]
        L.orc_extend.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
        L.orc_shade.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orc_connect.argtypes = [vp, i32, vp, vp, vp, vp]
        L.orc_connect_work.argtypes = [vp, i32, vp, vp, vp]
        L.orc_occluded.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.orc_focus.argtypes = [i32, i32, vp, vp, vp]
        L.orc_focus.restype = C.c_float
        L.orc_frame_work_bytes.argtypes = [i32, vp]
        L.orc_frame_work_bytes.restype = C.c_size_t
        L.orc_render_frame.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
        L.orc_render_bands.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
        L.orc_trace_normals.argtypes = [vp, vp, vp, i32, vp]
        L.orc_postproc.argtypes = [vp, i32, i32, i32, C.c_float, C.c_float, C.c_float, vp, vp]
        L.orc_math.argtypes = [i32, vp, vp, C.c_int64]
        L.orc_math_sweep.argtypes = [i32, i32, i32, vp, i32]
        L.orc_math_error.argtypes = [i32, C.c_float, C.c_float, i32, C.c_double, i32, vp]
        L.orc_xorshift32.argtypes = [vp]
        L.orc_xorshift32.restype = C.c_uint32
        L.orc_xorshift32_jump.argtypes = [C.c_uint32, C.c_uint64]
        L.orc_xorshift32_jump.restype = C.c_uint32
        L.orc_rejection_cycle.argtypes = [i32, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def seed_stream(first, n):
    s = np.zeros(n, dtype=np.uint32)
    lib().orc_seed_stream(_p(s), first, n)
    return s


def nonzero_seeds(seeds, what):
    """State 0 is the RNG's fixed point: every draw from it is 0.0f and sample_ball's rejection loop never ends.
    The oracle has the same loop, so a zero seed is refused here, as rt_set_seeds refuses it, instead of spinning."""
    if seeds is not None:
        z = np.flatnonzero(np.asarray(seeds) == 0)
        if len(z):
            raise ValueError(f"{what}: seeds[{int(z[0])}] is 0, the fixed point of the RNG ({len(z)} of {np.size(seeds)} seeds are 0)")
    return seeds


def xorshift32(state, steps=1):
    """The state after `steps` RNG steps from `state` (orc_xorshift32; more than a few steps go through orc_xorshift32_jump)."""
    if steps > 64:
        return int(lib().orc_xorshift32_jump(int(state), int(steps)))
    s = C.c_uint32(int(state))
    for _ in range(steps):
        lib().orc_xorshift32(C.addressof(s))
    return int(s.value)


OrcRejection = np.dtype([("states", "<u8"), ("rejected", "<u8"), ("longest", "<u4"), ("state", "<u4"), ("index", "<u4"), ("closed", "<i4")], align=True)


def rejection_cycle():
    """orc_rejection_cycle: sample_ball's rejection loop over the RNG's whole cycle; dict states, rejected, longest, state, index, closed."""
    r = np.zeros((), OrcRejection)
    if lib().orc_rejection_cycle(math_threads(), r.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("orc_rejection_cycle: bad argument")
    return {k: int(r[k]) for k in r.dtype.names}


def postproc(accum, frames, vignette=0.0, gamma=0.9, chromatic=0.0):
    a = np.ascontiguousarray(accum, dtype=np.float32)
    H, W = a.shape[:2]
    f = np.zeros((H, W, 4), np.float32)
    b = np.zeros((H, W, 4), np.uint8)
    lib().orc_postproc(_p(a), W, H, int(frames), float(vignette), float(gamma), float(chromatic), _p(f), _p(b))
    return f, b


OrcMathError = np.dtype([("max_err", "<f8"), ("arg", "<f4"), ("above", "<u8"), ("count", "<u8")], align=True)


def math_threads():
    """Threads of the exhaustive sweeps: the CPUs this process may use, at most 16."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def math(fn, x):
    """orc_math: x is an (n, in_words) array of 32-bit words (any 4-byte dtype); returns (n, out_words) uint32 (rt_debug_math layout)."""
    from magr_ray_tracer_amd import _lib as W
    wi, wo = W.MATH_WORDS[fn]
    a = np.ascontiguousarray(x).view(np.uint32).reshape(-1, wi)
    out = np.zeros((len(a), wo), np.uint32)
    if lib().orc_math(fn, _p(a), _p(out), len(a)) != 0:
        raise ValueError(f"orc_math: bad function id {fn}")
    return out


def math_sweep(fn, first_block=0, n_blocks=None):
    """orc_math_sweep: block hashes of a one-argument function (rt_debug_math_sweep layout)."""
    from magr_ray_tracer_amd import _lib as W
    if n_blocks is None:
        n_blocks = (1 << (32 - W.MATH_SWEEP_BLOCK_BITS)) - first_block
    h = np.zeros(n_blocks, np.uint64)
    if lib().orc_math_sweep(fn, first_block, n_blocks, _p(h), math_threads()) != 0:
        raise ValueError("orc_math_sweep: bad argument")
    return h


def math_error(fn, lo, hi, absolute=False, bound=np.inf):
    """orc_math_error: exhaustive error over the floats in [lo, hi] against libm double; dict max_err, arg, above, count."""
    r = np.zeros((), OrcMathError)
    if lib().orc_math_error(fn, lo, hi, int(absolute), float(bound), math_threads(), r.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("orc_math_error: bad argument")
    return {"max_err": float(r["max_err"]), "arg": np.float32(r["arg"]), "above": int(r["above"]), "count": int(r["count"])}


class Oracle:
    """Holds one scene (SceneArrays-like object with numpy arrays) + variant config."""

    def __init__(self, sa, width, height, shading=1, sampling=1, accel=0, russian_roulette=True, filter_fireflies=True,
                 max_bounces=7, schedule=S1, connect_order=REFERENCE_ORDER):
        """connect_order LATER_EXIT: shadow rays walk a BVH2 BLAS in the HIP path's any-hit order (oracle.h); only connect's node and
        primitive counts depend on it."""
        self.sa = sa
        self.cfg = np.zeros((), dtype=OrcConfig)
        c = self.cfg
        c["width"], c["height"], c["max_bounces"] = width, height, max_bounces
        c["shading"], c["sampling"], c["accel"] = shading, sampling, accel
        c["russian_roulette"], c["filter_fireflies"], c["schedule"] = int(russian_roulette), int(filter_fireflies), schedule
        c["connect_order"] = connect_order
        self.width, self.height = width, height
        s = _Scene()
        s.prims, s.nPrims = _p(sa.prims), len(sa.prims)
        s.mats, s.nMats = _p(sa.mats), len(sa.mats)
        s.tex, s.nTex = _p(sa.tex), len(sa.tex)
        s.lights, s.nLights = _p(sa.lights), len(sa.lights)
        s.bvh2, s.bvh4 = _p(sa.bvh2), _p(sa.bvh4)
        s.nNodes = len(sa.bvh2)
        s.primIdx, s.nIdx = _p(sa.primIdx), len(sa.primIdx)
        s.tlas, s.nTlas = _p(sa.tlas), len(sa.tlas)
        s.blas, s.nBlas = _p(sa.blas), len(sa.blas)
        self._scene = s

    @property
    def _sc(self):
        return C.cast(C.pointer(self._scene), C.c_void_p)

    @property
    def _cfg(self):
        return self.cfg.ctypes.data_as(C.c_void_p)

    def generate(self, cam, first_pixel, n, seeds, antiAliasing=1):
        from magr_ray_tracer_amd import _lib as W
        rays = np.zeros(n, dtype=W.Ray)
        nonzero_seeds(seeds, "Oracle.generate")
        c = np.ascontiguousarray(cam)
        lib().orc_generate(_p(rays), n, first_pixel, self._cfg, c.ctypes.data_as(C.c_void_p), antiAliasing, _p(seeds))
        return rays

    def extend(self, rays, renderBVH=0, accum=None, want_steps=False):
        steps = np.zeros(len(rays), dtype=np.int32) if want_steps else None
        ctr = np.zeros((), dtype=OrcCounters)
        lib().orc_extend(_p(rays), len(rays), self._sc, self._cfg, renderBVH, _p(accum) if accum is not None else None,
                         _p(steps) if steps is not None else None, ctr.ctypes.data_as(C.c_void_p))
        return steps, {k: int(ctr[k]) for k in ctr.dtype.names}

    def shade(self, rays, accum, seeds, shadow_capacity=None):
        from magr_ray_tracer_amd import _lib as W
        n = len(rays)
        nonzero_seeds(seeds, "Oracle.shade")
        out = np.zeros(max(n, 1), dtype=W.Ray)
        sh = np.zeros(max(shadow_capacity or n, 1), dtype=W.ShadowRay)
        nOut, nSh = C.c_int32(0), C.c_int32(0)
        lib().orc_shade(_p(rays), n, _p(out), C.addressof(nOut), _p(sh), C.addressof(nSh), self._sc, self._cfg, _p(accum), _p(seeds))
        return out[:nOut.value].copy(), sh[:nSh.value].copy()

    def connect(self, shadow, accum):
        ctr = np.zeros((), dtype=OrcCounters)
        if len(shadow):
            lib().orc_connect(_p(shadow), len(shadow), self._sc, self._cfg, _p(accum), ctr.ctypes.data_as(C.c_void_p))
        return {k: int(ctr[k]) for k in ctr.dtype.names}

    def connect_work(self, shadow):
        """Per shadow ray (OrcRayWork): node visits, primitive tests, TLAS and instance visits, occluded.  Accumulates nothing."""
        work = np.zeros(len(shadow), dtype=OrcRayWork)
        shadow = np.ascontiguousarray(shadow)
        if len(shadow):
            lib().orc_connect_work(_p(shadow), len(shadow), self._sc, self._cfg, _p(work))
        return work

    def occluded(self, origins, dirs, tmax=None):
        """orc_occluded: connect's traversal on rays (n, 3) or (n, 4) float32 with reach tmax (None: RT_REALLYFAR); n bools."""
        n = len(origins)
        o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        o4[:, :3], d4[:, :3] = np.asarray(origins, np.float32)[:, :3], np.asarray(dirs, np.float32)[:, :3]
        t = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        out = np.zeros(n, np.uint8)
        if n:
            lib().orc_occluded(_p(o4), _p(d4), None if t is None else _p(t), n, self._sc, self._cfg, _p(out))
        return out.astype(bool)

    def focus(self, x, y, cam):
        c = np.ascontiguousarray(cam)
        return np.float32(lib().orc_focus(x, y, self._sc, self._cfg, c.ctypes.data_as(C.c_void_p)))

    def render(self, cam, frames, accum=None, seeds=None, y0=0, y1=None, threads=1, antiAliasing=1):
        """frames x RayTrace() over rows [y0,y1); threads>1 splits into independent row bands (baseline mode)."""
        y1 = self.height if y1 is None else y1
        n = (y1 - y0) * self.width
        if accum is None:
            accum = np.zeros((self.height, self.width, 4), dtype=np.float32)
        if seeds is None:
            seeds = seed_stream(y0 * self.width, n)
        nonzero_seeds(seeds, "Oracle.render")
        e, c = np.zeros((), dtype=OrcCounters), np.zeros((), dtype=OrcCounters)
        cm = np.ascontiguousarray(cam)
        lib().orc_render_bands(self._sc, self._cfg, cm.ctypes.data_as(C.c_void_p), antiAliasing, y0, y1, frames, threads,
                               _p(accum), _p(seeds), e.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p))
        return accum, seeds, {k: int(e[k]) for k in e.dtype.names}, {k: int(c[k]) for k in c.dtype.names}

    def trace_normals(self, cam, threads=1):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        cm = np.ascontiguousarray(cam)
        lib().orc_trace_normals(self._sc, self._cfg, cm.ctypes.data_as(C.c_void_p), threads, _p(out))
        return out
