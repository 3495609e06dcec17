"""Device: Python face of one librt355.so context (one per GPU), i.e. the launch/upload half
of the reference's Renderer (src/renderer.cpp:64-94,142-263,289-301) behind the C-ABI of
include/rt355.h.  Everything that computes runs in the HIP kernels; this file only moves
pointers.  `Renderer` wraps the C++ Renderer mirror (Init / Tick / FocusCamera / energy).
"""
import ctypes as C

import numpy as np

from . import _lib


class RtError(RuntimeError):
    code = None   # the RT_E_* value, where the raising call records it


def traversal_plan(facts):
    """The traversal a context with these facts (Device.traversal_facts(), or a dict of _lib.TraversalFacts' fields; missing ones are 0)
    chooses under the RT355_* knobs of the environment (rt_debug_traversal_plan; no GPU): trav (_lib.TRAV_*), spillCap, coherent,
    topAuto, tuneBlocks, connectBlocks and the three tunes as dicts of _lib.TUNE_FIELDS."""
    lib = _lib.device_lib()
    f, p = np.zeros((), dtype=_lib.TraversalFacts), np.zeros((), dtype=_lib.TraversalPlan)
    for n, v in facts.items():
        f[n] = v
    if lib.rt_debug_traversal_plan(f.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)) != 0:
        raise RtError(lib.rt_last_error().decode())
    out = {n: int(p[n]) for n in ("trav", "spillCap", "coherent", "tuneBlocks", "connectBlocks")}
    out["topAuto"] = bool(p["topAuto"])
    for n in ("tune", "tuneConnect", "tune4"):
        out[n] = dict(zip(_lib.TUNE_FIELDS, (int(v) for v in p[n])))
    return out


def _update_args(prims, first, instances):
    p = None if prims is None else np.ascontiguousarray(prims, dtype=_lib.Primitive)
    b = None if instances is None else np.ascontiguousarray(instances, dtype=_lib.BVHInstance)
    st = np.zeros((), dtype=_lib.UpdateStats)
    args = (_lib.ptr(p) if p is not None and len(p) else None, int(first), 0 if p is None else len(p),
            _lib.ptr(b) if b is not None else None, 0 if b is None else len(b), _lib.ptr(st))
    return args, (p, b), st


def _update_dict(st):
    return {"gpu_ms": float(st["gpu_ms"]), "prims": int(st["prims"]), "nodes": int(st["nodes"]), "tlas_nodes": int(st["tlas_nodes"]),
            "tlas_depth": int(st["tlas_depth"]), "reconfigured": bool(st["reconfigured"])}


def _rebuild_args(prims, first, instances, builder, lbvh_options, alpha=None):
    from .scene import build_options, rebuild_builder
    which = rebuild_builder(builder, lbvh_options, alpha)
    (p_, f_, n_, b_, nb_, _), keep, _ = _update_args(prims, first, instances)
    opts = build_options(alpha=alpha, **lbvh_options)
    st = np.zeros((), dtype=_lib.RebuildStats)
    return (p_, f_, n_, b_, nb_, which, _lib.ptr(opts), _lib.ptr(st)), (keep, opts), st


def _ranges_args(plan, prims, first, instances, lbvh_options, alpha):
    from .scene import build_options, plan_words
    words = plan_words(plan, lbvh_options, alpha)
    (p_, f_, n_, b_, nb_, _), keep, _ = _update_args(prims, first, instances)
    opts = build_options(alpha=alpha, **lbvh_options)
    st = np.zeros((), dtype=_lib.RebuildStats)
    return (p_, f_, n_, b_, nb_, _lib.ptr(words) if len(words) else None, len(words), _lib.ptr(opts), _lib.ptr(st)), (keep, opts, words), st


def _rebuild_dict(st):
    d = {n: float(st[n]) for n in ("gpu_ms", "wall_ms", "stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms")}
    d.update({n: int(st[n]) for n in ("prims", "blas_built", "nodes", "n_idx", "max_depth", "tlas_nodes", "tlas_depth", "spatial_splits",
                                      "prims_clipped")})
    d["reconfigured"] = bool(st["reconfigured"])
    return d


def _resize_args(prims, range_counts, inst_range, instances, builder, lbvh_options, alpha):
    """The arguments of rt_resize_scene: `prims` a numpy array (host memory) or a torch tensor on the context's GPU, used where it lies."""
    from .scene import build_options, rebuild_builder
    which = rebuild_builder(builder, lbvh_options, alpha)
    if isinstance(prims, np.ndarray) or not hasattr(prims, "data_ptr"):
        p = np.ascontiguousarray(prims, dtype=_lib.Primitive)
        pp, n = _lib.ptr(p) if len(p) else None, len(p)
    else:   # a torch tensor: nothing is copied, the library checks where it lies
        p = prims if prims.is_contiguous() else prims.contiguous()
        nbytes = p.numel() * p.element_size()
        if nbytes % _lib.Primitive.itemsize:
            raise ValueError(f"a primitive tensor of {nbytes} bytes is no whole number of {_lib.Primitive.itemsize}-byte records")
        pp, n = (C.c_void_p(p.data_ptr()) if nbytes else None), nbytes // _lib.Primitive.itemsize
        if getattr(p, "is_cuda", False):
            import torch
            torch.cuda.current_stream(p.device).synchronize()   # what produced the records (and .contiguous()) has finished; the copy's stream is not torch's
    counts = np.ascontiguousarray(range_counts, dtype=np.int32).ravel()
    ir = np.arange(len(counts), dtype=np.int32) if inst_range is None else np.ascontiguousarray(inst_range, dtype=np.int32).ravel()
    b = None if instances is None else np.ascontiguousarray(instances, dtype=_lib.BVHInstance)
    if b is not None and len(b) != len(ir):
        raise ValueError(f"{len(b)} instance records for {len(ir)} instances")
    shape = np.zeros((), dtype=_lib.SceneShape)
    shape["nRanges"], shape["rangeCount"] = len(counts), counts.ctypes.data
    shape["nBlas"], shape["instRange"] = len(ir), ir.ctypes.data
    shape["blas"] = 0 if b is None else b.ctypes.data
    opts = build_options(alpha=alpha, **lbvh_options)
    st = np.zeros((), dtype=_lib.RebuildStats)
    return (pp, n, _lib.ptr(shape), which, _lib.ptr(opts), _lib.ptr(st)), (p, counts, ir, b, shape, opts), st


def _flat_pointer(a, dtype, what):
    """(void* or None, element count, what keeps it alive) of a numpy array (host memory) or a torch tensor, which is used where it lies
    (torch's current stream is waited for: the library's copy runs on a stream of its own); `dtype`: the numpy element type."""
    if isinstance(a, np.ndarray) or not hasattr(a, "data_ptr"):
        h = np.ascontiguousarray(a, dtype=dtype.base)
        if h.nbytes % dtype.itemsize:
            raise ValueError(f"{what}: {h.nbytes} bytes are no whole number of {dtype.itemsize}-byte elements")
        n = h.nbytes // dtype.itemsize
        return (_lib.ptr(h) if n else None), n, h
    t = a if a.is_contiguous() else a.contiguous()
    nbytes = t.numel() * t.element_size()
    if str(t.dtype) != {"float32": "torch.float32", "int32": "torch.int32"}[dtype.base.name] or nbytes % dtype.itemsize:
        raise ValueError(f"{what}: a {dtype.base.name} tensor of whole {dtype.itemsize}-byte elements expected, not {t.dtype} of {nbytes} bytes")
    if getattr(t, "is_cuda", False):
        import torch
        torch.cuda.current_stream(t.device).synchronize()
    return (C.c_void_p(t.data_ptr()) if nbytes else None), nbytes // dtype.itemsize, t


def _is_tensor(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _wait_for_torch(t):
    if getattr(t, "is_cuda", False):
        import torch
        torch.cuda.current_stream(t.device).synchronize()   # the library's copies and kernels run on a stream of its own


def _position_rows(a):
    """(address, stride in bytes, vertices, what keeps it alive) of positions: (n, 3) or (count, 3, 3) float32, a numpy array or a torch
    tensor, used where it lies.  Rows that are 4-byte-aligned slices of a wider row (x[:, :3] of an (n, 4) array) go through as they
    are, with the wider row as the stride; anything else that is not contiguous is copied."""
    if _is_tensor(a):
        if str(a.dtype) != "torch.float32" or a.dim() not in (2, 3) or tuple(a.shape[1:]) not in ((3,), (3, 3)):
            raise ValueError(f"positions: a float32 tensor of shape (n, 3) or (count, 3, 3) expected, not {a.dtype} {tuple(a.shape)}")
        if a.dim() == 2 and a.shape[0] > 0 and a.stride(1) == 1 and a.stride(0) >= 3:
            t, stride = a, a.stride(0) * 4
        else:
            t, stride = a.contiguous().view(-1, 3), 12
        return t.data_ptr(), stride, t.shape[0], t
    h = np.asarray(a, dtype=np.float32)
    if h.ndim not in (2, 3) or h.shape[1:] not in ((3,), (3, 3)):
        raise ValueError(f"positions: float32 of shape (n, 3) or (count, 3, 3) expected, not {h.shape}")
    if not (h.ndim == 2 and len(h) and h.strides[1] == 4 and h.strides[0] >= 12 and h.strides[0] % 4 == 0):
        h = np.ascontiguousarray(h).reshape(-1, 3)
    return h.ctypes.data, (h.strides[0] if len(h) else 12), len(h), h


def _geometry(first, prims, positions, indices):
    """An RtGeometry (a _lib.Geometry record) for the window that starts at `first`, and what keeps its memory alive.  prims: Primitive
    records; positions (+ indices: 3 per triangle, uint32 / int32): the vertex form; numpy arrays (host memory) or torch tensors, which
    are used where they lie after torch's current stream has been waited for."""
    g = np.zeros((), dtype=_lib.Geometry)
    g["first"] = int(first)
    keep = []
    if prims is not None and positions is not None:
        raise ValueError("both prims and positions are given: exactly one source of geometry is taken")
    if indices is not None and positions is None:
        raise ValueError("indices without positions")
    if prims is not None:
        if _is_tensor(prims):
            p = prims if prims.is_contiguous() else prims.contiguous()
            nbytes = p.numel() * p.element_size()
            if nbytes % _lib.Primitive.itemsize:
                raise ValueError(f"a primitive tensor of {nbytes} bytes is no whole number of {_lib.Primitive.itemsize}-byte records")
            g["prims"], g["count"] = (p.data_ptr() if nbytes else 0), nbytes // _lib.Primitive.itemsize
        else:
            p = np.ascontiguousarray(prims, dtype=_lib.Primitive)
            g["prims"], g["count"] = (p.ctypes.data if len(p) else 0), len(p)
        keep.append(p)
    elif positions is not None:
        addr, stride, n, k = _position_rows(positions)
        keep.append(k)
        corners = n
        if indices is not None:
            if _is_tensor(indices):
                i = indices if indices.is_contiguous() else indices.contiguous()
                if i.is_floating_point() or i.element_size() != 4:
                    raise ValueError(f"indices: a 32-bit integer tensor expected, not {i.dtype}")
                g["indices"], corners = i.data_ptr(), i.numel()
            else:
                i = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
                g["indices"], corners = i.ctypes.data, len(i)
            keep.append(i)
        if corners % 3:
            raise ValueError(f"{corners} corners are no whole number of triangles")
        g["count"] = corners // 3
        if g["count"]:
            g["positions"], g["positionStride"], g["nVertices"] = addr, stride, n
        else:
            g["indices"] = 0
    for k in keep:
        if _is_tensor(k):
            _wait_for_torch(k)
    return g, keep


def _instances_arg(instances):
    b = None if instances is None else np.ascontiguousarray(instances, dtype=_lib.BVHInstance)
    return (_lib.ptr(b) if b is not None else None, 0 if b is None else len(b)), b


def _update_geometry_args(first, prims, positions, indices, instances):
    g, keep = _geometry(first, prims, positions, indices)
    inst, b = _instances_arg(instances)
    st = np.zeros((), dtype=_lib.UpdateStats)
    return (_lib.ptr(g), *inst, _lib.ptr(st)), (g, keep, b), st


def _rebuild_geometry_args(first, prims, positions, indices, instances, builder, lbvh_options, alpha):
    from .scene import build_options, rebuild_builder
    which = rebuild_builder(builder, lbvh_options, alpha)
    g, keep = _geometry(first, prims, positions, indices)
    inst, b = _instances_arg(instances)
    opts = build_options(alpha=alpha, **lbvh_options)
    st = np.zeros((), dtype=_lib.RebuildStats)
    return (_lib.ptr(g), *inst, which, _lib.ptr(opts), _lib.ptr(st)), (g, keep, b, opts), st


def _geometry_ranges_args(plan, first, prims, positions, indices, instances, lbvh_options, alpha):
    from .scene import build_options, plan_words
    words = plan_words(plan, lbvh_options, alpha)
    g, keep = _geometry(first, prims, positions, indices)
    inst, b = _instances_arg(instances)
    opts = build_options(alpha=alpha, **lbvh_options)
    st = np.zeros((), dtype=_lib.RebuildStats)
    return (_lib.ptr(g), *inst, _lib.ptr(words) if len(words) else None, len(words), _lib.ptr(opts), _lib.ptr(st)), (g, keep, b, opts, words), st


def geometry_check(n_prims, first=0, prims=None, positions=None, indices=None, obj_types=None):
    """The checks of a replacement geometry that need no GPU (rt_geometry_check) against a scene of n_prims primitives whose objType
    values are obj_types (None: all triangles): raises RtError (.code) with the message the device calls would give."""
    lib = _lib.device_lib()
    g, keep = _geometry(first, prims, positions, indices)
    t = None if obj_types is None else np.ascontiguousarray(obj_types, dtype=np.int32)
    rc = lib.rt_geometry_check(_lib.ptr(g), int(n_prims), _lib.ptr(t))
    if rc != 0:
        e = RtError(lib.rt_last_error().decode())
        e.code = rc
        raise e


def _materials_args(mats, texels, tex_first, n_texels, prim_mat, prim_first):
    """The arguments of rt_update_materials: (RtMaterialUpdate*, RtMaterialStats*), what keeps them alive, the stats record."""
    u = np.zeros((), dtype=_lib.MaterialUpdate)
    keep = []
    if mats is not None:
        m = np.ascontiguousarray(mats, dtype=_lib.Material).ravel()
        u["mats"], u["nMats"] = m.ctypes.data, len(m)
        keep.append(m)
    if texels is not None:
        p, n, k = _flat_pointer(texels, _lib.f4, "texels")
        u["texels"], u["texCount"] = (p.value or 0) if p is not None else 0, n
        keep.append(k)
    u["texFirst"], u["nTexels"] = int(tex_first), -1 if n_texels is None else int(n_texels)
    if prim_mat is not None:
        p, n, k = _flat_pointer(prim_mat, np.dtype(np.int32), "prim_mat")
        u["primMat"], u["primCount"] = (p.value or 0) if p is not None else 0, n
        keep.append(k)
    u["primFirst"] = int(prim_first)
    st = np.zeros((), dtype=_lib.MaterialStats)
    return (_lib.ptr(u), _lib.ptr(st)), (u, keep), st


def _materials_dict(st):
    d = {"gpu_ms": float(st["gpu_ms"]), "wall_ms": float(st["wall_ms"])}
    d.update({n: int(st[n]) for n in ("mats", "texels", "prims", "lights")})
    d.update({n: bool(st[n]) for n in ("tables_staged_changed", "atlas_reallocated")})
    return d


class Device:
    def __init__(self, width, height, y0=0, y1=None, shading=_lib.SHADING_NEE, sampling=_lib.SAMPLING_COSINE,
                 accel=_lib.ACCEL_BVH2, russian_roulette=True, filter_fireflies=True, max_bounces=_lib.MAX_BOUNCES,
                 device=0, profile=False, extend_variant=0, shade_blocks_per_cu=0, persist_blocks_per_cu=0, lib=None, builtins=None):
        # builtins: None (the library's default: IEEE) | "ieee" (reproducible on a CPU, what the oracle checks) | "reference" (the
        # instruction sequences of the reference's own kernels: the reference's image from the reference's seeds)
        mode = _lib.builtins_value(builtins)
        self._lib = _lib.device_lib(lib)      # lib="refb": the build whose DEFAULT is "reference" (a yardstick of the tests)
        cfg = np.zeros((), dtype=_lib.Config)
        cfg["width"], cfg["height"], cfg["y0"], cfg["y1"] = width, height, y0, height if y1 is None else y1
        cfg["max_bounces"], cfg["shading"], cfg["sampling"], cfg["accel"] = max_bounces, shading, sampling, accel
        cfg["russian_roulette"], cfg["filter_fireflies"] = int(russian_roulette), int(filter_fireflies)
        cfg["device"], cfg["profile"], cfg["extend_variant"] = device, (2 if profile is True else int(profile)), extend_variant
        cfg["shade_blocks_per_cu"], cfg["persist_blocks_per_cu"] = shade_blocks_per_cu, persist_blocks_per_cu
        cfg["builtins"] = mode
        self.cfg = cfg
        self.width, self.height = width, height
        self.y0, self.y1 = int(cfg["y0"]), int(cfg["y1"])
        self.npix = (self.y1 - self.y0) * width
        self.first_pixel = self.y0 * width
        self.accel = accel
        h = C.c_void_p()
        self._h = None
        self._chk(self._lib.rt_create(cfg.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._h = h
        self._keep = None

    @classmethod
    def borrowed(cls, handle, cfg):
        """A Device view of a context somebody else owns (a lane of a Group): same methods, close() does not destroy it."""
        d = cls.__new__(cls)
        d._lib = _lib.device_lib()
        d.cfg = cfg
        d.width, d.height = int(cfg["width"]), int(cfg["height"])
        d.y0, d.y1 = int(cfg["y0"]), int(cfg["y1"])
        d.npix = (d.y1 - d.y0) * d.width
        d.first_pixel = d.y0 * d.width
        d.accel = int(cfg["accel"])
        d._h, d._keep, d._owned = C.c_void_p(handle), None, False
        return d

    def _chk(self, rc):
        if rc != 0:
            raise RtError(self._lib.rt_last_error().decode())

    def close(self):
        if self._h and getattr(self, "_owned", True):
            self._lib.rt_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- uploads (renderer.cpp:160-208)
    def upload(self, sa, from_bvh2=False):
        """Bind the scene arrays (rt_upload_scene).  from_bvh2=True hands over the BVH2 whatever the context's accel
        (rt_upload_scene_bvh2): a BVH4 context collapses it on the GPU and keeps it, so rebuild_scene works on the copy.  A refusal
        raises RtError (.code)."""
        nodes = sa.bvh2 if from_bvh2 else sa.nodes(self.accel)
        P = _lib.ptr
        self._chk_code((self._lib.rt_upload_scene_bvh2 if from_bvh2 else self._lib.rt_upload_scene)(
            self._h, P(sa.prims), len(sa.prims), P(sa.mats), len(sa.mats), P(sa.tex) if len(sa.tex) else None, len(sa.tex),
            P(sa.lights) if len(sa.lights) else None, len(sa.lights), P(nodes), len(nodes), P(sa.primIdx), len(sa.primIdx),
            P(sa.tlas), len(sa.tlas), P(sa.blas), len(sa.blas)))

    def _chk_code(self, rc):
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e

    def share_scene(self, other):
        """Render the scene `other` (a Device on the same GPU, same accel) holds, from ITS device copy (rt_share_scene)."""
        self._chk(self._lib.rt_share_scene(self._h, other._h))

    def update_scene(self, prims=None, first=0, instances=None):
        """Update the bound scene in place on the GPU (rt_update_scene): `prims` replace primitives [first, first + len(prims)) keeping
        their objType / matIdx, `instances` replace the instances (only invT may change); every BLAS is refit, the derived records are
        rewritten and the TLAS is rebuilt on the device.  Every context holding the scene sees the update.  Returns the stats."""
        args, keep, st = _update_args(prims, first, instances)
        self._chk(self._lib.rt_update_scene(self._h, *args))
        return _update_dict(st)

    def rebuild_scene(self, prims=None, first=0, instances=None, builder="sah", alpha=None, **lbvh_options):
        """Rebuild the bound scene's BLAS in place on the GPU (rt_rebuild_scene): `prims` / `instances` as for update_scene; then every
        BLAS is built anew over its primitive range with builder "sah" (BVH2::BuildBLAS, alpha 1), "lbvh" (lbvh_options: max_leaf,
        cost_traverse, cost_intersect) or "sbvh_gpu" (BVH2::BuildBLAS with `alpha` in [0, 1], default 0: spatial splits, for scenes
        bound as an SBVH), the TLAS is rebuilt and every derived array is produced on the device.  Use it when refits have degraded
        the trees (topology-changing motion).  builder="refit" (RT_REBUILD_REFIT) builds nothing: the bound trees are refit as
        update_scene refits them, which is also how a BVH4 context bound with from_bvh2=True follows a deformation (refit_info() tells
        whether its BVH4 records were rewritten in place).  Every context holding the scene sees it.  Returns the stats; a refusal
        raises RtError (.code) and leaves the scene as it was."""
        args, keep, st = _rebuild_args(prims, first, instances, builder, lbvh_options, alpha)
        rc = self._lib.rt_rebuild_scene(self._h, *args)
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e
        return _rebuild_dict(st)

    def rebuild_ranges(self, plan, prims=None, first=0, instances=None, alpha=None, **lbvh_options):
        """Rebuild only the BLAS that changed (rt_rebuild_ranges): plan[k], one of "keep", "refit", "sah", "lbvh", "sbvh_gpu" per distinct
        BLAS in the order of blas_blocks(), says whether that BLAS keeps its bound tree (moved on the GPU to where the new scene numbers
        it; "refit": and given new boxes from the primitives as they are afterwards, by update_scene's rules, for that BLAS alone) or
        is built anew by that builder, as rebuild_scene builds it; builders may differ from BLAS to BLAS (lbvh_options go to the "lbvh"
        ranges, alpha to the "sbvh_gpu" ranges).  `prims` / `first` / `instances` as for rebuild_scene; replaced primitives must not
        touch a kept BLAS (a refit or built one they may).  Every context holding the scene sees it.  Returns the stats (blas_built: the
        BLAS a builder built); ranges_info() tells what was derived and what was moved.  A refusal raises RtError (.code) and leaves
        the scene as it was."""
        args, keep, st = _ranges_args(plan, prims, first, instances, lbvh_options, alpha)
        self._chk_code(self._lib.rt_rebuild_ranges(self._h, *args))
        return _rebuild_dict(st)

    def update_geometry(self, first=0, prims=None, positions=None, indices=None, instances=None):
        """update_scene fed from wherever the geometry lies (rt_update_geometry).  The window starts at primitive `first`.  Either
        `prims` (Primitive records, as for update_scene) or `positions` gives it: positions is (n, 3) float32, and triangle i of the
        window takes vertices indices[3i .. 3i + 2] (indices: 3 integers per triangle), or without indices vertices 3i .. 3i + 2
        (positions may then be (count, 3, 3)).  From positions the GPU writes v0, v1, v2, N, centroid and area of each triangle by
        Scene.AddTriangle's rule (Scene.SetVertices is the host mirror); the window must hold triangles only.  Each of the three may be
        a numpy array or a torch tensor; a tensor on the context's GPU is used where it lies (torch's current stream is waited for
        first), and x[:, :3] of an (n, 4) float32 tensor goes through without a copy.  Returns update_scene's stats; a refusal raises
        RtError (.code) and leaves the scene as it was."""
        args, keep, st = _update_geometry_args(first, prims, positions, indices, instances)
        self._chk_code(self._lib.rt_update_geometry(self._h, *args))
        return _update_dict(st)

    def rebuild_geometry(self, first=0, prims=None, positions=None, indices=None, instances=None, builder="sah", alpha=None, **lbvh_options):
        """rebuild_scene fed as update_geometry is (rt_rebuild_geometry); builder, alpha and lbvh_options as for rebuild_scene."""
        args, keep, st = _rebuild_geometry_args(first, prims, positions, indices, instances, builder, lbvh_options, alpha)
        self._chk_code(self._lib.rt_rebuild_geometry(self._h, *args))
        return _rebuild_dict(st)

    def rebuild_geometry_ranges(self, plan, first=0, prims=None, positions=None, indices=None, instances=None, alpha=None, **lbvh_options):
        """rebuild_ranges fed as update_geometry is (rt_rebuild_geometry_ranges); plan, alpha and lbvh_options as for rebuild_ranges."""
        args, keep, st = _geometry_ranges_args(plan, first, prims, positions, indices, instances, lbvh_options, alpha)
        self._chk_code(self._lib.rt_rebuild_geometry_ranges(self._h, *args))
        return _rebuild_dict(st)

    def ranges_info(self):
        """The last successful rebuild_ranges of the bound scene copy (rt_ranges_info), counted from what it queued: ranges built, kept
        and refit; pairs_derived / pairs_relocated; slots_derived / slots_relocated (triangle-record slots); nodes_numbered (nodes of
        the trees the breadth-first numbering walked); leaves_refit.  All zero before any such call."""
        r = np.zeros((), _lib.RangesInfo)
        self._chk(self._lib.rt_ranges_info(self._h, _lib.ptr(r)))
        return {n: int(r[n]) for n in _lib.RANGES_INFO_FIELDS}

    def blas_blocks(self):
        """The distinct BLAS of the bound scene in plan order (rt_scene_blas_blocks): a list of dicts with prim_first, prim_count, nodes
        and idx_slots of the bound tree, and compact (only a compact tree can be kept by rebuild_ranges)."""
        n = C.c_int32(0)
        self._chk_code(self._lib.rt_scene_blas_blocks(self._h, C.byref(n), None, None, None, None, None, 0))
        a = np.zeros((5, max(n.value, 1)), np.int32)
        self._chk_code(self._lib.rt_scene_blas_blocks(self._h, C.byref(n), *[C.c_void_p(a[i].ctypes.data) for i in range(5)], n.value))
        return [dict(prim_first=int(a[0, k]), prim_count=int(a[1, k]), nodes=int(a[2, k]), idx_slots=int(a[3, k]), compact=bool(a[4, k]))
                for k in range(n.value)]

    def resize_scene(self, prims, range_counts, inst_range=None, instances=None, builder="sah", alpha=None, **lbvh_options):
        """Give the bound scene a new shape in place on the GPU (rt_resize_scene): `prims` is the whole new primitive array - a numpy
        array, or a torch tensor on the context's GPU, which is used where it lies (torch's current stream is waited for first) - with free objType / matIdx (the materials and
        textures stay as bound); range_counts[k] primitives, back to back, form BLAS k; inst_range[i] is the BLAS instance i renders
        (None: one instance per BLAS) under instances[i]["invT"] (None: the identity).  The light list, every BLAS (builder "sah",
        "lbvh" or "sbvh_gpu" as for rebuild_scene), the derived arrays and the TLAS are made on the device; every context holding
        the scene sees the new one.  Returns the stats; a refusal raises RtError (.code) and leaves the scene as it was."""
        args, keep, st = _resize_args(prims, range_counts, inst_range, instances, builder, lbvh_options, alpha)
        self._chk_code(self._lib.rt_resize_scene(self._h, *args))
        return _rebuild_dict(st)

    def update_materials(self, mats=None, texels=None, tex_first=0, n_texels=None, prim_mat=None, prim_first=0):
        """Change the bound scene's materials, texture atlas and material assignment in place on the GPU (rt_update_materials); each part
        that is None stays as bound.  mats: the whole new table (Material records).  texels: (n, 4) float32 that replace texels
        [tex_first, tex_first + n) of the atlas, whose new length is n_texels (None: as bound; kept texels stay, new ones are zero).
        prim_mat: int32 values, the new matIdx of primitives [prim_first, prim_first + len(prim_mat)).  texels and prim_mat may be numpy
        arrays, or torch tensors on the context's GPU, which are used where they lie (torch's current stream is waited for first).  With
        mats or prim_mat the light list and the light records are derived anew on the device; every context holding the scene sees the
        change.  Returns the stats as a dict; a refusal raises RtError (.code) and leaves the scene as it was."""
        args, keep, st = _materials_args(mats, texels, tex_first, n_texels, prim_mat, prim_first)
        self._chk_code(self._lib.rt_update_materials(self._h, *args))
        return _materials_dict(st)

    def refit_info(self):
        """The last successful rebuild_scene(builder="refit") of the bound scene copy (rt_refit_info): path (0 none yet, 1 in place,
        2 re-collapsed because changed_nodes > 0, 3 re-collapsed because RT355_REFIT_RECOLLAPSE=1 forced it), live_quads,
        changed_nodes, stack_need."""
        r = np.zeros((), _lib.RefitInfo)
        self._chk(self._lib.rt_refit_info(self._h, _lib.ptr(r)))
        return {n: int(r[n]) for n in r.dtype.names}

    def rebuild_allocations(self):
        """Device allocations that updates and rebuilds of the bound scene copy have made so far (rt_debug_rebuild_allocations)."""
        n = C.c_int64(0)
        self._chk(self._lib.rt_debug_rebuild_allocations(self._h, C.byref(n)))
        return n.value

    def scene_array(self, name):
        """A device array of the bound scene as raw bytes (rt_debug_get_scene_array; names: _lib.SCENE_ARRAYS, _lib.SCENE_ARRAYS_BVH4)."""
        which = {**_lib.SCENE_ARRAYS, **_lib.SCENE_ARRAYS_BVH4, **_lib.SCENE_ARRAYS_RESIZE, **_lib.SCENE_ARRAYS_MATERIALS}[name]
        n = C.c_int64(0)
        self._chk(self._lib.rt_debug_get_scene_array(self._h, which, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            self._chk(self._lib.rt_debug_get_scene_array(self._h, which, _lib.ptr(out), n.value, C.byref(n)))
        return out

    def kernel_info(self):
        """Which traversal kernels this context runs for the uploaded scene (rt_kernel_info)."""
        k = np.zeros((), dtype=_lib.KernelInfo)
        self._chk(self._lib.rt_kernel_info(self._h, k.ctypes.data_as(C.c_void_p)))
        return {n: int(k[n]) for n in k.dtype.names}

    def top_levels(self):
        """(extend, connect): levels of the BLAS the event loops descend from their LDS top table (rt_top_levels; 0 = no table)."""
        e, c = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.rt_top_levels(self._h, C.byref(e), C.byref(c)))
        return int(e.value), int(c.value)

    def traversal_facts(self):
        """What this context's traversal is planned from (rt_debug_traversal_facts): a dict for traversal_plan()."""
        f = np.zeros((), dtype=_lib.TraversalFacts)
        self._chk(self._lib.rt_debug_traversal_facts(self._h, f.ctypes.data_as(C.c_void_p)))
        return {n: int(f[n]) for n in f.dtype.names}

    def shade_footprint(self):
        """(lds_bytes, traversal_beside): the static LDS of a k_shade workgroup of this context, and how many workgroups of its
        persistent extend kernel (no top table) fit a CU beside one (rt_shade_footprint)."""
        b, t = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.rt_shade_footprint(self._h, C.byref(b), C.byref(t)))
        return int(b.value), int(t.value)

    def shade_tables(self):
        """(capacity_rows, staged): the 16-byte LDS rows k_shade reserves for the light records (six each) and materials (three each),
        and whether this context's launches read the uploaded scene's from there (rt_shade_tables)."""
        r, s = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.rt_shade_tables(self._h, C.byref(r), C.byref(s)))
        return int(r.value), bool(s.value)

    def primary_fused(self):
        """Whether this context's render() frames launch no k_generate: bounce 0's extend and shade launches compute the primary rays
        themselves (rt_primary_fused; RT355_FUSE_PRIMARY=0 turns it off).  Same bits either way."""
        f = C.c_int32(0)
        self._chk(self._lib.rt_primary_fused(self._h, C.byref(f)))
        return bool(f.value)

    @property
    def builtins(self):
        """The context's arithmetic as resolved by the library (rt_builtins): _lib.BUILTINS_IEEE or _lib.BUILTINS_REFERENCE."""
        rc = self._lib.rt_builtins(self._h)
        if rc < 0:
            self._chk(rc)
        return int(rc)

    def extend_kernel_name(self):
        k = self.kernel_info()
        if k["persist4"] == 3:
            return "k_trace_persist4_tlas<false, false, true> (LDS stack of %d entries per lane, deeper entries in global memory)" % k["stack_entries"]
        if k["persist4"] == 2:
            return "k_trace_persist4_tlas<false> (bounce 0: its one-ray-per-lane branch)"
        if k["persist4"]:
            return "k_trace_persist4<false>"
        if k["persist"] == 3:
            return "k_trace_persist_tlas<false, false, true> (LDS stack of %d entries per lane, deeper entries in global memory)" % k["stack_entries"]
        if k["persist"] == 2:
            return "k_trace_persist_tlas<false> (bounce 0: its one-ray-per-lane branch)"
        if k["persist"]:
            return "k_trace_persist<false> (bounce 0: <false, true>, node records of wave-uniform visits through the scalar cache)"
        return "k_extend<%s, %d>" % ("RT_ACCEL_BVH4" if self.accel == _lib.ACCEL_BVH4 else "RT_ACCEL_BVH2", k["layout"])

    def set_seeds(self, seeds):
        """One nonzero uint32 per band pixel (rt_set_seeds).  A zero seed raises RtError (.code RT_E_INVALID, the message names its
        index) and leaves the context's seeds as they were; a fresh context already holds seed_default()'s."""
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        self._chk_code(self._lib.rt_set_seeds(self._h, _lib.ptr(s), s.size))

    def seed_default(self):
        self._chk(self._lib.rt_seed_default(self._h))

    def get_seeds(self):
        s = np.zeros(self.npix, dtype=np.uint32)
        self._chk(self._lib.rt_get_seeds(self._h, _lib.ptr(s), s.size))
        return s

    def bind_accum(self, tensor):
        """Render into a torch CUDA tensor of shape (H, W, 4) float32 (kept alive by this object)."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == self.width * self.height * 4
        self._keep = tensor
        self._chk(self._lib.rt_bind_accum(self._h, C.c_void_p(tensor.data_ptr())))

    # ---- frame (renderer.cpp:26-94)
    def reset(self):
        self._chk(self._lib.rt_reset(self._h))

    def render(self, cam, frames=1, antiAliasing=1, renderBVH=0):
        s = np.zeros((), dtype=_lib.Settings)
        s["antiAliasing"], s["renderBVH"] = antiAliasing, renderBVH
        c = np.ascontiguousarray(cam)
        self._chk(self._lib.rt_render(self._h, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), int(frames)))

    def synchronize(self):
        self._chk(self._lib.rt_synchronize(self._h))

    def focus(self, x, y, cam):
        t = C.c_float(0)
        c = np.ascontiguousarray(cam)
        self._chk(self._lib.rt_focus(self._h, int(x), int(y), c.ctypes.data_as(C.c_void_p), C.byref(t)))
        return np.float32(t.value)

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self._lib.rt_read_accum(self._h, _lib.ptr(out)))
        return out

    def write_accum(self, accum):
        a = np.ascontiguousarray(accum, dtype=np.float32)
        assert a.shape == (self.height, self.width, 4)
        self._chk(self._lib.rt_write_accum(self._h, _lib.ptr(a)))

    def save_checkpoint(self, path, frames):
        """{accum, seeds, frames}: everything a render carries from one frame to the next."""
        np.savez_compressed(path, accum=self.read_accum(), seeds=self.get_seeds(), frames=np.int32(frames),
                            dims=np.array([self.width, self.height, self.y0, self.y1], np.int32))

    def load_checkpoint(self, path):
        g = np.load(path)
        assert tuple(g["dims"]) == (self.width, self.height, self.y0, self.y1), "checkpoint was taken with another frame/band"
        accum = g["accum"]
        assert accum.shape == (self.height, self.width, 4)
        self.set_seeds(g["seeds"])       # first: a checkpoint with a zero seed is refused whole (RtError), accumulator untouched
        self.write_accum(accum)
        return int(g["frames"])

    def postproc(self, frames, vignette=0.0, gamma=0.9, chromatic=0.0):
        """Renderer::PostProc + SaveFrame: returns (float image (H,W,4), RGBA8 image (H,W,4) uint8)."""
        f = np.zeros((self.height, self.width, 4), dtype=np.float32)
        b = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._chk(self._lib.rt_postproc(self._h, int(frames), float(vignette), float(gamma), float(chromatic), _lib.ptr(f), _lib.ptr(b)))
        return f, b

    def counters(self):
        c = np.zeros((), dtype=_lib.Counters)
        self._chk(self._lib.rt_read_counters(self._h, c.ctypes.data_as(C.c_void_p)))
        return {k: int(c[k]) for k in c.dtype.names}

    def reset_counters(self):
        self._chk(self._lib.rt_reset_counters(self._h))

    def stage_times(self):
        t = np.zeros((), dtype=_lib.StageTimes)
        self._chk(self._lib.rt_read_stage_times(self._h, t.ctypes.data_as(C.c_void_p)))
        return {k: (float(t[k]) if k.endswith("_ms") else int(t[k])) for k in t.dtype.names}

    def set_profile(self, level):
        self._chk(self._lib.rt_set_profile(self._h, int(level)))

    def reset_stage_times(self):
        self._chk(self._lib.rt_reset_stage_times(self._h))

    # ---- single stages (parity tests)
    def stage_begin_frame(self):
        self._chk(self._lib.rt_stage_begin_frame(self._h))

    def stage_generate(self, cam, antiAliasing=1):
        s = np.zeros((), dtype=_lib.Settings)
        s["antiAliasing"] = antiAliasing
        c = np.ascontiguousarray(cam)
        self._chk(self._lib.rt_stage_generate(self._h, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))

    def stage_extend(self, bounce, renderBVH=0):
        self._chk(self._lib.rt_stage_extend(self._h, bounce, renderBVH))

    def stage_shade(self, bounce):
        self._chk(self._lib.rt_stage_shade(self._h, bounce))

    def stage_connect(self, b0, b1):
        self._chk(self._lib.rt_stage_connect(self._h, b0, b1))

    def get_rays(self, bounce):
        n = C.c_int32(0)
        self._chk(self._lib.rt_debug_get_rays(self._h, bounce, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=_lib.Ray)
        if n.value:
            self._chk(self._lib.rt_debug_get_rays(self._h, bounce, _lib.ptr(out), n.value, C.byref(n)))
        return out

    def set_rays(self, bounce, rays):
        r = np.ascontiguousarray(rays, dtype=_lib.Ray)
        self._chk(self._lib.rt_debug_set_rays(self._h, bounce, _lib.ptr(r) if len(r) else _lib.ptr(np.zeros(1, dtype=_lib.Ray)), len(r)))

    def get_shadow(self, b0, b1):
        n = C.c_int32(0)
        self._chk(self._lib.rt_debug_get_shadow(self._h, b0, b1, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=_lib.ShadowRecord)
        if n.value:
            self._chk(self._lib.rt_debug_get_shadow(self._h, b0, b1, _lib.ptr(out), n.value, C.byref(n)))
        return out

    # ---- queries (rt_trace)
    def trace_window(self):
        """Rays one pass of trace() takes (rt_trace_window); a longer batch runs as several passes."""
        w = int(self._lib.rt_trace_window(self._h))
        if w < 0:
            self._chk_code(w)
        return w

    def trace_raw(self, mode, origin=0, dir=0, origin_stride=16, dir_stride=16, tmax=0, n=0, hit=0, point=0, normal=0, occluded=0):
        """rt_trace with the two structs filled from device addresses (integers; 0 = NULL).  Asynchronous; a refusal raises RtError (.code)."""
        b = np.zeros((), dtype=_lib.RayBatch)
        b["origin"], b["dir"], b["originStride"], b["dirStride"], b["tmax"], b["n"] = origin, dir, origin_stride, dir_stride, tmax, n
        o = np.zeros((), dtype=_lib.TraceOut)
        o["hit"], o["point"], o["normal"], o["occluded"] = hit, point, normal, occluded
        self._chk_code(self._lib.rt_trace(self._h, int(mode), b.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)))

    def trace(self, origins, dirs, tmax=None, mode="closest", point=False, normal=False):
        """Intersect caller rays with the bound scene (rt_trace).  origins, dirs: (n, 3) or (n, 4) float32, either torch tensors on the
        context's GPU - used in place through their row stride, which may be any multiple of 4 bytes from 12 up (a view of every second
        row of a wider tensor is fine) - or numpy arrays, which are copied over.  tmax: None or n float32.
        mode "closest" returns a dict: "hit" (n records of _lib.Hit: t, primIdx, u, v; a miss is (1e30, -1, 0, 0); with tmax, hits at
        t >= tmax are misses) and, on request, "point" and "normal" ((n, 4) float32: O + t * D and the surface normal facing the ray).
        mode "any" returns n uint8: 1 where something lies in front of tmax.  Results are torch tensors for torch input (hit as an
        (n, 4) float32 tensor whose column 1 holds primIdx's bits: .view(torch.int32)), numpy arrays for numpy input.  The tensor path
        waits for torch's current stream on entry; the call returns after rt_synchronize."""
        import torch
        which = {"closest": _lib.TRACE_CLOSEST, "any": _lib.TRACE_ANY}.get(mode)
        if which is None:
            raise ValueError(f"mode must be 'closest' or 'any', not {mode!r}")
        if which == _lib.TRACE_ANY and (point or normal):
            raise ValueError("point / normal are results of mode 'closest'")
        as_torch = isinstance(origins, torch.Tensor)
        dev = torch.device("cuda", int(self.cfg["device"]))

        def rows(a, name):
            if not as_torch:
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
            if not (isinstance(a, torch.Tensor) and a.is_cuda and a.device == dev and a.dtype == torch.float32 and a.dim() == 2 and a.shape[1] in (3, 4)):
                raise ValueError(f"{name} must be an (n, 3) or (n, 4) float32 array, or such a tensor on {dev}")
            if a.shape[0] > 1 and (a.stride(1) != 1 or a.stride(0) < 3):
                a = a.contiguous()
            return a, (a.stride(0) if a.shape[0] > 1 else 4) * 4

        o, o_stride = rows(origins, "origins")
        d, d_stride = rows(dirs, "dirs")
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError("origins and dirs differ in length")
        t = None
        if tmax is not None:
            t = tmax if isinstance(tmax, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tmax, dtype=np.float32))
            t = t.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            if t.shape[0] != n:
                raise ValueError("tmax must hold one value per ray")
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
        hit = new(n, 4) if which == _lib.TRACE_CLOSEST else None
        pt = new(n, 4) if point else None
        nm = new(n, 4) if normal else None
        occ = new(n, dtype=torch.uint8) if which == _lib.TRACE_ANY else None
        P = lambda x: 0 if x is None or x.numel() == 0 else x.data_ptr()   # noqa: E731
        torch.cuda.current_stream(dev).synchronize()   # what produced the inputs has finished; the context's stream is not torch's
        self.trace_raw(which, P(o), P(d), o_stride, d_stride, P(t), n, P(hit), P(pt), P(nm), P(occ))
        self.synchronize()
        back = (lambda x: x) if as_torch else (lambda x: x.cpu().numpy())
        if which == _lib.TRACE_ANY:
            return back(occ)
        res = {"hit": hit if as_torch else hit.cpu().numpy().view(_lib.Hit).reshape(-1)}
        if point:
            res["point"] = back(pt)
        if normal:
            res["normal"] = back(nm)
        return res

    def enable_steps(self, on=True):
        self._chk(self._lib.rt_debug_enable_steps(self._h, int(on)))

    def get_steps(self):
        n = C.c_int32(0)
        out = np.zeros(self.npix, dtype=np.int32)
        self._chk(self._lib.rt_debug_get_steps(self._h, _lib.ptr(out), out.size, C.byref(n)))
        return out


class Group:
    """One accumulation rendered as `lanes` interleaved sample streams behind one handle (rt_group_*, include/rt355.h): own context,
    stream, queues and seed slice per lane, ONE device copy of the scene, accumulator = sum of the lanes in lane order."""

    def __init__(self, width, height, lanes=4, y0=0, y1=None, shading=_lib.SHADING_NEE, sampling=_lib.SAMPLING_COSINE,
                 accel=_lib.ACCEL_BVH2, russian_roulette=True, filter_fireflies=True, max_bounces=_lib.MAX_BOUNCES,
                 device=0, profile=False, extend_variant=0, shade_blocks_per_cu=0, persist_blocks_per_cu=0, builtins=None):
        mode = _lib.builtins_value(builtins)   # as for Device; every lane gets it
        self._lib = _lib.device_lib()
        cfg = np.zeros((), dtype=_lib.Config)
        cfg["width"], cfg["height"], cfg["y0"], cfg["y1"] = width, height, y0, height if y1 is None else y1
        cfg["max_bounces"], cfg["shading"], cfg["sampling"], cfg["accel"] = max_bounces, shading, sampling, accel
        cfg["russian_roulette"], cfg["filter_fireflies"] = int(russian_roulette), int(filter_fireflies)
        cfg["device"], cfg["profile"], cfg["extend_variant"] = device, (2 if profile is True else int(profile)), extend_variant
        cfg["shade_blocks_per_cu"], cfg["persist_blocks_per_cu"] = shade_blocks_per_cu, persist_blocks_per_cu
        cfg["builtins"] = mode
        self.cfg, self.width, self.height, self.accel = cfg, width, height, accel
        self.y0, self.y1 = int(cfg["y0"]), int(cfg["y1"])
        h = C.c_void_p()
        self._h = None
        self._chk(self._lib.rt_group_create(cfg.ctypes.data_as(C.c_void_p), int(lanes), C.byref(h)))
        self._h = h
        self.devs = [Device.borrowed(self._lib.rt_group_lane(self._h, m), cfg) for m in range(lanes)]

    def _chk(self, rc):
        if rc != 0:
            raise RtError(self._lib.rt_last_error().decode())

    def __len__(self):
        return len(self.devs)

    def concurrency(self):
        """How many of the lanes' HIP streams were measured to run side by side when the group was created."""
        return int(self._lib.rt_group_concurrency(self._h))

    def stream_class(self):
        """The HIP stream priority class of the lanes' streams: "low", "normal", "high", or "mixed" (rt_group_stream_class)."""
        return {-1: "low", 0: "normal", 1: "high", 2: "mixed"}[int(self._lib.rt_group_stream_class(self._h))]

    def class_concurrency(self):
        """{class: S as measured in it when the group was created}, for the classes that were tried (rt_group_class_concurrency)."""
        seen = {name: int(self._lib.rt_group_class_concurrency(self._h, k)) for k, name in ((-1, "low"), (0, "normal"), (1, "high"))}
        return {name: s for name, s in seen.items() if s >= 0}

    def frames(self):
        return int(self._lib.rt_group_frames(self._h))

    def upload(self, sa, from_bvh2=False):
        """Device.upload for the group: one device copy that every lane holds (rt_group_upload_scene / rt_group_upload_scene_bvh2)."""
        nodes = sa.bvh2 if from_bvh2 else sa.nodes(self.accel)
        P = _lib.ptr
        self._chk((self._lib.rt_group_upload_scene_bvh2 if from_bvh2 else self._lib.rt_group_upload_scene)(
            self._h, P(sa.prims), len(sa.prims), P(sa.mats), len(sa.mats), P(sa.tex) if len(sa.tex) else None, len(sa.tex),
            P(sa.lights) if len(sa.lights) else None, len(sa.lights), P(nodes), len(nodes), P(sa.primIdx), len(sa.primIdx),
            P(sa.tlas), len(sa.tlas), P(sa.blas), len(sa.blas)))

    def share_scene(self, other):
        """Render the scene another Group on the same GPU holds, from its device copy."""
        self._chk(self._lib.rt_group_share_scene(self._h, other._h))

    def update_scene(self, prims=None, first=0, instances=None):
        """Device.update_scene for the group's scene copy (rt_group_update_scene): every lane sees the update."""
        args, keep, st = _update_args(prims, first, instances)
        self._chk(self._lib.rt_group_update_scene(self._h, *args))
        return _update_dict(st)

    def rebuild_scene(self, prims=None, first=0, instances=None, builder="sah", alpha=None, **lbvh_options):
        """Device.rebuild_scene for the group's scene copy (rt_group_rebuild_scene): every lane sees the rebuilt scene."""
        args, keep, st = _rebuild_args(prims, first, instances, builder, lbvh_options, alpha)
        rc = self._lib.rt_group_rebuild_scene(self._h, *args)
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e
        return _rebuild_dict(st)

    def rebuild_ranges(self, plan, prims=None, first=0, instances=None, alpha=None, **lbvh_options):
        """Device.rebuild_ranges for the group's scene copy (rt_group_rebuild_ranges): every lane sees the rebuilt scene."""
        args, keep, st = _ranges_args(plan, prims, first, instances, lbvh_options, alpha)
        rc = self._lib.rt_group_rebuild_ranges(self._h, *args)
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e
        return _rebuild_dict(st)

    def resize_scene(self, prims, range_counts, inst_range=None, instances=None, builder="sah", alpha=None, **lbvh_options):
        """Device.resize_scene for the group's scene copy (rt_group_resize_scene): every lane sees the new shape."""
        args, keep, st = _resize_args(prims, range_counts, inst_range, instances, builder, lbvh_options, alpha)
        rc = self._lib.rt_group_resize_scene(self._h, *args)
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e
        return _rebuild_dict(st)

    def update_materials(self, mats=None, texels=None, tex_first=0, n_texels=None, prim_mat=None, prim_first=0):
        """Device.update_materials for the group's scene copy (rt_group_update_materials): every lane sees the change."""
        args, keep, st = _materials_args(mats, texels, tex_first, n_texels, prim_mat, prim_first)
        rc = self._lib.rt_group_update_materials(self._h, *args)
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e
        return _materials_dict(st)

    def _chk_code(self, rc):
        if rc != 0:
            e = RtError(self._lib.rt_last_error().decode())
            e.code = rc
            raise e

    def update_geometry(self, first=0, prims=None, positions=None, indices=None, instances=None):
        """Device.update_geometry for the group's scene copy (rt_group_update_geometry): every lane sees the update."""
        args, keep, st = _update_geometry_args(first, prims, positions, indices, instances)
        self._chk_code(self._lib.rt_group_update_geometry(self._h, *args))
        return _update_dict(st)

    def rebuild_geometry(self, first=0, prims=None, positions=None, indices=None, instances=None, builder="sah", alpha=None, **lbvh_options):
        """Device.rebuild_geometry for the group's scene copy (rt_group_rebuild_geometry): every lane sees the rebuilt scene."""
        args, keep, st = _rebuild_geometry_args(first, prims, positions, indices, instances, builder, lbvh_options, alpha)
        self._chk_code(self._lib.rt_group_rebuild_geometry(self._h, *args))
        return _rebuild_dict(st)

    def rebuild_geometry_ranges(self, plan, first=0, prims=None, positions=None, indices=None, instances=None, alpha=None, **lbvh_options):
        """Device.rebuild_geometry_ranges for the group's scene copy (rt_group_rebuild_geometry_ranges): every lane sees the rebuilt scene."""
        args, keep, st = _geometry_ranges_args(plan, first, prims, positions, indices, instances, lbvh_options, alpha)
        self._chk_code(self._lib.rt_group_rebuild_geometry_ranges(self._h, *args))
        return _rebuild_dict(st)

    def seed(self, first_stream=0):
        self._chk(self._lib.rt_group_seed(self._h, int(first_stream)))

    def reset(self):
        self._chk(self._lib.rt_group_reset(self._h))

    def render(self, cam, frames=1, antiAliasing=1):
        s = np.zeros((), dtype=_lib.Settings)
        s["antiAliasing"] = antiAliasing
        c = np.ascontiguousarray(cam)
        self._chk(self._lib.rt_group_render(self._h, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), int(frames)))

    def synchronize(self):
        self._chk(self._lib.rt_group_synchronize(self._h))

    def sum_into(self, tensor):
        """Lane-ordered sum of the lanes' accumulators into a torch CUDA tensor (H, W, 4) float32, queued behind the pending frames."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == self.width * self.height * 4
        self._chk(self._lib.rt_group_sum(self._h, C.c_void_p(tensor.data_ptr())))

    def focus(self, x, y, cam):
        t = C.c_float(0)
        c = np.ascontiguousarray(cam)
        self._chk(self._lib.rt_group_focus(self._h, int(x), int(y), c.ctypes.data_as(C.c_void_p), C.byref(t)))
        return np.float32(t.value)

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self._lib.rt_group_read_accum(self._h, _lib.ptr(out)))
        return out

    def postproc(self, frames=0, vignette=0.0, gamma=0.9, chromatic=0.0):
        f = np.zeros((self.height, self.width, 4), dtype=np.float32)
        b = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._chk(self._lib.rt_group_postproc(self._h, int(frames), float(vignette), float(gamma), float(chromatic), _lib.ptr(f), _lib.ptr(b)))
        return f, b

    def counters(self):
        """Work totals over the lanes."""
        tot = {}
        for d in self.devs:
            for k, v in d.counters().items():
                tot[k] = tot.get(k, 0) + v
        return tot

    def close(self):
        if self._h:
            self.devs = []
            self._lib.rt_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Renderer:
    """The C++ Renderer mirror (host/renderer.cpp): Init(), Tick(), accumulator read-back, energy."""

    def __init__(self, scene, width, height, device=0, y0=0, y1=-1, shading=_lib.SHADING_NEE, sampling=_lib.SAMPLING_COSINE,
                 bvh=_lib.ACCEL_BVH2, russian_roulette=True, filter_fireflies=True, builtins=None):
        mode = _lib.builtins_value(builtins)   # as for Device
        self._lib = _lib.host_lib()
        self.width, self.height = width, height
        self._h = self._lib.rth_renderer_create(scene._h, width, height, device, y0, y1, shading, sampling, bvh,
                                                int(russian_roulette), int(filter_fireflies))
        if not self._h:
            raise RtError(self._lib.rth_last_error().decode())
        if mode != _lib.BUILTINS_DEFAULT:
            self.SetBuiltins(mode)

    def _chk(self, rc):
        if rc < 0:
            raise RtError(self._lib.rth_last_error().decode())

    def SetBuiltins(self, mode):
        """Before Init(): the arithmetic of the context(s) Init() creates (_lib.BUILTINS_*)."""
        self._chk(self._lib.rth_renderer_set_builtins(self._h, int(mode)))

    def SetCamera(self, origin, forward, fov=110.0, aperture=0.1):
        self._chk(self._lib.rth_renderer_set_camera(self._h, _lib.fvec(origin), _lib.fvec(forward), float(fov), float(aperture)))

    def SetLanes(self, lanes):
        """Before Init(): render the accumulation as `lanes` interleaved sample streams; a Tick() is then `lanes` frames."""
        self._chk(self._lib.rth_renderer_set_lanes(self._h, int(lanes)))

    def Init(self):
        self._chk(self._lib.rth_renderer_init(self._h))

    def Tick(self, frames=1):
        self._chk(self._lib.rth_renderer_tick(self._h, int(frames)))

    def camera(self):
        cam = np.zeros((), dtype=_lib.Camera)
        self._chk(self._lib.rth_renderer_camera(self._h, cam.ctypes.data_as(C.c_void_p)))
        return cam

    def read(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        e = C.c_float(0)
        self._chk(self._lib.rth_renderer_read(self._h, _lib.ptr(out), C.byref(e)))
        return out, float(e.value)

    def Move(self, camdir):
        self._chk(self._lib.rth_renderer_camera_move(self._h, int(camdir)))

    def MouseMove(self, dx, dy):
        self._chk(self._lib.rth_renderer_camera_mouse(self._h, float(dx), float(dy)))

    def Zoom(self, offset):
        self._chk(self._lib.rth_renderer_camera_zoom(self._h, float(offset)))

    def frames(self):
        return int(self._lib.rth_renderer_frames(self._h))

    def SaveFrame(self, path):
        self._chk(self._lib.rth_renderer_save_frame(self._h, str(path).encode()))

    def close(self):
        if self._h:
            self._lib.rth_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
