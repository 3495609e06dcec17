"""Scene: Python face of the host-side Scene / BVH2 / BVH4 / TLAS mirror (librt355_host.so).

Method names and argument meaning follow the reference (src/scene.h:5-34, src/bvh.h:4-56,
src/tlas.h:2-12); the heavy lifting (normals, Heron areas, binned-SAH / SBVH build, 4-wide
collapse, TLAS clustering) is C++ (magr_ray_tracer_amd/host/*.cpp).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib


def _view(fn, scene, dtype):
    n = C.c_int(0)
    p = fn(scene, C.byref(n))
    if not p or n.value == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n.value * dtype.itemsize)).from_address(p)
    return np.frombuffer(buf, dtype=dtype, count=n.value).copy()


@dataclass
class SceneArrays:
    """The flat arrays Renderer::InitBuffers uploads (reference src/renderer.cpp:145-208)."""
    prims: np.ndarray
    mats: np.ndarray
    tex: np.ndarray
    lights: np.ndarray
    bvh2: np.ndarray
    bvh4: np.ndarray
    primIdx: np.ndarray
    tlas: np.ndarray
    blas: np.ndarray

    def nodes(self, accel):
        return self.bvh4 if accel == _lib.ACCEL_BVH4 else self.bvh2


def material(color=(0, 0, 0), specular=0.0, n1=0.0, n2=0.0, dielectric=False, absorption=(0, 0, 0), light=False,
             emittance=(0, 0, 0)):
    m = np.zeros((), dtype=_lib.Material)
    m["color"][:3] = color
    m["absorption"][:3] = absorption
    m["specular"], m["n1"], m["n2"] = specular, n1, n2
    m["isDielectric"], m["isLight"] = int(dielectric), int(light)
    m["texIdx"] = -1
    m["emittance"][:3] = emittance
    return m


class Scene:
    def __init__(self):
        self._lib = _lib.host_lib()
        self._h = self._lib.rth_scene_create()
        if not self._h:
            raise RuntimeError("rth_scene_create failed")
        self.num_prims = 0

    def close(self):
        if self._h:
            self._lib.rth_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self._lib.rth_last_error().decode())
        return rc

    # reference: Scene::AddMaterial (scene.cpp:84-100)
    def AddMaterial(self, name, mat=None):
        m = np.ascontiguousarray(mat) if mat is not None else None
        return self._chk(self._lib.rth_add_material(self._h, name.encode(), _lib.ptr(m) if m is not None else None))

    def AddTexture(self, name, texels):
        t = np.ascontiguousarray(texels, dtype=np.float32)
        h, w = t.shape[:2]
        assert t.shape[2] == 4
        return self._chk(self._lib.rth_add_texture(self._h, name.encode(), _lib.ptr(t), w, h))

    # reference: Scene::LoadTexture (scene.cpp:244-256); PNG, JPEG, TGA and Radiance HDR files
    def LoadTexture(self, filename, name):
        """Read an image file into the texture atlas and add a material `name` that points at it; returns the material index."""
        return self._chk(self._lib.rth_load_texture(self._h, str(filename).encode(), name.encode()))

    def AddSphere(self, pos, radius, material):
        self._chk(self._lib.rth_add_sphere(self._h, _lib.fvec(pos), float(radius), material.encode()))
        self.num_prims += 1

    def AddPlane(self, N, d, material):
        self._chk(self._lib.rth_add_plane(self._h, _lib.fvec(N), float(d), material.encode()))
        self.num_prims += 1

    def AddTriangle(self, v0, v1, v2, material, uv0=(0, 0), uv1=(0, 0), uv2=(0, 0), flipNormal=False):
        self._chk(self._lib.rth_add_triangle(self._h, _lib.fvec(v0), _lib.fvec(v1), _lib.fvec(v2), _lib.fvec(uv0),
                                             _lib.fvec(uv1), _lib.fvec(uv2), material.encode(), int(flipNormal)))
        self.num_prims += 1

    def AddQuad(self, v0, v1, v2, v3, material, flipNormal=False):
        self._chk(self._lib.rth_add_quad(self._h, _lib.fvec(v0), _lib.fvec(v1), _lib.fvec(v2), _lib.fvec(v3),
                                         material.encode(), int(flipNormal)))
        self.num_prims += 2

    def AddTriangles(self, verts, material, uvs=None, flipNormal=False):
        """verts: (n,3,3) float32 triangle soup; uvs: (n,3,2) or None."""
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        u = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        self._chk(self._lib.rth_add_triangles(self._h, _lib.ptr(v), _lib.ptr(u) if u is not None else None, v.shape[0],
                                              material.encode(), int(flipNormal)))
        self.num_prims += v.shape[0]

    # reference: Scene::LoadModel (scene.cpp:178-243)
    def LoadModel(self, filename, defaultMaterial, pos=(0, 0, 0), forceDefaultMat=False):
        n = self._chk(self._lib.rth_load_model(self._h, str(filename).encode(), defaultMaterial.encode(), _lib.fvec(pos), int(forceDefaultMat)))
        self.num_prims += n
        return n

    # reference: BVH2::BuildBLAS (bvh.cpp:46-82), bvh2->alpha = 1 -> plain SAH BVH, 0 -> full SBVH
    def BuildBLAS(self, startIdx=0, alpha=1.0, threads=1, builder="sah", device=0, **lbvh_options):
        """A BLAS over the primitives [startIdx, end).

        builder="sah" (default): the reference's binned SAH / SBVH builder; threads > 1: task-parallel build, numbered afterwards in
        the reference's LIFO order (identical arrays).
        builder="lbvh": the linear BVH builder (rt_build_bvh2) on HIP device `device`, or its host restatement when device is None
        (identical arrays); lbvh_options: max_leaf, cost_traverse, cost_intersect.  It has no spatial splits: alpha must stay 1.
        builder="sah_gpu": builder="sah" with alpha 1, built on HIP device `device` (rt_build_bvh2_sah) or by its host restatement
        when device is None; the arrays equal builder="sah"'s byte for byte.  alpha and threads must stay 1.
        builder="sbvh_gpu": builder="sah" with any alpha in [0, 1] (spatial splits), built on HIP device `device`
        (rt_build_bvh2_sbvh) or by its host restatement when device is None; arrays and statistics equal builder="sah"'s with that
        alpha byte for byte.  threads must stay 1."""
        if builder == "sah":
            if lbvh_options:
                raise ValueError(f"options {sorted(lbvh_options)} apply to builder='lbvh' only")
            self._lib.rth_set_build_threads(self._h, int(threads))
            self._chk(self._lib.rth_build_blas(self._h, int(startIdx), float(alpha)))
        elif builder == "lbvh":
            if alpha != 1.0:
                raise ValueError("builder='lbvh' has no spatial splits: alpha must be 1")
            opts = build_options(**lbvh_options)
            self._chk(self._lib.rth_build_blas_lbvh(self._h, int(startIdx), -1 if device is None else int(device), _lib.ptr(opts)))
        elif builder == "sah_gpu":
            if lbvh_options:
                raise ValueError(f"options {sorted(lbvh_options)} apply to builder='lbvh' only")
            if alpha != 1.0:
                raise ValueError("builder='sah_gpu' has no spatial splits: alpha must be 1")
            if threads != 1:
                raise ValueError("builder='sah_gpu' takes no host threads: threads must be 1")
            self._chk(self._lib.rth_build_blas_sah_gpu(self._h, int(startIdx), -1 if device is None else int(device)))
        elif builder == "sbvh_gpu":
            if lbvh_options:
                raise ValueError(f"options {sorted(lbvh_options)} apply to builder='lbvh' only")
            if threads != 1:
                raise ValueError("builder='sbvh_gpu' takes no host threads: threads must be 1")
            self._chk(self._lib.rth_build_blas_sbvh_gpu(self._h, int(startIdx), float(alpha), -1 if device is None else int(device)))
        else:
            raise ValueError(f"unknown builder {builder!r} (expected 'sah', 'lbvh', 'sah_gpu' or 'sbvh_gpu')")

    def lbvh_stats(self):
        """Statistics of the last builder='lbvh' BuildBLAS (RtBuildStats)."""
        st = np.zeros((), _lib.BuildStats)
        self._chk(self._lib.rth_lbvh_stats(self._h, _lib.ptr(st)))
        return _stats_dict(st)

    def BuildBVH4(self, builder="host", device=0):
        """The BVH4 of the scene's BVH2 (reference: new BVH4(*bvh2)).  builder="host": BVH4::Convert / Collapse, sequential.
        builder="gpu": the level-wise collapse (rt_build_bvh4) on HIP device `device`, or its host restatement when device is None; the
        arrays are the same byte for byte.  A refused "gpu" build raises BuildError and keeps the BVH4 the scene had."""
        if builder == "host":
            self._chk(self._lib.rth_build_bvh4(self._h))
        elif builder == "gpu":
            rc = self._lib.rth_build_bvh4_gpu(self._h, -1 if device is None else int(device))
            if rc != 0:
                raise BuildError(rc, self._lib.rth_last_error().decode())
        else:
            raise ValueError(f"unknown builder {builder!r} (expected 'host' or 'gpu')")

    def BuildTLAS(self):
        self._chk(self._lib.rth_build_tlas(self._h))

    def SetPrimitives(self, first, prims):
        """Replace primitives [first, first + len(prims)) with records of the same objType and matIdx (rth_set_primitives), e.g. the
        `arrays().prims` of a second Scene built with the same calls and moved vertices.  The trees are not touched: Refit() next."""
        p = np.ascontiguousarray(prims, dtype=_lib.Primitive)
        self._chk(self._lib.rth_set_primitives(self._h, int(first), len(p), _lib.ptr(p) if len(p) else None))

    def SetVertices(self, first, positions, indices=None):
        """Move the triangles from primitive `first` on to new vertices (rth_set_vertices), as Device.update_geometry(positions=...)
        does on the GPU by the same rule (csrc/geometry_common.h, Scene::AddTriangle's): positions is (n, 3) float32 - rows of a wider
        row, such as x[:, :3], are taken as they lie - and triangle i takes vertices indices[3i .. 3i + 2], or 3i .. 3i + 2 without
        indices (positions may then be (count, 3, 3)).  v0, v1, v2, N, centroid and area are written anew, everything else stays.  The
        trees are not touched: Refit() next.  Raises BuildError (.code RT_E_INVALID) and changes nothing when refused."""
        p = np.asarray(positions, dtype=np.float32)
        if p.ndim not in (2, 3) or p.shape[1:] not in ((3,), (3, 3)):
            raise ValueError(f"positions: float32 of shape (n, 3) or (count, 3, 3) expected, not {p.shape}")
        if not (p.ndim == 2 and len(p) and p.strides[1] == 4 and p.strides[0] >= 12 and p.strides[0] % 4 == 0):
            p = np.ascontiguousarray(p).reshape(-1, 3)
        i = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).ravel()
        corners = len(p) if i is None else len(i)
        if corners % 3:
            raise ValueError(f"{corners} corners are no whole number of triangles")
        self._chk_build(self._lib.rth_set_vertices(self._h, int(first), corners // 3, C.c_void_p(p.ctypes.data), p.strides[0] if len(p) else 12, len(p),
                                                   _lib.ptr(i) if i is not None and len(i) else None))

    def _chk_build(self, rc):
        if rc != 0:
            raise BuildError(rc, self._lib.rth_last_error().decode())

    def SetMaterials(self, mats):
        """Replace the whole material table (rth_set_materials; Material records), as Device.update_materials(mats=...) does on the GPU:
        every texture window must lie inside the atlas and every primitive's matIdx inside the new table; the light list follows by
        the Scene rule.  The trees are not touched.  Raises BuildError (.code RT_E_INVALID) and changes nothing when refused."""
        m = np.ascontiguousarray(mats, dtype=_lib.Material).ravel()
        self._chk_build(self._lib.rth_set_materials(self._h, _lib.ptr(m) if len(m) else None, len(m)))

    def SetTexels(self, texels=None, first=0, n_texels=None):
        """Give the atlas n_texels texels (None: as it is; kept texels stay, new ones are zero) and write `texels` ((n, 4) float32) at
        [first, first + n) (rth_set_texels), as Device.update_materials(texels=..., tex_first=..., n_texels=...) does on the GPU.  Raises
        BuildError (.code RT_E_INVALID) and changes nothing when refused."""
        t = None if texels is None else np.ascontiguousarray(texels, dtype=np.float32).reshape(-1, 4)
        n = 0 if t is None else len(t)
        self._chk_build(self._lib.rth_set_texels(self._h, _lib.ptr(t) if n else None, int(first), n, -1 if n_texels is None else int(n_texels)))

    def SetPrimMaterials(self, first, mat_idx):
        """Write mat_idx (int32) into the matIdx of primitives [first, first + len(mat_idx)) (rth_set_prim_materials), as
        Device.update_materials(prim_mat=..., prim_first=...) does on the GPU; the light list follows by the Scene rule.  Raises
        BuildError (.code RT_E_INVALID) and changes nothing when refused."""
        m = np.ascontiguousarray(mat_idx, dtype=np.int32).ravel()
        self._chk_build(self._lib.rth_set_prim_materials(self._h, int(first), len(m), _lib.ptr(m) if len(m) else None))

    def Refit(self):
        """Refit every BLAS of the BVH2 in place by the rules rt_update_scene runs on the GPU (rth_refit); arrays() / BuildTLAS() then
        rebuild the TLAS (and the BVH4) from the refit tree."""
        self._chk(self._lib.rth_refit(self._h))

    def RefitBVH4(self):
        """After Refit(): bring the scene's BVH4 (the collapse of the BVH2 as it was before the refit) up to the refit BVH2 the way
        rt_rebuild_scene's RT_REBUILD_REFIT does on the GPU (rth_bvh4_refit): the live records are recomputed, and only if one of
        them changed a slot is the tree collapsed level by level again.  Returns True when the records were rewritten in place.
        Either way the BVH4 equals BuildBVH4()'s of the refit BVH2 byte for byte.  Raises BuildError when refused."""
        changed = C.c_int32(0)
        rc = self._lib.rth_refit_bvh4(self._h, C.byref(changed))
        if rc != 0:
            raise BuildError(rc, self._lib.rth_last_error().decode())
        return changed.value == 0

    def Rebuild(self, builder="sah", alpha=None, **lbvh_options):
        """Discard the BVH2 and build every BLAS again over the primitive range it covers, as rt_rebuild_scene does on the GPU
        (rth_rebuild): builder="sah" is the GPU SAH builder's host restatement (BuildBLAS with alpha 1), "lbvh" the linear builder's
        (lbvh_options: max_leaf, cost_traverse, cost_intersect), "sbvh_gpu" the GPU SBVH builder's (BuildBLAS with `alpha` in [0, 1],
        default 0: spatial splits; stats() then reports the new trees' spatial_splits / prims_clipped).  Instance transforms stay;
        arrays() / BuildTLAS() then rebuild the TLAS (and the BVH4).  Raises BuildError (.code, an RT_E_* value) and changes nothing
        when refused."""
        if builder == "refit":
            raise ValueError("builder='refit' is a device-side name (Device.rebuild_scene): on the host, Scene.Refit() refits the trees")
        which = rebuild_builder(builder, lbvh_options, alpha)
        rc = self._lib.rth_rebuild(self._h, which, _lib.ptr(build_options(alpha=alpha, **lbvh_options)))
        if rc != 0:
            raise BuildError(rc, self._lib.rth_last_error().decode())

    def RebuildRanges(self, plan, alpha=None, **lbvh_options):
        """Rebuild under a per-range plan, as rt_rebuild_ranges does on the GPU (rth_rebuild_ranges): plan[k], one of "keep", "refit",
        "sah", "lbvh", "sbvh_gpu" per distinct BLAS in increasing order of the primitive ranges.  A built BLAS is built as Rebuild builds
        it (lbvh_options go to the "lbvh" ranges, alpha to the "sbvh_gpu" ranges); a kept BLAS keeps its tree, moved to where the new
        scene numbers it; a "refit" BLAS keeps its tree likewise and takes new boxes from the primitives as they are, by Refit()'s rules,
        so only that BLAS loses the clipped boxes of an SBVH tree.  The primitives of a kept BLAS must not have changed.  Raises
        BuildError (.code) and changes nothing when refused (a BLAS that is not compact can be neither kept nor refit)."""
        words = plan_words(plan, lbvh_options, alpha)
        rc = self._lib.rth_rebuild_ranges(self._h, _lib.ptr(words) if len(words) else None, len(words), _lib.ptr(build_options(alpha=alpha, **lbvh_options)))
        if rc != 0:
            raise BuildError(rc, self._lib.rth_last_error().decode())

    def blas_ranges(self):
        """The primitive range (first, count) of every instance's BLAS (rt_blas_ranges); raises BuildError with RT_E_UNSUPPORTED when
        the BLAS do not cover contiguous, disjoint ranges in the order of their roots (such a scene cannot be rebuilt in place)."""
        n = len(_view(self._lib.rth_blas_nodes, self._h, _lib.BVHInstance))
        first, count = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        rc = self._lib.rth_blas_ranges(self._h, _lib.ptr(first), _lib.ptr(count))
        if rc != 0:
            raise BuildError(rc, _lib.device_lib().rt_last_error().decode())
        return [(int(a), int(b)) for a, b in zip(first[:n], count[:n])]

    def SetInstanceTransform(self, blas, invT):
        self._chk(self._lib.rth_set_instance_transform(self._h, int(blas), _lib.fvec(np.asarray(invT, dtype=np.float32).ravel())))

    def AddInstance(self, blas, invT=None):
        """A further instance of the BLAS that instance `blas` renders (rth_add_instance), under invT (16 floats, row-major; None: the
        identity): the new record carries that BLAS's root, and the next BuildTLAS() / arrays() gives its TLAS leaf the bounds every
        instance's gets.  Returns the new instance's index."""
        t = None if invT is None else _lib.fvec(np.asarray(invT, dtype=np.float32).ravel())
        return self._chk(self._lib.rth_add_instance(self._h, int(blas), t))

    def SwapInstances(self, a, b):
        """Instances a and b trade places (rth_swap_instances): the instance order is free, and need not be the order of the BLAS."""
        self._chk(self._lib.rth_swap_instances(self._h, int(a), int(b)))

    def stats(self):
        u = np.zeros(5, dtype=np.uint32)
        f = np.zeros(2, dtype=np.float32)
        self._lib.rth_bvh_stats(self._h, _lib.ptr(u), _lib.ptr(f))
        return {"depth": int(u[0]), "nodes": int(u[1]), "spatial_splits": int(u[2]), "prims_clipped": int(u[3]),
                "prims": int(u[4]), "sah_cost": float(f[0]), "build_ms": float(f[1])}

    def texture_array(self):
        """Scene::textures as an (n, 4) float32 view (no acceleration structure needed)."""
        return _view(self._lib.rth_textures, self._h, np.dtype((np.float32, 4)))

    def material_array(self):
        return _view(self._lib.rth_materials, self._h, _lib.Material)

    def arrays(self, bvh4=True):
        L = self._lib
        if bvh4:
            self.BuildBVH4()
        self.BuildTLAS()
        return SceneArrays(
            prims=_view(L.rth_primitives, self._h, _lib.Primitive), mats=_view(L.rth_materials, self._h, _lib.Material),
            tex=_view(L.rth_textures, self._h, np.dtype((np.float32, 4))), lights=_view(L.rth_lights, self._h, np.dtype("<u4")),
            bvh2=_view(L.rth_bvh2_nodes, self._h, _lib.BVHNode2), bvh4=_view(L.rth_bvh4_nodes, self._h, _lib.BVHNode4),
            primIdx=_view(L.rth_prim_idx, self._h, np.dtype("<u4")), tlas=_view(L.rth_tlas_nodes, self._h, _lib.TLASNode),
            blas=_view(L.rth_blas_nodes, self._h, _lib.BVHInstance))


LBVH_DEFAULTS = dict(max_leaf=8, cost_traverse=1.0, cost_intersect=1.0)   # lbvh_common.h


def build_options(max_leaf=None, cost_traverse=None, cost_intersect=None, alpha=None):
    """RtBuildOptions: the linear builder's options (None = its default) and the SBVH rebuild's alpha (None = 0)."""
    o = np.zeros((), _lib.BuildOptions)
    o["max_leaf"] = LBVH_DEFAULTS["max_leaf"] if max_leaf is None else int(max_leaf)
    o["cost_traverse"] = LBVH_DEFAULTS["cost_traverse"] if cost_traverse is None else float(cost_traverse)
    o["cost_intersect"] = LBVH_DEFAULTS["cost_intersect"] if cost_intersect is None else float(cost_intersect)
    o["alpha"] = 0.0 if alpha is None else float(alpha)
    return o


def light_list(prims, mats):
    """The light list rt_resize_scene derives for `prims` under the materials `mats` (rth_light_list, csrc/resize_common.h): the indices,
    in increasing order, of the primitives whose material is a light."""
    lib = _lib.host_lib()
    p = np.ascontiguousarray(prims, dtype=_lib.Primitive)
    m = np.ascontiguousarray(mats, dtype=_lib.Material)
    out = np.zeros(max(len(p), 1), np.uint32)
    n = lib.rth_light_list(_lib.ptr(p), len(p), _lib.ptr(m), len(m), _lib.ptr(out))
    if n < 0:
        raise BuildError(n, lib.rth_last_error().decode())
    return out[:n].copy()


REBUILD_BUILDERS = {"sah": _lib.REBUILD_SAH, "lbvh": _lib.REBUILD_LBVH, "sbvh_gpu": _lib.REBUILD_SBVH, "refit": _lib.REBUILD_REFIT}


def rebuild_builder(builder, lbvh_options=None, alpha=None):
    """RT_REBUILD_* of a builder name; the linear builder's options apply to "lbvh" only, alpha to "sbvh_gpu" only ("refit", which
    builds nothing, takes neither)."""
    if builder not in REBUILD_BUILDERS:
        raise ValueError(f"unknown builder {builder!r} (expected 'sah', 'lbvh', 'sbvh_gpu' or 'refit')")
    if builder != "lbvh" and lbvh_options:
        raise ValueError(f"options {sorted(lbvh_options)} apply to builder='lbvh' only")
    if builder != "sbvh_gpu" and alpha is not None:
        raise ValueError("alpha applies to builder='sbvh_gpu' only")
    return REBUILD_BUILDERS[builder]


PLAN_WORDS = {"keep": _lib.REBUILD_KEEP, "refit": _lib.REBUILD_REFIT_RANGE, "sah": _lib.REBUILD_SAH, "lbvh": _lib.REBUILD_LBVH, "sbvh_gpu": _lib.REBUILD_SBVH}


def plan_words(plan, lbvh_options=None, alpha=None):
    """The RT_REBUILD_* words (int32) of a per-range plan, a list of "keep" | "refit" | "sah" | "lbvh" | "sbvh_gpu" (integers pass through, so a
    test can hand the library a word it must refuse); the linear builder's options need an "lbvh" range, alpha an "sbvh_gpu" range."""
    plan = list(plan)
    for w in plan:
        if not isinstance(w, (int, np.integer)) and w not in PLAN_WORDS:
            raise ValueError(f"unknown plan word {w!r} (expected 'keep', 'refit', 'sah', 'lbvh' or 'sbvh_gpu')")
    if lbvh_options and "lbvh" not in plan:
        raise ValueError(f"options {sorted(lbvh_options)} apply to 'lbvh' ranges only")
    if alpha is not None and "sbvh_gpu" not in plan:
        raise ValueError("alpha applies to 'sbvh_gpu' ranges only")
    return np.array([w if isinstance(w, (int, np.integer)) else PLAN_WORDS[w] for w in plan], np.int32)


def blas_ranges(sa):
    """rt_blas_ranges of SceneArrays (or anything with bvh2 / primIdx / prims / blas): [(first, count)] per instance; raises BuildError
    (RT_E_UNSUPPORTED) when rt_rebuild_scene would not take the scene."""
    L = _lib.device_lib()
    nodes, idx = np.ascontiguousarray(sa.bvh2, _lib.BVHNode2), np.ascontiguousarray(sa.primIdx, np.uint32)
    inst = np.ascontiguousarray(sa.blas, _lib.BVHInstance)
    first, count = np.zeros(max(len(inst), 1), np.int32), np.zeros(max(len(inst), 1), np.int32)
    rc = L.rt_blas_ranges(_lib.ptr(nodes), len(nodes), _lib.ptr(idx), len(idx), len(sa.prims), _lib.ptr(inst), len(inst), _lib.ptr(first), _lib.ptr(count))
    if rc != 0:
        raise BuildError(rc, L.rt_last_error().decode())
    return [(int(a), int(b)) for a, b in zip(first[:len(inst)], count[:len(inst)])]


def blas_blocks(sa):
    """rt_blas_blocks of SceneArrays: per distinct BLAS in plan order a dict with prim_first, prim_count, nodes, idx_slots and compact
    (only a compact tree can be kept by Device.rebuild_ranges); raises BuildError like blas_ranges."""
    L = _lib.device_lib()
    nodes, idx = np.ascontiguousarray(sa.bvh2, _lib.BVHNode2), np.ascontiguousarray(sa.primIdx, np.uint32)
    inst = np.ascontiguousarray(sa.blas, _lib.BVHInstance)
    n, a = C.c_int32(0), np.zeros((5, max(len(inst), 1)), np.int32)
    rc = L.rt_blas_blocks(_lib.ptr(nodes), len(nodes), _lib.ptr(idx), len(idx), len(sa.prims), _lib.ptr(inst), len(inst), C.byref(n),
                          *[C.c_void_p(a[i].ctypes.data) for i in range(5)], a.shape[1])
    if rc != 0:
        raise BuildError(rc, L.rt_last_error().decode())
    return [dict(prim_first=int(a[0, k]), prim_count=int(a[1, k]), nodes=int(a[2, k]), idx_slots=int(a[3, k]), compact=bool(a[4, k]))
            for k in range(n.value)]


def _stats_dict(st):
    return {k: (float(st[k]) if k in ("sah_cost", "device_ms", "wall_ms") else int(st[k]))
            for k in ("nodes", "leaves", "depth", "morton_bits", "sah_cost", "device_ms", "wall_ms")}


class BuildError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{msg} (RT_E code {code})")
        self.code = code


def _build_args(prims, first, count, nodes, idx, node_cap=None, lengths=True):
    """(primitive array, count, node_cap, nodes, idx) of a build_* call: nodes / idx are the caller's arrays, or new ones of node_cap
    (default 2 * count - 1) and count records; their dtype, and with `lengths` their lengths, are checked."""
    p = np.ascontiguousarray(prims, dtype=_lib.Primitive)
    n = len(p) - int(first) if count is None else int(count)
    cap = max(2 * n - 1, 1) if node_cap is None else int(node_cap)
    nodes = np.zeros(max(cap, 1), _lib.BVHNode2) if nodes is None else nodes
    idx = np.zeros(max(n, 1), np.uint32) if idx is None else idx
    if nodes.dtype != _lib.BVHNode2 or idx.dtype != np.uint32 or (lengths and (len(nodes) < cap or len(idx) < max(n, 1))):
        raise ValueError("nodes / idx: BVHNode2[node_cap] and uint32[count] arrays expected" if lengths else
                         "nodes / idx: BVHNode2 and uint32 arrays expected")
    return p, n, cap, nodes, idx


def _build_call(host_fn, device_fn, device, *args):
    """device_fn(device, *args) of the device library, or the host restatement host_fn(*args) of the host library when device is None.
    Returns (rc, the message of the library that was called when it refused)."""
    if device is None:
        L = _lib.host_lib()
        rc, msg = getattr(L, host_fn)(*args), L.rth_last_error
    else:
        L = _lib.device_lib()
        rc, msg = getattr(L, device_fn)(int(device), *args), L.rt_last_error
    return rc, (msg().decode() if rc != 0 else "")


def build_lbvh(prims, first=0, count=None, device=None, node_base=0, idx_base=0, node_cap=None, **options):
    """The linear BVH builder on a primitive array (Primitive records): rt_build_bvh2 on HIP device `device`, or its host
    restatement (rth_build_bvh2_lbvh) when device is None.  Returns (nodes, primIdx, stats); raises BuildError (with .code, an RT_E_*
    value) when the call is refused.  node_cap defaults to what the call needs (2 * count - 1)."""
    p, n, cap, nodes, idx = _build_args(prims, first, count, None, None, node_cap)
    st = np.zeros((), _lib.BuildStats)
    written = C.c_int32(0)
    opts = build_options(**options)
    rc, text = _build_call("rth_build_bvh2_lbvh", "rt_build_bvh2", device, _lib.ptr(opts), _lib.ptr(p), len(p), int(first), n, int(node_base),
                           int(idx_base), _lib.ptr(nodes), cap, C.byref(written), _lib.ptr(idx), _lib.ptr(st))
    if rc != 0:
        raise BuildError(rc, text)
    return nodes[:written.value].copy(), idx[:n].copy(), _stats_dict(st)


def build_sah_gpu(prims, first=0, count=None, device=None, node_base=0, idx_base=0, node_cap=None, nodes=None, idx=None):
    """BVH2::BuildBLAS with alpha 1 on a primitive array: rt_build_bvh2_sah on HIP device `device`, or its host restatement
    (rth_build_bvh2_sah) when device is None.  Returns (nodes, primIdx, stats); raises BuildError (with .code, an RT_E_* value) when
    the call is refused.  node_cap defaults to what the call needs (2 * count - 1).  nodes / idx: the caller's arrays to write into
    (at least node_cap / count records), e.g. pre-filled to see that a refused call leaves them alone."""
    p, n, cap, nodes, idx = _build_args(prims, first, count, nodes, idx, node_cap)
    st = np.zeros((), _lib.BuildStats)
    written = C.c_int32(0)
    rc, text = _build_call("rth_build_bvh2_sah", "rt_build_bvh2_sah", device, _lib.ptr(p), len(p), int(first), n, int(node_base), int(idx_base),
                           _lib.ptr(nodes), cap, C.byref(written), _lib.ptr(idx), _lib.ptr(st))
    if rc != 0:
        raise BuildError(rc, text)
    return nodes[:written.value].copy(), idx[:n].copy(), _stats_dict(st)


def _sbvh_stats_dict(st):
    return {k: (float(st[k]) if k in ("sah_cost", "device_ms", "wall_ms") else int(st[k])) for k in _lib.SbvhStats.names}


def build_sbvh_gpu(prims, alpha, first=0, count=None, device=None, node_base=0, idx_base=0, nodes=None, idx=None):
    """BVH2::BuildBLAS with bvh2->alpha = alpha (spatial splits) on a primitive array: rt_build_bvh2_sbvh on HIP device `device`, or
    its host restatement (rth_build_bvh2_sbvh) when device is None.  Returns (nodes, primIdx, stats); raises BuildError (with .code,
    an RT_E_* value, and .needed = (nodes, primIdx entries) after a capacity refusal) when the call is refused.  Without nodes / idx
    the call starts with 2 * count - 1 nodes and count indices and, told that the tree is larger, calls once more with the sizes it
    was given.  nodes / idx: the caller's arrays to write into; their lengths are the capacities, and there is no second call."""
    own = nodes is None and idx is None
    p, n, _, nodes, idx = _build_args(prims, first, count, nodes, idx, lengths=False)
    st = np.zeros((), _lib.SbvhStats)
    for attempt in (0, 1):
        nn, ni = C.c_int32(0), C.c_int32(0)
        rc, text = _build_call("rth_build_bvh2_sbvh", "rt_build_bvh2_sbvh", device, float(alpha), _lib.ptr(p), len(p), int(first), n, int(node_base),
                               int(idx_base), _lib.ptr(nodes), len(nodes), C.byref(nn), _lib.ptr(idx), len(idx), C.byref(ni), _lib.ptr(st))
        if rc == 0:
            return nodes[:nn.value].copy(), idx[:ni.value].copy(), _sbvh_stats_dict(st)
        if own and attempt == 0 and rc == _lib.RT_E_INVALID and "capacity" in text:
            nodes, idx = np.zeros(nn.value, _lib.BVHNode2), np.zeros(ni.value, np.uint32)
            continue
        err = BuildError(rc, text)
        err.needed = (nn.value, ni.value)
        raise err


def build_bvh4_gpu(nodes2, roots, n_idx, device=None, out=None, derived=False):
    """The BVH2 -> BVH4 collapse of BVHNode2 records whose BLAS roots are `roots` (the instances' bvhIdx, in instance order) and whose
    leaves index n_idx primIdx slots: rt_build_bvh4 on HIP device `device`, or its host restatement (rth_build_bvh4_levels) when device
    is None.  Returns (BVHNode4 array, stats); raises BuildError (.code) when refused.  out: the caller's BVHNode4 array to write into
    (e.g. pre-filled to see that a refused call leaves it alone).  derived=True (host restatement only): also returns what the upload
    derives, (nodes4, stats, quads (live, 8, 4) float32, rootEntry, quadNode)."""
    n2 = np.ascontiguousarray(nodes2, dtype=_lib.BVHNode2)
    r = np.ascontiguousarray(roots, dtype=np.uint32)
    out = np.zeros(max(len(n2), 1), _lib.BVHNode4) if out is None else out
    if out.dtype != _lib.BVHNode4 or len(out) < len(n2):
        raise ValueError("out: a BVHNode4 array of len(nodes2) records expected")
    if derived and device is not None:
        raise ValueError("derived=True is the host restatement's (device=None)")
    st = np.zeros((), _lib.Bvh4Stats)
    args = [_lib.ptr(n2) if len(n2) else None, len(n2), int(n_idx), _lib.ptr(r) if len(r) else None, len(r), _lib.ptr(out), _lib.ptr(st)]
    if device is None:
        quads = np.zeros((max(len(n2), 1), 8, 4), np.float32) if derived else None
        entry, qnode = (np.zeros(max(len(r), 1), np.uint32), np.zeros(max(len(n2), 1), np.uint32)) if derived else (None, None)
        args += [_lib.ptr(quads), _lib.ptr(entry), _lib.ptr(qnode)]
    rc, text = _build_call("rth_build_bvh4_levels", "rt_build_bvh4", device, *args)
    if rc != 0:
        raise BuildError(rc, text)
    stats = {k: (float(st[k]) if k in ("device_ms", "wall_ms") else int(st[k])) for k in _lib.Bvh4Stats.names}
    if derived:
        live = stats["live_nodes"]
        return out[:len(n2)], stats, quads[:live].copy(), entry[:len(r)].copy(), qnode[:live].copy()
    return out[:len(n2)], stats


def make_camera(width, height, origin, forward, fov=110.0, aperture=0.1, focalLength=1.0, type=0):
    """CameraManager(fov, type) + UpdateCamVec() (reference src/camera.h:24-34,101-121); camera looks along -forward."""
    cam = np.zeros((), dtype=_lib.Camera)
    rc = _lib.host_lib().rth_camera(int(width), int(height), float(fov), int(type), _lib.fvec(origin), _lib.fvec(forward),
                                    float(aperture), float(focalLength), cam.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise RuntimeError(_lib.host_lib().rth_last_error().decode())
    return cam


def save_png(path, image):
    """SaveImageF (template/template.cpp:1629-1644): (H,W,4) float image -> 8-bit RGB PNG."""
    a = np.ascontiguousarray(image, dtype=np.float32)
    if _lib.host_lib().rth_save_png(str(path).encode(), a.shape[1], a.shape[0], _lib.ptr(a)) < 0:
        raise RuntimeError(_lib.host_lib().rth_last_error().decode())
