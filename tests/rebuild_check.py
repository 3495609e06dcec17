"""Shared pieces of the in-place rebuild's tests (test_rebuild_cpu.py, test_gpu_rebuild.py): the scenes of refit_check built twice by
the same calls - once as bound, once deformed and built from scratch with the rebuild's builder, which is what a rebuild must
reproduce - and the host restatement of a rebuild (Scene.SetPrimitives + Scene.Rebuild + BuildTLAS)."""
import numpy as np

import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials

BUILDERS = ["sah", "lbvh"]
ROT = C.invT(C.rot(1, 23.0) @ C.rot(0, -11.0), (0.31, -0.17, 0.45))

# name: (deformation factory, spheres)
DEFORMS = {
    "jitter": (lambda: R.jitter(), 2),
    "scramble": (lambda: R.scramble(), 2),
    "rigid_blas": (lambda: R.rigid_blas(0), 2),
    "spheres_moved": (lambda: R.spheres_moved(), 3),
}
# how the scene was built before the rebuild: (alpha, builder)
FIRST_BUILDS = {"sah": (1.0, "sah"), "sbvh": (0.0, "sah"), "lbvh": (1.0, "lbvh")}


def pair(deform, first_build, builder, blas, spheres=2, tris=220, transforms=None, transforms_to=None):
    """(gt0, sa0) the scene as first built; (gt1, sa1) the deformed scene built from scratch with `builder` (alpha 1): the arrays a
    rebuild of the first to the second's primitives (and transforms_to, if given) must give; and the view."""
    alpha, b0 = FIRST_BUILDS[first_build]
    gt0, sa0, view = R.build(alpha=alpha, blas=blas, spheres=spheres, tris=tris, builder=b0, transforms=transforms)
    gt1, sa1, _ = R.build(deform, alpha=1.0, blas=blas, spheres=spheres, tris=tris, builder=builder,
                          transforms=transforms if transforms_to is None else transforms_to)
    return (gt0, sa0), (gt1, sa1), view


def host_rebuild(s, prims, inst=None, builder="sah", bvh4=False, **options):
    """The host restatement of rt_rebuild_scene on Scene `s`; returns its arrays."""
    if prims is not None:
        s.SetPrimitives(0, prims)
    if inst is not None:
        for b, r in enumerate(inst):
            s.SetInstanceTransform(b, r["invT"].reshape(4, 4))
    s.Rebuild(builder, **options)
    return s.arrays(bvh4=bvh4)


def host_refit(s, prims, inst=None):
    s.SetPrimitives(0, prims)
    if inst is not None:
        for b, r in enumerate(inst):
            s.SetInstanceTransform(b, r["invT"].reshape(4, 4))
    s.Refit()
    return s.arrays(bvh4=False)


WIRE = ("prims", "bvh2", "primIdx", "blas", "tlas")


def same_wire_arrays(got, want, what):
    """prims, nodes, primIdx, instances and TLAS equal byte for byte, sizes included."""
    for k in WIRE:
        a, b = getattr(got, k), getattr(want, k)
        assert len(a) == len(b), f"{what}: {k} has {len(a)} records, expected {len(b)}"
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), f"{what}: {k} differs"


def depth(sa, b=None):
    """Height in edges of the BLAS of instance b (None: the deepest)."""
    n = sa.bvh2
    best = 0
    for root in ([int(sa.blas["bvhIdx"][b])] if b is not None else [int(r) for r in sa.blas["bvhIdx"]]):
        st = [(root, 0)]
        while st:
            i, d = st.pop()
            best = max(best, d)
            if n["count"][i] == 0:
                st += [(int(n["first"][i]), d + 1), (int(n["first"][i]) + 1, d + 1)]
    return best


def validate(sa):
    P = W.ptr
    L = W.device_lib()
    rc = L.rt_validate_scene(W.ACCEL_BVH2, P(sa.prims), len(sa.prims), P(sa.mats), len(sa.mats), P(sa.tex) if len(sa.tex) else None, len(sa.tex),
                             P(sa.lights) if len(sa.lights) else None, len(sa.lights), P(sa.bvh2), len(sa.bvh2), P(sa.primIdx), len(sa.primIdx),
                             P(sa.tlas), len(sa.tlas), P(sa.blas), len(sa.blas))
    assert rc == 0, L.rt_last_error()


def ladder_scene(clip, builder="sah"):
    """192 thin triangles along x at 2^e, e = max(-93 .. 98, clip), 1e-30 wide (two of them lights), one BLAS: every split of the binned
    SAH peels off the few farthest ones, a level per 8x of extent.  clip = -90 gives a tree 64 levels deep, the deepest a context
    takes; clip = -93 one of 65 levels, which rt_upload_scene, rt_rebuild_scene and rth_rebuild refuse.  Same primitive count, types
    and materials for every clip."""
    x = 2.0 ** np.maximum(np.arange(-93, 99), clip).astype(np.float64)
    t = np.zeros((len(x), 3, 3))
    t[:, :, 0] = x[:, None] * np.array([1.0, 1.0 + 2.0 ** -20, 1.0])
    t[:, 1, 1] = 1e-30
    t[:, 2, 2] = 1e-30
    t = t.astype(np.float32)
    s = Scene()
    _std_materials(s)
    s.AddTriangles(t[:2], "white-light")
    s.AddTriangles(t[2:], "sand")
    if builder == "lbvh":
        s.BuildBLAS(0, builder="lbvh", device=None)
    else:
        s.BuildBLAS(0)
    return s
