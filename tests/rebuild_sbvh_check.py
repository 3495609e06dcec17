"""Shared pieces of the SBVH in-place rebuild's tests (test_rebuild_sbvh_cpu.py, test_gpu_rebuild_sbvh.py): the scenes of
rebuild_check, where the ground truth is always the deformed scene built from scratch by the reference-exact host BuildBLAS(alpha)
(refit_check.build with builder="sah"), which shares no code with csrc/sbvh_common.h; and the host restatement of an SBVH rebuild
(Scene.SetPrimitives + Scene.Rebuild("sbvh_gpu", alpha) + BuildTLAS)."""
import collections

import numpy as np

import rebuild_check as RB
import refit_check as R

BUILDER = "sbvh_gpu"
_SCRATCH = {}


def from_scratch(deform, blas, alpha, transforms=None, tris=220, spheres=None):
    """(gt, arrays, view) of the deformed scene `deform` (a name of RB.DEFORMS) built from scratch with BuildBLAS(alpha); built once
    per argument set (without transforms) and shared: nobody changes it."""
    mk, sp = RB.DEFORMS[deform]
    sp = sp if spheres is None else spheres
    if transforms is not None:
        return R.build(mk(), alpha=alpha, blas=blas, spheres=sp, tris=tris, builder="sah", transforms=transforms)
    key = (deform, blas, float(alpha), tris, sp)
    if key not in _SCRATCH:
        _SCRATCH[key] = R.build(mk(), alpha=alpha, blas=blas, spheres=sp, tris=tris, builder="sah")
    return _SCRATCH[key]


def pair(deform, first_build, blas, alpha, transforms=None, tris=220, spheres=None):
    """(gt0, sa0) the scene as first built (RB.FIRST_BUILDS), a Scene of the caller's own; (gt1, sa1) the deformed scene built from
    scratch with BuildBLAS(alpha) - what an SBVH rebuild of the first to the second's primitives must give; and the view."""
    mk, sp = RB.DEFORMS[deform]
    sp = sp if spheres is None else spheres
    alpha0, b0 = RB.FIRST_BUILDS[first_build]
    gt0, sa0, view = R.build(alpha=alpha0, blas=blas, spheres=sp, tris=tris, builder=b0, transforms=transforms)
    gt1, sa1, _ = from_scratch(deform, blas, alpha, transforms, tris, sp)
    return (gt0, sa0), (gt1, sa1), view


def host_rebuild(s, prims, alpha, inst=None, bvh4=False):
    """The host restatement of rt_rebuild_scene with RT_REBUILD_SBVH on Scene `s`; returns its arrays (views of the Scene)."""
    if prims is not None:
        s.SetPrimitives(0, prims)
    if inst is not None:
        for b, r in enumerate(inst):
            s.SetInstanceTransform(b, r["invT"].reshape(4, 4))
    s.Rebuild(BUILDER, alpha=alpha)
    return s.arrays(bvh4=bvh4)


Wire = collections.namedtuple("Wire", RB.WIRE)


def wire_copy(sa):
    """The wire arrays of a Scene's arrays() as copies that survive the Scene's next build."""
    return Wire(*[np.array(getattr(sa, k), copy=True) for k in RB.WIRE])


def largest_leaf(sa):
    return int(sa.bvh2["count"].max())
