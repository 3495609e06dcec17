"""The rule for rays with a bad component, read off the oracle (tests/edge_rays.py builds the rays; DESIGN.md section 2, "Non-finite
rays"): in the oracle's traversal - the reference's, restated - a ray with a NaN or infinite component in origin or direction misses in
extend and occludes nothing in connect, over the BVH2 and the BVH4; every finite ray of the set, FLT_MAX, 1e30, zero and subnormal
components included, gets the float64 closest hit of tests/geom64.py wherever that is decidable.  A zero direction is traced as given
and held to nothing here: it can report a sphere it starts inside.  test_gpu_edge_rays.py holds every HIP traversal path to the same
oracle on the same rays."""
import numpy as np
import pytest

import edge_rays as E
import geom64 as G
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from oracle.oracle_py import Oracle

SCENES = {"soup": ("soup", 0.0), "few spheres": ("few spheres", 0.0), "tlas": ("tlas", 0.0)}
_SETS = {}


def scene_set(name):
    """(gt, sa, rays, names) of a scene: its edge set, built once from camera rays traced over the BVH2."""
    if name not in _SETS:
        gt, sa, view = C._scene(SCENES[name])
        o = Oracle(sa, C.WD, C.HD, accel=W.ACCEL_BVH2, **C.FRAME)
        cam_rays, _, _ = C.camera_rays(o, sa, view)
        rays, names = E.edge_set(E.pick_base(cam_rays, C._extend(o, cam_rays)))
        _SETS[name] = (gt, sa, rays, names)
    return _SETS[name]


@pytest.mark.parametrize("accel", [W.ACCEL_BVH2, W.ACCEL_BVH4], ids=["bvh2", "bvh4"])
@pytest.mark.parametrize("name", list(SCENES))
def test_a_non_finite_ray_misses_and_a_finite_one_gets_the_float64_hit(name, accel):
    gt, sa, rays, names = scene_set(name)
    nb = 2 * E.N_BASE
    o = Oracle(sa, C.WD, C.HD, accel=accel, **C.FRAME)
    bad = E.non_finite(rays)
    assert bad.sum() == (6 * 3 + 3) * nb and len(rays) == (6 * 11 + 6) * nb
    with np.errstate(all="ignore"):
        got = C._extend(o, rays)
    # ---- non-finite: a miss, the record as initRay left it
    wrong = np.where(bad & ((got["primIdx"] != -1) | (got["t"] != W.REALLYFAR)))[0]
    assert not len(wrong), f"{name} accel {accel}: {len(wrong)} non-finite rays hit, e.g. {E.label(names, nb, wrong[0])}: prim {got['primIdx'][wrong[0]]} t {got['t'][wrong[0]]}"
    assert not got["I"][bad].any() and not got["N"][bad].any() and not got["u"][bad].any() and not got["v"][bad].any()
    # ---- ... and unoccluded in connect whatever the reach: as records {I, L, dist} of orc_connect, and as the rays those records are
    # (orc_occluded, what test_gpu_edge_rays.py holds rt_trace's any-hit to: the same traversal, the same verdicts)
    O, D = np.ascontiguousarray(rays["O"][:, :3]), np.ascontiguousarray(rays["D"][:, :3])
    for tmax in (1e30, 1.0, np.inf):
        with np.errstate(all="ignore"):
            dist, origin, reach = E.shadow_form(O, D, tmax)
            occ = E.oracle_occluded(o, O, D, dist)
            assert np.array_equal(o.occluded(origin, D, reach), occ), f"{name} accel {accel} tmax {tmax}: orc_occluded is not orc_connect's traversal"
            direct = o.occluded(O, D, np.float32(tmax))
        for which, verdict in (("records", occ), ("rays", direct)):
            wrong = np.where(bad & verdict)[0]
            assert not len(wrong), f"{name} accel {accel} tmax {tmax} ({which}): {len(wrong)} non-finite rays occluded, e.g. {E.label(names, nb, wrong[0])}"
        assert occ[~bad].any() and direct[~bad].any() or tmax == 1.0
    # ---- finite: float64 (a zero direction excepted)
    fin = ~bad & ~E.zero_dir(rays)
    assert fin.sum() == len(rays) - bad.sum() - 2 * nb
    # the rays with a FLT_MAX direction component are undecidable by construction (geom64.PRODUCT_CEIL): the floor of the issue holds
    # with them counted, and the others are held to their own - 0.99, below the 0.998 the oracle measured on them - so that a loss
    # among the ordinary edge rays cannot hide behind those kinds
    huge = E.huge_dir(rays)
    assert (huge & fin).sum() == E.HUGE_KINDS * nb
    with np.errstate(all="ignore"):
        frac = G.compare(gt, rays[fin], got[fin], "adversarial", f"{name} accel {accel}: finite edge rays")
        dec = G.closest_hit(gt, rays["O"][fin & ~huge], rays["D"][fin & ~huge])["decidable"]
    assert not G.closest_hit(gt, rays["O"][fin & huge], rays["D"][fin & huge])["decidable"].any()
    assert dec.mean() >= 0.99, f"{name} accel {accel}: only {dec.mean():.4f} of the finite rays without a FLT_MAX direction component are decidable"
    hits = int((got["primIdx"][fin] >= 0).sum())
    assert 0 < hits < fin.sum()
    print(name, accel, "finite rays", int(fin.sum()), "hits", hits, "decidable", round(frac, 4), "without FLT_MAX directions", round(float(dec.mean()), 4),
          "zero-direction hits", int((got["primIdx"][E.zero_dir(rays)] >= 0).sum()))


# The six kinds whose verdict at tmax = +inf differs between the two BVH2 orders on these scenes: every kind with a FLT_MAX direction
# component but D.z = -FLT_MAX, the one that flies INTO the scene (the camera looks down -z) and finds its garbage hit in both orders
PRUNED_AT_INF = ("D.x = 3.40282e+38", "D.x = -3.40282e+38", "D.y = 3.40282e+38", "D.y = -3.40282e+38", "D.z = 3.40282e+38", "D = (FLT_MAX)^3")


@pytest.mark.parametrize("name", list(SCENES))
def test_connect_verdicts_do_not_depend_on_the_order_except_where_pinned(name):
    """Connect over a BVH2 in the kernels' any-hit order (LATER_EXIT, what helpers.oracle_for holds every BVH2 context to) against the
    reference's own loop (REFERENCE_ORDER) and the BVH4, on the whole edge set and every tmax of the GPU test.  They agree on every ray
    and every tmax but one: at tmax = +inf the reference's loop - and the BVH4's - descends into boxes the ray misses (a failed box
    reports 1e30, which is below that tmax), finds a triangle whose test overflows to t = 0 and calls the ray occluded; the kernels'
    BVH2 any-hit prunes those boxes.  That happens to exactly the rays of PRUNED_AT_INF - all of them rays float32 decides nothing
    for - and is documented for rt_trace (include/rt355.h)."""
    from oracle.oracle_py import LATER_EXIT, REFERENCE_ORDER
    gt, sa, rays, names = scene_set(name)
    nb = 2 * E.N_BASE
    O, D = np.ascontiguousarray(rays["O"][:, :3]), np.ascontiguousarray(rays["D"][:, :3])
    ref = Oracle(sa, C.WD, C.HD, accel=W.ACCEL_BVH2, connect_order=REFERENCE_ORDER, **C.FRAME)
    later = Oracle(sa, C.WD, C.HD, accel=W.ACCEL_BVH2, connect_order=LATER_EXIT, **C.FRAME)
    quad = Oracle(sa, C.WD, C.HD, accel=W.ACCEL_BVH4, **C.FRAME)
    assert names.count(PRUNED_AT_INF[0]) == 1 and all(k in names for k in PRUNED_AT_INF), names
    pinned = np.isin(np.arange(len(rays)) // nb, [names.index(k) for k in PRUNED_AT_INF])
    assert pinned.sum() == 6 * nb and E.huge_dir(rays)[pinned].all() and not E.non_finite(rays)[pinned].any()
    for tmax in E.TMAX:
        with np.errstate(all="ignore"):
            r, l, q = (o.occluded(O, D, None if tmax is None else np.float32(tmax)) for o in (ref, later, quad))
        assert np.array_equal(q, r), f"{name} tmax {tmax}: the BVH4 decides {int((q != r).sum())} rays differently from the reference's BVH2 loop"
        differ = l != r
        if tmax == np.inf:
            assert np.array_equal(differ, pinned), (f"{name} tmax +inf: the orders differ on {int(differ.sum())} rays, "
                                                    f"{int((differ & ~pinned).sum())} of them outside the pinned kinds, {int((pinned & ~differ).sum())} pinned rays agree")
            assert r[pinned].all() and not l[pinned].any()
        else:
            assert not differ.any(), f"{name} tmax {tmax}: the orders differ on {int(differ.sum())} rays, e.g. {E.label(names, nb, np.where(differ)[0][0])}"
