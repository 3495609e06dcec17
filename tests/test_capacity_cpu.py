"""The capacity trees of tests/capacity_check.py on the CPU: upload validation admits every capacity at its limit and refuses one past
it, the float64 occupancy model shows that the worst ray of each tree fills its stack exactly, and the oracle - whose stacks are fixed
arrays of 64 / 32 entries with the same zero slack - returns the float64 answer with the model's `steps`.  The HIP kernels meet the
same trees on every traversal path in test_gpu_capacity.py."""
import re

import numpy as np
import pytest

import capacity_check as CC
import geom64 as G
import lbvh_check as K
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W, scenes
from oracle.oracle_py import Oracle, seed_stream

FRAME = C.FRAME
B2, B4 = W.ACCEL_BVH2, W.ACCEL_BVH4


def _accepted(c, accel):
    rc = K.validate(c.sa, accel)
    assert rc == 0, (c.name, accel, W.device_lib().rt_last_error())


def _refused(c, accel, message):
    assert K.validate(c.sa, accel) == W.RT_E_UNSUPPORTED, (c.name, accel)
    err = W.device_lib().rt_last_error().decode()
    assert re.search(message, err), (c.name, err)


def check_extend(c, accel, need=None, tlas=None, every=1):
    """Validation accepts; the model's worst ray holds `need` BLAS entries (and `tlas` TLAS siblings under them) with every deciding
    distance MIN_MARGIN apart; the oracle agrees with float64 on every ray (all decidable, each its own triangle) and with the model's
    steps."""
    _accepted(c, accel)
    w = CC.worst(c, accel, every=every)
    if need is not None:
        assert w["blas"] == need, (c.name, accel, w["blas"], need)
        assert w["pending"] == need + (tlas or 0) and w["tlas"] == (tlas or 0), (c.name, w["pending"], w["tlas"])
    assert w["margin"] >= CC.MIN_MARGIN, (c.name, w["margin"])
    o = Oracle(c.sa, 64, 48, accel=accel, **FRAME)
    got = c.rays.copy()
    steps, ctr = o.extend(got, want_steps=True)
    assert G.compare(c.gt, c.rays, got, "adversarial", f"{c.name} accel {accel}") == 1.0
    assert np.array_equal(got["primIdx"], c.expect), c.name
    assert np.array_equal(steps[w["pick"]], w["steps"]), (c.name, steps[w["pick"]], w["steps"])
    return steps, ctr, w


@pytest.mark.parametrize("h", [1, 5, 21, 22, 63, 64])
def test_bvh2_caterpillar_fills_a_stack_of_its_height(h):
    c = CC.chain(h)
    steps, ctr, _ = check_extend(c, B2, need=h)
    assert (steps == 2 * h).all()                                   # every ray forks on every level
    assert ctr["prim_tests"] == (h + 1) ** 2                        # ... and pops every leaf: no entry is pruned
    check_extend(c, B4)                                             # the collapse a user gets (its need is only about h / 3)


@pytest.mark.parametrize("levels, need", [(2, 7), (21, 64)])
def test_bvh4_comb_fills_a_stack_of_three_entries_per_level(levels, need):
    c = CC.comb(levels)
    assert c.need[B4] == need
    steps, ctr, _ = check_extend(c, B4, need=need)
    assert (steps == 4 * levels + 1).all() and ctr["prim_tests"] == need * need


def test_one_entry_more_than_the_stacks_hold_is_refused():
    _refused(CC.chain(65), B2, "needs 65 stack entries")
    _refused(CC.comb(22), B4, "needs 67 stack entries")
    for accel in (B2, B4):
        _refused(CC.tlas_chain(33, 2), accel, "depth 33 exceeds the 32-entry")


@pytest.mark.parametrize("m", [127, 128])
def test_fat_leaves_on_both_sides_of_the_packed_count(m):
    """A leaf of 127 primitives is the largest the packed entry encodes, one of 128 the smallest it does not: both are valid scenes and
    every triangle of the leaf is its own ray's only hit."""
    c = CC.chain(5, fat=m)
    assert c.sa.bvh2["count"].max() == m and c.sa.bvh4["count"].max() == m and len(c.fat) == m
    check_extend(c, B2, need=5, every=9)
    check_extend(c, B4, every=9)
    c = CC.comb(2, fat=m)
    assert c.sa.bvh4["count"].max() == m
    check_extend(c, B4, need=7, every=9)


@pytest.mark.parametrize("d, h", [(1, 12), (8, 12), (8, 13), (9, 12), (32, 12), (8, 64)])
def test_tlas_chain_holds_its_depth_under_a_full_blas_stack(d, h):
    c = CC.tlas_chain(d, h)
    assert abs(np.linalg.det(c.sa.blas["invT"][max(1, d // 2)].reshape(4, 4)[:3, :3]) - 1.0) < 1e-6      # the turned instance is rigid
    steps, ctr, _ = check_extend(c, B2, need=h, tlas=d, every=1 if h < 64 else 7)
    assert ctr["inst_visits"] == len(c.rays) * (d + 1) and ctr["tlas_visits"] == len(c.rays) * d     # every pending sibling pushed and popped
    _, ctr, w = check_extend(c, B4, every=1 if h < 64 else 7)
    assert w["tlas"] == d and ctr["inst_visits"] == len(c.rays) * (d + 1)


FRAMES = {"chain(5)": lambda: CC.chain(5, frame=True), "chain(64)": lambda: CC.chain(64, frame=True),
          "tlas_chain(8, 12)": lambda: CC.tlas_chain(8, 12, frame=True), "tlas_chain(8, 64)": lambda: CC.tlas_chain(8, 64, frame=True)}


def shadow_rays(sh):
    """Origin, direction and tmax of the shadow rays connect traces for the oracle's records (wavefront.cl:144-201)."""
    eps = np.float32(C.W_EPS)
    return (sh["I"] + sh["L"] * eps)[:, :3], sh["L"][:, :3], sh["dist"] - np.float32(2) * eps


def check_shadow_occupancy(c, accel, org, L, tmax, want, n=160):
    """The model over n evenly spaced shadow rays in connect's order: the fullest reaches `want` pending entries, those starting on the
    receiver all do, its verdict is the float64 one; returns how many reached it."""
    pick = np.unique(np.linspace(0, len(org) - 1, n).astype(np.int64))
    m = [CC.occupancy(c.sa, accel, org[i], L[i], True, tmax[i]) for i in pick]
    pend = np.array([x["pending"] for x in m])
    assert pend.max() == want, (c.name, pend.max(), want)
    assert min(x["margin"] for x in m) >= CC.MIN_MARGIN
    occ, dec = G.any_hit(c.gt, org[pick], L[pick], tmax[pick])
    assert np.array_equal(np.array([x["hit"] for x in m])[dec], occ[dec]), c.name
    return int((pend == want).sum()), len(pick)


@pytest.mark.parametrize("case", list(FRAMES))
def test_frames_shadow_rays_start_in_the_leaf_pushed_first(case):
    """A frame through the oracle: camera rays and the shadow rays of bounce 0 against float64; the model shows that connect's order
    takes those shadow rays to the bottom with every level (and every TLAS sibling) pending."""
    c = FRAMES[case]()
    WD, HD = 96, 72
    for accel in (B2, B4):
        _accepted(c, accel)
        o = Oracle(c.sa, WD, HD, accel=accel, **FRAME)
        got = c.rays.copy()
        o.extend(got)
        assert G.compare(c.gt, c.rays, got, "adversarial", f"{c.name} accel {accel}") == 1.0
        cam = scenes.camera_for(c.view, WD, HD)
        seeds = seed_stream(0, WD * HD)
        rays = o.generate(cam, 0, WD * HD, seeds)
        got = rays.copy()
        o.extend(got)
        G.compare(c.gt, rays, got, "camera", f"{c.name} accel {accel}: camera rays")
        acc = np.zeros((WD * HD, 4), np.float32)
        _, sh = o.shade(got, acc, seeds)
        org, L, tmax = shadow_rays(sh)
        occ, dec = G.any_hit(c.gt, org, L, tmax)
        a = np.zeros((WD * HD, 4), np.float32)
        o.connect(sh, a)
        lit = np.any(a[sh["pixelIdx"]] != 0, axis=1)
        chk = dec & (sh["dotNL"] > 0) & np.all(sh["intensity"][:, :3] > 0, axis=1) & np.all(sh["BRDF"][:, :3] > 0, axis=1)
        assert not (chk & (lit == occ)).any(), (c.name, accel, int((chk & (lit == occ)).sum()))
        assert dec.sum() >= 1000 and dec.mean() >= G.MIN_DECIDABLE["shadow"] and occ[chk].any() and (~occ[chk]).any(), (c.name, dec.sum(), dec.mean())
        # the entries pushed first (popped last) and last (the column's last slot at full occupancy) each decide some records alone
        sole = {k: CC.sole_occluder(c.gt, c.info[k], org, L, tmax) for k in ("guard", "last")}
        assert min(sole.values()) >= 5, (c.name, sole)
        if accel == B2:
            full, n = check_shadow_occupancy(c, accel, org, L, tmax, c.need[B2] + c.depth)
            assert full >= n // 2, (c.name, full, n)
            print(c.name, "shadow rays", len(sh), "decidable", float(dec.mean()), "occluded", float(occ[dec].mean()), "at full occupancy", full, "of", n)
