"""The fixtures of test_gpu_bvh4_tlas.py reach what they claim, shown without a GPU: the combs under a TLAS of depth 8 fill the tagged
column of k_trace_persist4_tlas to the entry they are named for (the float64 replay of the push / pop rules in capacity_check), every
scene passes rt_validate_scene and the access audit, and the oracle finds the primitive every ray is aimed at."""
import numpy as np
import pytest

import bvh4_tlas_check as K4
import capacity_check as CC
import geom64 as G
import validate_sweep as S
import wire_audit as A
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd import scenes
from oracle.oracle_py import Oracle, seed_stream

B4 = W.ACCEL_BVH4
FRAME = dict(shading=1, sampling=1, russian_roulette=False, filter_fireflies=True)


def _legal(sa):
    rc, msg = S.validate(sa, B4)
    assert rc == W.RT_OK, msg
    assert A.audit_both(sa, B4) == []


@pytest.mark.parametrize("need", list(range(1, 65)))
def test_every_need_has_a_comb(need):
    levels, tail = K4.comb_levels(need)
    assert levels >= 1 and 1 <= tail <= 4 and 3 * (levels - 1) + tail == need
    if need % 3 == 1 and need > 1:
        assert tail == 4 and levels == (need - 4) // 3 + 1          # capacity_check.comb's own trees


def test_column_sizes():
    assert K4.column_entries(12, 8) == K4.FIT_SEVEN and K4.need_for_column(K4.FIT_SEVEN, 8) == 12      # 13 + 8 + 1: whole in LDS by default
    assert K4.column_entries(13, 8) == K4.FIT_SEVEN + 1 and K4.need_for_column(K4.FIT_SEVEN + 1, 8) == 13
    assert K4.column_entries(64, 8) == 73 and K4.column_entries(64, 8) - K4.SPILL_CAP == 61
    assert K4.lds_entries_admitted(65536) == 54 and K4.need_for_column(54, 8) == 44                     # 64 KB of dynamic LDS
    assert K4.lds_entries_admitted(163840) >= 73                                                        # 160 KB: the longest column fits


# the needs test_gpu_bvh4_tlas.py runs: either side of the switch, the LDS column at 64 KB, one more, and the deepest
@pytest.mark.parametrize("need", [12, 13, 44, 45, 64])
def test_tlas_comb_fills_the_column_to_need_plus_depth(need):
    c = K4.tlas_comb(8, need)
    assert len(c.sa.prims) < 1000 and len(c.sa.blas) == 9
    _legal(c.sa)
    w = CC.worst(c, B4, every=1 if len(c.rays) < 200 else 7)
    assert w["margin"] >= CC.MIN_MARGIN, w["margin"]
    assert w["blas"] == need and w["tlas"] == 8 and w["pending"] == need + 8, w
    assert w["pending"] < K4.column_entries(need, 8)                   # the column holds it
    r = c.rays.copy()
    steps, ctr = Oracle(c.sa, 64, 48, accel=B4, **FRAME).extend(r, want_steps=True)
    assert np.array_equal(r["primIdx"], c.expect)
    assert G.compare(c.gt, c.rays, r, "adversarial", c.name) == 1.0
    assert np.array_equal(steps[w["pick"]], w["steps"])
    assert ctr["tlas_visits"] > 0 and ctr["inst_visits"] >= len(r)


# the same needs as frames: connect's shadow rays, from the receiver in instance 0 to the light in instance 8
@pytest.mark.parametrize("need", [12, 13, 44, 64])
def test_frame_comb_shadow_rays_fill_the_column_under_connect(need):
    """A frame through the oracle: camera rays and the shadow rays of bounce 0 against float64; the replay in connect's order shows
    that those shadow rays hold 8 TLAS siblings and `need` BVH4 entries at once, and that the triangle in the leaf pushed first and
    the one in the leaf pushed last each occlude some of them alone."""
    c = K4.tlas_comb(8, need, frame=True)
    assert len(c.sa.prims) < 1000 and len(c.sa.blas) == 9
    _legal(c.sa)
    WD, HD = 96, 72
    o = Oracle(c.sa, WD, HD, accel=B4, **FRAME)
    seeds = seed_stream(0, WD * HD)
    rays = o.generate(scenes.camera_for(c.view, WD, HD), 0, WD * HD, seeds)
    got = rays.copy()
    o.extend(got)
    G.compare(c.gt, rays, got, "camera", f"{c.name}: camera rays")
    acc = np.zeros((WD * HD, 4), np.float32)
    _, sh = o.shade(got, acc, seeds)
    org, L, tmax = K4.shadow_rays(sh["I"], sh["L"], sh["dist"])
    occ, dec = G.any_hit(c.gt, org, L, tmax)
    a = np.zeros((WD * HD, 4), np.float32)
    o.connect(sh, a)
    lit = np.any(a[sh["pixelIdx"]] != 0, axis=1)
    chk = dec & (sh["dotNL"] > 0) & np.all(sh["intensity"][:, :3] > 0, axis=1) & np.all(sh["BRDF"][:, :3] > 0, axis=1)
    assert not (chk & (lit == occ)).any(), (c.name, int((chk & (lit == occ)).sum()))
    assert dec.sum() >= 1000 and dec.mean() >= G.MIN_DECIDABLE["shadow"] and occ[chk].any() and (~occ[chk]).any(), (c.name, dec.sum(), dec.mean())
    sole = {k: CC.sole_occluder(c.gt, c.info[k], org, L, tmax) for k in ("guard", "last")}
    assert min(sole.values()) >= 5, (c.name, sole)
    full, n = K4.shadow_occupancy(c, org, L, tmax)
    assert full >= n // 2, (c.name, full, n)
    print(c.name, "shadow rays", len(sh), "decidable", float(dec.mean()), "occluded", float(occ[dec].mean()), "full", full, "of", n, sole)


def test_fat_leaf_of_128_is_legal():
    c = K4.tlas_comb(1, 4, fat=128)
    _legal(c.sa)
    assert (c.sa.bvh4["count"] == 128).sum() == 1


@pytest.mark.parametrize("make", [K4.holes_multi, K4.leaf_127_multi], ids=["holes", "leaf-127"])
def test_odd_multi_blas_scenes_are_legal_and_on_the_ground_truth(make):
    e = make()
    _legal(e.sa)
    assert len(e.sa.blas) == 2 and len(e.sa.prims) < 1000
    if make is K4.leaf_127_multi:
        assert (e.sa.bvh4["count"] == 127).sum() == 1
    rng = np.random.default_rng(5)
    rays = G.inside_box_rays(rng, G.tlas_leaf_boxes(e.sa), 800)
    r = rays.copy()
    Oracle(e.sa, 64, 48, accel=B4, **FRAME).extend(r)
    assert G.compare(e.gt, rays, r, "adversarial", e.name) >= G.MIN_DECIDABLE["adversarial"]
    assert (r["primIdx"] >= len(e.sa.prims) - 90).any()               # the second BLAS is hit


def test_living_scene_starts_deep():
    s, sa = K4.living()
    rc, msg = S.validate(sa, W.ACCEL_BVH2)
    assert rc == W.RT_OK, msg
    n4 = np.zeros(len(sa.bvh2) - int(sa.blas["bvhIdx"][1]), W.BVHNode4)
    n2 = sa.bvh2[int(sa.blas["bvhIdx"][1]):].copy()
    n2["first"] -= np.where(n2["count"] == 0, int(sa.blas["bvhIdx"][1]), 40).astype(np.uint32)
    assert W.host_lib().rth_bvh4_from_nodes(W.ptr(n2), len(n2), W.ptr(n4)) == 0
    first, count = n4["first"].tolist(), n4["count"].tolist()

    def need(node):              # push every interior child in slot order, pop the last: child j runs over j pending siblings
        kids = [first[node][k] for k in range(4) if first[node][k] != -1 and count[node][k] == 0]
        return max([len(kids)] + [j + need(k) for j, k in enumerate(kids)])
    assert need(0) == 3 * (K4.LEVELS - 1) + 4, need(0)
    assert K4.column_entries(need(0), 1) > K4.FIT_SEVEN
