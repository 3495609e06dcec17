"""The oracle's connect_order LATER_EXIT (oracle.h) - the order the HIP path's connect walks a BVH2 BLAS in - pinned on the CPU: against
a second restatement of the rule (anyhit_check.replay), against answers worked out by hand, on ties, and as what it must be for the
oracle to stay the checker of everything else: a change of connect's node and triangle counts and of nothing besides.  Nothing here
runs a kernel; test_gpu_connect_counts.py and the counter helpers of the GPU suite hold the kernels to this order."""
import numpy as np
import pytest

import anyhit_check as A
import hand_trees as H
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import scenes
from magr_ray_tracer_amd.scenes import Scene, _std_materials, box_tris
from oracle.oracle_py import LATER_EXIT, REFERENCE_ORDER, Oracle

WD, HD = 320, 240       # the frame of test_gpu_connect_counts.py: its queues are made for these seeds


def _oracle(sa, order, **kw):
    return Oracle(sa, WD, HD, connect_order=order, **dict(A.FRAME, **kw))


# ---- known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(A.KNOWN)))
def test_known_answers_worked_out_by_hand(k):
    name, I, L, dist, want = A.KNOWN[k]
    sa = A.hand(name)
    sh = A.shadow_rays(I, L, dist)
    w = _oracle(sa, LATER_EXIT).connect_work(sh)[0]
    assert tuple(int(w[f]) for f in w.dtype.names) == want, (name, I, L, dist)
    r = A.replay(sa, sh[0])
    assert tuple(r[f] for f in w.dtype.names) == want, (name, I, L, dist)


def test_the_two_ladder_rays_differ_from_the_reference_order():
    """The figures in KNOWN's comments for near child first: the flag really selects another walk."""
    sa = A.hand("ladder")
    o = _oracle(sa, REFERENCE_ORDER)
    for I, L, dist, want in (((0, 2.5, 0), (1, 0, 0), 5.0, (3, 1)), ((5, 2.5, 0), (-1, 0, 0), 6.0, (4, 1))):
        w = o.connect_work(A.shadow_rays(I, L, dist))[0]
        assert (int(w["node_visits"]), int(w["prim_tests"]), int(w["occluded"])) == want + (1,)


# ---- the second restatement ---------------------------------------------------------------------------------------------------------
def _hand_shadow_rays(name):
    """Shadow rays of a hand-built scene: those its GPU queue makes (floor to light, past or into the slats) and rays along and
    across the row that no surface point would send."""
    sa = A.hand(name)
    sh = A.shadow_queue(sa, H.floor_rays(300), WD, HD)
    rng = np.random.default_rng(5)
    k = 120
    I = np.r_[np.c_[rng.uniform(-1, 0.9, k), rng.uniform(2.0, 3.0, k), rng.uniform(-1.2, 1.2, k)],
              np.c_[rng.uniform(3.0, 5.0, k), rng.uniform(2.0, 3.0, k), rng.uniform(-1.2, 1.2, k)],
              rng.uniform([-4, -1, -4], [4, 5, 4], (k, 3))]
    L = np.r_[np.c_[np.ones(k), rng.normal(scale=0.05, size=(k, 2))], np.c_[-np.ones(k), rng.normal(scale=0.05, size=(k, 2))],
              rng.normal(size=(k, 3))]
    L /= np.linalg.norm(L, axis=1)[:, None]
    return sa, np.concatenate([sh, A.shadow_rays(I, L, rng.uniform(0.5, 7.0, 3 * k))])


@pytest.mark.parametrize("name", list(A.HAND_TREES))
def test_replay_gives_the_oracles_figures_ray_by_ray_on_the_hand_built_trees(name):
    sa, sh = _hand_shadow_rays(name)
    work = _oracle(sa, LATER_EXIT).connect_work(sh)
    rep = A.replay_all(sa, sh)
    A.same_work(work, rep, name)
    assert work["occluded"].any() and not work["occluded"].all()
    if name in ("ladder", "identical-siblings"):
        assert rep["both"].sum() > 100


def test_replay_gives_the_oracles_figures_on_a_soup_under_a_tlas():
    """A few hundred triangles in four instances, three of them rotated and moved: the TLAS walk (near child first), the ray in the
    instance's space, then the rule."""
    sa, view = A.soup_instances()
    sh = A.shadow_queue(sa, A.bounce_rays(sa, view, 40, 30), WD, HD)
    assert 500 < len(sh) < 1300
    work = _oracle(sa, LATER_EXIT).connect_work(sh)
    rep = A.replay_all(sa, sh)
    A.same_work(work, rep, "soup instances")
    assert work["occluded"].any() and not work["occluded"].all() and rep["both"].sum() > len(sh)
    assert work["tlas_visits"].sum() > len(sh) and work["inst_visits"].max() >= 3


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
def test_a_tie_goes_to_child_one():
    """Identical siblings: every both-hit visit at the root is a tie.  The oracle's totals are the replay's with ties to child 1 and
    NOT the replay's with ties to child 2 (`>=`): child 1 is the single leaf, child 2 the same triangles as a tree, so which one an
    occluded ray enters first shows in both counts."""
    sa, sh = _hand_shadow_rays("identical-siblings")
    work = _oracle(sa, LATER_EXIT).connect_work(sh)
    first1, first2 = A.replay_all(sa, sh, tie_first=1), A.replay_all(sa, sh, tie_first=2)
    A.same_work(work, first1, "ties to child 1")
    assert first1["ties"].sum() > len(sh) // 2                                    # the root, for every ray that meets the scene's box
    assert np.array_equal(first1["occluded"], first2["occluded"])
    t1, t2 = A.totals(first1), A.totals(first2)
    assert t1["node_visits"] != t2["node_visits"] and t1["prim_tests"] != t2["prim_tests"], (t1, t2)
    assert A.totals(work) == t1
    differ = (first1["node_visits"] != first2["node_visits"]) | (first1["prim_tests"] != first2["prim_tests"])
    assert differ.any() and work["occluded"][differ].all()                        # unoccluded rays walk both children whatever the order


def test_the_room_queues_hold_ties():
    """The closed room's walls are axis-aligned and siblings share a wall plane: a ray that leaves both children through it leaves
    them at the same distance.  Of the 1,742 shadow rays test_gpu_connect_counts.py traces through the closed-room soup, 1,024 meet
    such a visit: 1,674 of their 15,112 both-hit visits are ties; of the 1,836 through the soup instances 1,544 rays, at 1,544 of
    10,455 visits.  So a kernel that ordered on `>=` has these queues to get past, not only the hand-built tree."""
    ties = {}
    for name, (sa, view) in (("room", A.soup_room()), ("instances", A.soup_instances())):
        sh = A.shadow_queue(sa, A.bounce_rays(sa, view), WD, HD)
        rep = A.replay_all(sa, sh)
        A.same_work(_oracle(sa, LATER_EXIT).connect_work(sh), rep, name)
        ties[name] = (int(rep["ties"].sum()), int(rep["both"].sum()), int((rep["ties"] > 0).sum()), len(sh))
        print(name, "ties, both-hit visits, rays with a tie, rays:", ties[name])
    assert ties["room"][0] > 0 and ties["instances"][0] > 0, ties


# ---- the order changes connect's counts and nothing else ---------------------------------------------------------------------------
def _spheres_and_planes():
    rng = np.random.default_rng(2)
    s = Scene()
    _std_materials(s)
    s.AddTriangles(C._soup(rng, 200, -3, 3, 0.4), "sand")
    for k in range(30):
        s.AddSphere(rng.uniform(-3, 3, 3), rng.uniform(0.2, 0.7), ["red", "mirror", "white-glass"][k % 3])
        if k == 15:
            s.AddPlane((0, 1, 0), 3.0, "grey")
    s.AddTriangles(box_tris((-6, -4, -6), (6, 6, 12)), "white")
    s.AddQuad((-1, 4.5, -1), (1, 4.5, -1), (1, 4.5, 1), (-1, 4.5, 1), "white-light")
    s.BuildBLAS(0)
    return s, dict(origin=(0.2, 0.3, 10.0), forward=(0.0, 0.0, 1.0), fov=62.0, aperture=0.01)


FAMILIES = {
    "cube": scenes.cube_scene,
    "bunny32": lambda: scenes.bunny_class(32),
    "sponza.2": lambda: scenes.sponza_class(0.2),
    "room-soup": lambda: A.soup_room(),
    "two-blas": lambda: scenes.two_blas_scene(alpha=0.0, n=20),
    "spheres-planes": _spheres_and_planes,
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_order_changes_connects_counts_and_nothing_else(family):
    """slab_any's claim: which shadow rays are occluded does not depend on the order in which the children that pass the visit test
    are visited.  Frames: accumulator and RNG state bit for bit, extend's counters and connect's rays, TLAS and instance visits equal;
    ray by ray the verdicts of a frame's shadow rays equal.  And the flag is read: connect's node visits differ, and on the
    sponza-class scene, most of whose shadow rays are occluded, later exit first needs fewer."""
    s, view = FAMILIES[family]()
    sa = s if family == "room-soup" else s.arrays()
    Wd, Hd = 96, 54
    cam = scenes.camera_for(view, Wd, Hd)
    out = {}
    for order in (REFERENCE_ORDER, LATER_EXIT):
        o = Oracle(sa, Wd, Hd, connect_order=order, **DEFAULT)
        acc, seeds, e, c = o.render(cam, 2)
        sh = A.shadow_queue(sa, A.bounce_rays(sa, view, Wd, Hd), Wd, Hd)
        out[order] = (acc, seeds, e, c, o.connect_work(sh), o.connect(sh, np.zeros((Wd * Hd, 4), np.float32)))
    (a0, s0, e0, c0, w0, t0), (a1, s1, e1, c1, w1, t1) = out[REFERENCE_ORDER], out[LATER_EXIT]
    assert_bits(a1, a0, family + ": accumulator")
    assert np.array_equal(s1, s0) and e1 == e0
    for k in ("rays", "tlas_visits", "inst_visits"):
        assert c1[k] == c0[k], (family, k)
    assert c0["rays"] > 1000 and c1["node_visits"] != c0["node_visits"], (family, c0, c1)
    assert len(w0) > 50 and np.array_equal(w1["occluded"], w0["occluded"])
    for k in ("tlas_visits", "inst_visits"):
        assert np.array_equal(w1[k], w0[k]), (family, k)
    for w, t in ((w0, t0), (w1, t1)):                              # orc_connect_work's totals are what orc_connect counts
        assert A.totals(w) == {k: t[k] for k in A.totals(w)} and t["rays"] == len(w)
    if family == "sponza.2":
        assert w0["occluded"].mean() > 0.5 and c1["node_visits"] < c0["node_visits"], (w0["occluded"].mean(), c0, c1)


def test_the_bvh4_and_the_default_are_untouched():
    """connect_order does not reach the BVH4 traversal, and an Oracle built without the keyword is the reference-order one."""
    s, view = scenes.sponza_class(0.2)
    sa = s.arrays()
    cam = scenes.camera_for(view, 96, 54)
    base = Oracle(sa, 96, 54, **DEFAULT)
    assert int(base.cfg["connect_order"]) == REFERENCE_ORDER
    ref = base.render(cam, 1)
    same = Oracle(sa, 96, 54, connect_order=REFERENCE_ORDER, **DEFAULT).render(cam, 1)
    assert_bits(same[0], ref[0], "default order")
    assert same[2:] == ref[2:]
    b4 = [Oracle(sa, 96, 54, connect_order=order, **dict(DEFAULT, accel=1)).render(cam, 1) for order in (REFERENCE_ORDER, LATER_EXIT)]
    assert_bits(b4[1][0], b4[0][0], "BVH4 accumulator")
    assert b4[1][2:] == b4[0][2:] and b4[0][3]["node_visits"] > 0
