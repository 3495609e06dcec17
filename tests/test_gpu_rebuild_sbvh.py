"""In-place SBVH rebuilds on the MI355X (rt_rebuild_scene with RT_REBUILD_SBVH, builder "sbvh_gpu"): after a rebuild the eleven device
arrays and kernel_info are those of a fresh upload of the scene built from scratch on the host by BuildBLAS(alpha); the sets grow to
trees of more index slots (and, with a small RT355_REBUILD_INITIAL_CAP, more nodes) than they were allocated for and give the same
arrays; a repeated rebuild stops allocating; frames are bit-exact with the oracle on every BVH2 traversal path; sharing contexts and
group lanes render the new scene; every refusal leaves the bound scene rendering as before."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rebuild_check as RB
import rebuild_sbvh_check as RS
import refit_check as R
import test_gpu_groundtruth as GT
import test_gpu_rebuild as TR
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = TR.Wd, TR.Hd
B = RS.BUILDER


# ---- array identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("deform,first_build,blas", TR.CASES, ids=[f"{a}-{b}-{c}" for a, b, c in TR.CASES])
def test_sbvh_rebuild_gives_the_arrays_of_a_fresh_upload(deform, first_build, blas, alpha):
    T0 = None if blas < 2 else [None, RB.ROT] + [None] * (blas - 2)
    (gt0, sa0), (gt1, sa1), _ = RS.pair(deform, first_build, blas, alpha, transforms=T0)
    what = f"{deform} / {first_build} / {blas} BLAS / sbvh_gpu alpha {alpha}"
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        st = d.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=alpha)
        host = gt1.s.stats()
        print(what, {k: st[k] for k in ("nodes", "n_idx", "max_depth", "spatial_splits", "prims_clipped")}, len(sa1.prims))
        assert st["blas_built"] == blas and st["nodes"] == len(sa1.bvh2) and st["n_idx"] == len(sa1.primIdx) and st["max_depth"] == RB.depth(sa1)
        assert st["spatial_splits"] == host["spatial_splits"] and st["prims_clipped"] == host["prims_clipped"]
        if alpha == 0.0 and deform == "jitter":
            assert st["spatial_splits"] > 0
        TR._check(d, sa1, what)
        # the host restatement says the same
        RB.same_wire_arrays(RS.host_rebuild(gt0.s, sa1.prims, alpha), sa1, "host restatement")
    finally:
        d.close()


def test_the_other_builders_report_no_spatial_splits():
    (gt0, sa0), (gt1, sa1), _ = RB.pair(R.jitter(), "sbvh", "sah", 2)
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        for builder in RB.BUILDERS:
            st = d.rebuild_scene(sa1.prims, 0, None, builder=builder)
            assert st["spatial_splits"] == 0 == st["prims_clipped"]
    finally:
        d.close()


# ---- growth ----------------------------------------------------------------------------------------------------------------------------
def growth_sequence(out=None):
    """scramble / first built as an SBVH / 4 BLAS: an update (the staging nodes are allocated), a rebuild to the full SBVH (more index
    slots than primitives), one with "sah", the full SBVH again (the other set), then an update of the rebuilt scene, which has more
    nodes than the staging array was made for.  Every step is compared with a fresh upload of its host restatement.  Returns (and
    saves) the arrays after every step and the allocation count after each."""
    (gt0, sa0), (gt1, sa1), _ = RS.pair("scramble", "sbvh", 4, 0.0)
    p2 = R.build(R.jitter(0.03, seed=7), blas=4, spheres=2)[1].prims
    s = gt0.s
    steps, allocs = {}, []
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)

        def done(name, want):
            TR._check(d, want, name)
            for k, v in TR._arrays(d).items():
                steps[f"{name}.{k}"] = v
            allocs.append(d.rebuild_allocations())

        nodes0 = len(sa0.bvh2)
        d.update_scene(sa0.prims[:10], 0)
        done("update0", RB.host_refit(s, sa0.prims))
        st = d.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=0.0)
        assert st["n_idx"] > len(sa1.prims) and st["nodes"] > nodes0, st
        done("sbvh1", RS.host_rebuild(s, sa1.prims, 0.0))
        d.rebuild_scene(builder="sah")
        done("sah", RB.host_rebuild(s, None, builder="sah"))
        d.rebuild_scene(builder=B, alpha=0.0)
        done("sbvh2", RS.host_rebuild(s, None, 0.0))
        live = np.frombuffer(d.scene_array("instances").tobytes(), W.BVHInstance)
        assert np.array_equal(live["bvhIdx"], s.arrays(bvh4=False).blas["bvhIdx"])
        d.update_scene(p2, 0)
        done("update1", RB.host_refit(s, p2))
    finally:
        d.close()
    if out:
        np.savez(out, allocs=np.asarray(allocs), **steps)
    return steps, allocs


_GROWTH_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import test_gpu_rebuild_sbvh as T
T.growth_sequence({out!r})
"""


def test_the_sets_grow_and_give_the_same_arrays(tmp_path):
    """In a child process with RT355_REBUILD_INITIAL_CAP=64 every tree-sized array starts at 64 index slots and 128 nodes and grows,
    nodes included, BLAS by BLAS; without the knob only the index slots (and what follows them) grow.  Both give, step by step, the
    arrays of the host restatement, and so the same arrays."""
    assert "RT355_REBUILD_INITIAL_CAP" not in os.environ
    steps, allocs = growth_sequence()
    out = str(tmp_path / "growth.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    code = _GROWTH_CHILD.format(tests=here, out=out)
    env = dict(os.environ, RT355_REBUILD_INITIAL_CAP="64")
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, cwd=os.path.dirname(here), env=env)
    other = np.load(out)
    assert sorted(other.files) == sorted(list(steps) + ["allocs"])
    for k, v in steps.items():
        assert len(other[k]) == len(v) and np.array_equal(other[k], v), f"{k} differs between the two initial capacities"
    small = [int(x) for x in other["allocs"]]
    print("allocations per step: default capacity", allocs, "initial capacity 64", small)
    # the small start has more to grow: each of the four BLAS of the first SBVH rebuild outgrows the set again
    assert small[1] - small[0] > allocs[1] - allocs[0]
    assert small[4] > small[3]          # the staging nodes grew for the rebuilt scene's node count


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_sbvh_rebuilds_give_identical_arrays_and_the_third_allocates_nothing():
    (gt0, sa0), (gt1, sa1), _ = RS.pair("scramble", "sbvh", 4, 0.0)
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        assert d.rebuild_allocations() == 0
        d.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=0.0)
        first, a1 = TR._arrays(d), d.rebuild_allocations()
        d.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=0.0)          # (writes the other set: it allocates and grows as the first did)
        TR._same(TR._arrays(d), first, "rebuild 2")
        a2 = d.rebuild_allocations()
        assert a1 > 0 and a2 > a1
        for k in range(3):
            d.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=0.0)
            TR._same(TR._arrays(d), first, f"rebuild {k + 3}")
            assert d.rebuild_allocations() == a2, f"rebuild {k + 3} allocated device memory ({d.rebuild_allocations() - a2} allocations)"
    finally:
        d.close()


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
_SC = {}


def _scenes(kind):
    """(original arrays, deformed records, arrays of the host rebuild to the full SBVH, view): one SBVH BLAS, or four under transforms."""
    if kind not in _SC:
        T = None if kind == "one" else [None, None, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
        blas, tris = (1, 600) if kind == "one" else (4, 220)
        (gt0, sa0), (gt1, sa1), view = RS.pair("scramble", "sbvh", blas, 0.0, transforms=T, tris=tris, spheres=3)
        prims = sa1.prims.copy()
        _SC[kind] = (sa0, prims, RS.host_rebuild(gt0.s, prims, 0.0, bvh4=True), view)
    return _SC[kind]


@pytest.mark.parametrize("case", TR.BVH2_PATHS)
def test_frames_across_an_sbvh_rebuild_match_the_oracle(case, monkeypatch):
    """Two frames, a rebuild to the full SBVH, two more: accumulator, seeds and the extend work counters equal the oracle rendering
    the same sequence over the from-scratch scene, accumulator carried."""
    kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sa0, prims, saR, view = _scenes(kind)
    assert len(saR.primIdx) > len(saR.prims)
    cam = scenes.camera_for(view, Wd, Hd)
    v = dict(DEFAULT, accel=accel)
    o0, o1 = Oracle(sa0, Wd, Hd, **v), Oracle(saR, Wd, Hd, **v)
    acc, seeds0, _, _ = o0.render(cam, 2)
    seeds0 = seeds0.copy()          # (the oracle advances the seed array it is given in place)
    acc, seeds, _, _ = o1.render(cam, 2, accum=acc, seeds=seeds0.copy())
    d = Device(Wd, Hd, extend_variant=variant, **v)
    try:
        d.upload(sa0)
        for k, wv in want.items():
            assert d.kernel_info()[k] == wv, (case, d.kernel_info())
        d.seed_default()
        d.render(cam, 2)
        d.rebuild_scene(prims, 0, None, builder=B, alpha=0.0)
        info = d.kernel_info()
        for k, wv in want.items():
            assert info[k] == wv, (case, info)
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, f"{case}: frames across an SBVH rebuild vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        got = d.counters()
        f = Device(Wd, Hd, extend_variant=variant, **v)
        try:
            f.upload(saR)
            assert f.kernel_info() == info
            f.set_seeds(seeds0)
            f.render(cam, 2)
            ref = f.counters()
        finally:
            f.close()
        for k in ("extend_rays", "extend_node_visits", "extend_prim_tests", "connect_rays", "connect_node_visits", "connect_prim_tests"):
            assert got[k] == ref[k], (case, k, got[k], ref[k])
    finally:
        d.close()


# ---- holders ---------------------------------------------------------------------------------------------------------------------------
def test_shared_contexts_and_group_lanes_render_the_sbvh_rebuilt_scene():
    (gt0, sa0), (gt1, sa1), view = RS.pair("scramble", "sah", 2, 0.0)
    cam = scenes.camera_for(view, Wd, Hd)
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=4)
    try:
        a.upload(sa0)
        b.share_scene(a)
        g.upload(sa0)
        g.seed(0)
        b.seed_default()
        b.render(cam, 1)          # work in flight on a holder that is not the one rebuilding
        st = a.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=0.0)
        st2 = g.rebuild_scene(sa1.prims, 0, None, builder=B, alpha=0.0)
        assert st["n_idx"] == len(sa1.primIdx) == st2["n_idx"] and st["max_depth"] == RB.depth(sa1) == st2["max_depth"]
        want_arrays, want_info = TR._fresh(sa1, **DEFAULT)
        for h in [a, b] + g.devs:
            assert h.kernel_info()["stack_entries"] == want_info["stack_entries"]
        assert a.kernel_info() == want_info and b.kernel_info() == want_info
        TR._same(TR._arrays(b), want_arrays, "the sharing partner's arrays")
        TR._same(TR._arrays(g.devs[3]), want_arrays, "lane 3's arrays")
        ref = Oracle(sa1, Wd, Hd, **DEFAULT).render(cam, 1)[0]
        for dv in (a, b):
            dv.seed_default()
            dv.reset()
            dv.render(cam, 1)
            assert_bits(dv.read_accum(), ref, "shared pair after an SBVH rebuild")
        g.seed(0)
        g.reset()
        g.render(cam, 4)
        exp = None
        for m in range(4):
            r = Oracle(sa1, Wd, Hd, **DEFAULT).render(cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0]
            exp = r if exp is None else exp + r
        assert_bits(g.read_accum(), exp, "4-lane group after an SBVH rebuild")
    finally:
        g.close()
        b.close()
        a.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_sbvh_refusals_return_their_code_and_change_nothing():
    gt, sa, view = R.build(alpha=0.0, blas=4, spheres=2)
    cam = scenes.camera_for(view, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        d.rebuild_scene(builder=B, alpha=0.0)   # (so that a grown set exists and the live one is a rebuilt one)
        TR._check(d, sa, "rebuilt to itself", **DEFAULT)
        before, info = TR._arrays(d), d.kernel_info()
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        inf = sa.prims.copy()
        inf["v1"][500, 1] = np.inf
        I, U = W.RT_E_INVALID, W.RT_E_UNSUPPORTED
        for what, code, args, kw in (("alpha NaN", I, (), dict(builder=B, alpha=float("nan"))), ("alpha -0.1", I, (), dict(builder=B, alpha=-0.1)),
                                     ("alpha 1.5", I, (), dict(builder=B, alpha=1.5)),
                                     ("infinite vertex", U, (inf, 0, None), dict(builder=B, alpha=0.0)),
                                     ("infinite vertex, alpha 1", U, (inf, 0, None), dict(builder=B, alpha=1.0))):
            TR._refused(d, code, before, info, cam, ref, what, *args, **kw)
        for builder in RB.BUILDERS:
            with pytest.raises(ValueError, match="alpha"):
                d.rebuild_scene(builder=builder, alpha=0.0)
        with pytest.raises(ValueError, match="max_leaf"):
            d.rebuild_scene(builder=B, max_leaf=4)
        with pytest.raises(ValueError):
            d.rebuild_scene(builder="sbvh")
        L = W.device_lib()
        st = np.zeros((), W.RebuildStats)
        assert L.rt_rebuild_scene(d._h, None, 0, 0, None, 0, 7, None, W.ptr(st)) == I      # builder 7 stays unknown
        TR._same(TR._arrays(d), before, "after the unknown builder")
        assert L.rt_rebuild_scene(d._h, None, 0, 0, None, 0, W.REBUILD_SBVH, None, W.ptr(st)) == W.RT_OK   # NULL options: alpha 0
        TR._same(TR._arrays(d), before, "after a rebuild with NULL options")
    finally:
        d.close()


def test_an_sbvh_rebuild_that_would_change_the_layout_is_refused():
    """The 128 coincident triangles of test_gpu_rebuild: no split separates them, the builder makes one leaf of 128 primitives."""
    s, coincident = TR._coincident()
    sa = s.arrays(bvh4=False)
    view = dict(origin=(0.5, 0.5, 8.0), forward=(0.0, 0.0, 1.0), fov=64.0, aperture=0.01)
    cam = scenes.camera_for(view, Wd, Hd)
    prims = sa.prims.copy()
    for k in ("v0", "v1", "v2"):
        prims[k][40:168, :3] = coincident[:, "v0 v1 v2".split().index(k)]
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        assert d.kernel_info()["layout"] == 1
        before, info = TR._arrays(d), d.kernel_info()
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        for alpha in (0.0, 0.5):
            TR._refused(d, W.RT_E_UNSUPPORTED, before, info, cam, ref, f"layout-changing (alpha {alpha})", prims, 0, None, builder=B, alpha=alpha)
        d.rebuild_scene(prims, 0, None, builder="lbvh")              # the linear builder's leaves hold at most max_leaf: fine
        assert d.kernel_info()["layout"] == 1
    finally:
        d.close()
