"""The linear BVH builder on the MI355X (rt_build_bvh2): its arrays equal the host restatement's bit for bit, repeat builds are
identical, and the traversal kernels walking its trees are bit-exact with the oracle and match the float64 ground truth on every
traversal path (each confirmed through kernel_info)."""
import numpy as np
import pytest

import lbvh_check as K
import test_gpu_groundtruth as GT
import test_gpu_group_streams as GS
import test_groundtruth_cpu as C
import test_lbvh_cpu as L
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device
from magr_ray_tracer_amd.scene import BuildError, build_lbvh
from oracle.oracle_py import Oracle

pytestmark = pytest.mark.gpu

_BIG = {}


def _big(name):
    """Primitive arrays and ranges of the large inputs: sponza_class (264,946 triangles), both BLAS of config 5, a 1M soup."""
    if name not in _BIG:
        if name == "sponza_class":
            s, _ = scenes.sponza_class(1.0)
            p = K.prims_of(s)
            _BIG[name] = (p, [(0, len(p))])
        elif name == "config5":
            s, _ = scenes.config5_scene(0.0)
            sa = s.arrays(bvh4=False)
            first1 = _config5_split(sa)
            _BIG[name] = (sa.prims, [(0, first1), (first1, len(sa.prims) - first1)])
        else:
            _BIG[name] = (K.prims_of(K.soup(1 << 20, seed=12)), [(0, 1 << 20)])
    return _BIG[name]


def _config5_split(sa):
    """First primitive of config 5's second BLAS: the primitives its subtree references."""
    nodes, root = sa.bvh2, int(sa.blas["bvhIdx"][1])
    st, lo = [root], len(sa.prims)
    while st:
        i = st.pop()
        if nodes["count"][i]:
            f, c = int(nodes["first"][i]), int(nodes["count"][i])
            lo = min(lo, int(sa.primIdx[f:f + c].min()))
        else:
            st += [int(nodes["first"][i]), int(nodes["first"][i]) + 1]
    return lo


def _same(dev, host, what):
    dn, di, ds = dev
    hn, hi_, hs = host
    assert np.array_equal(dn.view(np.uint8), hn.view(np.uint8)), f"{what}: node arrays differ"
    assert np.array_equal(di, hi_), f"{what}: primIdx differs"
    for k in ("nodes", "leaves", "depth", "morton_bits", "sah_cost"):
        assert ds[k] == hs[k], (what, k, ds[k], hs[k])
    assert ds["device_ms"] > 0


@pytest.mark.parametrize("name", list(K.INPUTS) + ["sponza_class", "config5", "soup-1M"])
def test_device_build_equals_host_restatement(name):
    if name in K.INPUTS:
        p = K.prims_of(K.INPUTS[name]())
        ranges = [(0, len(p))]
    else:
        p, ranges = _big(name)
    for first, count in ranges:
        dev = build_lbvh(p, first, count, device=0, node_base=13, idx_base=9)
        host = build_lbvh(p, first, count, device=None, node_base=13, idx_base=9)
        _same(dev, host, f"{name} [{first}, +{count})")
        if count <= 300000:
            K.check_tree(p, first, count, dev[0], dev[1], dev[2], 13, 9, what=name)
        print(name, count, {k: round(v, 3) if isinstance(v, float) else v for k, v in dev[2].items()})


def test_ten_device_builds_are_identical():
    p, _ = _big("sponza_class")
    ref = build_lbvh(p, device=0)
    for _ in range(9):
        got = build_lbvh(p, device=0)
        assert np.array_equal(got[0].view(np.uint8), ref[0].view(np.uint8)) and np.array_equal(got[1], ref[1])


def test_error_paths_return_codes_then_a_build_succeeds():
    p = K.prims_of(K.soup(64))
    for kw, code in [(dict(node_cap=126), W.RT_E_INVALID), (dict(count=0), W.RT_E_INVALID), (dict(first=60, count=5), W.RT_E_INVALID),
                     (dict(max_leaf=200), W.RT_E_INVALID), (dict(device=99), W.RT_E_INVALID), (dict(device=-1), W.RT_E_INVALID)]:
        kw = dict(kw)
        dev = kw.pop("device", 0)
        with pytest.raises(BuildError) as e:
            build_lbvh(p, device=dev, **kw)
        assert e.value.code == code, (kw, e.value.code, str(e.value))
        _same(build_lbvh(p, device=0), build_lbvh(p, device=None), f"valid build after {kw}")
    s = K.soup(64)
    s.BuildBLAS(0, builder="lbvh", device=0)
    assert s.lbvh_stats()["device_ms"] > 0


# ---- traversal over LBVH trees -------------------------------------------------------------------------------------------------------
def _lbvh_gt_scenes():
    with pytest.MonkeyPatch.context() as m:
        m.setattr(C.G, "GTScene", L.LbvhGT)
        return {"one": C.soup_scene(1.0, room=True), "multi": C.tlas_scene(1.0, room=True)}


_SC = {}


def lbvh_scenes():
    if not _SC:
        _SC.update(_lbvh_gt_scenes())
    return _SC


PATHS = ["bvh2-persist", "bvh2-layout0", "bvh2-one-ray-per-lane", "bvh4-persist", "tlas-lds", "tlas-spill"]


@pytest.mark.parametrize("case", PATHS)
def test_hip_on_lbvh_trees_matches_float64_ground_truth(case, monkeypatch):
    """test_gpu_groundtruth's checks (camera, bounce and adversarial rays, every connect) on LBVH trees, path confirmed by kernel_info."""
    monkeypatch.setattr(GT, "_SCENES", lbvh_scenes())
    GT.test_hip_traversal_matches_float64_ground_truth(case, monkeypatch)


@pytest.mark.parametrize("case", PATHS)
def test_lbvh_frames_bit_exact_vs_oracle(case, monkeypatch):
    """Two frames over an LBVH scene: accumulator, seeds and extend counters equal the oracle's on the same arrays."""
    kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gt, sa, view = lbvh_scenes()[kind]
    Wd, Hd = 320, 240
    cam = scenes.camera_for(view, Wd, Hd)
    v = dict(DEFAULT, accel=accel)
    ref, seeds, e, c = Oracle(sa, Wd, Hd, **v).render(cam, 2)
    d = Device(Wd, Hd, extend_variant=variant, **v)
    try:
        d.upload(sa)
        info = d.kernel_info()
        for k, want_v in want.items():
            assert info[k] == want_v, (case, info)
        d.seed_default()
        d.render(cam, 2)
        assert_bits(d.read_accum(), ref, f"{case}: LBVH frames vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        ctr = d.counters()
        for k in ("rays", "node_visits", "prim_tests"):
            assert ctr["extend_" + k] == e.get(k, 0), (case, k, ctr["extend_" + k], e.get(k, 0))
    finally:
        d.close()


def test_lbvh_group_of_four_lanes_vs_oracle(monkeypatch):
    """A 4-lane rt_group over a device-built LBVH sponza_class: every lane and the group sum equal the oracle bit for bit."""
    s, view = scenes.sponza_class(0.2, builder="lbvh", device=0)
    assert s.lbvh_stats()["device_ms"] > 0
    sa = s.arrays()
    cam = scenes.camera_for(view, GS.Wd, GS.Hd)
    host = scenes.sponza_class(0.2, builder="lbvh", device=None)[0].arrays()
    assert np.array_equal(sa.bvh2.view(np.uint8), host.bvh2.view(np.uint8)) and np.array_equal(sa.primIdx, host.primIdx)
    ref = GS._oracle(sa, cam, 4)
    got = GS._render(sa, cam, 4, None, monkeypatch)
    exp = None
    for m in range(4):
        assert_bits(got["acc_b"][m], ref[m]["acc_b"], f"LBVH group lane {m}")
        exp = ref[m]["acc_b"] if exp is None else exp + ref[m]["acc_b"]
    assert_bits(got["sum_b"], exp, "LBVH group sum")
