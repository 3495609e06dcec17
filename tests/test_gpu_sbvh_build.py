"""The GPU build of SBVH BLAS trees on the MI355X (rt_build_bvh2_sbvh): its arrays and statistics equal BVH2::BuildBLAS's (16 host
threads) and the host restatement's byte for byte at alpha 0 and 1e-5 on every input of test_sbvh_gpu_cpu and on both BLAS of config 5
(every second triangle); the ref arrays grow when they start too small; repeat builds are identical; refusals are found by the
status word, return their codes and write nothing; frames over its trees are bit-identical to frames over the host's."""
import numpy as np
import pytest

import lbvh_check as K
import sbvh_check as C
import test_gpu_group_streams as GS
import test_sah_gpu_cpu as S
import test_sbvh_gpu_cpu as T
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device
from magr_ray_tracer_amd.scene import build_sbvh_gpu

pytestmark = pytest.mark.gpu

GPU_ALPHAS = (0.0, 1e-5)
COUNTS = ("nodes", "leaves", "n_idx", "depth", "spatial_splits", "prims_clipped", "forced_leaves", "levels", "sah_cost", "peak_refs")


def _device_block(p, alpha, first, count, nb, ib, nodes, idx, what):
    dev = C.build(p, alpha, first, count, device=0, node_base=nb, idx_base=ib)
    C.same(dev, nodes, idx, what)
    host = C.build(p, alpha, first, count, device=None, node_base=nb, idx_base=ib)
    C.same(host, nodes, idx, what + " (restatement)")
    for k in COUNTS:
        assert dev[2][k] == host[2][k], (what, k, dev[2][k], host[2][k])
    assert dev[2]["device_ms"] > 0
    print(what, count, {k: round(v, 3) if isinstance(v, float) else v for k, v in dev[2].items()})
    return dev


@pytest.mark.parametrize("alpha", GPU_ALPHAS)
@pytest.mark.parametrize("name", list(C.INPUTS))
def test_device_arrays_equal_buildblas(name, alpha):
    p = C.prims(name)
    nodes, idx, st = C.reference(name, alpha, 16)
    dev = _device_block(p, alpha, 0, len(p), 0, 0, nodes, idx, f"{name}, alpha {alpha}")
    C.same_stats(dev[2], st, f"{name}, alpha {alpha}")


@pytest.mark.parametrize("alpha", GPU_ALPHAS)
def test_sponza_class_two_blas_and_config5_at_their_offsets(alpha):
    p, blocks = C.sponza_blocks(alpha)
    for nb, ib, nodes, idx, st in blocks:
        dev = _device_block(p, alpha, 0, len(p), nb, ib, nodes, idx, f"sponza_class(0.2), alpha {alpha}, node base {nb}")
        if st is not None:
            C.same_stats(dev[2], st, "sponza_class(0.2)")
    p, blocks, st = C.two_blas_blocks(alpha, 16)
    got = [_device_block(p, alpha, *b, f"two_blas_scene({alpha}) [{b[0]}, +{b[1]})") for b in blocks]
    assert sum(g[2]["spatial_splits"] for g in got) == st["spatial_splits"] and sum(g[2]["prims_clipped"] for g in got) == st["prims_clipped"]


def test_config5_every_second_triangle():
    """Both BLAS of config5_scene(0.0, decimate=2) at their offsets: 37,810 triangles, 42,915 refs, 48,938 nodes, 1,727 spatial splits."""
    p, blocks, st = C.config5_blocks(2)
    got = [_device_block(p, 0.0, *b, f"config5(decimate 2) [{b[0]}, +{b[1]})") for b in blocks]
    assert (len(p), sum(len(g[1]) for g in got), sum(len(g[0]) for g in got), sum(g[2]["spatial_splits"] for g in got)) == (37810, 42915, 48938, 1727)
    assert sum(g[2]["spatial_splits"] for g in got) == st["spatial_splits"] and sum(g[2]["prims_clipped"] for g in got) == st["prims_clipped"]
    assert max(g[2]["depth"] for g in got) == st["depth"]


def test_ref_arrays_grow(monkeypatch):
    """soup-5000-seed9 at alpha 0 with an initial ref capacity of 5,000: the refs reach 1.92x, so the arrays grow at least once."""
    p = C.prims("soup-5000-seed9")
    nodes, idx, _ = C.reference("soup-5000-seed9", 0.0, 16)
    monkeypatch.setenv("RT355_SBVH_INITIAL_REFS", "5000")
    small = build_sbvh_gpu(p, 0.0, device=0)
    monkeypatch.delenv("RT355_SBVH_INITIAL_REFS")
    C.same(small, nodes, idx, "initial ref capacity 5000")
    assert small[2]["peak_refs"] > 5000
    C.same(build_sbvh_gpu(p, 0.0, device=0), nodes, idx, "default initial ref capacity")


def test_capacity_protocol_on_the_device():
    C.capacity_protocol(build_sbvh_gpu, C.prims("soup-600"), 0.0, device=0)


def test_ten_device_builds_are_identical():
    p, _ = C.sponza_blocks(0.0)
    ref = build_sbvh_gpu(p, 0.0, device=0)
    for _ in range(9):
        got = build_sbvh_gpu(p, 0.0, device=0)
        assert np.array_equal(got[0].view(np.uint8), ref[0].view(np.uint8)) and np.array_equal(got[1], ref[1])
        assert all(got[2][k] == ref[2][k] for k in COUNTS)


def test_refusals_return_their_codes_and_write_nothing():
    for make in (K.mixed, C.spheres_300):
        C.refused_call(build_sbvh_gpu, K.prims_of(make()), 0.0, W.RT_E_UNSUPPORTED, "bin index", device=0)
    for name, (make, frag) in S.REFUSED.items():
        C.refused_call(build_sbvh_gpu, K.prims_of(make()), 0.0, W.RT_E_UNSUPPORTED, frag, device=0)
    p = K.prims_of(K.soup(50))
    for kw, frag in S.BAD_ARGS:
        if "node_cap" not in kw:
            C.refused_call(build_sbvh_gpu, p, 0.0, W.RT_E_INVALID, frag, device=0, **kw)
    for alpha in (float("nan"), -0.1, 1.5):
        C.refused_call(build_sbvh_gpu, p, alpha, W.RT_E_INVALID, "alpha", device=0)
    C.refused_call(build_sbvh_gpu, p, 0.0, W.RT_E_INVALID, "device", device=99)
    # the lazy rule: mixed at alpha 0.5 builds; and a valid build after the refusals is correct
    pm = K.prims_of(K.mixed())
    dev, host = build_sbvh_gpu(pm, 0.5, device=0), build_sbvh_gpu(pm, 0.5, device=None)
    C.same(dev, host[0], host[1], "mixed, alpha 0.5")
    dev, host = build_sbvh_gpu(p, 0.0, device=0), build_sbvh_gpu(p, 0.0, device=None)
    C.same(dev, host[0], host[1], "a valid build after the refusals")
    # through the scene: mixed()'s primitives (its plane among them) appended behind a BLAS, refused on the device, scene unchanged
    assert "bin index" in T._scene_unchanged(K.mixed, 0.0, builder="sbvh_gpu", device=0)


def test_frames_over_gpu_built_trees_equal_host_built():
    """config5_scene(0.0, decimate=4) built with builder='sbvh_gpu' on the GPU and with the host builder: equal arrays, a 2-frame render
    of one BVH2 context and of one BVH4 context bit-identical, and a 4-lane group bit-identical."""
    sg, view = scenes.config5_scene(0.0, decimate=4, builder="sbvh_gpu", device=0)
    sh, _ = C._factory_at(16, lambda: scenes.config5_scene(0.0, decimate=4))
    assert {k: v for k, v in sg.stats().items() if k != "build_ms"} == {k: v for k, v in sh.stats().items() if k != "build_ms"}
    assert sg.stats()["spatial_splits"] > 0
    a, b = sg.arrays(), sh.arrays()
    for k in ("bvh2", "primIdx", "blas", "bvh4", "tlas"):
        assert np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)), k
    cam = scenes.camera_for(view, GS.Wd, GS.Hd)
    for accel in (W.ACCEL_BVH2, W.ACCEL_BVH4):
        out = []
        for sa in (a, b):
            d = Device(GS.Wd, GS.Hd, **dict(DEFAULT, accel=accel))
            try:
                d.upload(sa)
                d.seed_default()
                d.render(cam, 2)
                out.append(d.read_accum())
            finally:
                d.close()
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), accel
    with pytest.MonkeyPatch.context() as m:
        got = GS._render(a, cam, 4, None, m)
        ref = GS._render(b, cam, 4, None, m)
    for lane in range(4):
        assert_bits(got["acc_b"][lane], ref["acc_b"][lane], f"lane {lane}")
    assert_bits(got["sum_b"], ref["sum_b"], "group sum")
