"""The GPU build of the default SAH BLAS on the MI355X (rt_build_bvh2_sah): its arrays equal BVH2::BuildBLAS's (alpha = 1) byte for
byte on every input of test_sah_gpu_cpu and on sponza-class, both BLAS of config 5 and a 1M soup; stats equal; repeat builds are
identical; refusals return their codes and write nothing; frames over its trees are bit-identical to frames over the host's."""
import numpy as np
import pytest

import lbvh_check as K
import test_gpu_group_streams as GS
import test_sah_gpu_cpu as S
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device
from magr_ray_tracer_amd.scene import build_sah_gpu

pytestmark = pytest.mark.gpu


def _config5_split(sa):
    """First primitive of config 5's second BLAS: the lowest primitive its subtree references."""
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


def _blocks(name):
    """Primitive array and, per BLAS, (first, count, nodeBase, idxBase, host nodes, host primIdx) of BuildBLAS(alpha = 1)."""
    if name == "config5":
        s, _ = scenes.config5_scene(1.0)
        sa = s.arrays(bvh4=False)
        f1, r1 = _config5_split(sa), int(sa.blas["bvhIdx"][1])
        return sa.prims, [(0, f1, 0, 0, sa.bvh2[:r1], sa.primIdx[:f1]),
                          (f1, len(sa.prims) - f1, r1, f1, sa.bvh2[r1:], sa.primIdx[f1:])]
    s = scenes.sponza_class(1.0)[0] if name == "sponza_class" else K.soup(1 << 20, seed=12)
    p = K.prims_of(s)
    if name == "sponza_class":              # the factory's BLAS (one thread), then the same primitives appended at 16 threads
        n1, i1, _ = S.raw(s)
        s.BuildBLAS(0, threads=16)
        nodes, idx, _ = S.raw(s)
        return p, [(0, len(p), 0, 0, n1, i1), (0, len(p), len(n1), len(i1), nodes[len(n1):], idx[len(i1):])]
    s.BuildBLAS(0, threads=16)
    nodes, idx, _ = S.raw(s)
    return p, [(0, len(p), 0, 0, nodes, idx)]


@pytest.mark.parametrize("name", list(S.CASES) + ["sponza_class", "config5", "soup-1M"])
def test_device_arrays_equal_buildblas(name):
    if name in S.CASES:
        s = S.CASES[name]()
        p = K.prims_of(s)
        s.BuildBLAS(0, threads=16)
        nodes, idx, _ = S.raw(s)
        blocks = [(0, len(p), 0, 0, nodes, idx)]
    else:
        p, blocks = _blocks(name)
    for first, count, nb, ib, nodes, idx in blocks:
        dev = build_sah_gpu(p, first, count, device=0, node_base=nb, idx_base=ib)
        S.same(dev, nodes, idx, f"{name} [{first}, +{count})")
        host = build_sah_gpu(p, first, count, device=None, node_base=nb, idx_base=ib)
        for k in ("nodes", "leaves", "depth", "morton_bits", "sah_cost"):
            assert dev[2][k] == host[2][k], (name, k, dev[2][k], host[2][k])
        assert dev[2]["device_ms"] > 0
        print(name, count, {k: round(v, 3) if isinstance(v, float) else v for k, v in dev[2].items()})


def test_ten_device_builds_are_identical():
    p = K.prims_of(scenes.sponza_class(1.0)[0])
    ref = build_sah_gpu(p, device=0)
    for _ in range(9):
        got = build_sah_gpu(p, device=0)
        assert np.array_equal(got[0].view(np.uint8), ref[0].view(np.uint8)) and np.array_equal(got[1], ref[1])


def test_refusals_return_their_codes_and_write_nothing():
    for name, (make, frag) in S.REFUSED.items():
        S.refused_call(K.prims_of(make()), W.RT_E_UNSUPPORTED, frag, device=0)
    p = K.prims_of(K.soup(50))
    for kw, frag in S.BAD_ARGS:
        S.refused_call(p, W.RT_E_INVALID, frag, device=0, **kw)
    S.refused_call(p, W.RT_E_INVALID, "device", device=99)
    dev, host = build_sah_gpu(p, device=0), build_sah_gpu(p, device=None)
    S.same(dev, host[0], host[1], "a valid build after the refusals")


def test_group_frames_over_gpu_built_trees_equal_host_built():
    """sponza-class built with builder='sah_gpu' on the GPU and with the host SAH builder: a 4-lane group renders the same
    accumulators bit for bit, and so does one context on the BVH4 path."""
    sg, view = scenes.sponza_class(0.2, builder="sah_gpu", device=0)
    sh, _ = scenes.sponza_class(0.2)
    a, b = sg.arrays(), sh.arrays()
    for k in ("bvh2", "primIdx", "blas", "bvh4", "tlas"):
        assert np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)), k
    cam = scenes.camera_for(view, GS.Wd, GS.Hd)
    with pytest.MonkeyPatch.context() as m:
        got = GS._render(a, cam, 4, None, m)
        ref = GS._render(b, cam, 4, None, m)
    for lane in range(4):
        assert_bits(got["acc_b"][lane], ref["acc_b"][lane], f"lane {lane}")
    assert_bits(got["sum_b"], ref["sum_b"], "group sum")
    out = []
    for sa in (a, b):
        d = Device(GS.Wd, GS.Hd, **dict(DEFAULT, accel=W.ACCEL_BVH4))
        try:
            d.upload(sa)
            d.seed_default()
            d.render(cam, 2)
            out.append(d.read_accum())
        finally:
            d.close()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
