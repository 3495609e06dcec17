"""Every traversal path obeys the rule for rays with a bad component (tests/edge_rays.py, test_edge_rays_cpu.py; include/rt355.h,
rt_trace): a ray with a NaN or infinite component in origin or direction misses and occludes nothing; every other ray - zero, subnormal,
1e30 and FLT_MAX components included - is traced as given, which means: bit for bit what rt_stage_extend computes on the same context
and what the oracle's extend / connect compute on the CPU (NaN payloads aside: x86 and the GPU produce different ones).

On every case of test_gpu_trace.py (the nested loops over BVH2 and BVH4, k_trace_persist with its scalar-cache bounce, the TLAS
kernels with and without spill, k_trace_persist4 and k_trace_persist4_tlas), the set is traced as it is - the one-ray-per-lane
branches - and tiled past 65,536 rays - the event loops - through the in-place, packed float3 and strided forms, that is through
k_trace_load / k_trace_store too.  The base rays are camera rays of test_groundtruth_cpu's scenes without their room, 40 that hit the
soup and 40 that pass it; the GPU scenes are the same scenes inside a room, where the latter hit a wall."""
import numpy as np
import pytest

import edge_rays as E
import test_edge_rays_cpu as EC
import test_gpu_trace as T
from helpers import oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from oracle.oracle_py import REFERENCE_ORDER, Oracle

pytestmark = pytest.mark.gpu

TMAX = E.TMAX
_REF = {}


def _set(kind):
    gt, sa, rays, names = EC.scene_set("soup" if kind == "one" else "tlas")
    return rays, names


def _tiled(rays):
    return np.concatenate([rays] * (T.EVENT // len(rays) + 1))[:T.EVENT + 1024]


def _oracle(kind, accel, sa):
    """The oracle's extend of a scene's edge set (computed once per scene and accel), and the oracle itself."""
    key = (kind, accel)
    if key not in _REF:
        o = oracle_for(sa, T.WD, T.HD, accel=accel, **T.FRAME)
        want = _set(kind)[0].copy()
        with np.errstate(all="ignore"):
            o.extend(want)
        _REF[key] = (o, want)
    return _REF[key]


def _same_as_oracle(hit, point, normal, want, names, what):
    nb = 2 * E.N_BASE
    bad = np.where(hit["primIdx"] != want["primIdx"])[0]
    assert not len(bad), f"{what}: primIdx differs from the oracle's on {len(bad)} rays, e.g. {E.label(names, nb, bad[0])}: {hit['primIdx'][bad[0]]}, oracle {want['primIdx'][bad[0]]}"
    for got, ref, field in ((hit["t"], want["t"], "t"), (hit["u"], want["u"], "u"), (hit["v"], want["v"], "v"), (point, want["I"], "point"), (normal, want["N"], "normal")):
        bad = E.differing(got, ref)
        assert not len(bad), f"{what}: {field} differs from the oracle's on {len(bad)} rays, e.g. {E.label(names, nb, bad[0])}: {got[bad[0]]}, oracle {ref[bad[0]]}"


@pytest.mark.parametrize("case", list(T.CASES))
def test_closest_obeys_the_rule_on_every_path(case, monkeypatch):
    d, gt, sa, view = T._device(case, monkeypatch)
    try:
        kind, accel = T.CASES[case][0], T.CASES[case][1]
        rays, names = _set(kind)
        o, want = _oracle(kind, accel, sa)
        m, bad = len(rays), E.non_finite(rays)
        assert want["primIdx"][~bad].max() >= 0 and (want["primIdx"][bad] == -1).all()
        # ---- as it is: the one-ray-per-lane branches
        ref = T._stage_route(d, rays)
        hit, point, normal = T._trace_layouts(d, rays)          # in place = packed float3 = strided, asserted inside
        T._same_as_stage(hit, point, normal, ref, f"{case}: edge set")
        _same_as_oracle(hit, point, normal, want, names, f"{case}: edge set")
        miss = np.zeros(int(bad.sum()), dtype=W.Hit)
        miss[:] = T.MISS
        assert hit[bad].tobytes() == miss.tobytes(), f"{case}: a non-finite ray did not return exactly the miss record"
        assert not point[bad].view(np.uint32).any() and not normal[bad].view(np.uint32).any(), f"{case}: point / normal of a non-finite ray"
        # ---- tiled past EVENT rays: the event loops, where the path has them
        tiled = _tiled(rays)
        assert len(tiled) > T.EVENT
        ref = T._stage_route(d, tiled)
        thit, tpoint, tnormal = T._trace_layouts(d, tiled)
        T._same_as_stage(thit, tpoint, tnormal, ref, f"{case}: tiled edge set")
        _same_as_oracle(thit[:m], tpoint[:m], tnormal[:m], want, names, f"{case}: first copy of the tiled edge set")
        for at in range(m, len(tiled), m):                       # every (partial) copy traced as the first
            k = len(tiled[at:at + m])
            assert thit[at:at + k].tobytes() == thit[:k].tobytes() and tpoint[at:at + k].tobytes() == tpoint[:k].tobytes() and \
                tnormal[at:at + k].tobytes() == tnormal[:k].tobytes(), f"{case}: copy at {at} of the tiled batch traced differently"
        assert thit[:m][bad].tobytes() == miss.tobytes() and not tpoint[:m][bad].view(np.uint32).any() and not tnormal[:m][bad].view(np.uint32).any()
    finally:
        d.close()


@pytest.mark.parametrize("case", T.ANY_CASES)
def test_any_obeys_the_rule_whatever_tmax(case, monkeypatch):
    d, gt, sa, view = T._device(case, monkeypatch)
    try:
        kind, accel = T.CASES[case][0], T.CASES[case][1]
        rays, names = _set(kind)
        o, _ = _oracle(kind, accel, sa)
        o_ref = Oracle(sa, T.WD, T.HD, accel=accel, connect_order=REFERENCE_ORDER, **T.FRAME)
        nb, m, bad = 2 * E.N_BASE, len(rays), E.non_finite(rays)
        O, D = np.ascontiguousarray(rays["O"][:, :3]), np.ascontiguousarray(rays["D"][:, :3])
        seen = set()
        tl = lambda x: np.concatenate([x] * (T.EVENT // m + 1))[:T.EVENT + 1024]      # noqa: E731
        for tmax in TMAX:
            what = f"{case}: tmax {tmax}"
            reach = None if tmax is None else np.full(m, tmax, np.float32)
            with np.errstate(all="ignore"):
                want = o.occluded(O, D, reach)                   # connect's traversal on the same bits (test_edge_rays_cpu.py: = orc_connect)
            got = d.trace(O, D, tmax=reach, mode="any")
            assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
            wrong = np.where(got.astype(bool) != want)[0]
            assert not len(wrong), f"{what}: {len(wrong)} rays decided differently from the oracle's connect, e.g. {E.label(names, nb, wrong[0])}: oracle {bool(want[wrong[0]])}"
            assert not got[bad].any(), f"{what}: a non-finite ray is occluded"
            # ... and the reference's own loop (near child first, failed boxes entered at tmax > 1e30) decides every ray alike whose
            # primitive tests float32 can compute: only a ray with a FLT_MAX direction component may differ (include/rt355.h)
            with np.errstate(all="ignore"):
                ref = o_ref.occluded(O, D, reach)
            off = got.astype(bool) != ref
            assert E.huge_dir(rays)[off].all(), f"{what}: {int((off & ~E.huge_dir(rays)).sum())} rays without a FLT_MAX direction component decided differently from the reference's order"
            seen |= set(np.unique(got).tolist())
            # tiled: the event loops
            tgot = d.trace(tl(O), tl(D), tmax=None if tmax is None else tl(reach), mode="any")
            assert np.array_equal(tgot, tl(got)), f"{what}: the tiled batch decides differently"
        assert seen == {0, 1}
    finally:
        d.close()


@pytest.mark.parametrize("case", list(T.CASES))
def test_edge_queries_leave_the_next_frame_alone(case, monkeypatch):
    a, gt, sa, view = T._device(case, monkeypatch, w=160, h=96, tune=False, profile=2)
    b, *_ = T._device(case, monkeypatch, w=160, h=96, tune=False, profile=2)
    try:
        cam = scenes.camera_for(view, 160, 96)
        for x in (a, b):
            x.seed_default()
            x.reset()
            x.render(cam, 1)
        before = T._frame_state(a)
        rays, _ = _set(T.CASES[case][0])
        O, D = T._t(rays["O"]), T._t(rays["D"])
        a.trace(O, D)                                                                         # in place
        a.trace(O[:, :3].contiguous(), D[:, :3].contiguous(), point=True, normal=True)        # through the query's own arrays
        for tmax in (np.nan, np.inf, 5.0):
            a.trace(O, D, tmax=T._t(np.full(len(rays), tmax, np.float32)), mode="any")
        after = T._frame_state(a)
        for k in before:
            assert before[k] == after[k], f"{case}: {k} changed across the edge queries"
        for x in (a, b):
            x.render(cam, 1)
        sa_, sb_ = T._frame_state(a), T._frame_state(b)
        for k in sa_:
            assert sa_[k] == sb_[k], f"{case}: {k} of the next frame differs from a context that never traced"
    finally:
        a.close()
        b.close()
