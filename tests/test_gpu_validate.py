"""Odd but legal scenes on the GPU, refused uploads, and the checks of rt_debug_set_rays.

validate_catalogue.py holds hand-made wire arrays that are not what the builders emit.  Each runs on every traversal path of
test_gpu_groundtruth.CASES that applies to it, the path selected the same way (the environment knobs, then `kernel_info` must report
it): over 2 frames the accumulator, the seeds and the extend counters must be the oracle's bit for bit, and the camera rays and the
extension rays of bounces 1 and 2 must be on the float64 closest hit of geom64 (its tolerances and decidability floors; the CPU
suite holds the same scenes above those floors with the oracle in place of the kernels).

Safety: nothing reaches the GPU unaudited.  `_upload` asserts that rt_validate_scene accepts the arrays and that the access audit
(wire_audit.py) is empty immediately before every upload.  A refused mutant is only ever handed to rt_upload_scene, which must refuse
it as rt_validate_scene did and leave the bound scene as it was; its traversal is never tried."""
import numpy as np
import pytest

import geom64 as G
import test_gpu_groundtruth as T
import validate_catalogue as K
import validate_sweep as S
import wire_audit as A
from helpers import assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, RtError
from oracle.oracle_py import seed_stream
from test_gpu_parity import _ctr_equal

pytestmark = pytest.mark.gpu

WD, HD, TUNE, EVENT, FRAME = T.WD, T.HD, T.TUNE, T.EVENT, T.FRAME
_ORACLE = {}


def _upload(d, sa, accel):
    rc, msg = S.validate(sa, accel)
    assert rc == W.RT_OK, msg
    assert A.audit_both(sa, accel) == []
    d.upload(sa)


def _entries_of(case):
    kind, accel, variant, env, want = T.CASES[case]
    out = []
    for name in K.CATALOGUE:
        e = K.entry(name)
        if e.kind == kind and accel in e.accels and (variant == 1 or not e.layout0_only):
            out.append(name)
    return out


def _oracle_frames(name, accel):
    """Two frames of the entry through the oracle: (accumulator, seeds, extend counters, connect counters), once per entry and accel."""
    key = (name, accel, "frames")
    if key not in _ORACLE:
        e = K.entry(name)
        _ORACLE[key] = oracle_for(e.sa, WD, HD, accel=accel, **FRAME).render(scenes.camera_for(e.view, WD, HD), 2)
    return _ORACLE[key]


def _oracle_extend(name, accel, q, tag):
    key = (name, accel, tag)
    if key not in _ORACLE:
        r = q.copy()
        _, ctr = oracle_for(K.entry(name).sa, 64, 48, accel=accel, **FRAME).extend(r, want_steps=True)
        _ORACLE[key] = (r, ctr)
    return _ORACLE[key]


def _frames(d, name, accel, what):
    e = K.entry(name)
    acc, seeds, ec, cc = _oracle_frames(name, accel)
    d.seed_default()
    d.render(scenes.camera_for(e.view, WD, HD), 2)
    assert_bits(d.read_accum(), acc, f"{what}: accumulator after 2 frames")
    assert np.array_equal(d.get_seeds(), seeds), f"{what}: seeds after 2 frames"
    _ctr_equal(d.counters(), ec, cc)
    assert acc[..., :3].sum() > 0


def _ground_truth(d, name, what):
    """Camera rays and the extension rays of bounces 1 and 2, as the GPU's own shade leaves them, against float64."""
    e = K.entry(name)
    n = WD * HD
    d.set_seeds(seed_stream(0, n))
    d.reset()
    d.stage_begin_frame()
    d.stage_generate(scenes.camera_for(e.view, WD, HD))
    fr = []
    for b in range(3):
        rays = d.get_rays(b)
        assert len(rays) > 1000, (what, b, len(rays))
        d.stage_extend(b)
        got = d.get_rays(b)
        s = T._sub(len(rays))
        fr.append(round(G.compare(e.gt, rays[s], got[s], "camera" if b == 0 else "bounce", f"{what}: bounce {b} ({len(rays)} rays)"), 4))
        d.stage_shade(b)
        d.stage_connect(b, b)
    return fr


def _tree_rays(d, name, accel, what):
    """An entry without a camera (the fat leaves): its own rays, tiled past the event loops' threshold and as they are."""
    e = K.entry(name)
    rays = e.rays if len(e.rays) % 2 else np.concatenate([e.rays, e.rays[:1]])
    m = len(rays)
    tiled = np.concatenate([rays] * (EVENT // m + 2))[:EVENT + 1024]
    for b, q, tag in ((1, tiled, "tiled"), (2, rays, "plain")):
        d.reset_counters()
        got = T._inject(d, b, q)
        assert G.compare(e.gt, rays, got[:m], "adversarial", f"{what} ({tag})") == 1.0
        want, ctr = _oracle_extend(name, accel, q, tag)
        assert np.array_equal(got["primIdx"], want["primIdx"]) and G.mismatch_rows(got["t"][:, None], want["t"][:, None]) == 0, f"{what} ({tag})"
        dev = d.counters()
        for k in ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests"):
            assert dev["extend_" + k] == ctr[k], (what, tag, k, dev["extend_" + k], ctr[k])
    return [1.0]


@pytest.mark.parametrize("case", list(T.CASES))
def test_odd_but_legal_scenes_on_every_path(case, monkeypatch):
    kind, accel, variant, env, want = T.CASES[case]
    monkeypatch.setenv("RT355_TUNE", TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    names = _entries_of(case)
    assert len(names) >= 3, (case, names)
    for name in names:
        e = K.entry(name)
        what = f"{case}: {name}"
        d = Device(WD, HD, accel=accel, extend_variant=variant, **FRAME)
        try:
            _upload(d, e.sa, accel)
            info = d.kernel_info()
            if e.view is not None:
                _frames(d, name, accel, what)
                fr = _ground_truth(d, name, what)
            else:
                fr = _tree_rays(d, name, accel, what)
            for k, v in want.items():
                assert info[k] == v, (what, info)
            assert info["n_blas"] == len(e.sa.blas), (what, info)
        finally:
            d.close()
        print(what, info, "decidable", fr)


# ---- refused uploads ----------------------------------------------------------------------------------------------------------------------
def _raw_upload(d, sa, accel, counts=None, no_lights_pointer=False):
    n = A.counts_of(sa, accel)
    n.update(counts or {})
    P, nodes = W.ptr, sa.nodes(accel)
    lights = None if no_lights_pointer or not len(sa.lights) else P(sa.lights)
    rc = d._lib.rt_upload_scene(d._h, P(sa.prims), n["nPrims"], P(sa.mats), n["nMats"], P(sa.tex) if len(sa.tex) else None, n["nTexels"], lights,
                                n["nLights"], P(nodes), n["nNodes"], P(sa.primIdx), n["nIdx"], P(sa.tlas), n["nTlas"], P(sa.blas), n["nBlas"])
    return rc, d._lib.rt_last_error().decode()


def _refusals(sa, accel):
    """One representative per refusal message of validate_scene: (message part, code, arrays, counts)."""
    INV, UNS = W.RT_E_INVALID, W.RT_E_UNSUPPORTED
    mut = lambda *m: S.apply(sa, list(m))
    tl = int(np.where(sa.tlas["leftRight"] != 0)[0][0])
    tleaf = int(np.where(sa.tlas["leftRight"] == 0)[0][0])
    root = int(sa.blas["bvhIdx"][0])
    mat = int(sa.prims["matIdx"][0])
    out = [
        ("missing array", INV, sa, dict(nPrims=0)),
        ("negative count", INV, sa, dict(nTexels=-1)),
        ("matIdx", INV, mut(("prims", 0, "matIdx", None, len(sa.mats))), None),
        ("objType", INV, mut(("prims", 0, "objType", None, 3)), None),
        ("primIdx[", INV, mut(("primIdx", 5, None, None, len(sa.prims))), None),
        ("lights[", INV, mut(("lights", 0, None, None, len(sa.prims))), None),
        ("texture window", INV, mut(("mats", mat, "texIdx", None, 0), ("mats", mat, "texW", None, 1), ("mats", mat, "texH", None, 1)), None),
        ("BLASidx out of range", INV, mut(("tlas", tleaf, "BLASidx", None, len(sa.blas))), None),
        ("child out of range", INV, mut(("tlas", tl, "leftRight", "hi", len(sa.tlas))), None),
        ("reachable twice", INV, mut(("tlas", tl, "leftRight", "hi", tl)), None),
        ("bvhIdx out of range", INV, mut(("blas", 1, "bvhIdx", None, len(sa.nodes(accel)))), None),
    ]
    if accel == 0:
        out += [("malformed BVH", INV, mut(("bvh2", root, "first", None, root)), None),
                ("leaf range exceeds primIdx", INV, mut(("bvh2", int(np.where(sa.bvh2["count"] > 0)[0][0]), "first", None, len(sa.primIdx))), None)]
    else:
        i, k = [(i, k) for i in sorted(S.topology(sa, 1)["bvh4"]) for k in range(4) if sa.bvh4["count"][i][k] > 0 and sa.bvh4["first"][i][k] != -1][0]
        out += [("malformed BVH", INV, mut(("bvh4", i, "count", k, 0), ("bvh4", i, "first", k, i)), None),
                (f"bvh4 node {i} slot {k}", INV, mut(("bvh4", i, "first", k, -5)), None),
                (f"bvh4 node {i} slot {k}", INV, mut(("bvh4", i, "count", k, -3), ("bvh4", i, "first", k, 7000000)), None)]
    for name, lim, a, ok in S.limit_scenes():                 # beyond the stacks and the 15-bit ids
        if not ok and a == accel:
            out.append(({"chain": "stack entries", "comb": "stack entries", "tlas_chain": "tlas: depth"}.get(name.split("(")[0], "32768"), UNS, lim, None))
    return out


@pytest.mark.parametrize("accel", [W.ACCEL_BVH2, W.ACCEL_BVH4], ids=["bvh2", "bvh4"])
def test_a_refused_upload_answers_as_validation_did_and_changes_nothing(accel):
    """rt_upload_scene returns the code (and message) rt_validate_scene gave, the bound scene's device arrays are byte for byte what
    they were, and the next frame is bit-identical to the one before."""
    sa = scenes.two_blas_scene(0.0, 8)[0].arrays()
    view = scenes.two_blas_scene(0.0, 8)[1]
    cam = scenes.camera_for(view, 96, 54)
    d = Device(96, 54, accel=accel, **FRAME)
    try:
        _upload(d, sa, accel)

        def frame():
            d.seed_default()
            d.reset()
            d.render(cam, 1)
            return d.read_accum().copy(), d.get_seeds().copy()
        acc0, seeds0 = frame()
        assert acc0[..., :3].sum() > 0
        before = {k: d.scene_array(k).copy() for k in W.SCENE_ARRAYS}
        cases = _refusals(sa, accel)
        assert len(cases) >= 14
        for part, code, arrays, counts in cases:
            vrc, vmsg = S.validate(arrays, accel, counts)
            assert vrc == code and part in vmsg, (part, vrc, vmsg)
            rc, msg = _raw_upload(d, arrays, accel, counts)
            assert (rc, msg) == (vrc, vmsg), (part, rc, msg)
            for k, v in before.items():
                assert np.array_equal(d.scene_array(k), v), (part, k)
            acc, seeds = frame()
            assert_bits(acc, acc0, f"frame after the refusal '{part}'")
            assert np.array_equal(seeds, seeds0), part
        rc, msg = _raw_upload(d, sa, accel, no_lights_pointer=True)
        assert rc == W.RT_E_INVALID and "lights == NULL" in msg
        assert_bits(frame()[0], acc0, "frame after the refusal of a NULL lights pointer")
    finally:
        d.close()


# ---- rt_debug_set_rays --------------------------------------------------------------------------------------------------------------------
def test_debug_set_rays_refuses_pixels_outside_the_band_and_unknown_primitives():
    """The kernels index the accumulator by a ray's pixelIdx and the primitive array by its primIdx: rt_debug_set_rays refuses a
    record outside the context's band or outside [-1, nPrims) with RT_E_INVALID, and a refused call leaves the queue as it was."""
    sa = scenes.two_blas_scene(0.0, 8)[0].arrays()
    d = Device(64, 48, y0=8, y1=24, **FRAME)
    try:
        _upload(d, sa, 0)
        first, npix = d.first_pixel, d.npix
        rng = np.random.default_rng(3)
        rays = G.make_rays(rng.uniform(-1, 1, (200, 3)), G._rand_dirs(rng, 200))
        rays["pixelIdx"] = first + np.arange(200)
        rays["pixelIdx"][-1], rays["primIdx"][-1], rays["t"][-1] = first + npix - 1, len(sa.prims) - 1, 1.0     # the last valid values
        d.set_rays(1, rays)
        q0 = d.get_rays(1)
        assert len(q0) == 200 and np.array_equal(q0["pixelIdx"], rays["pixelIdx"]) and q0["primIdx"][-1] == len(sa.prims) - 1
        for field, value, part in (("pixelIdx", first - 1, "band"), ("pixelIdx", first + npix, "band"), ("pixelIdx", -1, "band"),
                                   ("primIdx", len(sa.prims), "primIdx"), ("primIdx", -2, "primIdx"), ("primIdx", S.I32_MIN, "primIdx")):
            bad = rays[:50].copy()
            bad[field][17] = value
            with pytest.raises(RtError, match=part):
                d.set_rays(1, bad)
            q = d.get_rays(1)
            assert q.tobytes() == q0.tobytes(), (field, value)
    finally:
        d.close()
