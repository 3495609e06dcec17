"""GPU suite (-m gpu): the arithmetic of the seven builtins (normalize / length / exp / sin / cos / acospi / atan2pi) as a run-time
mode of ONE library (RtConfig.builtins, include/rt355.h).

REFERENCE mode of librt355.so is held (a) to the reference's own OpenCL kernels - whole frames on 64 uncurated bands, k_shade launch by
launch, bit for bit - and (b) to the second library, librt355_refb.so, whose default is that mode: equal as bytes, stage by stage.  The
IEEE mode (the default) stays what the oracle computes, also with a REFERENCE context rendering beside it from the same scene copy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import builtins_check as B
import mathsets as M
import ref_gpu
from helpers import DEFAULT, assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device
from oracle.oracle_py import seed_stream

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not ref_gpu.available(), reason="oracle/_ref not built (needs /root/reference at build time)")
RT_E_INVALID, RT_E_UNSUPPORTED = -1, -4


# ---- 1. the config word is honoured ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["pinhole", "fisheye"])
def test_config_word_15_selects_the_reference_builtins(camera):
    """A context created through raw ctypes with config word 15 = RT_BUILTINS_REFERENCE renders two frames of branch_scene (textured
    sphere, glass with absorption, sphere light; fisheye camera too): accumulator, per-slot seeds and the seven queue lengths equal
    those of the second library bit for bit - and the accumulator differs from the IEEE context's."""
    Wd, Hd, frames = 192, 108, 2
    s, view = scenes.branch_scene()
    if camera == "fisheye":
        view = dict(view, type=1, fov=75.0)
    sa = s.arrays()
    cam = scenes.camera_for(view, Wd, Hd)
    refb = Device(Wd, Hd, lib="refb", **DEFAULT)
    refb.upload(sa)
    cam["focalLength"] = refb.focus(Wd // 2, Hd // 2, cam)
    ieee = Device(Wd, Hd, **DEFAULT)
    ieee.upload(sa)
    raw = B.RawDevice(B.raw_config(Wd, Hd, B.REFERENCE, **DEFAULT))
    raw.dev.upload(sa)
    got = {}
    for name, d in (("refb", refb), ("ieee", ieee), ("raw", raw.dev)):
        d.seed_default()
        d.render(cam, frames)
        got[name] = B.frame_state(d)
    refb.close()
    ieee.close()
    raw.close()
    assert got["refb"][0][..., :3].sum() > 0
    assert not B.same_bytes(got["refb"][0], got["ieee"][0]), "the two arithmetics give the same image: the scene does not tell them apart"
    assert B.same_bytes(got["raw"][0], got["refb"][0]), \
        "accumulator of the context created with config word 15 = RT_BUILTINS_REFERENCE differs from librt355_refb.so's" + \
        (" and equals the IEEE context's: the word is ignored" if B.same_bytes(got["raw"][0], got["ieee"][0]) else "")
    assert np.array_equal(got["raw"][1], got["refb"][1]), "per-slot seeds"
    assert got["raw"][2] == got["refb"][2], ("queue lengths", got["raw"][2], got["refb"][2])


# ---- 2. REFERENCE mode against the reference's own kernels, uncurated ---------------------------------------------------------------
UNCURATED_BANDS = list(range(352, 368))   # sixteen consecutive one-row bands; none selected, none skipped


@needs_ref
@pytest.mark.parametrize("case", ["nee", "kajiya_hemi_norr", "fisheye", "nee_bvh4"])
def test_reference_mode_whole_frames_uncurated_bands_vs_reference_kernels(case):
    """Whole frames, both sides free running from the same seeds under schedule S1 (RefGPU.frame_s1 against rt_render of librt355.so
    with builtins="reference"), on the sixteen consecutive bands 352-367: identical queue lengths at all seven bounces, identical
    per-slot RNG states after the frame, the accumulator within 1e-6 relative (denominator floor 1e-3) on every pixel - the tolerance of
    test_ref_builtins_whole_frames_uncurated_bands_vs_reference_kernels; the second library measured 0.0 on exactly these 64 bands
    (profiles/r03_hip_refb_vs_reference_s1_bands.log)."""
    from test_gpu_reference import FRAME_VARIANTS, RH, RW
    fn, vo, _, vi = FRAME_VARIANTS[case]
    v = dict(DEFAULT, **vi)
    s, view = fn()
    sa = s.arrays()
    worst = 0.0
    for y in UNCURATED_BANDS:
        cam = scenes.camera_for(dict(view, **vo), RW, RH)
        ref = ref_gpu.RefGPU(sa, **v)
        cam["focalLength"] = ref.focus(RW // 2, y, cam)
        r = ref.frame_s1(cam, y, y + 1, shading=v["shading"], russian_roulette=v["russian_roulette"])
        ref.close()
        d = Device(RW, RH, y0=y, y1=y + 1, builtins="reference", **v)
        assert d.builtins == B.REFERENCE
        d.upload(sa)
        d.set_seeds(seed_stream(y * RW, RW))
        d.render(cam, 1)
        got = d.read_accum().reshape(-1, 4)[y * RW:(y + 1) * RW]
        assert [len(d.get_rays(b)) for b in range(7)] == r["n_in"], (case, y)
        assert np.array_equal(d.get_seeds(), r["seeds"]), (case, y, "per-slot RNG states after the frame")
        d.close()
        rel = (np.abs(got.astype(np.float64) - r["accum"]) / np.maximum(np.abs(r["accum"]), 1e-3)).max(1)
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 1e-6 and r["accum"][:, :3].sum() > 0, (case, y, float(rel.max()))
    print(case, "bands", UNCURATED_BANDS[0], "-", UNCURATED_BANDS[-1], "accumulator max relative error", worst)


# ---- 3. k_shade per bounce, bit for bit --------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("case", ["nee", "fisheye"])
def test_reference_mode_shade_every_bounce_is_bit_exact_vs_reference_kernel(case):
    """k_shade of the shipped library in REFERENCE mode against the reference's own shade kernel under schedule S1 on the rays of every
    bounce of a reference frame (the body of test_ref_builtins_shade_every_bounce_is_bit_exact_vs_reference_kernel): every float of
    every survivor and shadow ray, the RNG states and the launch's accumulator, bit for bit."""
    from test_gpu_reference import RH, RW, _reference_frame
    fn, v, sa, cam, cap, (y0, y1) = _reference_frame(case, (359, 361))
    ref = ref_gpu.RefGPU(sa, **v)
    d = Device(RW, RH, y0=y0, y1=y1, builtins="reference", **v)
    d.upload(sa)
    first, n0 = y0 * RW, (y1 - y0) * RW
    for b, ext in enumerate(cap["ext"]):
        n = len(ext)
        seeds = seed_stream(7919 * (b + 1), n0)
        ref.clear_accum()
        rout, rsh, rseeds = ref.shade_s1(ext, seeds[:n].copy())
        racc = ref.rd(ref.accum, np.float32, 4 * RW * y1).reshape(-1, 4)[first:]
        d.set_rays(b, ext)
        d.set_seeds(seeds)
        d.reset()
        d.stage_shade(b)
        out = d.get_rays(b + 1)
        assert len(out) == len(rout), (b, len(out), len(rout))
        for f in ("pixelIdx", "bounces", "inside", "lastSpecular"):
            assert np.array_equal(out[f], rout[f]), (b, f)
        assert np.array_equal(d.get_seeds()[:n], rseeds[:n]), f"bounce {b}: RNG states after shade"
        for f in ("O", "D", "intensity"):
            assert np.array_equal(out[f].view(np.uint32), rout[f].view(np.uint32)), (b, f, float(np.abs(out[f] - rout[f]).max()))
        sh = d.get_shadow(b, b)
        assert len(sh) == len(rsh), (b, len(sh), len(rsh))
        if len(sh):
            assert np.array_equal(sh["pixelIdx"], rsh["pixelIdx"])
            assert np.array_equal(sh["tmax"], rsh["dist"] - np.float32(2e-4))
        got = d.read_accum().reshape(-1, 4)[first:first + n0]
        assert np.array_equal(got, racc[:n0]), (b, float(np.abs(got - racc[:n0]).max()))
    d.close()
    ref.close()


# ---- 4. stage by stage against the second library ----------------------------------------------------------------------------------
STAGE_VARIANTS = {"nee": dict(), "kajiya_hemi_norr": dict(shading=0, sampling=0, russian_roulette=False)}


def _pair_of_contexts(sa, Wd, Hd, v):
    a = Device(Wd, Hd, builtins="reference", **v)
    b = Device(Wd, Hd, lib="refb", **v)
    for d in (a, b):
        d.upload(sa)
    return a, b


@pytest.mark.parametrize("camera,aa", [("pinhole", 1), ("fisheye", 1), ("pinhole", 0)])
def test_stage_generate_equals_the_second_library(camera, aa):
    Wd, Hd = 192, 108
    s, view = scenes.branch_scene()
    if camera == "fisheye":
        view = dict(view, type=1, fov=75.0)
    sa = s.arrays()
    cam = scenes.camera_for(view, Wd, Hd)
    a, b = _pair_of_contexts(sa, Wd, Hd, DEFAULT)
    fa, fb = a.focus(Wd // 2, Hd // 2, cam), b.focus(Wd // 2, Hd // 2, cam)
    assert fa.tobytes() == fb.tobytes(), ("rt_focus", fa, fb)
    cam["focalLength"] = fa
    out = []
    for d in (a, b):
        d.set_seeds(seed_stream(0, Wd * Hd))
        d.reset()
        d.stage_begin_frame()
        d.stage_generate(cam, antiAliasing=aa)
        out.append((d.get_rays(0), d.get_seeds()))
        d.close()
    for f in ("O", "D", "intensity", "pixelIdx", "bounces", "inside", "lastSpecular"):
        B.assert_same_bytes(out[0][0][f], out[1][0][f], f"generate {f}")
    assert np.array_equal(out[0][1], out[1][1]), "seeds after generate"


@pytest.mark.parametrize("scene", ["branch", "mixed"])
@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
@pytest.mark.parametrize("accel", [0, 1])
def test_stage_shade_every_bounce_equals_the_second_library(scene, variant, accel):
    """One frame stage by stage on both libraries: after generate and after every shade the exported rays, the shadow records of the
    bounce and the seeds are identical as bytes; so are rt_focus and the accumulator at the end."""
    Wd, Hd = 192, 108
    s, view = scenes.branch_scene() if scene == "branch" else scenes.mixed_scene()
    sa = s.arrays()
    v = dict(DEFAULT, accel=accel, **STAGE_VARIANTS[variant])
    cam = scenes.camera_for(view, Wd, Hd)
    a, b = _pair_of_contexts(sa, Wd, Hd, v)
    fa, fb = a.focus(Wd // 2, Hd // 2, cam), b.focus(Wd // 2, Hd // 2, cam)
    assert fa.tobytes() == fb.tobytes(), ("rt_focus", fa, fb)
    cam["focalLength"] = fa
    for d in (a, b):
        d.set_seeds(seed_stream(0, Wd * Hd))
        d.reset()
        d.stage_begin_frame()
        d.stage_generate(cam)
    shaded = 0
    for bounce in range(W.MAX_BOUNCES):
        for d in (a, b):
            d.stage_extend(bounce)
            d.stage_shade(bounce)
        ra, rb = a.get_rays(bounce + 1), b.get_rays(bounce + 1)
        B.assert_same_bytes(ra, rb, f"{scene} {variant} accel {accel}: rays after shade({bounce})")
        B.assert_same_bytes(a.get_shadow(bounce, bounce), b.get_shadow(bounce, bounce), f"shadow records of bounce {bounce}")
        assert np.array_equal(a.get_seeds(), b.get_seeds()), f"seeds after shade({bounce})"
        shaded += len(ra)
    if v["shading"] == 1:
        for d in (a, b):
            d.stage_connect(0, W.MAX_BOUNCES - 1)
    B.assert_same_bytes(a.read_accum(), b.read_accum(), "accumulator")
    assert shaded > 0 and a.read_accum()[..., :3].sum() > 0      # the comparison was not of empty queues and a black frame
    a.close()
    b.close()


# ---- 5. the default is untouched, side by side -------------------------------------------------------------------------------------
def test_device_without_the_argument_is_ieee():
    d = Device(64, 36)
    assert d.builtins == B.IEEE == W.BUILTINS_IEEE
    d.close()
    d = Device(64, 36, builtins="ieee")
    assert d.builtins == B.IEEE
    d.close()
    d = Device(64, 36, lib="refb")
    assert d.builtins == B.REFERENCE      # what DEFAULT means in that build; explicit modes work there too
    d.close()
    d = Device(64, 36, lib="refb", builtins="ieee")
    assert d.builtins == B.IEEE
    d.close()


@pytest.mark.parametrize("case", ["mixed", "branch", "branch_kajiya_hemi", "two_blas_glass", "fisheye", "config5_small"])
def test_ieee_and_reference_contexts_side_by_side_on_one_scene_copy(case):
    """One process, one device copy of the scene (share_scene), an IEEE and a REFERENCE context with their frames interleaved, on the
    scenes of test_scenes_with_transcendentals_are_bit_exact: the IEEE context's accumulator, seeds and extend counters equal the
    oracle's bit for bit, the REFERENCE context equals the second library, and both run the same kernels and grids."""
    v = dict(DEFAULT)
    Wd, Hd, frames = 192, 108, 3
    if case == "mixed":
        s, view = scenes.mixed_scene()
    elif case.startswith("branch"):
        s, view = scenes.branch_scene()
        if case == "branch_kajiya_hemi":
            v = dict(DEFAULT, shading=0, sampling=0, russian_roulette=False)
    elif case == "two_blas_glass":
        s, view = scenes.two_blas_scene(alpha=0.0, n=16)
    elif case == "fisheye":
        s, view = scenes.branch_scene()
        view = dict(view, type=1, fov=75.0)
    else:
        s, view = scenes.config5_scene(alpha=1.0, decimate=4)
    sa = s.arrays()
    cam = scenes.camera_for(view, Wd, Hd)
    o = oracle_for(sa, Wd, Hd, **v)
    ieee = Device(Wd, Hd, **v)
    ieee.upload(sa)
    refm = Device(Wd, Hd, builtins="reference", **v)
    refm.share_scene(ieee)                        # equal modes are not required: the scene copy does not depend on the arithmetic
    refb = Device(Wd, Hd, lib="refb", **v)
    refb.upload(sa)
    f = o.focus(Wd // 2, Hd // 2, cam)
    assert ieee.focus(Wd // 2, Hd // 2, cam) == f
    cam["focalLength"] = f
    assert (ieee.builtins, refm.builtins) == (B.IEEE, B.REFERENCE)
    assert ieee.kernel_info() == refm.kernel_info()
    ref, seeds, e, c = o.render(cam, frames)
    for d in (ieee, refm, refb):
        d.seed_default()
    for _ in range(frames):                       # interleaved: neither context disturbs the other's queues, seeds or kernels
        ieee.render(cam, 1)
        refm.render(cam, 1)
    refb.render(cam, frames)
    assert_bits(ieee.read_accum(), ref, case + " accumulator of the IEEE context")
    assert np.array_equal(ieee.get_seeds(), seeds)
    B.ctr_equal(ieee.counters(), e, c)
    B.assert_same_bytes(refm.read_accum(), refb.read_accum(), case + " accumulator of the REFERENCE context vs the second library")
    assert np.array_equal(refm.get_seeds(), refb.get_seeds())
    for d in (refm, ieee, refb):
        d.close()


# ---- 6. groups ---------------------------------------------------------------------------------------------------------------------
def test_group_of_reference_lanes_is_the_lane_ordered_sum_of_the_second_library():
    from magr_ray_tracer_amd.renderer import Group
    Wd, Hd, lanes = 192, 108, 4
    s, view = scenes.branch_scene()
    sa = s.arrays()
    cam = scenes.camera_for(view, Wd, Hd)
    g = Group(Wd, Hd, lanes=lanes, builtins="reference", **DEFAULT)
    g.upload(sa)
    assert [d.builtins for d in g.devs] == [B.REFERENCE] * lanes
    g.seed(0)
    cam["focalLength"] = g.focus(Wd // 2, Hd // 2, cam)
    g.render(cam, lanes)                          # four frames: one per lane
    total = g.read_accum()
    lane_acc = [d.read_accum() for d in g.devs]
    g.close()
    exp = None
    for m in range(lanes):
        d = Device(Wd, Hd, lib="refb", **DEFAULT)
        d.upload(sa)
        d.set_seeds(seed_stream(m * Wd * Hd, Wd * Hd))
        d.render(cam, 1)
        acc = d.read_accum()
        d.close()
        B.assert_same_bytes(lane_acc[m], acc, f"lane {m}")
        exp = acc if exp is None else exp + acc
    assert_bits(total, exp, "group accumulator = the second library's renders added in lane order")
    ieee = Group(Wd, Hd, lanes=2, **DEFAULT)
    assert [d.builtins for d in ieee.devs] == [B.IEEE] * 2
    ieee.close()


# ---- 7. math on its own ------------------------------------------------------------------------------------------------------------
def test_math_of_each_mode_on_the_stratified_sets():
    """rt_debug_math_mode(REFERENCE) equals the second library's rt_debug_math on the sets of tests/mathsets.py (normalize4, length4,
    sphere texel, exp, sin, cos), rt_debug_math_mode(IEEE) equals rt_debug_math, and the REFERENCE set has no acos / atan / atan2."""
    v = M.vec4_set()
    sets = [(W.MATH_LENGTH4, M.words(v, W.MATH_LENGTH4)), (W.MATH_NORMALIZE4, M.words(v, W.MATH_NORMALIZE4)), (W.MATH_SPHERE_TEXEL, M.texel_set())]
    x = np.concatenate([M.specials(), M.logu(np.random.default_rng(3), 1 << 20, 0, 254)]).astype(np.float32)
    sets += [(fn, M.bits(x)[:, None]) for fn in (W.MATH_EXP, W.MATH_SIN, W.MATH_COS)]
    differ = 0
    for fn, words in sets:
        rc, want = B.math_mode(None, fn, words, "refb")
        assert rc == 0
        rc, got = B.math_mode(B.REFERENCE, fn, words)
        assert rc == 0, W.device_lib().rt_last_error().decode()
        B.assert_same_bytes(got, want, f"math fn {fn}: REFERENCE mode vs the second library")
        rc, plain = B.math_mode(None, fn, words)
        assert rc == 0
        rc, ieee = B.math_mode(B.IEEE, fn, words)
        assert rc == 0
        B.assert_same_bytes(ieee, plain, f"math fn {fn}: IEEE mode vs rt_debug_math")
        rc, dflt = B.math_mode(0, fn, words)
        assert rc == 0
        B.assert_same_bytes(dflt, plain, f"math fn {fn}: RT_BUILTINS_DEFAULT vs rt_debug_math")
        differ += fn != W.MATH_SPHERE_TEXEL and not B.same_bytes(ieee, got)
    assert differ == len(sets) - 1, "hardware sqrt / rsq and the ocml functions differ from the IEEE sequences somewhere on a million inputs each"
    atan2 = M.words(M.atan2_set(1 << 10), W.MATH_ATAN2)
    for fn, words in ((W.MATH_ACOS, x[:16].view(np.uint32)[:, None]), (W.MATH_ATAN, x[:16].view(np.uint32)[:, None]), (W.MATH_ATAN2, atan2)):
        assert B.math_mode(B.REFERENCE, fn, words)[0] == RT_E_UNSUPPORTED
        assert "REFERENCE" in W.device_lib().rt_last_error().decode()
        rc, ieee = B.math_mode(B.IEEE, fn, words)
        assert rc == 0
        B.assert_same_bytes(ieee, B.math_mode(None, fn, words)[1], f"math fn {fn}: IEEE mode vs rt_debug_math")
    for bad in (3, -1):
        assert B.math_mode(bad, W.MATH_EXP, x[:4].view(np.uint32)[:, None])[0] == RT_E_INVALID
        assert B.sweep_mode(bad, W.MATH_EXP)[0] == RT_E_INVALID


@pytest.mark.parametrize("name,fn", [("exp", W.MATH_EXP), ("sin", W.MATH_SIN), ("cos", W.MATH_COS)])
def test_math_sweep_of_each_mode_over_every_float(name, fn):
    rc, want = B.sweep_mode(None, fn, "refb")
    assert rc == 0
    rc, got = B.sweep_mode(B.REFERENCE, fn)
    assert rc == 0, W.device_lib().rt_last_error().decode()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} of {len(got)} blocks differ between REFERENCE mode and the second library, first block {int(bad[0])}"
    rc, plain = B.sweep_mode(None, fn)
    assert rc == 0
    rc, ieee = B.sweep_mode(B.IEEE, fn)
    assert rc == 0 and np.array_equal(ieee, plain)
    assert not np.array_equal(ieee, got)


def test_math_sweep_refuses_acos_and_atan_in_reference_mode():
    for fn in (W.MATH_ACOS, W.MATH_ATAN):
        L = W.device_lib()
        h = np.zeros(1, np.uint64)
        assert L.rt_debug_math_sweep_mode(B.REFERENCE, fn, 0, 1, h.ctypes.data_as(C.c_void_p)) == RT_E_UNSUPPORTED
        assert L.rt_debug_math_sweep_mode(B.IEEE, fn, 0, 1, h.ctypes.data_as(C.c_void_p)) == 0 and h[0] != 0


# ---- 8. refusals and the C++ caller ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", [3, -1])
def test_unknown_builtins_values_are_refused(word):
    rc, h, msg = B.raw_create(B.raw_config(64, 36, word))
    assert rc == RT_E_INVALID and not h.value, (rc, h.value)
    assert "builtins" in msg and str(word) in msg, msg
    L = W.device_lib()
    g = C.c_void_p()
    words = B.raw_config(64, 36, word)
    assert L.rt_group_create(words.ctypes.data_as(C.c_void_p), 2, C.byref(g)) == RT_E_INVALID and not g.value
    assert "builtins" in L.rt_last_error().decode()


def _cornell_like():
    """The scene examples/headless_tick.cpp builds (cornell_like + its five materials), through the Python Scene API."""
    from magr_ray_tracer_amd.scene import Scene, material
    s = Scene()
    s.AddMaterial("white", material(color=(0.9, 0.9, 0.9)))
    s.AddMaterial("red", material(color=(0.9, 0.15, 0.1)))
    s.AddMaterial("green", material(color=(0.15, 0.8, 0.2)))
    s.AddMaterial("mirror", material(color=(0.9, 0.9, 0.9), specular=0.5))
    s.AddMaterial("light", material(color=(1, 1, 1), light=True, emittance=(40, 40, 40)))
    a = 5.0
    s.AddQuad((-a, 0, -a), (-a, 0, a), (a, 0, a), (a, 0, -a), "white")
    s.AddQuad((-a, 2 * a, -a), (a, 2 * a, -a), (a, 2 * a, a), (-a, 2 * a, a), "white")
    s.AddQuad((-a, 0, -a), (a, 0, -a), (a, 2 * a, -a), (-a, 2 * a, -a), "white")
    s.AddQuad((-a, 0, -a), (-a, 2 * a, -a), (-a, 2 * a, a), (-a, 0, a), "red")
    s.AddQuad((a, 0, -a), (a, 0, a), (a, 2 * a, a), (a, 2 * a, -a), "green")
    f = np.float32
    top = f(2 * a) - f(0.01)
    s.AddQuad((-1.5, top, -1.5), (1.5, top, -1.5), (1.5, top, 1.5), (-1.5, top, 1.5), "light")
    for k in range(2):
        c = np.array([2.0 if k else -2.0, 0.0, -1.0 if k else 1.0], np.float32)
        h = 3.0 if k else 4.5
        p0, p1, p2 = c + np.array([-1.5, 0, -1.0], f), c + np.array([1.5, 0, -1.0], f), c + np.array([0, 0, 1.6], f)
        t = c + np.array([0, h, 0], f)
        m = "mirror" if k else "white"
        s.AddTriangle(p0, p1, t, m)
        s.AddTriangle(p1, p2, t, m)
        s.AddTriangle(p2, p0, t, m)
    s.BuildBLAS(0, 1.0)
    return s


def test_cpp_headless_tick_renders_the_frame_of_the_python_path_in_reference_mode(tmp_path):
    """examples/headless_tick --builtins reference (C++: Renderer::builtins -> RtConfig.builtins) writes the PNG the Python Renderer
    with builtins="reference" writes for the same scene, camera and sample count; --builtins ieee is the default's frame and another."""
    from magr_ray_tracer_amd.renderer import Renderer
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "headless_tick")
    assert os.path.exists(exe), "examples/headless_tick is built by magr_ray_tracer_amd.build.build_examples()"
    Wd, Hd, spp = 320, 180, 8

    def run(out, *extra):
        r = subprocess.run([exe, "--size", str(Wd), str(Hd), "--spp", str(spp), "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return out.read_bytes()

    png_ref = run(tmp_path / "ref.png", "--builtins", "reference")
    png_ieee = run(tmp_path / "ieee.png", "--builtins", "ieee")
    png_dflt = run(tmp_path / "dflt.png")
    assert png_ieee == png_dflt and png_ref != png_ieee
    r = subprocess.run([exe, "--builtins", "bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--builtins" in r.stderr
    py = {}
    for mode in ("reference", None):
        scene = _cornell_like()
        rd = Renderer(scene, Wd, Hd, builtins=mode)
        rd.SetCamera((0, 5, 14), (0, 0, 1), fov=60.0, aperture=0.0)
        rd.Init()
        rd.Tick(spp)
        path = tmp_path / f"py_{mode}.png"
        rd.SaveFrame(path)
        py[mode] = path.read_bytes()
        rd.close()
        scene.close()
    assert py[None] == png_dflt, "the Python Renderer and the C++ example disagree on the default frame: the scenes differ"
    assert py["reference"] == png_ref
