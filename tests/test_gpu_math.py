"""The kernels' math functions on the GPU (rt_debug_math): bit for bit with the oracle, and within the bounds of tests/mathsets.py
against float64.

(a) every one-argument function over all 2^32 inputs, compared through block hashes; (b) atan2, the sphere texel index, normalize4
and length4 on the stratified sets; (c) the texel index against float64 atan2pi / acospi, seam and poles pinned; (d) the same sets
through librt355_refb.so (the reference's ocml builtins), whose figures are printed.
"""
import ctypes as C

import numpy as np
import pytest

import mathsets as M
from magr_ray_tracer_amd import _lib as W
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

RT_E_UNSUPPORTED = -4
ONE_ARG = {"exp": W.MATH_EXP, "sin": W.MATH_SIN, "cos": W.MATH_COS, "acos": W.MATH_ACOS, "atan": W.MATH_ATAN, "f2i": W.MATH_F2I}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def dev_math(fn, words, variant=None):
    L = W.device_lib(variant)
    wi, wo = W.MATH_WORDS[fn]
    a = np.ascontiguousarray(words, np.uint32).reshape(-1, wi)
    out = np.zeros((len(a), wo), np.uint32)
    rc = L.rt_debug_math(fn, _p(a), _p(out), len(a))
    assert rc == 0, L.rt_last_error().decode()
    return out


def dev_sweep(fn, variant=None):
    L = W.device_lib(variant)
    h = np.zeros(1 << (32 - W.MATH_SWEEP_BLOCK_BITS), np.uint64)
    rc = L.rt_debug_math_sweep(fn, 0, len(h), _p(h))
    assert rc == 0, L.rt_last_error().decode()
    return h


def _first_difference(fn, block):
    b = (np.arange(1 << W.MATH_SWEEP_BLOCK_BITS, dtype=np.uint64) + (block << W.MATH_SWEEP_BLOCK_BITS)).astype(np.uint32)[:, None]
    g, o = dev_math(fn, b)[:, 0], O.math(fn, b)[:, 0]
    if fn != W.MATH_F2I:
        g, o = M.canon(g), M.canon(o)
    i = np.flatnonzero(g != o)
    if not i.size:
        return f"block {block}: hashes differ but no output does"
    x = b[i[0], 0]
    return (f"block {block}: {i.size} inputs differ, first x = {M.f32(x)!r} (0x{x:08x}): gpu 0x{g[i[0]]:08x} "
            f"({M.f32(g[i[0]])!r}), oracle 0x{o[i[0]]:08x} ({M.f32(o[i[0]])!r})")


@pytest.mark.parametrize("name", list(ONE_ARG))
def test_one_argument_functions_match_the_oracle_on_every_float(name):
    fn = ONE_ARG[name]
    g, o = dev_sweep(fn), O.math_sweep(fn)
    bad = np.flatnonzero(g != o)
    assert bad.size == 0, f"{name}: {bad.size} of {len(g)} blocks differ; " + "; ".join(_first_difference(fn, int(k)) for k in bad[:3])


def _assert_same(fn, inp, got, what):
    want = O.math(fn, inp)
    if fn not in (W.MATH_SPHERE_TEXEL,):
        got, want = M.canon(got), M.canon(want)
    bad = np.flatnonzero(np.any(got != want, 1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(inp)} differ from the oracle; first input words "
                           f"{[hex(v) for v in inp[bad[0]]]} ({M.f32(inp[bad[0]])}): gpu {got[bad[0]]}, oracle {want[bad[0]]}")


def test_atan2_matches_the_oracle_and_float64():
    yx = M.atan2_set()
    inp = M.words(yx, W.MATH_ATAN2)
    got = dev_math(W.MATH_ATAN2, inp)
    _assert_same(W.MATH_ATAN2, inp, got, "atan2")
    err, bad = M.atan2_errors(yx, got)
    print(f"\natan2 (gpu): {len(yx)} pairs, max {err.max():.4f} ulp")
    assert bad.size == 0 and err.max() <= M.BOUND["atan2"]


def test_length4_and_normalize4_match_the_oracle_and_float64():
    v = M.vec4_set()
    inp = M.words(v, W.MATH_LENGTH4)
    gl, gn = dev_math(W.MATH_LENGTH4, inp), dev_math(W.MATH_NORMALIZE4, inp)
    _assert_same(W.MATH_LENGTH4, inp, gl, "length4")
    _assert_same(W.MATH_NORMALIZE4, inp, gn, "normalize4")
    el, en = M.length4_errors(v, gl), M.normalize4_errors(v, gn)
    print(f"\nlength4 (gpu): max {el.max():.4f} ulp; normalize4: max {en.max():.4f} x 2^-24")
    assert el.max() <= M.BOUND["length4"] and en.max() <= M.BOUND["normalize4"]


def test_one_argument_functions_on_the_thresholds():
    # the thresholds themselves, through the array entry as well as the sweep
    x = M.bits(M.specials())[:, None]
    for name, fn in ONE_ARG.items():
        _assert_same(fn, x, dev_math(fn, x), name)


def test_sphere_texel_index_matches_the_oracle_and_float64():
    rows = M.texel_set()
    got = dev_math(W.MATH_SPHERE_TEXEL, rows)
    _assert_same(W.MATH_SPHERE_TEXEL, rows, got, "sphere texel index")
    bad, decided = M.texel_check(rows, got, M.TEXEL_BOUND)
    print(f"\ntexel index (gpu): {decided:.3f} of the unit normals decided, {bad.size} wrong")
    assert bad.size == 0 and decided > 0.75
    srows, want = M.seam_and_pole_rows()
    assert np.array_equal(dev_math(W.MATH_SPHERE_TEXEL, srows).view(np.int32), want)


def test_refb_build_on_the_same_sets():
    """librt355_refb.so evaluates ocml's exp / sin / cos / acospi / atan2pi / rsqrt / hardware sqrt.  Its figures are printed; what
    is asserted is what this test measures: texel indices against float64 on the normals decided with a looser margin, and finite
    length4 / normalize4 results for finite nonzero vectors."""
    L = W.device_lib("refb")
    one = np.zeros(1, np.uint32)
    for fn in (W.MATH_ACOS, W.MATH_ATAN, W.MATH_ATAN2):
        assert L.rt_debug_math(fn, _p(np.zeros(2, np.uint32)), _p(one), 1) == RT_E_UNSUPPORTED
    v = M.vec4_set()
    inp = M.words(v, W.MATH_LENGTH4)
    el = M.length4_errors(v, dev_math(W.MATH_LENGTH4, inp, "refb"))
    en = M.normalize4_errors(v, dev_math(W.MATH_NORMALIZE4, inp, "refb"))
    rows = M.texel_set()
    bad, decided = M.texel_check(rows, dev_math(W.MATH_SPHERE_TEXEL, rows, "refb"), 2.0 ** -20)
    for name, fn in (("exp", W.MATH_EXP), ("sin", W.MATH_SIN), ("cos", W.MATH_COS)):
        x = M.logu(np.random.default_rng(3), 1 << 20, 0, 133)
        x = x[np.abs(x) <= (M.EXP_HI if fn == W.MATH_EXP else M.TRIG_MAX)]
        g = M.f32(dev_math(fn, M.bits(x)[:, None], "refb")[:, 0])
        t = {W.MATH_EXP: np.exp, W.MATH_SIN: np.sin, W.MATH_COS: np.cos}[fn](x.astype(np.float64))
        e = M.ulp_err(g, t) if fn == W.MATH_EXP else np.abs(g - t) * 2.0 ** 24
        print(f"\nrefb {name}: max {e.max():.4f} {'ulp' if fn == W.MATH_EXP else 'x 2^-24'} on {len(x)} inputs")
    print(f"refb length4: max {el.max():.4f} ulp; normalize4: max {en.max():.4f} x 2^-24; texel: {bad.size} wrong, {decided:.3f} decided")
    assert np.all(np.isfinite(el)) and np.all(np.isfinite(en))
    assert bad.size == 0 and decided > 0.75
