"""The oracle's math functions (oracle/oracle.c orc_expf ... normalize4, the same sequences the kernels evaluate) against float64.

The one-argument functions are swept exhaustively over their domains; atan2, the sphere texel index, normalize4 and length4 over the
stratified sets of tests/mathsets.py.  tests/test_gpu_math.py holds the device's copies to the oracle bit for bit on the same inputs.
"""
import math

import numpy as np
import pytest

import mathsets as M
from magr_ray_tracer_amd import _lib as W
from oracle import oracle_py as O

F32 = np.float32
INF = F32(np.inf)


def one(fn, x):
    return M.f32(O.math(fn, M.bits(np.atleast_1d(np.asarray(x, np.float32)))[:, None])[:, 0])


@pytest.mark.parametrize("name,fn,lo,hi,absolute,bound", [
    ("exp", W.MATH_EXP, M.EXP_LO, M.EXP_HI, False, M.BOUND["exp"]),
    ("sin", W.MATH_SIN, -M.TRIG_MAX, M.TRIG_MAX, True, M.BOUND["sin_abs"]),
    ("cos", W.MATH_COS, -M.TRIG_MAX, M.TRIG_MAX, True, M.BOUND["cos_abs"]),
    ("acos", W.MATH_ACOS, F32(-1), F32(1), False, M.BOUND["acos"]),
    ("atan", W.MATH_ATAN, -INF, INF, False, M.BOUND["atan"]),
])
def test_exhaustive_error_against_float64(name, fn, lo, hi, absolute, bound):
    r = O.math_error(fn, lo, hi, absolute, bound)
    unit = "x 2^-24 absolute" if absolute else "ulp"
    print(f"\n{name} over [{lo}, {hi}]: {r['count']} floats, max error {r['max_err']:.4f} {unit} at {r['arg']!r}")
    assert r["count"] > 2_000_000_000
    assert r["above"] == 0, f"{name}: {r['above']} inputs above {bound} {unit}; worst {r['max_err']} at {r['arg']!r}"


def test_error_metric_uses_the_spacing_at_the_exact_value():
    # a correctly rounded subnormal is within half an ulp of the subnormal spacing, not 10^6 ulp of FLT_MIN's
    t = np.array([3.4 * 2.0 ** -149, 1.5 * 2.0 ** -140, 1.0 + 2.0 ** -25])
    got = t.astype(np.float32)
    assert np.all(M.ulp_err(got, t) <= 0.5)
    assert M.ulp_err(np.float32(2.0 ** -149), np.array([2.0 ** -148]))[0] == 1.0
    assert M.ulp_err(np.float32(np.inf), np.array([3.5e38]))[0] == 0.0      # rounds to inf
    assert M.ulp_err(np.float32(np.inf), np.array([3.0e38]))[0] == np.inf


def _spread(step=1021):
    """every step-th float32 bit pattern plus every threshold's neighbourhood"""
    b = np.arange(0, 1 << 32, step, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([M.f32(b), M.specials()])


def test_outside_the_domains():
    x = _spread()
    with np.errstate(invalid="ignore"):
        e = one(W.MATH_EXP, x)
        assert np.all(e[x > M.EXP_HI] == np.inf)
        lo = e[x < M.EXP_LO]
        assert np.all((lo == 0) & ~np.signbit(lo))
        far = np.isfinite(x) & (np.abs(x) > M.TRIG_MAX)
        for fn in (W.MATH_SIN, W.MATH_COS):                  # Cephes: total loss of precision -> 0
            r = one(fn, x)
            assert np.all(M.bits(r[far]) == 0)
        a = one(W.MATH_ACOS, x)
        assert np.all(np.isnan(a[np.abs(x) > 1]))
    nan = np.isnan(x)
    assert nan.sum() > 1000
    for fn in (W.MATH_EXP, W.MATH_SIN, W.MATH_COS, W.MATH_ACOS, W.MATH_ATAN):
        assert np.all(np.isnan(one(fn, x[nan])))


def _exact(v):
    return M.bits(np.float32(v))[()]


def test_annex_f_special_values():
    pi, hpi = math.pi, math.pi / 2
    cases = [  # (fn, x, exact value): rounded to float32 and compared bit for bit (a list: 0.0 and -0.0 are one dict key)
        (W.MATH_EXP, 0.0, 1.0), (W.MATH_EXP, -0.0, 1.0), (W.MATH_EXP, -np.inf, 0.0), (W.MATH_EXP, np.inf, np.inf),
        (W.MATH_SIN, 0.0, 0.0), (W.MATH_SIN, -0.0, -0.0), (W.MATH_COS, 0.0, 1.0), (W.MATH_COS, -0.0, 1.0),
        (W.MATH_ATAN, 0.0, 0.0), (W.MATH_ATAN, -0.0, -0.0), (W.MATH_ATAN, np.inf, hpi), (W.MATH_ATAN, -np.inf, -hpi),
        (W.MATH_ACOS, 1.0, 0.0), (W.MATH_ACOS, -1.0, pi), (W.MATH_ACOS, 0.0, hpi), (W.MATH_ACOS, -0.0, hpi),
    ]
    for fn, x, want in cases:
        got = one(fn, x)[0]
        assert M.bits(got) == _exact(want), (fn, x, got, want)
    for fn in (W.MATH_SIN, W.MATH_COS):
        assert np.all(np.isnan(one(fn, [np.inf, -np.inf]))), "sin / cos of an infinity is NaN"
    # atan2 (C99 F.9.1.4): every listed (y, x) class against the float32 rounding of its exact value
    fin = [1e-45, 1e-30, 0.7, 3.0, 1e30, 3.4e38]
    pairs = []
    for s in (1.0, -1.0):
        pairs += [(s * 0.0, 0.0, s * 0.0), (s * 0.0, -0.0, s * pi), (s * np.inf, np.inf, s * pi / 4), (s * np.inf, -np.inf, s * 3 * pi / 4)]
        for v in fin:
            pairs += [(s * 0.0, -v, s * pi), (s * 0.0, v, s * 0.0), (-v, s * 0.0, -hpi), (v, s * 0.0, hpi),
                      (s * v, -np.inf, s * pi), (s * v, np.inf, s * 0.0), (s * np.inf, v, s * hpi), (s * np.inf, -v, s * hpi)]
    yx = np.array([(y, x) for y, x, _ in pairs], np.float32)
    got = M.f32(O.math(W.MATH_ATAN2, M.words(yx, W.MATH_ATAN2))[:, 0])
    want = np.array([w for _, _, w in pairs], np.float32)
    bad = np.flatnonzero(M.bits(got) != M.bits(want))
    assert bad.size == 0, [(tuple(yx[i]), got[i], want[i]) for i in bad[:8]]
    nan = np.array([(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.nan), (0.0, np.nan)], np.float32)
    assert np.all(np.isnan(M.f32(O.math(W.MATH_ATAN2, M.words(nan, W.MATH_ATAN2))[:, 0])))


def test_f2i_converts_as_the_gpu():
    x = np.concatenate([_spread(4099), np.array([2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, 0.99999994, -0.99999994])
                        .astype(np.float32)])
    got = O.math(W.MATH_F2I, M.bits(x)[:, None])[:, 0].view(np.int32)
    with np.errstate(invalid="ignore"):
        want = np.where(np.isnan(x), 0, np.clip(np.trunc(x.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    assert np.array_equal(got.astype(np.int64), want)


def test_atan2_on_the_stratified_set():
    yx = M.atan2_set()
    err, bad = M.atan2_errors(yx, O.math(W.MATH_ATAN2, M.words(yx, W.MATH_ATAN2)))
    fin = np.flatnonzero(np.all(np.isfinite(yx), 1))
    i = int(np.argmax(err))
    print(f"\natan2: {len(yx)} pairs, max {err[i]:.4f} ulp at (y, x) = {tuple(yx[fin[i]])}")
    assert bad.size == 0, yx[bad[:8]]
    assert err.max() <= M.BOUND["atan2"]


def test_length4_and_normalize4_on_the_stratified_set():
    v = M.vec4_set()
    el = M.length4_errors(v, O.math(W.MATH_LENGTH4, M.words(v, W.MATH_LENGTH4)))
    en = M.normalize4_errors(v, O.math(W.MATH_NORMALIZE4, M.words(v, W.MATH_NORMALIZE4)))
    print(f"\nlength4: max {el.max():.4f} ulp; normalize4: max {en.max():.4f} x 2^-24 per component ({len(v)} vectors)")
    assert el.max() <= M.BOUND["length4"]
    assert en.max() <= M.BOUND["normalize4"]
    # the zero vector stays as it is, signs included
    z = np.array([[0.0, -0.0, 0.0, -0.0]], np.float32)
    assert np.array_equal(O.math(W.MATH_NORMALIZE4, M.words(z, W.MATH_NORMALIZE4)), M.bits(z))


def test_sphere_texel_index_against_float64():
    rows = M.texel_set()
    out = O.math(W.MATH_SPHERE_TEXEL, rows)
    bad, decided = M.texel_check(rows, out, M.TEXEL_BOUND)
    print(f"\ntexel index: {len(rows)} rows, {decided:.3f} of the unit normals decided, {bad.size} wrong")
    assert bad.size == 0, [(M.f32(rows[i, :4]), rows[i, 4:].view(np.int32), out[i].view(np.int32)) for i in bad[:8]]
    assert decided > 0.75


def test_sphere_texel_seam_and_poles():
    rows, want = M.seam_and_pole_rows()
    got = O.math(W.MATH_SPHERE_TEXEL, rows).view(np.int32)
    assert np.array_equal(got, want), np.concatenate([got, want], 1)


def test_device_math_fails_loudly_without_gpu():
    from conftest import has_gpu
    if has_gpu():
        pytest.skip("GPU present")
    import ctypes as C
    L = W.device_lib()
    x = np.zeros(4, np.uint32)
    h = np.zeros(1, np.uint64)
    assert L.rt_debug_math(W.MATH_EXP, x.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), 4) == -2
    assert b"no HIP device" in L.rt_last_error()
    assert L.rt_debug_math_sweep(W.MATH_EXP, 0, 1, h.ctypes.data_as(C.c_void_p)) == -2
    assert b"no HIP device" in L.rt_last_error()
