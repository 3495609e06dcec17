"""Stratified input sets and float64 truths for the kernels' math functions (rt_debug_math / orc_math, include/rt355.h).

Used by tests/test_math_cpu.py (the oracle's copies) and tests/test_gpu_math.py (the device's copies, bit for bit with the oracle).
Errors are measured at the float spacing of the exact value: a subnormal result is judged in units of 2^-149, not of FLT_MIN's ulp.
"""
import numpy as np

from magr_ray_tracer_amd import _lib as W

F32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
PI = np.pi

# Bounds the suite asserts, measured exhaustively (one-argument functions, tests/test_math_cpu.py) or on the sets below.  exp / acos /
# atan / atan2 / length4: ulps of the float spacing at the exact value.  sin / cos: absolute, in units of 2^-24 (their relative error
# near a zero of the function is unbounded by construction).  normalize4: absolute per component, units of 2^-24.
# atan2: atan's bound plus the rounding of the quotient y / x.  TEXEL_BOUND: the error of ux and uy, in units of the texture size.
BOUND = {"exp": 1.0, "acos": 1.3, "atan": 2.9, "atan2": 3.4, "sin_abs": 1.31, "cos_abs": 1.32, "length4": 1.5, "normalize4": 3.3}
TEXEL_BOUND = 2.0 ** -22
# Domains of the bounds: beyond them exp returns inf / 0 and sin / cos return 0 (|x| > 8192, Cephes' loss-of-precision cutoff)
EXP_HI, EXP_LO, TRIG_MAX = F32(88.7228394), F32(-103.972076), F32(8192.0)
# every threshold the functions test
THRESHOLDS = [88.7228394, -103.972076, 8192.0, -8192.0, 0.5, -0.5, 1.0, -1.0, 2.414213562373095, 0.4142135623730950, 1.0e-4,
              FLT_MIN, FLT_MAX, 2.0 ** -149]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(b):
    return np.ascontiguousarray(b, np.uint32).view(np.float32)


def canon(b):
    """32-bit float words with every NaN as 0x7fc00000 (x86 and the GPU produce different NaN bits)."""
    b = np.array(b, np.uint32, copy=True)
    b[(b & 0x7fffffff) > 0x7f800000] = 0x7fc00000
    return b


def neighbours(v, k=2):
    """v and its k float neighbours on either side (float32)."""
    v = F32(v)
    out = [v]
    if not np.isfinite(v):
        return out
    lo = hi = v
    with np.errstate(over="ignore"):   # FLT_MAX's upper neighbour is inf
        for _ in range(k):
            lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
            out += [lo, hi]
    return out


def specials():
    """+-0, +-inf, NaN, subnormals, FLT_MIN, FLT_MAX and every threshold with its neighbours, both signs."""
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, FLT_MIN * (1 - 2.0 ** -23)]
    for t in THRESHOLDS:
        v += [float(x) for x in neighbours(t)]
    v = np.array(v, np.float32)
    return np.concatenate([v, -v])


def logu(rng, n, lo_exp=0, hi_exp=254):
    """float32 log-uniform over biased exponents [lo_exp, hi_exp] (0: subnormals), random sign and mantissa."""
    e = rng.integers(lo_exp, hi_exp + 1, n, dtype=np.uint32)
    m = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    s = rng.integers(0, 2, n, dtype=np.uint32)
    return f32(s << 31 | e << 23 | m)


def ulp_at(t):
    """float32 spacing at the exact value(s) t (float64), subnormal spacing below FLT_MIN."""
    t = np.abs(np.asarray(t, np.float64))
    e = np.frexp(np.maximum(t, FLT_MIN))[1]
    return np.ldexp(1.0, e - 24)


def ulp_err(got, t):
    """|got - t| in ulps at t; a NaN, or an infinity where t does not round to one, is an infinite error."""
    got = np.asarray(got, np.float32).astype(np.float64)
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - t) / ulp_at(t)
        rounds_inf = np.isinf(t.astype(np.float32))
        inf_ok = np.isinf(got) & rounds_inf & (np.sign(got) == np.sign(t))
    err = np.where(inf_ok, 0.0, err)
    err[np.isnan(got) | (np.isinf(got) & ~inf_ok) | (rounds_inf & ~inf_ok)] = np.inf
    return err


# ---- stratified sets (seeded; n is the size of each random stratum) --------------------------------------------------------
def atan2_set(n=1 << 20, seed=7):
    """(y, x) pairs, float32 (m, 2)."""
    rng = np.random.default_rng(seed)
    parts = [np.stack([logu(rng, n), logu(rng, n)], 1)]
    sp = specials()
    parts.append(np.stack(np.meshgrid(sp, sp, indexing="ij"), -1).reshape(-1, 2))
    # quotients on atan's reduction thresholds 2.414 / 1 / 0.4142 and their neighbours, over moderate x of either sign
    x = logu(rng, n, 100, 154)
    t = np.array([float(v) for th in (2.414213562373095, 1.0, 0.4142135623730950) for v in neighbours(th, 3)], np.float32)
    q = t[rng.integers(0, len(t), n)] * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)
    parts.append(np.stack([(q * x).astype(np.float32), x], 1))
    # quotients that underflow into / overflow out of the float range, and tiny / subnormal y
    parts.append(np.stack([logu(rng, n // 4, 0, 30), logu(rng, n // 4, 100, 254)], 1))
    parts.append(np.stack([logu(rng, n // 4, 200, 254), logu(rng, n // 4, 0, 60)], 1))
    parts.append(np.stack([logu(rng, n // 4, 0, 0), logu(rng, n // 4, 0, 0)], 1))
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


def unit_normals(rng, n):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32)


TEX_SIZES = np.array([1, 2, 3, 7, 64, 255, 256, 1000, 1024, 2048, 4096, 8192, 16384], np.int32)


def texel_set(n=1 << 20, seed=11):
    """(N.x, N.y, N.z, N.w, texW, texH) rows as 32-bit words (m, 6) uint32; N float32, texW / texH int32."""
    rng = np.random.default_rng(seed)
    N = []
    u = unit_normals(rng, n)
    N.append(np.concatenate([u, np.zeros((n, 1), np.float32)], 1))
    # polluted w lane, and the non-unit normals it leaves behind (|N.y| > 1 near a pole: acos NaN -> row 0)
    p = unit_normals(rng, n // 4) * (1 + rng.uniform(-1e-3, 1e-3, (n // 4, 1))).astype(np.float32)
    N.append(np.concatenate([p, logu(rng, n // 4, 60, 130)[:, None]], 1))
    # the seam: N.z = +-0 with N.x < 0 (atan2 = +-pi: ux = 1 -> x = texW, or ux = 0), and N.z tiny of either sign
    m = n // 8
    sx = -np.abs(unit_normals(rng, m)[:, 0])
    sy = rng.uniform(-1, 1, m).astype(np.float32)
    sz = np.where(rng.random(m) < 0.5, F32(0.0), F32(-0.0)).astype(np.float32)
    tz = logu(rng, m, 0, 110)
    N.append(np.stack([sx, sy, sz, np.zeros(m, np.float32)], 1))
    N.append(np.stack([sx, sy, tz, np.zeros(m, np.float32)], 1))
    # the poles: N.y = +-1 and its neighbours, N.x / N.z tiny or zero
    py = np.array([float(v) for s in (1, -1) for v in neighbours(s, 3)], np.float32)
    py = py[rng.integers(0, len(py), m)]
    N.append(np.stack([logu(rng, m, 0, 120), py, logu(rng, m, 0, 120), np.zeros(m, np.float32)], 1))
    # N.y on acos' thresholds +-0.5
    hy = np.array([float(v) for s in (0.5, -0.5) for v in neighbours(s, 3)], np.float32)
    hu = unit_normals(rng, m)
    N.append(np.stack([hu[:, 0], hy[rng.integers(0, len(hy), m)], hu[:, 2], np.zeros(m, np.float32)], 1))
    # specials in every lane
    sp = specials()
    N.append(sp[rng.integers(0, len(sp), (m, 4))])
    N = np.concatenate(N).astype(np.float32)
    k = len(N)
    tw = TEX_SIZES[rng.integers(0, len(TEX_SIZES), k)]
    th = TEX_SIZES[rng.integers(0, len(TEX_SIZES), k)]
    return np.ascontiguousarray(np.concatenate([N.view(np.uint32), tw.view(np.uint32)[:, None], th.view(np.uint32)[:, None]], 1))


def vec4_set(n=1 << 20, seed=13):
    """4-vectors (m, 4) float32 for normalize4 / length4."""
    rng = np.random.default_rng(seed)
    parts = [logu(rng, 4 * n).reshape(n, 4)]
    # components of one scale: the dot product straddles FLT_MIN (scale ~ 2^-63) and overflow (scale ~ 2^64)
    k = rng.choice(np.concatenate([np.arange(-150, 128), np.arange(-70, -56), np.arange(56, 70)]), n)
    d = rng.standard_normal((n, 4)) * np.ldexp(1.0, k)[:, None]
    d[rng.random((n, 4)) < 0.15] = 0.0
    with np.errstate(over="ignore"):
        parts.append(d.astype(np.float32))
    # unit normals with a polluted w lane
    u = unit_normals(rng, n)
    parts.append(np.concatenate([u, logu(rng, n, 40, 127)[:, None]], 1))
    sp = specials()
    parts.append(sp[rng.integers(0, len(sp), (n // 8, 4))])
    parts.append(np.zeros((2, 4), np.float32) * np.array([[1], [-1]], np.float32))
    v = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(v)


# ---- float64 truths -----------------------------------------------------------------------------------------------------------
def atan2_truth(yx):
    return np.arctan2(yx[:, 0].astype(np.float64), yx[:, 1].astype(np.float64))


def texel_truth(rows):
    """float64 texel column / row (floor of atan2pi / acospi scaled) and each one's distance from the nearest texel edge, in texels;
    NaN where N.y lies outside [-1, 1] or N is not finite."""
    N = f32(rows[:, :4]).astype(np.float64)
    tw = rows[:, 4].view(np.int32).astype(np.float64)
    th = rows[:, 5].view(np.int32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ux = (1 + np.arctan2(N[:, 2], N[:, 0]) / PI) * 0.5
        uy = np.arccos(N[:, 1]) / PI
    sx, sy = ux * tw, uy * th
    return np.floor(sx), np.floor(sy), np.abs(sx - np.round(sx)), np.abs(sy - np.round(sy))


def length4_truth(v):
    return np.sqrt(np.sum(v.astype(np.float64) ** 2, axis=1))


def normalize4_truth(v):
    v = v.astype(np.float64)
    return v / np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))


# ---- error figures of one build's outputs on the sets (same layout as rt_debug_math) ----------------------------------------------
def atan2_errors(yx, out):
    """ulp errors on the finite (y, x) pairs and the indices of the Annex F special cases that fail."""
    got = f32(out[:, 0])
    y, x = yx[:, 0], yx[:, 1]
    fin = np.isfinite(y) & np.isfinite(x)
    err = ulp_err(got[fin], atan2_truth(yx[fin]))
    # infinities (C99 Annex F): atan2 of two infinities and of one infinity is exact up to the rounding of pi/4, pi/2, 3pi/4, pi
    inf = ~fin & ~np.isnan(y) & ~np.isnan(x)
    want = atan2_truth(yx[inf]).astype(np.float32)
    g = got[inf]
    bad = np.flatnonzero(inf)[(bits(g) != bits(want))]
    nan = np.isnan(y) | np.isnan(x)
    bad = np.concatenate([bad, np.flatnonzero(nan & ~np.isnan(got))])
    return err, bad


def texel_check(rows, out, bound_texels):
    """Indices of the rows whose texel index differs from the float64 one although the exact position lies more than
    bound_texels (+ the rounding of the product) from a texel edge; and the fraction of unit-normal rows so decided."""
    tx, ty, dx, dy = texel_truth(rows)
    gx, gy = out[:, 0].view(np.int32), out[:, 1].view(np.int32)
    tw = rows[:, 4].view(np.int32).astype(np.float64)
    th = rows[:, 5].view(np.int32).astype(np.float64)
    N = f32(rows[:, :4])
    ok_n = np.all(np.isfinite(N[:, :3]), 1) & (np.abs(N[:, 1]) <= 1)
    with np.errstate(invalid="ignore"):
        mx = ok_n & (dx > bound_texels * tw + 2.0 ** -23 * tw) & np.isfinite(tx)
        my = ok_n & (dy > bound_texels * th + 2.0 ** -23 * th) & np.isfinite(ty)
    bad = np.flatnonzero((mx & (gx != tx)) | (my & (gy != ty)))
    return bad, float(np.mean(mx[ok_n] & my[ok_n]))


def length4_errors(v, out):
    t = length4_truth(v)
    fin = np.all(np.isfinite(v), 1)
    return ulp_err(f32(out[fin, 0]), t[fin])


def normalize4_errors(v, out):
    """max |component error| * 2^24 per finite, nonzero 4-vector."""
    fin = np.all(np.isfinite(v), 1) & np.any(v != 0, 1)
    t = normalize4_truth(v[fin])
    got = f32(out[fin]).reshape(-1, 4).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.max(np.abs(got - t), 1) * 2.0 ** 24
    e[np.isnan(e)] = np.inf
    return e


def seam_and_pole_rows():
    """(N, texW, texH) -> the reference's (x, y) at the texture seam and the poles, kept as they are."""
    W_, H_ = 256, 128
    cases = [((-1.0, 0.0, 0.0), (W_, H_ // 2)),       # atan2(+0, -1) = pi: ux = 1 -> x = texW
             ((-1.0, 0.0, -0.0), (0, H_ // 2)),       # atan2(-0, -1) = -pi: ux = 0
             ((-0.6, 0.8, 0.0), (W_, 26)),
             ((0.0, -1.0, 0.0), (W_ // 2, H_)),       # acos(-1) = pi: uy = 1 -> y = texH
             ((0.0, 1.0, 0.0), (W_ // 2, 0)),
             ((-0.0, -1.0, -0.0), (0, H_)),           # atan2(-0, -0) = -pi
             ((1.0, 0.0, -0.0), (W_ // 2, H_ // 2)),  # atan2(-0, 1) = -0: ux = 0.5
             ((0.0, 1.0000001, 0.0), (W_ // 2, 0))]   # |N.y| > 1: acos NaN -> row 0
    rows = np.zeros((len(cases), 6), np.uint32)
    for i, (n, _) in enumerate(cases):
        rows[i, :3] = bits(np.array(n, np.float32))
        rows[i, 4:] = np.array([W_, H_], np.int32).view(np.uint32)
    return rows, np.array([xy for _, xy in cases], np.int32)


def words(a, fn):
    """Input of rt_debug_math / orc_math for a set: contiguous 32-bit words."""
    wi, _ = W.MATH_WORDS[fn]
    return np.ascontiguousarray(np.asarray(a).view(np.uint32).reshape(-1, wi))
