"""Shared helpers of the parity tests."""
import os

import numpy as np

from magr_ray_tracer_amd import scenes

DEFAULT = dict(shading=1, sampling=1, accel=0, russian_roulette=True, filter_fireflies=True)


def bits_equal(a, b):
    """Bit-exact for floats except that +0 == -0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))
    return bool(np.array_equal(a, b))


def mismatch(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype == np.float32:
        bad = (a.view(np.uint32) != b.view(np.uint32)) & ~((a == 0) & (b == 0))
    else:
        bad = a != b
    return int(bad.sum())


def assert_bits(a, b, what):
    n = mismatch(a, b)
    assert n == 0, f"{what}: {n}/{np.asarray(a).size} elements differ"


def assert_concurrency(measured, lanes):
    """`measured` = how many of `lanes` HIP streams the library found running side by side.  HIP maps a process's streams onto
    GPU_MAX_HW_QUEUES hardware queues (default 4, the null stream included): with one queue per lane beside the null stream every lane
    must run concurrently; with fewer the library can only report fewer, but never none and never more than `lanes`."""
    queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    assert 1 <= measured <= lanes, (measured, lanes)
    if queues >= lanes + 1:
        assert measured == lanes, f"{measured} of {lanes} streams concurrent on {queues} hardware queues"


def max_rel(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))) if a.size else 0.0


def oracle_for(sa, W, H, **variant):
    """The oracle a device context of this configuration is held to, connect's node and triangle counts included.  A `variant` is what
    Device takes; of it the oracle reads the reference's settings and `accel`.  Over a BVH2 the kernels' connect walks a BLAS in its
    own any-hit order (rt355_kernels.h slab_any), which the oracle restates as connect_order LATER_EXIT; over a BVH4 it keeps the
    reference's slot order.  Nothing but connect's node_visits and prim_tests depends on the choice (tests/test_anyhit_cpu.py) - for
    rays whose primitive tests float32 can compute: the verdict of a ray with a direction component near FLT_MAX may depend on it, and
    does at tmax = +inf (tests/test_edge_rays_cpu.py pins those rays)."""
    from oracle.oracle_py import LATER_EXIT, REFERENCE_ORDER, Oracle
    v = {k: x for k, x in variant.items() if k in ("shading", "sampling", "accel", "russian_roulette", "filter_fireflies", "max_bounces", "schedule")}
    return Oracle(sa, W, H, connect_order=REFERENCE_ORDER if v.get("accel", 0) == 1 else LATER_EXIT, **v)


def build(scene_fn, W, H):
    s, view = scene_fn()
    sa = s.arrays()
    cam = scenes.camera_for(view, W, H)
    return s, sa, cam


# ---- whole frames of the reference's own kernels (schedule S0) against the oracle ------------------------------------------
REF_W, REF_H = 1280, 720     # the reference's compile-time frame (src/constants.h:3-4)
EXT_EXACT = ("pixelIdx", "primIdx", "bounces", "inside", "lastSpecular")


def oracle_frame_s0(o, cam, y0, y1, bounces=7):
    """The oracle (schedule S0) driven stage by stage through Renderer::RayTrace() (reference src/renderer.cpp:64-94) over rows
    [y0, y1): same capture layout as tests/ref_gpu.py RefGPU.frame_s0."""
    from oracle.oracle_py import seed_stream
    Wd = o.width
    first, n = y0 * Wd, (y1 - y0) * Wd
    seeds = seed_stream(first, n)
    rays = o.generate(cam, first, n, seeds)
    cap = dict(gen=rays.copy(), gen_seeds=seeds.copy(), ext=[], n_in=[], n_out=[], n_shadow=[], seed0=[], shadow=[])
    acc = np.zeros((o.height * Wd, 4), np.float32)
    nee, rr = int(o.cfg["shading"]) == 1, bool(o.cfg["russian_roulette"])
    pend = []
    for b in range(bounces):
        o.extend(rays)
        cap["n_in"].append(len(rays))
        cap["ext"].append(rays.copy())
        out, sh = o.shade(rays, acc, seeds)
        pend.append(sh)
        cap["n_out"].append(len(out))
        cap["seed0"].append(int(seeds[0]))
        if not rr and nee:
            cap["n_shadow"].append(len(sh))
            cap["shadow"].append(sh.copy())
            o.connect(sh, acc)
            pend = []
        else:
            cap["n_shadow"].append(sum(len(p) for p in pend))
        rays = out
    cap["last_out"] = rays.copy()
    if rr:
        allsh = np.concatenate(pend) if pend else np.zeros(0, dtype=out.dtype)
        cap["shadow"] = [allsh]
        if nee:
            o.connect(allsh, acc)
    cap["accum"] = acc[first:first + n].copy()
    cap["first_pixel"] = first
    return cap


def branch_counts(cap, sa):
    """How often the reference's frame went through each shading branch (from its own captured rays)."""
    c = dict(light_spec=0, light_nospec=0, light_spec_later=0, tex_tri=0, tex_sphere=0, inside=0, inside_dielectric=0, tir=0,
             sphere_light_shadow=0, tri_light_shadow=0, last_bounce=0)
    for rays in cap["ext"]:
        hit = rays["primIdx"] != -1
        p = sa.prims[np.where(hit, rays["primIdx"], 0)]
        m = sa.mats[p["matIdx"]]
        light = hit & (m["isLight"] != 0)
        c["light_spec"] += int((light & (rays["lastSpecular"] != 0)).sum())
        c["light_spec_later"] += int((light & (rays["lastSpecular"] != 0) & (rays["bounces"] > 0)).sum())
        c["light_nospec"] += int((light & (rays["lastSpecular"] == 0)).sum())
        tex = hit & (m["texIdx"] != -1) & ~light
        c["tex_tri"] += int((tex & (p["objType"] == 2)).sum())
        c["tex_sphere"] += int((tex & (p["objType"] == 0)).sum())
        c["inside"] += int((rays["inside"] != 0).sum())
        ins = hit & (rays["inside"] != 0) & (m["isDielectric"] != 0)
        c["inside_dielectric"] += int(ins.sum())
        if ins.any():
            ci = -(rays["N"][ins].astype(np.float64) * rays["D"][ins]).sum(1)
            fr = (m["n2"][ins] / m["n1"][ins]).astype(np.float64)
            c["tir"] += int((1 - fr * fr * (1 - ci * ci) < 0).sum())
    for sh in cap["shadow"] or []:
        if len(sh):
            t = sa.prims["objType"][sh["lightIdx"]]
            c["sphere_light_shadow"] += int((t == 0).sum())
            c["tri_light_shadow"] += int((t == 2).sum())
    c["last_bounce"] = int((cap["last_out"]["bounces"] == 7).sum()) if len(cap["last_out"]) else 0
    return c


def _is_sphere_hit(rays, sa):
    hit = rays["primIdx"] != -1
    return hit & (sa.prims["objType"][np.where(hit, rays["primIdx"], 0)] == 0)


def teacher_forced_s0(o, cap, sa, what="", full_rays=True, collect=None):
    """The reference's own frame (cap, from RefGPU.frame_s0 or a refframe_*.npz fixture) against the oracle, launch by launch: at
    every bounce the oracle gets the REFERENCE's rays and RNG state and must reproduce what the reference's kernels did with them -
    extend bit for bit; shade's queue lengths, order, pixel / flag words and the RNG state exactly and its floats to the few ulp
    of the library normalize()/length(); the accumulator, summed over all launches, to 1e-4 relative per pixel.
    (Free running, the same few ulp flip a handful of knife-edge decisions per 10^4 rays - a reflected ray re-hitting its own
    sphere at t ~ 1e-6, an origin one ulp on either side of a wall - and since slots index the RNG streams, one flipped path
    renumbers every later ray; compare_frames_s0 covers bands where no such flip occurs.)"""
    nb = len(cap["n_in"])
    nee, rr = int(o.cfg["shading"]) == 1, bool(o.cfg["russian_roulette"])
    acc = np.zeros((o.height * o.width, 4), np.float32)
    stats = dict(bounces=nb, rays=int(sum(cap["n_in"])), D_rel=0.0, O_abs=0.0, intensity_rel=0.0, shadow_rel=0.0)
    pend = []
    for b in range(nb):
        ref = cap["ext"][b]
        assert len(ref) == cap["n_in"][b]
        rays = ref.copy()
        rays["t"], rays["primIdx"] = 1e30, -1          # as initRay left them (ray.cl:4-19); u, v keep their stale values
        if full_rays:
            rays["I"], rays["N"] = 0, 0
        o.extend(rays)
        for f in ("t", "primIdx", "u", "v") + (("I", "N") if full_rays else ()):
            assert_bits(rays[f], ref[f], f"{what} bounce {b} extend {f}")
        if collect is not None:
            collect.append(rays.copy())                # the oracle's own extend output (with I and N)
        seed = np.array([cap["gen_seeds"][0] if b == 0 else cap["seed0"][b - 1]], np.uint32)
        out, sh = o.shade(rays, acc, seed)
        nxt = cap["ext"][b + 1] if b + 1 < nb else cap["last_out"]
        assert len(out) == cap["n_out"][b] == len(nxt), f"{what} bounce {b}: {len(out)} extension rays, reference {cap['n_out'][b]}"
        assert int(seed[0]) == cap["seed0"][b], f"{what} bounce {b}: RNG state after shade"
        for f in ("pixelIdx", "bounces", "inside", "lastSpecular"):
            assert np.array_equal(out[f], nxt[f]), f"{what} bounce {b}: extension rays differ in {f}"
        if len(out) and "D" in nxt.dtype.names:
            stats["D_rel"] = max(stats["D_rel"], float((np.abs(out["D"] - nxt["D"]).max(1) / np.abs(nxt["D"]).max(1)).max()))
            stats["O_abs"] = max(stats["O_abs"], float(np.abs(out["O"] - nxt["O"]).max()))
            irel = (np.abs(out["intensity"].astype(np.float64) - nxt["intensity"]) / np.maximum(np.abs(nxt["intensity"]), 1e-6)).max(1)
            # a sphere-texture lookup is a knife edge too: acos / atan2 a few ulp apart (device library there, Cephes here) land on the
            # neighbouring texel once in ~10^5 lookups and the child ray's throughput changes with the albedo
            stats["texel_flips"] = stats.get("texel_flips", 0) + int((irel > 1e-3).sum())
            stats["intensity_rel"] = max(stats["intensity_rel"], float(irel[irel <= 1e-3].max()) if (irel <= 1e-3).any() else 0.0)
        pend.append(sh)
        if not rr and nee:
            rsh = cap["shadow"][b]
            _cmp_shadow(sh, rsh, stats, f"{what} bounce {b}")
            assert cap["n_shadow"][b] == len(sh)
            o.connect(rsh if "I" in rsh.dtype.names else sh, acc)
            pend = []
        else:
            assert cap["n_shadow"][b] == sum(len(p) for p in pend), f"{what} bounce {b}: shadow rays so far"
    if rr and nee:
        allsh = np.concatenate(pend)
        rsh = cap["shadow"][0]
        _cmp_shadow(allsh, rsh, stats, what)
        o.connect(rsh if "I" in rsh.dtype.names else allsh, acc)
    first = int(cap["first_pixel"])
    a, r = acc[first:first + len(cap["accum"])].astype(np.float64), cap["accum"].astype(np.float64)
    assert not acc[:first].any() and not acc[first + len(cap["accum"]):].any()
    rel = np.abs(a - r) / np.maximum(np.abs(r), 1e-3)
    stats["accum_max_rel"] = float(rel.max())
    stats["accum_pixels_over_1e-6"] = int((rel.max(axis=1) > 1e-6).sum())
    # directions and origins: a few ulp.  Throughput and the shadow ray's dotNL / Nl.L carry dot(N, sampled direction), which
    # cancels for grazing samples: its few-ulp ABSOLUTE error is a 1e-4 relative one on a throughput that is itself ~1e-3 of the
    # parent's - invisible in the accumulator (measured 2e-7), which is what the north star's 1e-4 is about.
    assert stats["D_rel"] < 2e-6 and stats["O_abs"] < 2e-5 and stats["shadow_rel"] < 1e-3 and stats.get("texel_flips", 0) <= 2, stats
    assert stats["accum_max_rel"] < 1e-4, stats
    return stats


def _cmp_shadow(sh, rsh, stats, what):
    assert len(sh) == len(rsh), f"{what}: {len(sh)} shadow rays, reference {len(rsh)}"
    if len(sh):
        for f in ("lightIdx", "pixelIdx"):
            assert np.array_equal(sh[f], rsh[f]), f"{what}: shadow rays differ in {f}"
        if "I" in rsh.dtype.names:
            for f in ("I", "L", "Nl", "intensity", "BRDF", "dotNL", "dist"):
                stats["shadow_rel"] = max(stats["shadow_rel"], max_rel(sh[f], rsh[f], 1e-3))


def compare_frames_s0(ref, orc, what="", max_bad_pixels=0.01):
    """Reference kernels vs oracle, FREE RUNNING over the whole frame (nothing fed back).  Queue lengths, RNG state, pixel /
    primitive indices and flags must be IDENTICAL at every bounce.  Floats: the two sides differ by the few ulp of the library
    normalize()/length() at bounce 0 and path tracing amplifies that along knife-edge paths (a grazing
    sphere hit turns 1e-7 in D into 1e-4 in the reflected direction, and so on for seven bounces), so `t` and the throughput of a
    few rays end up percent apart although every discrete decision is the same.  The accumulator is therefore held to 1e-4
    relative on all but `max_bad_pixels` of the pixels, and the maxima are returned (and printed by the tests)."""
    stats = dict(bounces=len(ref["n_in"]), rays=int(sum(ref["n_in"])), shadow_rays=int(sum(len(s) for s in ref["shadow"] or [])))
    assert_bits(orc["gen"]["O"], ref["gen"]["O"], what + " generate O")
    assert np.array_equal(orc["gen_seeds"], ref["gen_seeds"]), what + " seeds after generate"
    stats["gen_D_abs"] = float(np.abs(orc["gen"]["D"] - ref["gen"]["D"]).max())
    assert stats["gen_D_abs"] < 1e-6
    t_rel = i_rel = 0.0
    for b in range(len(ref["n_in"])):
        for k in ("n_in", "n_out", "n_shadow", "seed0"):
            assert orc[k][b] == ref[k][b], f"{what} bounce {b}: {k} {orc[k][b]} != {ref[k][b]} (reference)"
        r, o = ref["ext"][b], orc["ext"][b]
        for f in EXT_EXACT:
            bad = int((r[f] != o[f]).sum())
            assert bad == 0, f"{what} bounce {b}: {bad}/{len(r)} rays differ in {f}"
        hit = r["primIdx"] != -1
        if hit.any():
            t_rel = max(t_rel, max_rel(o["t"][hit], r["t"][hit], 1e-3))
        i_rel = max(i_rel, max_rel(o["intensity"], r["intensity"], 1e-4))
    stats["t_rel"], stats["intensity_rel"] = t_rel, i_rel
    for f in ("pixelIdx", "bounces", "inside", "lastSpecular"):
        assert np.array_equal(orc["last_out"][f], ref["last_out"][f]), what + " rays left after the last shade: " + f
    for rs, os_ in zip(ref["shadow"] or [], orc["shadow"] or []):
        assert len(rs) == len(os_)
        if len(rs):
            for f in ("lightIdx", "pixelIdx"):
                assert np.array_equal(rs[f], os_[f]), what + " shadow " + f
    a, b = orc["accum"].astype(np.float64), ref["accum"].astype(np.float64)
    rel = (np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max(axis=1)
    stats["accum_max_rel"] = float(rel.max())
    stats["accum_pixels"] = len(rel)
    stats["accum_pixels_over_1e-4"] = int((rel > 1e-4).sum())
    stats["accum_pixels_over_1e-6"] = int((rel > 1e-6).sum())
    assert stats["accum_pixels_over_1e-4"] <= max_bad_pixels * len(rel), stats
    return stats


class _SA:
    pass


def load_frame_fixture(path):
    """tests/golden/refframe_*.npz (written by tests/golden/make_golden.py on the MI355X from the reference's own kernels) ->
    (scene arrays, variant dict, camera, capture in the layout of RefGPU.frame_s0, reference heat-map values, branch counts)."""
    from magr_ray_tracer_amd import _lib as W
    g = np.load(path)
    sa = _SA()
    for k in ("prims", "mats", "tex", "lights", "bvh2", "bvh4", "primIdx", "tlas", "blas"):
        setattr(sa, k, g[k])
    v = {k: int(g["variant"][i]) for i, k in enumerate(("shading", "sampling", "accel", "russian_roulette", "filter_fireflies"))}
    cam = g["cam"].view(W.Camera)[0]
    Wd, Hd, y0, y1 = (int(x) for x in g["dims"])
    n_in, n_out = g["n_in"].tolist(), g["n_out"].tolist()
    total = sum(n_in) + n_out[-1]
    rays = np.zeros(total, dtype=W.Ray)
    for f in ("O", "D", "intensity", "t", "primIdx", "u", "v", "pixelIdx"):
        rays[f] = g["ray_" + f]
    with np.errstate(divide="ignore", invalid="ignore"):
        rays["rD"] = np.float32(1.0) / rays["D"]          # initRay (ray.cl:4-19): IEEE 1 / D, all four lanes
    fl = g["ray_flags"]
    rays["bounces"], rays["inside"], rays["lastSpecular"] = fl & 15, (fl >> 4) & 1, (fl >> 5) & 1
    ext, at = [], 0
    for n in n_in:
        ext.append(rays[at:at + n].copy())
        at += n
    shd = np.dtype([("lightIdx", "<i4"), ("pixelIdx", "<i4")])
    shadow, sat = [], 0
    for n in g["shadow_len"].tolist():
        a = np.zeros(n, dtype=shd)
        a["lightIdx"], a["pixelIdx"] = g["shadow_lightIdx"][sat:sat + n], g["shadow_pixelIdx"][sat:sat + n]
        shadow.append(a)
        sat += n
    cap = dict(gen=ext[0], gen_seeds=g["gen_seeds"], ext=ext, last_out=rays[at:].copy(), n_in=n_in, n_out=n_out, n_shadow=g["n_shadow"].tolist(),
               seed0=g["seed0"].tolist(), shadow=shadow, accum=g["accum"], first_pixel=y0 * Wd)
    bc = dict(zip(g["branch_names"].tolist(), g["branch_counts"].tolist()))
    return sa, v, cam, (Wd, Hd, y0, y1), cap, g["heat"], bc


# ---- post-processing fixtures ------------------------------------------------------------------------------------------------
POST_SETS = [(1, 0.0, 1.0, 0.0), (4, 0.6, 1.0, 0.02), (4, 0.0, 0.9, 0.0), (3, 0.35, 0.9, 0.015), (2, 1.0, 2.2, 0.25)]


def post_test_accum(rows):
    """A deterministic accumulator band with values on both sides of the clamp and exact zeros."""
    i = np.arange(rows * REF_W, dtype=np.float64)
    a = np.zeros((rows * REF_W, 4), np.float32)
    a[:, 0] = (np.abs(np.sin(i * 0.0137)) * 5.0).astype(np.float32)
    a[:, 1] = ((i % 977) / 977.0 * 3.5).astype(np.float32)
    a[:, 2] = (np.abs(np.cos(i * 0.0031)) ** 3 * 1.7).astype(np.float32)
    a[::13, :3] = 0
    return a


# ---- the image a bench.py run reduces -----------------------------------------------------------------------------------------
def bench_oracle_image(o, cam, shard, world, lanes, total, warmup=0, band_rows=None):
    """The accumulator `bench.py --gpus world --shard shard --lanes lanes --total-steps total --warmup warmup` reduces, rendered by the
    oracle `o`: every rank runs one group of `lanes` lanes per context of its plan (dist.plans); lane m renders its seed slice, first
    its share of the warmup's frames (their accumulation is discarded by the reset, their RNG state is not) and then its share of the
    timed frames; a group's lanes are added in lane order, the ranks' zero-padded accumulators in rank order.  Exact for the band plans
    (a pixel has one non-zero addend) and for two ranks of the sample plan (two addends commute)."""
    from magr_ray_tracer_amd import dist as rdist
    from oracle.oracle_py import seed_stream
    Wd, Hd = o.width, o.height
    exp = np.zeros((Hd, Wd, 4), np.float32)
    for rank in range(world):
        mine = rdist.rank_frames(total, rank, world) if shard == "samples" else total
        warm = rdist.lane_frames(warmup * (lanes if shard == "samples" else 1), lanes)
        timed = rdist.lane_frames(mine, lanes)
        part = np.zeros((Hd, Wd, 4), np.float32)
        for k in range(len(rdist.plans(shard, Wd, Hd, rank, world, 0, lanes, band_rows))):
            group = None
            for m in range(lanes):
                p = rdist.plans(shard, Wd, Hd, rank, world, m, lanes, band_rows)[k]
                seeds = seed_stream(p["seed_first"], p["seed_count"])
                if warm[m]:
                    _, seeds, _, _ = o.render(cam, warm[m], seeds=seeds, y0=p["y0"], y1=p["y1"])
                acc = np.zeros((Hd, Wd, 4), np.float32)
                if timed[m]:
                    o.render(cam, timed[m], accum=acc, seeds=seeds, y0=p["y0"], y1=p["y1"])
                group = acc if group is None else group + acc
            part = part + group
        exp = exp + part
    return exp
