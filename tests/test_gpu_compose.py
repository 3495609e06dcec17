"""The composition of the image (-m gpu): lane and band accumulators into the image a user gets - rt_group_sum (k_sum_lanes) into a
torch tensor and into the group's own buffer (rt_group_read_accum), rt_group_postproc of the summed accumulator, rt_group_focus of a
band group, and dist.Groups.sum_into followed by the one all_reduce of bench.py - against plain restatements and the CPU oracle.

Every stage that produces a sample is pinned elsewhere (traversal, math, builders, refit); here the frames are small and the
question is only whether the right samples are added up, in the right order, into the right rows, at the right time.  Bit for bit
throughout, except the post-processing allowances of test_gpu_parity.test_postproc_chain_matches_oracle (vignetting goes through the
hardware sqrt, gamma through pow)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from magr_ray_tracer_amd import _lib, dist as rdist, scenes
from magr_ray_tracer_amd.renderer import Device, Group
from oracle.oracle_py import Oracle, postproc, seed_stream
from helpers import DEFAULT, assert_bits, bench_oracle_image, max_rel, mismatch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xC2A5A5A5       # a finite float32 (about -82.8) that no accumulator holds: rows a sum must not touch are filled with it


def _sponza(Wd, Hd):
    s, view = scenes.sponza_class(0.2)
    sa = s.arrays(bvh4=False)
    return sa, scenes.camera_for(view, Wd, Hd)


def _group(sa, Wd, Hd, lanes, y0=0, y1=None):
    g = Group(Wd, Hd, lanes=lanes, y0=y0, y1=y1, **DEFAULT)
    g.upload(sa)
    g.seed(0)
    return g


def _sentinel_tensor(Wd, Hd):
    _lib.device_lib()       # torch after librt355.so: the process stays on the HIP runtime the rest of the suite runs on
    import torch
    t = torch.from_numpy(np.full((Hd, Wd, 4), SENTINEL, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()        # the sum runs on a library stream that torch's does not order against
    return t


def _outside(a, y0, y1):
    return np.concatenate([a[:y0], a[y1:]])


class _OracleGroup:
    """The oracle standing in for a Group over rows [y0, y1) seeded with seed(0): lane m renders sample stream m of those rows (dist's
    band plans), frame j of the accumulation is lane j mod L's (the round-robin continues across calls and restarts at a reset - the
    seeds do not), and the group's accumulator is the lanes' sum in lane order."""

    def __init__(self, o, cam, lanes, y0=0, y1=None):
        self.o, self.cam = o, cam
        self.y0, self.y1 = y0, o.height if y1 is None else y1
        Wd, Hd = o.width, o.height
        self.seeds = [seed_stream(m * Wd * Hd + self.y0 * Wd, (self.y1 - self.y0) * Wd) for m in range(lanes)]
        self.reset()

    def reset(self):
        self.acc = [np.zeros((self.o.height, self.o.width, 4), np.float32) for _ in self.seeds]
        self.next = 0

    def render(self, frames):
        L = len(self.seeds)
        for m in range(L):
            n = sum(1 for j in range(self.next, self.next + frames) if j % L == m)
            if n:
                self.o.render(self.cam, n, accum=self.acc[m], seeds=self.seeds[m], y0=self.y0, y1=self.y1)
        self.next = (self.next + frames) % L

    def sum(self):
        s = self.acc[0].copy()
        for a in self.acc[1:]:
            s = s + a
        return s


# ---- a. k_sum_lanes at band and lane edges ----------------------------------------------------------------------------------------
EDGE_W, EDGE_H = 130, 90
EDGE_BANDS = [(0, 90), (0, 1), (37, 61), (61, 90)]     # pixel counts 11700, 130, 3120, 3770: none a multiple of the 256-thread block


@pytest.mark.parametrize("lanes", [1, 2, 3, 5, 8])
def test_sum_lanes_matches_a_plain_sum_and_the_oracle_at_band_edges(lanes):
    """rt_group_sum into a tensor writes the lane-ordered float32 sum into the band's rows and not one bit elsewhere; the group's own
    sum (rt_group_read_accum) is that sum inside the band and +0.0 outside; each lane is the oracle's sample stream, so the band is the
    oracle's lane-ordered sum.  An uneven frame count (2L + 1, then L + 1 after a reset) leaves the lanes with unequal frame counts."""
    Wd, Hd = EDGE_W, EDGE_H
    sa, cam = _sponza(Wd, Hd)
    o = Oracle(sa, Wd, Hd, **DEFAULT)
    for y0, y1 in EDGE_BANDS:
        g = _group(sa, Wd, Hd, lanes, y0, y1)
        ref = _OracleGroup(o, cam, lanes, y0, y1)
        try:
            for k, frames in enumerate((2 * lanes + 1, lanes + 1)):
                what = f"lanes={lanes} rows [{y0}, {y1}) pass {k} ({frames} frames)"
                if k:
                    g.reset()
                    ref.reset()
                g.render(cam, frames)
                ref.render(frames)
                lane = [d.read_accum() for d in g.devs]
                for m in range(lanes):
                    assert_bits(lane[m], ref.acc[m], f"{what}: lane {m} vs the oracle")
                exp = lane[0]
                for a in lane[1:]:
                    exp = exp + a                          # k_sum_lanes restated: float32, lane order, left to right
                assert_bits(exp[y0:y1], ref.sum()[y0:y1], f"{what}: lane-ordered sum vs the oracle")
                t = _sentinel_tensor(Wd, Hd)
                g.sum_into(t)
                g.synchronize()
                got = t.cpu().numpy()
                assert_bits(got[y0:y1], exp[y0:y1], f"{what}: sum_into, the band's rows")
                assert (_outside(got, y0, y1).view(np.uint32) == SENTINEL).all(), f"{what}: sum_into wrote outside the band"
                acc = g.read_accum()
                assert_bits(acc[y0:y1], exp[y0:y1], f"{what}: read_accum, the band's rows")
                assert (_outside(acc, y0, y1).view(np.uint32) == 0).all(), f"{what}: read_accum is not +0.0 outside the band"
        finally:
            g.close()


# ---- b. a sum the host does not wait for -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 2, 3, None])
def test_sums_queued_between_frames_without_host_sync(streams, monkeypatch):
    """render(N) -> sum_into(t1) -> render(K) -> sum_into(t2) -> reset() -> render(J) -> sum_into(t3), then ONE synchronize: the sum
    must not read a lane before its queued frames are done, and the lanes must not overwrite (render on, reset) an accumulator before
    the sum has read it - on the lanes' own streams and on fewer worker streams than lanes (RT355_GROUP_STREAMS)."""
    Wd, Hd, lanes, N, K, J = 160, 90, 4, 5, 6, 7
    if streams is None:
        monkeypatch.delenv("RT355_GROUP_STREAMS", raising=False)
    else:
        monkeypatch.setenv("RT355_GROUP_STREAMS", str(streams))
    sa, cam = _sponza(Wd, Hd)
    ref = _OracleGroup(Oracle(sa, Wd, Hd, **DEFAULT), cam, lanes)
    exp = []
    for reset, frames in ((False, N), (False, K), (True, J)):
        if reset:
            ref.reset()
        ref.render(frames)
        exp.append(ref.sum())
    g = _group(sa, Wd, Hd, lanes)
    try:
        t = [_sentinel_tensor(Wd, Hd) for _ in range(3)]
        g.render(cam, N)
        g.sum_into(t[0])
        g.render(cam, K)
        g.sum_into(t[1])
        g.reset()
        g.render(cam, J)
        g.sum_into(t[2])
        g.synchronize()
        S = g.concurrency()
        assert g.frames() == J
        for k, (tk, name) in enumerate(zip(t, (f"after {N} frames", f"after {N} + {K} frames", f"after a reset and {J} frames"))):
            assert_bits(tk.cpu().numpy(), exp[k], f"S={S} (RT355_GROUP_STREAMS={streams}): sum {name}")
    finally:
        g.close()


# ---- c. post-processing of the composed image --------------------------------------------------------------------------------------
POST = [(0.0, 1.0, 0.0), (0.7, 1.0, 0.0), (0.0, 1.0, 0.15), (0.5, 1.0, 0.05), (0.3, 0.9, 0.05), (0.0, 0.9, 0.0)]


@pytest.mark.parametrize("band", [None, (23, 61)], ids=["full", "band"])
def test_group_postproc_of_the_summed_lanes_matches_the_oracle(band):
    """rt_group_postproc post-processes the lanes' sum with the divisor g.frames() (frames = 0) or the one given; compared with the
    oracle's chain applied to the oracle's composed accumulator.  A band group's other rows are post-processed zeros."""
    Wd, Hd, lanes, frames = 160, 90, 4, 7
    y0, y1 = band or (0, Hd)
    sa, cam = _sponza(Wd, Hd)
    ref = _OracleGroup(Oracle(sa, Wd, Hd, **DEFAULT), cam, lanes, y0, y1)
    ref.render(frames)
    acc, zero = ref.sum(), np.zeros((Hd, Wd, 4), np.float32)
    g = _group(sa, Wd, Hd, lanes, y0, y1)
    try:
        g.render(cam, frames)
        assert g.frames() == frames
        for div in (0, 5):
            for vig, gamma, chroma in POST:
                what = f"rows [{y0}, {y1}) frames={div} vignette={vig} gamma={gamma} chromatic={chroma}"
                f, b = g.postproc(div, vignette=vig, gamma=gamma, chromatic=chroma)
                ef, eb = postproc(acc, div or frames, vig, gamma, chroma)
                if vig == 0.0 and gamma == 1.0:
                    assert_bits(f, ef, what + ": float image")
                    assert np.array_equal(b, eb), what + ": RGBA8"
                elif gamma == 1.0:
                    assert max_rel(f, ef, 1e-6) < 3e-6 and np.abs(b.astype(int) - eb.astype(int)).max() <= 1, what
                else:
                    assert np.abs(f - ef).max() < 1e-5 and np.abs(b.astype(int) - eb.astype(int)).max() <= 1, what
                if band and chroma == 0.0:                  # (the chromatic shift reads neighbouring rows)
                    zf, zb = postproc(zero, div or frames, vig, gamma, chroma)
                    assert_bits(_outside(f, y0, y1), _outside(zf, y0, y1), what + ": rows outside the band")
                    assert np.array_equal(_outside(b, y0, y1), _outside(zb, y0, y1)), what + ": RGBA8 rows outside the band"
    finally:
        g.close()


# ---- d. focus through a band ------------------------------------------------------------------------------------------------------
def test_group_focus_from_a_band_without_the_focus_pixel():
    """bench.py focuses through the first context of each rank, whose band need not hold the focus pixel: the focal distance is
    traced over the whole frame, so it equals rt_focus of a full-frame context and the oracle's."""
    Wd, Hd = 160, 90
    sa, cam = _sponza(Wd, Hd)
    x, y = Wd // 2, Hd // 2
    exp = Oracle(sa, Wd, Hd, **DEFAULT).focus(x, y, cam)
    d = Device(Wd, Hd, **DEFAULT)
    d.upload(sa)
    full = d.focus(x, y, cam)
    d.close()
    assert full.view(np.uint32) == exp.view(np.uint32), (full, exp)
    for y0, y1 in ((0, 23), (61, 90)):
        g = _group(sa, Wd, Hd, 2, y0, y1)
        try:
            for got, who in ((g.focus(x, y, cam), "rt_group_focus"), (g.devs[0].focus(x, y, cam), "lane 0's rt_focus")):
                assert got.view(np.uint32) == exp.view(np.uint32), (who, y0, y1, got, exp)
        finally:
            g.close()


# ---- e. the reduce of bench.py after a warmup ---------------------------------------------------------------------------------------
# (shard, ranks, lanes, --band-rows): neither 23 nor 50 divides 180 rows; 50 gives bands 0 and 3 to rank 0, 1 and 2 to the others.
# The sample plan (every rank owns every row) is the control.
BENCH_CASES = [("bands", 2, 2, 0), ("ibands", 2, 2, 23), ("ibands", 3, 1, 50), ("samples", 2, 2, 0)]


def _first_mismatch(got, exp, shard, world, rows):
    bad = (got.view(np.uint32) != exp.view(np.uint32)) & ~((got == 0) & (exp == 0))
    if not bad.any():
        return ""
    y, x, c = (int(v) for v in np.argwhere(bad)[0])
    owner = [r for r in range(world) for p in rdist.plans(shard, got.shape[1], got.shape[0], r, world, band_rows=rows or None) if p["y0"] <= y < p["y1"]]
    return (f"{int(bad.any(axis=(1, 2)).sum())} rows differ; first at y={y} x={x} (rows of rank {owner}): got {got[y, x].tolist()}, "
            f"expected {exp[y, x].tolist()}")


@pytest.mark.parametrize("shard,world,lanes,rows", BENCH_CASES, ids=[f"{s}-{n}ranks-{m}lanes" for s, n, m, _ in BENCH_CASES])
def test_bench_reduce_after_a_warmup(tmp_path, shard, world, lanes, rows):
    """`bench.py --gpus N --total-steps T --warmup 2` (rehearsal form: same device, gloo) reduces the same buffer twice - after the
    warmup and after the timed region.  The second reduce must see only the timed frames: every rank's rows of the image once, and
    exact zeros from the ranks that do not own them (no left-over of the first reduce).  The expected image is the oracle's, with the
    warmup's frames advancing every lane's RNG state."""
    Wd, Hd, total, warmup = 320, 180, 5, 2
    if shard == "ibands":
        assert all(rdist.interleaved_bands(Hd, r, world, rows) for r in range(world))      # bench.py needs a band on every rank
    dump = tmp_path / "acc.npy"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--same-device", "--backend", "gloo",
           "--total-steps", str(total), "--warmup", str(warmup), "--shard", shard, "--lanes", str(lanes), "--no-cpu-baseline", "--no-single",
           "--width", str(Wd), "--height", str(Hd), "--detail", "0.2", "--dump-accum", str(dump)]
    if rows:
        cmd += ["--band-rows", str(rows)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == world and line["scaling"] == "strong" and line["steps"] == total and line["warmup"] == warmup
    got = np.load(dump)
    sa, cam = _sponza(Wd, Hd)
    o = Oracle(sa, Wd, Hd, **DEFAULT)
    cam["focalLength"] = o.focus(Wd // 2, Hd // 2, cam)          # = every rank's focus through its first band (test d)
    exp = bench_oracle_image(o, cam, shard, world, lanes, total, warmup=warmup, band_rows=rows or None)
    assert mismatch(got, exp) == 0, f"{shard}, {world} ranks x {lanes} lanes: " + _first_mismatch(got, exp, shard, world, rows)
    assert got[..., :3].sum() > 0
