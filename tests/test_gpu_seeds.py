"""No launch ever sees RNG state 0 (include/rt355.h, "seedBuffer"; DESIGN.md section 2, "State 0").

State 0 is the fixed point of the RNG step: every draw from it is 0.0f and k_shade's sample_ball would never leave its rejection loop.
The library keeps it out on the host: a fresh context is seeded as rt_seed_default would seed it, a fresh group as rt_group_seed(g, 0)
would, and rt_set_seeds refuses a zero seed before it copies anything (test_rng_cpu.py pins why that suffices).

EVERY TEST HERE READS THE SEEDS BACK AND ASSERTS THAT NONE IS 0 BEFORE ANYTHING IS LAUNCHED (_nonzero_seeds): on a library that
leaves a context unseeded, or accepts a zero, the test fails on the host and starts no kernel.  No test hands a zero state to a
launch, on the GPU or in the oracle."""
import numpy as np
import pytest

import test_rng_cpu as R
from helpers import DEFAULT, assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle import oracle_py as O
from oracle.oracle_py import seed_stream
from test_gpu_shade_lds import EPS, room_scene

pytestmark = pytest.mark.gpu

WD, HD = 64, 8                    # 512 slots: one k_shade tile of a context alone
_ROOM = {}


def _room():
    if not _ROOM:
        s, view = room_scene()
        _ROOM["sa"], _ROOM["view"] = s.arrays(), view
    return _ROOM["sa"], _ROOM["view"]


def _nonzero_seeds(d, want=None):
    """The context's seeds, read back; nothing may be launched on `d` before this has passed."""
    got = d.get_seeds()
    assert got.all(), f"{int((got == 0).sum())} of {len(got)} seeds are 0, the first at {int(np.flatnonzero(got == 0)[0])}: nothing is launched"
    if want is not None:
        assert np.array_equal(got, want)
    return got


def _oracle_frame(sa, view, w, h, seeds, y0=0, y1=None, **variant):
    o = oracle_for(sa, w, h, **variant)
    acc, seeds_after, _, _ = o.render(scenes.camera_for(view, w, h), 1, seeds=seeds.copy(), y0=y0, y1=y1)
    return acc, seeds_after


# ---- 1. fresh contexts are seeded ------------------------------------------------------------------------------------------------------
def test_a_fresh_context_holds_the_default_seeds_and_renders_with_them():
    sa, view = _room()
    d = Device(WD, HD, **DEFAULT)
    try:
        seeds = _nonzero_seeds(d, seed_stream(0, WD * HD))                 # no other call made
        d.upload(sa)
        d.render(scenes.camera_for(view, WD, HD), 1)
        want, after = _oracle_frame(sa, view, WD, HD, seeds, **DEFAULT)
        assert_bits(d.read_accum(), want, "a frame rendered without a seeding call")
        assert np.array_equal(d.get_seeds(), after) and want[..., :3].sum() > 0
    finally:
        d.close()


def test_a_fresh_row_band_holds_its_slice_of_the_stream():
    sa, view = _room()
    h, y0, y1 = 24, 8, 16
    d = Device(WD, h, y0=y0, y1=y1, **DEFAULT)
    try:
        seeds = _nonzero_seeds(d, seed_stream(y0 * WD, (y1 - y0) * WD))
        assert not np.array_equal(seeds, seed_stream(0, (y1 - y0) * WD))
        d.upload(sa)
        d.render(scenes.camera_for(view, WD, h), 1)
        want, after = _oracle_frame(sa, view, WD, h, seeds, y0=y0, y1=y1, **DEFAULT)
        assert_bits(d.read_accum(), want, "a band's frame rendered without a seeding call")
        assert np.array_equal(d.get_seeds(), after) and want[y0:y1, :, :3].sum() > 0 and not want[:y0].any() and not want[y1:].any()
    finally:
        d.close()


def test_a_fresh_group_holds_sample_streams_0_to_3():
    sa, view = _room()
    lanes, n = 4, WD * HD
    g = Group(WD, HD, lanes=lanes, **DEFAULT)
    try:
        seeds = [_nonzero_seeds(g.devs[m], seed_stream(m * n, n)) for m in range(lanes)]     # every lane, before the first launch
        g.upload(sa)
        g.render(scenes.camera_for(view, WD, HD), lanes)                                      # one frame per lane
        g.synchronize()
        for m in range(lanes):
            want, after = _oracle_frame(sa, view, WD, HD, seeds[m], **DEFAULT)
            assert_bits(g.devs[m].read_accum(), want, f"lane {m}'s frame rendered without a seeding call")
            assert np.array_equal(g.devs[m].get_seeds(), after)
        g.seed(0)                                                                             # what creation left, again
        for m in range(lanes):
            assert np.array_equal(g.devs[m].get_seeds(), seeds[m])
    finally:
        g.close()


# ---- 2. zero seeds are refused ------------------------------------------------------------------------------------------------------------
def test_a_zero_seed_is_refused_and_the_seeds_stay(tmp_path):
    sa, view = _room()
    n = WD * HD
    d = Device(WD, HD, **DEFAULT)
    try:
        _nonzero_seeds(d)
        old = seed_stream(1000, n)
        d.set_seeds(old)
        for name, at in (("first", [0]), ("last", [n - 1]), ("middle", [n // 2 + 3]), ("two", [77, 300]), ("all", list(range(n)))):
            bad = seed_stream(5000, n)
            bad[at] = 0
            with pytest.raises(RtError) as e:
                d.set_seeds(bad)
            assert e.value.code == W.RT_E_INVALID and f"seeds[{at[0]}]" in str(e.value), (name, e.value.code, str(e.value))
            _nonzero_seeds(d, old)                                         # nothing was copied
        # a checkpoint with one zero seed: refused whole - seeds and accumulator stay
        d.upload(sa)
        cam = scenes.camera_for(view, WD, HD)
        d.render(cam, 1)
        want, after = _oracle_frame(sa, view, WD, HD, old, **DEFAULT)
        assert_bits(d.read_accum(), want, "the frame after the refusals (the old seeds)")
        path = str(tmp_path / "ck.npz")
        d.save_checkpoint(path, 1)
        g = dict(np.load(path))
        assert g["seeds"].all() and np.array_equal(g["seeds"], after)
        g["seeds"] = g["seeds"].copy()
        g["seeds"][n - 2] = 0
        g["accum"] = g["accum"] + 1
        bad_path = str(tmp_path / "bad.npz")
        np.savez_compressed(bad_path, **g)
        with pytest.raises(RtError) as e:
            d.load_checkpoint(bad_path)
        assert e.value.code == W.RT_E_INVALID and f"seeds[{n - 2}]" in str(e.value)
        _nonzero_seeds(d, after)
        assert_bits(d.read_accum(), want, "the accumulator after a refused checkpoint")
        assert d.load_checkpoint(path) == 1                                # the good one restores
        _nonzero_seeds(d, after)
        d.render(cam, 1)                                                   # ... and the next frame is the oracle's second
        o = oracle_for(sa, WD, HD, **DEFAULT)
        two, _, _, _ = o.render(cam, 2, seeds=old.copy())
        assert_bits(d.read_accum(), two, "the frame after the restored checkpoint")
    finally:
        d.close()


def test_a_group_and_its_lanes_refuse_zero_seeds():
    lanes, n = 2, WD * HD
    g = Group(WD, HD, lanes=lanes, **DEFAULT)
    try:
        before = [_nonzero_seeds(g.devs[m]) for m in range(lanes)]
        bad = seed_stream(0, n)
        bad[9] = 0
        with pytest.raises(RtError) as e:
            g.devs[1].set_seeds(bad)
        assert e.value.code == W.RT_E_INVALID and "seeds[9]" in str(e.value)
        g.seed(3)                                                          # a valid seeding still works: streams 3 and 4
        for m in range(lanes):
            _nonzero_seeds(g.devs[m], seed_stream((3 + m) * n, n))
        assert not np.array_equal(g.devs[0].get_seeds(), before[0])
    finally:
        g.close()


# ---- 3. the worst state is really walked --------------------------------------------------------------------------------------------------
def _draws(a, b, limit=400):
    """RNG steps from state a to state b."""
    k = 0
    while a != b:
        a = O.xorshift32(a)
        k += 1
        assert k <= limit
    return k


def test_the_longest_rejection_run_is_walked_as_the_oracle_walks_it():
    """WORST_STATE and the 15 states before it in 16 slots of a one-tile frame of the room (NEE, cosine sampling, no Russian roulette:
    every slot that hits a wall samples a direction).  Generate and the light sample consume a few draws first, so one of the slots
    enters sample_ball exactly in WORST_STATE and makes all 28 attempts."""
    sa, view = _room()
    n = WD * HD
    variant = dict(DEFAULT, russian_roulette=False)
    back = [R.step_back(R.WORST_STATE, k) for k in range(16)]
    assert all(back) and len(set(back)) == 16 and O.xorshift32(back[15], 15) == R.WORST_STATE
    slots = np.arange(16) * 32 + 5
    seeds = seed_stream(0, n)
    seeds[slots] = back
    cam = scenes.camera_for(view, WD, HD)
    o = oracle_for(sa, WD, HD, **variant)
    ref_seeds = seeds.copy()
    rays = o.generate(cam, 0, n, ref_seeds)
    o.extend(rays)
    acc = np.zeros((n, 4), np.float32)
    out, sh = o.shade(rays, acc, ref_seeds)
    d = Device(WD, HD, **variant)
    try:
        _nonzero_seeds(d)
        d.set_seeds(seeds)
        _nonzero_seeds(d, seeds)
        d.upload(sa)
        d.reset()
        d.stage_begin_frame()
        d.stage_generate(cam)
        d.stage_extend(0)
        d.stage_shade(0)
        got, rec, after = d.get_rays(1), d.get_shadow(0, 0), d.get_seeds()
        assert len(got) == len(out) and len(rec) == len(sh) and len(out) > n // 2 and len(sh) > n // 2
        for k in ("pixelIdx", "bounces", "inside", "lastSpecular"):
            assert np.array_equal(got[k], out[k]), k
        for k in ("O", "D", "intensity"):
            assert_bits(got[k], out[k], f"extension rays {k}")
        assert np.array_equal(rec["pixelIdx"], sh["pixelIdx"])
        assert_bits(rec["tmax"], sh["dist"] - np.float32(2) * EPS, "shadow records tmax")
        assert_bits(rec["l"], sh["L"][:, :3], "shadow records l")
        assert_bits(rec["o"], (sh["I"] + sh["L"] * EPS)[:, :3], "shadow records o")
        assert np.array_equal(after, ref_seeds) and after.all()
        used = np.array([_draws(int(a), int(b)) for a, b in zip(seeds, after)])
        # a slot that samples a direction at its first attempt: `pre` draws in front of sample_ball, then three
        pre = int(np.bincount(used).argmax()) - 3
        assert 0 <= pre < 16, (pre, np.bincount(used))
        worst = 3 * (R.LONGEST_RUN + 1)
        assert used.max() >= worst                                          # some slot made every attempt of the longest run
        assert used[slots[pre]] == pre + worst == used.max(), (pre, used[slots].tolist())
        print("draws in front of sample_ball", pre, "draws of the 16 slots", used[slots].tolist())
    finally:
        d.close()
