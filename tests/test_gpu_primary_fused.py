"""The fused primary path of rt_render (rt_primary_fused): bounce 0's extend launch computes every pixel's primary ray from the camera and
the pixel's seed instead of loading what k_generate stored (k_trace_primary), bounce 0's shade launch computes it again (k_shade<..,
PRIMARY>), and the frame has no k_generate launch and no stored primary queue.  Nothing a frame leaves behind may change, so every case
compares, bit for bit, the accumulator, the per-slot seeds, the eight queue lengths of the last frame and the work counters

  with the oracle       frames driven stage by stage (generate, 7 x (extend, shade), connect), so that the queue lengths are the oracle's
                        own; its free-running render() must agree with that before it is used for anything;
  with the old path     the same context class under RT355_FUSE_PRIMARY=0 in ONE fresh child process that runs every case (the knob is
                        read when a context plans its traversal; the child asserts that no context of its fuses).

Every case asserts what rt_primary_fused reports before it renders, so that none silently tests the fallback: the single-BLAS BVH2 and
BVH4 contexts fuse, the two-BLAS scene (k_trace_persist_tlas has its own short-queue branch) stays on k_generate and says so.

What can go wrong, and the case that shows it: the slot -> pixel map of a frame that is no multiple of the 8x8 tile or of 256 slots
(odd), and of one that is (tiles); a band's first pixel (band); the seed carried from frame to frame - advanced by generate, again by
shade, and stored by shade even for a pixel whose primary ray misses (asserted: such pixels exist) - over three frames; the camera
branches (aperture 0 and > 0, anti-aliasing on and off, the fisheye camera with its zero rays outside the unit circle); both shading
kernels (NEE, Kajiya), both tile sizes and both arithmetic modes (the REFERENCE builtins have no CPU oracle: they are held to the old
path and to the stage-level frame); a shade grid smaller than its tile count; the host's frame state when fused frames and stage-level
frames (rt_stage_generate .. rt_stage_connect, which never fuse) alternate on one context; a renderBVH frame, which has no shade launch
to store the advanced seed; a frame with rt_debug_enable_steps; a group of two lanes."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import DEFAULT, assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, dist as rdist, scenes
from magr_ray_tracer_amd.renderer import Device, Group
from oracle.oracle_py import seed_stream

pytestmark = pytest.mark.gpu

KAJIYA = dict(DEFAULT, shading=0)
BVH4 = dict(DEFAULT, accel=1)
CTR_KEYS = tuple(k for k in W.Counters.names if k != "frames")     # (rt_render counts frames, the stage-level calls do not)
WORK = ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests")

# name -> what run_case does.  scene / W, H / band rows / view overrides / antiAliasing / variant (what Device and the oracle take) /
# further Device arguments / environment while the context is created / mode / whether the context must report the fused path
_D = dict(scene="branch", Wd=70, Hd=37, y0=0, y1=None, view={}, aa=1, variant=DEFAULT, dev={}, env={}, mode="render", frames=3, fused=True)
CASES = {
    "odd":            dict(_D),                                                  # 70 x 37: no multiple of 8, 2,590 slots: no multiple of 256
    "tiles":          dict(_D, Wd=64, Hd=40),                                    # 8x8 tiles per wave, 2,560 slots = ten workgroups exactly
    "band":           dict(_D, y0=5, y1=29),                                     # firstPixel = 350
    "open":           dict(_D, scene="cube"),                                    # primary rays that miss, pinhole camera
    "pinhole-aa":     dict(_D, view=dict(aperture=0.0)),
    "pinhole-noaa":   dict(_D, view=dict(aperture=0.0), aa=0),
    "aperture-noaa":  dict(_D, aa=0),
    "fisheye":        dict(_D, view=dict(type=1, fov=75.0)),                      # the corners lie outside the unit circle: zero rays
    "fisheye-noaa":   dict(_D, view=dict(type=1, fov=75.0), aa=0),
    "kajiya":         dict(_D, variant=KAJIYA),
    "kajiya-256":     dict(_D, variant=KAJIYA, dev=dict(shade_blocks_per_cu=2)),
    "tile-256":       dict(_D, dev=dict(shade_blocks_per_cu=2)),
    "reference":      dict(_D, dev=dict(builtins="reference")),
    "reference-fish": dict(_D, dev=dict(builtins="reference", shade_blocks_per_cu=2), view=dict(type=1, fov=75.0)),
    "small-grid":     dict(_D, scene="cube", Wd=330, Hd=205, frames=1, dev=dict(shade_blocks_per_cu=1), env=dict(RT355_SHADE_PER_CU="1")),
    "stage":          dict(_D, mode="stage", frames=1),
    "render-1":       dict(_D, frames=1),
    "mixed-rsr":      dict(_D, mode="rsr"),
    "mixed-srs":      dict(_D, mode="srs"),
    "render-bvh":     dict(_D, mode="bvh", frames=2),
    "steps":          dict(_D, mode="steps", frames=2),
    "group-2":        dict(_D, mode="group"),
    "bvh4":           dict(_D, variant=BVH4),
    "two-blas":       dict(_D, scene="two-blas", fused=False),
}
NO_ORACLE = ("reference", "reference-fish")     # REFERENCE builtins: no CPU restatement exists; the old path is their yardstick


@functools.lru_cache(maxsize=None)
def _scene(name):
    s, view = {"branch": scenes.branch_scene, "cube": scenes.cube_scene, "two-blas": lambda: scenes.two_blas_scene(n=12)}[name]()
    return s, s.arrays(), view          # (the Scene is kept: the arrays are views of its memory)


def _setup(c):
    _, sa, view = _scene(c["scene"])
    y1 = c["Hd"] if c["y1"] is None else c["y1"]
    cam = scenes.camera_for(dict(view, **c["view"]), c["Wd"], c["Hd"])
    first, n = c["y0"] * c["Wd"], (y1 - c["y0"]) * c["Wd"]
    return sa, cam, y1, first, n


@contextlib.contextmanager
def _env(extra):
    old = {k: os.environ.get(k) for k in extra}
    os.environ.update(extra)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _lens(d):
    return np.array([len_of(d, b) for b in range(W.MAX_BOUNCES + 1)], np.int64)


def len_of(d, bounce):
    import ctypes as C
    n = C.c_int32(0)
    d._chk(d._lib.rt_debug_get_rays(d._h, bounce, None, 0, C.byref(n)))
    return int(n.value)


def _ctr(d):
    c = d.counters()
    return np.array([c[k] for k in CTR_KEYS], np.int64)


def _work(d, out, suffix=""):
    """Everything a context holds after its frames, under `suffix`."""
    out["acc" + suffix], out["seeds" + suffix], out["lens" + suffix], out["ctr" + suffix] = d.read_accum(), d.get_seeds(), _lens(d), _ctr(d)
    out["frames" + suffix] = np.array([d.counters()["frames"]], np.int64)


def _stage_frame(d, cam, aa, nee):
    d.stage_begin_frame()
    d.stage_generate(cam, antiAliasing=aa)
    for b in range(W.MAX_BOUNCES):
        d.stage_extend(b)
        d.stage_shade(b)
    if nee:
        d.stage_connect(0, W.MAX_BOUNCES - 1)


def run_case(name, expect_fused=None):
    """What the device leaves behind in case `name`: {key: array}.  Runs in the test process and, under RT355_FUSE_PRIMARY=0, in the child."""
    c = CASES[name]
    sa, cam, y1, first, n = _setup(c)
    want = c["fused"] if expect_fused is None else expect_fused
    out = {}
    with _env(c["env"]):
        if c["mode"] == "group":
            g = Group(c["Wd"], c["Hd"], lanes=2, **c["variant"])
            try:
                g.upload(sa)
                assert [d.primary_fused() for d in g.devs] == [want, want], (name, "rt_primary_fused of the lanes")
                g.seed(0)
                g.render(cam, c["frames"], antiAliasing=c["aa"])
                g.synchronize()
                out["sum"] = g.read_accum()
                for m, d in enumerate(g.devs):
                    _work(d, out, str(m))
            finally:
                g.close()
            return out
        d = Device(c["Wd"], c["Hd"], y0=c["y0"], y1=y1, **c["variant"], **c["dev"])
    try:
        d.upload(sa)
        assert d.primary_fused() == want, (name, "rt_primary_fused")
        d.set_seeds(seed_stream(first, n))
        nee = int(d.cfg["shading"]) == W.SHADING_NEE
        if c["mode"] == "steps":
            d.enable_steps()
        if c["mode"] in ("render", "steps"):
            d.render(cam, c["frames"], antiAliasing=c["aa"])
        elif c["mode"] == "stage":
            for _ in range(c["frames"]):
                _stage_frame(d, cam, c["aa"], nee)
        elif c["mode"] in ("rsr", "srs"):
            for f, kind in enumerate(c["mode"]):
                if kind == "r":
                    d.render(cam, 1, antiAliasing=c["aa"])
                else:
                    _stage_frame(d, cam, c["aa"], nee)
                d.synchronize()
                out[f"acc_after{f}"], out[f"seeds_after{f}"], out[f"lens_after{f}"] = d.read_accum(), d.get_seeds(), _lens(d)
        elif c["mode"] == "bvh":
            d.render(cam, 1, antiAliasing=c["aa"], renderBVH=1)
            d.synchronize()
            out["heat"], out["seeds_heat"] = d.read_accum(), d.get_seeds()
            d.render(cam, c["frames"] - 1, antiAliasing=c["aa"])
        d.synchronize()
        _work(d, out)
        if c["mode"] == "steps":
            out["steps"] = d.get_steps()
    finally:
        d.close()
    return out


# ---- the oracle's frames -------------------------------------------------------------------------------------------------------------
def _oracle_frames(c, seeds, frames, acc=None, skip_generate_of=None):
    """`frames` frames stage by stage from `seeds` (advanced in place): per frame the accumulator, the seeds and the eight queue lengths;
    the summed work counters of extend and connect; how many primary rays of the first frame miss."""
    sa, cam, y1, first, n = _setup(c)
    o = oracle_for(sa, c["Wd"], c["Hd"], **c["variant"])
    acc = np.zeros((c["Wd"] * c["Hd"], 4), np.float32) if acc is None else acc
    e, k = {}, {}
    per, miss = [], 0
    for _ in range(frames):
        rays = o.generate(cam, first, n, seeds, antiAliasing=c["aa"])
        if not per:
            miss = int((_traced(o, rays)["primIdx"] == -1).sum())
        lens, shadows = [], []
        for b in range(W.MAX_BOUNCES):
            for key, v in o.extend(rays)[1].items():
                e[key] = e.get(key, 0) + v
            lens.append(len(rays))
            rays, sh = o.shade(rays, acc, seeds)
            shadows.append(sh)
        lens.append(len(rays))
        if c["variant"]["shading"] == 1:
            for key, v in o.connect(np.concatenate(shadows), acc).items():
                k[key] = k.get(key, 0) + v
        per.append(dict(acc=acc.reshape(c["Hd"], c["Wd"], 4).copy(), seeds=seeds.copy(), lens=np.array(lens, np.int64)))
    return o, per, e, k, miss


def _traced(o, rays):
    r = rays.copy()
    o.extend(r)
    return r


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's frames of case `name`; its free-running render() of the same frames must be the same image and the same seeds."""
    c = CASES[name]
    sa, cam, y1, first, n = _setup(c)
    seeds = seed_stream(first, n)
    frames = 3 if c["mode"] in ("rsr", "srs") else c["frames"]
    o, per, e, k, miss = _oracle_frames(c, seeds, frames)
    acc, sd, e2, k2 = o.render(cam, frames, seeds=seed_stream(first, n), y0=c["y0"], y1=y1, antiAliasing=c["aa"])
    assert_bits(acc, per[-1]["acc"], f"{name}: the oracle's render() against its own stages, accumulator")
    assert np.array_equal(sd, per[-1]["seeds"]), f"{name}: the oracle's render() against its own stages, seeds"
    assert all(e2[x] == e.get(x, 0) and k2[x] == k.get(x, 0) for x in WORK), (name, e2, e, k2, k)
    return dict(per=per, e=e, k=k, miss=miss, n=n, frames=frames)


def _ctr_vs_oracle(ctr, ref, what, frames=None):
    dev = dict(zip(CTR_KEYS, (int(x) for x in ctr)))
    for x in WORK:
        assert dev["extend_" + x] == ref["e"].get(x, 0), (what, "extend_" + x, dev["extend_" + x], ref["e"].get(x, 0))
        assert dev["connect_" + x] == ref["k"].get(x, 0), (what, "connect_" + x, dev["connect_" + x], ref["k"].get(x, 0))
    frames = ref["frames"] if frames is None else frames
    assert dev["primary_rays"] == frames * ref["n"], (what, dev["primary_rays"], frames, ref["n"])


def _frame_vs_oracle(got, want, what, suffix=""):
    assert_bits(got["acc" + suffix], want["acc"], f"{what}: accumulator")
    assert np.array_equal(got["seeds" + suffix], want["seeds"]), f"{what}: seeds"
    assert np.array_equal(got["lens" + suffix], want["lens"]), f"{what}: queue lengths {got['lens' + suffix].tolist()}, oracle {want['lens'].tolist()}"


# ---- the old path, once ---------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np
sys.path.insert(0, {tests!r})
import test_gpu_primary_fused as T
out = {{}}
for name in T.CASES:
    for k, v in T.run_case(name, expect_fused=False).items():
        out[name + "/" + k] = v
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def unfused(tmp_path_factory):
    """Every case on the same context class with RT355_FUSE_PRIMARY=0, in one fresh process: {case: {key: array}}."""
    path = str(tmp_path_factory.mktemp("primary_fused") / "unfused.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([sys.executable, "-c", _CHILD.format(tests=here, out=path)], check=True, timeout=600, cwd=os.path.dirname(here),
                   env=dict(os.environ, RT355_FUSE_PRIMARY="0"))
    g = np.load(path)
    out = {}
    for key in g.files:
        name, k = key.split("/", 1)
        out.setdefault(name, {})[k] = g[key]
    return out


def _same_as_unfused(got, old, what):
    assert sorted(got) == sorted(old), (what, sorted(got), sorted(old))
    for k in got:
        if got[k].dtype == np.float32:
            assert_bits(got[k], old[k], f"{what}: {k} against RT355_FUSE_PRIMARY=0")
        else:
            assert np.array_equal(got[k], old[k]), f"{what}: {k} against RT355_FUSE_PRIMARY=0: {got[k].tolist()[:16]} / {old[k].tolist()[:16]}"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
PLAIN = [n for n, c in CASES.items() if c["mode"] == "render"]


@pytest.mark.parametrize("name", PLAIN)
def test_fused_frames_are_the_oracles_and_the_old_paths(name, unfused, monkeypatch):
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    got = run_case(name)
    _same_as_unfused(got, unfused[name], name)
    if name in NO_ORACLE:
        return
    ref = _reference(name)
    if name in ("open", "fisheye", "fisheye-noaa"):
        assert 0 < ref["miss"] < ref["n"], (name, ref["miss"], "primary rays that miss: shade(0) stores their advanced seeds")
    _frame_vs_oracle(got, ref["per"][-1], name)
    _ctr_vs_oracle(got["ctr"], ref, name)
    assert int(got["frames"][0]) == ref["frames"] and got["acc"][..., :3].sum() > 0


def test_reference_builtins_fused_frame_is_the_stage_level_frame(monkeypatch):
    """The arithmetic without an oracle, held to k_generate's stored queue in the same process too: one fused frame against one
    stage-level frame of the same context class (the IEEE pair is test_a_stage_level_frame_... below)."""
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    for base in NO_ORACLE:
        CASES["_r"], CASES["_s"] = dict(CASES[base], frames=1), dict(CASES[base], frames=1, mode="stage")
        try:
            r, s = run_case("_r"), run_case("_s")
        finally:
            del CASES["_r"], CASES["_s"]
        assert (int(r.pop("frames")[0]), int(s.pop("frames")[0])) == (1, 0)
        _same_as_unfused(r, s, f"{base}: fused frame against stage-level frame")


def test_a_stage_level_frame_equals_a_fused_frame(unfused, monkeypatch):
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    stage, fused = run_case("stage"), run_case("render-1")
    _same_as_unfused(stage, unfused["stage"], "stage")
    assert (int(fused.pop("frames")[0]), int(stage.pop("frames")[0])) == (1, 0)
    _same_as_unfused(stage, fused, "stage-level frame against fused frame")
    ref = _reference("stage")
    _frame_vs_oracle(stage, ref["per"][0], "stage-level frame")
    _ctr_vs_oracle(stage["ctr"], ref, "stage-level frame")


@pytest.mark.parametrize("name", ["mixed-rsr", "mixed-srs"])
def test_fused_and_stage_level_frames_alternate_on_one_context(name, unfused, monkeypatch):
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    got = run_case(name)
    _same_as_unfused(got, unfused[name], name)
    ref = _reference(name)
    for f in range(3):
        _frame_vs_oracle(got, ref["per"][f], f"{name}: after frame {f} ({'fused' if CASES[name]['mode'][f] == 'r' else 'stage-level'})", f"_after{f}")
    _frame_vs_oracle(got, ref["per"][2], name)
    _ctr_vs_oracle(got["ctr"], ref, name)


def test_a_render_bvh_frame_keeps_the_advanced_seeds(unfused, monkeypatch):
    """renderBVH: generate and extend(0) only - the heat map steps / 255 in every component, the seeds as generate leaves them - and the
    next frame starts from those seeds."""
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    name = "render-bvh"
    got = run_case(name)
    _same_as_unfused(got, unfused[name], name)
    c = CASES[name]
    sa, cam, y1, first, n = _setup(c)
    o = oracle_for(sa, c["Wd"], c["Hd"], **c["variant"])
    seeds = seed_stream(first, n)
    rays = o.generate(cam, first, n, seeds, antiAliasing=c["aa"])
    steps, e0 = o.extend(rays, want_steps=True)
    heat = steps.astype(np.uint32).astype(np.float32) / np.float32(255.0)
    assert not np.array_equal(seeds, seed_stream(first, n))
    assert_bits(got["heat"].reshape(-1, 4), np.repeat(heat[:, None], 4, axis=1), "heat map")
    assert np.array_equal(got["seeds_heat"], seeds), "seeds after the renderBVH frame"
    _, per, e, k, _ = _oracle_frames(c, seeds, c["frames"] - 1, acc=np.repeat(heat[:, None], 4, axis=1).copy())
    _frame_vs_oracle(got, per[-1], "the frame after the renderBVH frame")
    for x in WORK:
        e[x] = e.get(x, 0) + e0[x]
    _ctr_vs_oracle(got["ctr"], dict(e=e, k=k, n=n, frames=c["frames"]), name)


def test_a_frame_with_debug_steps(unfused, monkeypatch):
    """rt_debug_enable_steps: the STEPS instantiations run the later bounces; the per-slot steps and the path-issue counters have no
    oracle and are held to the old path, everything else to the oracle too."""
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    got = run_case("steps")
    _same_as_unfused(got, unfused["steps"], "steps")
    ref = _reference("steps")
    _frame_vs_oracle(got, ref["per"][-1], "steps")
    _ctr_vs_oracle(got["ctr"], ref, "steps")


def test_a_group_of_two_lanes(unfused, monkeypatch):
    monkeypatch.delenv("RT355_FUSE_PRIMARY", raising=False)
    monkeypatch.delenv("RT355_GROUP_STREAMS", raising=False)
    name = "group-2"
    got = run_case(name)
    _same_as_unfused(got, unfused[name], name)
    c = CASES[name]
    n = c["Wd"] * c["Hd"]
    total = None
    for m, frames in enumerate(rdist.lane_frames(c["frames"], 2)):
        o, per, e, k, _ = _oracle_frames(c, seed_stream(m * n, n), frames)
        assert int(got[f"frames{m}"][0]) == frames
        _frame_vs_oracle(got, per[-1], f"lane {m}", str(m))
        _ctr_vs_oracle(got[f"ctr{m}"], dict(e=e, k=k, n=n, frames=frames), f"lane {m}")
        total = per[-1]["acc"] if total is None else total + per[-1]["acc"]
    assert_bits(got["sum"], total, "the group's lane-ordered sum")
