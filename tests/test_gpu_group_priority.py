"""The stream priority class of a group's lanes (rt_group_create, RT355_GROUP_PRIORITY): more workers, the same bits.

HIP keeps one pool of hardware queues per stream priority, so rt_group_create may replace the lanes' streams by streams of another
priority class when more of them run side by side there.  Frame j of a group is lane j mod L's sample on whatever worker stream,
so every lane's accumulator, seeds and work counters, and the group's lane-ordered sum, must be the oracle's for every class - the
scene and the call sequence are those of test_gpu_group_streams.  How many workers a class yields is the runtime's business and is
not asserted; what is: 1 <= S <= lanes, the class the group names is the one asked for (auto: the one its own rule picks from what
it measured), auto never has fewer workers than normal, and a Device beside the group renders its own oracle frames.

`normal` and the commit before the classes existed: normal creates no stream but the lanes' own (rt_create's, unchanged) and runs
the same nap test over them, which is all that commit did.  The test holds that to what can be observed in one process: normal
tries no other class, reports the same S on every creation, and auto's own measurement of the normal class - taken first, over
the same kind of streams - is that S."""
import functools

import numpy as np
import pytest

from magr_ray_tracer_amd.renderer import Device, Group
from helpers import DEFAULT, assert_bits, oracle_for
from test_gpu_group_streams import CALLS_A, CALLS_B, FIRST, Hd, Wd, _ctr_vs_oracle, _oracle, _scene

KNOBS = ("normal", "low", "high", "auto", "mixed")


@functools.lru_cache(maxsize=None)
def _scene_once():
    return _scene()


@functools.lru_cache(maxsize=None)
def _oracle_once(lanes):
    sa, cam = _scene_once()
    return _oracle(sa, cam, lanes)


@functools.lru_cache(maxsize=None)
def _single_oracle(frames):
    sa, cam = _scene_once()
    acc, *_ = oracle_for(sa, Wd, Hd, **DEFAULT).render(cam, frames)
    return acc


def _group(lanes, knob, monkeypatch):
    monkeypatch.delenv("RT355_GROUP_STREAMS", raising=False)
    if knob is None:
        monkeypatch.delenv("RT355_GROUP_PRIORITY", raising=False)
    else:
        monkeypatch.setenv("RT355_GROUP_PRIORITY", knob)
    return Group(Wd, Hd, lanes=lanes, **DEFAULT)


def _auto_choice(seen):
    """The rule of rt_group_create over what it measured: normal unless another class holds more workers, then the lower at a tie."""
    best = "normal"
    for k in ("low", "high"):
        if k in seen and seen[k] > seen[best]:
            best = k
    return best


def _check_class(g, lanes, knob):
    S, cls, seen = g.concurrency(), g.stream_class(), g.class_concurrency()
    print(f"lanes={lanes} RT355_GROUP_PRIORITY={knob}: S={S} class={cls} measured={seen}")
    assert 1 <= S <= lanes, (knob, S)
    for k, s in seen.items():
        assert 1 <= s <= lanes, (knob, k, s)
    if knob in ("normal", "low", "high"):
        assert cls == knob and seen == {knob: S}, (knob, cls, seen, S)
    else:
        assert "normal" in seen and S >= seen["normal"], (knob, S, seen)
        if seen["normal"] == lanes:
            assert seen == {"normal": lanes} and cls == "normal", (knob, cls, seen)   # a queue per lane already: nothing else is tried
        if knob in ("auto", None):
            assert cls == _auto_choice(seen) and S == seen[cls], (knob, cls, seen, S)
        else:
            assert S >= max(seen.values()), (knob, S, seen)
            assert cls in ("normal", "low", "high", "mixed") and (cls == "mixed" or (cls == _auto_choice(seen) and S == seen[cls])), (knob, cls, seen, S)
    return S, cls, seen


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("lanes", [4, 8])
def test_group_bits_do_not_depend_on_the_stream_class(lanes, knob, monkeypatch):
    sa, cam = _scene_once()
    ref = _oracle_once(lanes)
    g = _group(lanes, knob, monkeypatch)
    try:
        S, cls, _ = _check_class(g, lanes, knob)
        g.upload(sa)
        g.seed(FIRST)
        for f in CALLS_A:
            g.render(cam, f)
        acc_a = [d.read_accum() for d in g.devs]
        seeds_a = [d.get_seeds() for d in g.devs]
        sum_a = g.read_accum()
        g.reset()
        for f in CALLS_B:
            g.render(cam, f)
        sum_b = g.read_accum()
        acc_b = [d.read_accum() for d in g.devs]
        seeds_b = [d.get_seeds() for d in g.devs]
        ctr = [d.counters() for d in g.devs]
        assert g.frames() == sum(CALLS_B)
        assert (g.concurrency(), g.stream_class()) == (S, cls)
    finally:
        g.close()
    exp_a = exp_b = None
    for m in range(lanes):
        r, tag = ref[m], f"lanes={lanes} {knob} (class {cls}, S={S}) lane {m}"
        assert_bits(acc_a[m], r["acc_a"], tag + " accumulator after render(4), render(3)")
        assert np.array_equal(seeds_a[m], r["seeds_a"]), tag + " seeds after render(4), render(3)"
        assert_bits(acc_b[m], r["acc_b"], tag + " accumulator after reset, render(5)")
        assert np.array_equal(seeds_b[m], r["seeds_b"]), tag + " seeds after reset, render(5)"
        _ctr_vs_oracle(ctr[m], r["e"], r["c"], tag)
        exp_a = r["acc_a"] if exp_a is None else exp_a + r["acc_a"]
        exp_b = r["acc_b"] if exp_b is None else exp_b + r["acc_b"]
    assert_bits(sum_a, exp_a, f"lanes={lanes} {knob} (class {cls}, S={S}) group sum after render(4), render(3)")
    assert_bits(sum_b, exp_b, f"lanes={lanes} {knob} (class {cls}, S={S}) group sum after reset, render(5)")


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 8])
def test_auto_has_no_fewer_workers_than_normal_and_normal_is_the_lanes_own_streams(lanes, monkeypatch):
    got = []
    for knob in ("normal", "auto", None, "normal"):
        g = _group(lanes, knob, monkeypatch)
        try:
            got.append(_check_class(g, lanes, knob))
        finally:
            g.close()
    (n1, _, _), (a, _, seen_a), (u, cls_u, seen_u), (n2, _, _) = got
    assert n1 == n2, (n1, n2)                        # the lanes' own streams, measured the same way every time
    assert seen_a["normal"] == n1 and seen_u["normal"] == n1, (n1, seen_a, seen_u)
    assert a >= n1 and u >= n1, (n1, a, u)
    assert (u, cls_u, seen_u) == got[1], "unset is auto"


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["low", "high", "auto"])
def test_device_beside_a_group_renders_its_own_oracle_frames(knob, monkeypatch):
    """A single context keeps its normal-priority stream whatever class the group beside it took, and its frames are its own."""
    sa, cam = _scene_once()
    lanes, frames = 4, 2
    ref = _oracle_once(lanes)
    g = _group(lanes, knob, monkeypatch)
    d = None
    try:
        d = Device(Wd, Hd, **DEFAULT)
        g.upload(sa)
        g.seed(FIRST)
        d.upload(sa)
        d.seed_default()
        g.render(cam, CALLS_A[0])                    # both at work at once
        d.render(cam, frames)
        g.render(cam, CALLS_A[1])
        got = d.read_accum()
        acc = [x.read_accum() for x in g.devs]
    finally:
        if d is not None:
            d.close()
        g.close()
    assert_bits(got, _single_oracle(frames), f"Device beside a group of class {knob}")
    for m in range(lanes):
        assert_bits(acc[m], ref[m]["acc_a"], f"lane {m} of a group of class {knob} beside a Device")
