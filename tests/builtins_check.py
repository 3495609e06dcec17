"""Helpers of tests/test_gpu_builtins.py: contexts of the shipped library in either arithmetic (RtConfig.builtins) beside the second
library (librt355_refb.so, whose RT_BUILTINS_DEFAULT is REFERENCE), compared as bytes."""
import ctypes as C

import numpy as np

from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.renderer import Device

IEEE, REFERENCE = 1, 2          # RT_BUILTINS_IEEE, RT_BUILTINS_REFERENCE (include/rt355.h)
BUILTINS_WORD = 15              # RtConfig is sixteen int32 words; `builtins` is the last one (byte 60)
CONFIG_WORDS = ("width", "height", "y0", "y1", "max_bounces", "shading", "sampling", "accel", "russian_roulette", "filter_fireflies",
                "device", "extend_variant", "profile", "shade_blocks_per_cu", "persist_blocks_per_cu")


def raw_config(width, height, word15, shading=1, sampling=1, accel=0, russian_roulette=True, filter_fireflies=True, **more):
    """An RtConfig as sixteen raw int32 words: the fifteen named ones and `word15` in the place of RtConfig.builtins."""
    v = dict(width=width, height=height, y0=0, y1=height, max_bounces=W.MAX_BOUNCES, shading=shading, sampling=sampling, accel=accel,
             russian_roulette=int(russian_roulette), filter_fireflies=int(filter_fireflies), **more)
    words = np.zeros(16, np.int32)
    for i, n in enumerate(CONFIG_WORDS):
        words[i] = v.get(n, 0)
    words[BUILTINS_WORD] = word15
    return words


def raw_create(words):
    """rt_create through ctypes with the raw words -> (rc, handle, error message)."""
    L = W.device_lib()
    h = C.c_void_p()
    rc = L.rt_create(words.ctypes.data_as(C.c_void_p), C.byref(h))
    return rc, h, L.rt_last_error().decode()


class RawDevice:
    """A context created from raw config words, with the methods of Device (a borrowed view; destroyed here)."""

    def __init__(self, words):
        rc, h, msg = raw_create(words)
        assert rc == 0, msg
        self._words = words
        self.dev = Device.borrowed(h.value, words.view(W.Config)[0])
        self._handle = h

    def close(self):
        if self._handle:
            self.dev._h = None
            W.device_lib().rt_destroy(self._handle)
            self._handle = None


def frame_state(d):
    """What a render leaves behind: accumulator, per-slot seeds, the seven queue lengths."""
    return d.read_accum(), d.get_seeds(), [len(d.get_rays(b)) for b in range(W.MAX_BOUNCES)]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        wa, wb = np.frombuffer(a.tobytes(), np.uint8), np.frombuffer(b.tobytes(), np.uint8)
        bad = np.flatnonzero(wa != wb)
        raise AssertionError(f"{what}: {bad.size} of {wa.size} bytes differ, first at byte {int(bad[0])}")


def ctr_equal(dev, e, c):
    """The extend and the connect counters equal the oracle's (e, c of helpers.oracle_for): tests/test_gpu_parity.py _ctr_equal."""
    for k in ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests"):
        assert dev["extend_" + k] == e[k], ("extend_" + k, dev["extend_" + k], e[k])
    for k in ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests"):
        assert dev["connect_" + k] == c[k], ("connect_" + k, dev["connect_" + k], c[k])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def math_mode(mode, fn, words, variant=None):
    """rt_debug_math_mode(mode, ...) of the shipped library, or rt_debug_math of a variant library when mode is None -> (rc, out)."""
    L = W.device_lib(variant)
    wi, wo = W.MATH_WORDS[fn]
    a = np.ascontiguousarray(words, np.uint32).reshape(-1, wi)
    out = np.zeros((len(a), wo), np.uint32)
    if mode is None:
        rc = L.rt_debug_math(fn, _p(a), _p(out), len(a))
    else:
        rc = L.rt_debug_math_mode(mode, fn, _p(a), _p(out), len(a))
    return rc, out


def sweep_mode(mode, fn, variant=None):
    L = W.device_lib(variant)
    h = np.zeros(1 << (32 - W.MATH_SWEEP_BLOCK_BITS), np.uint64)
    if mode is None:
        rc = L.rt_debug_math_sweep(fn, 0, len(h), _p(h))
    else:
        rc = L.rt_debug_math_sweep_mode(mode, fn, 0, len(h), _p(h))
    return rc, h
