"""RtConfig.builtins without a GPU: the layout of the word on both sides of the C-ABI, the host Renderer mirror's setting, and the
Python front ends' argument check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from magr_ray_tracer_amd import _lib as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_dtype_names_the_word_at_byte_60():
    assert W.Config.itemsize == 64
    assert W.Config.fields["builtins"][1] == 60 and W.Config.fields["builtins"][0] == np.dtype("<i4")
    assert W.Config.names[-1] == "builtins" and "reserved" not in W.Config.names
    assert (W.BUILTINS_DEFAULT, W.BUILTINS_IEEE, W.BUILTINS_REFERENCE) == (0, 1, 2)
    assert np.zeros((), W.Config)["builtins"] == W.BUILTINS_DEFAULT       # a zero-filled struct asks for the default


def test_sizeof_rtconfig_as_compiled(tmp_path):
    src = tmp_path / "cfg.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "rt355.h"\n'
                   'int main() { printf("%zu %zu %d %d %d\\n", sizeof(RtConfig), offsetof(RtConfig, builtins), RT_BUILTINS_DEFAULT, RT_BUILTINS_IEEE, RT_BUILTINS_REFERENCE); }\n')
    exe = tmp_path / "cfg"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["64", "60", "0", "1", "2"]


def test_new_entry_points_are_exported():
    import subprocess as sp
    out = sp.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "magr_ray_tracer_amd", "librt355.so")], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"rt_builtins", "rt_debug_math_mode", "rt_debug_math_sweep_mode"} <= names
    out = sp.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "magr_ray_tracer_amd", "librt355_host.so")], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"rth_renderer_set_builtins", "rth_renderer_builtins"} <= names


def test_host_renderer_mirror_stores_the_setting_and_refuses_unknown_values():
    from magr_ray_tracer_amd import scenes
    L = W.host_lib()
    s, _ = scenes.cube_scene()
    h = L.rth_renderer_create(s._h, 64, 36, 0, 0, -1, 1, 1, 0, 1, 1)
    assert h
    try:
        assert L.rth_renderer_builtins(h) == W.BUILTINS_DEFAULT
        for mode in (W.BUILTINS_REFERENCE, W.BUILTINS_IEEE, W.BUILTINS_DEFAULT, W.BUILTINS_REFERENCE):
            assert L.rth_renderer_set_builtins(h, mode) == 0
            assert L.rth_renderer_builtins(h) == mode
        for bad in (3, -1, 1 << 20):
            assert L.rth_renderer_set_builtins(h, bad) == -1
            assert b"builtins" in L.rth_last_error()
            assert L.rth_renderer_builtins(h) == W.BUILTINS_REFERENCE        # unchanged
        assert L.rth_renderer_set_builtins(None, W.BUILTINS_IEEE) == -1
    finally:
        L.rth_renderer_destroy(h)


def test_python_front_ends_refuse_unknown_names_before_any_library_call(monkeypatch):
    from magr_ray_tracer_amd import renderer

    def no_library(*a, **k):
        raise AssertionError("a native library was loaded before the argument was checked")
    monkeypatch.setattr(W, "device_lib", no_library)
    monkeypatch.setattr(W, "host_lib", no_library)
    for bad in ("bogus", "IEEE", 2, b"reference"):
        with pytest.raises(ValueError, match="builtins"):
            renderer.Device(64, 36, builtins=bad)
        with pytest.raises(ValueError, match="builtins"):
            renderer.Group(64, 36, lanes=2, builtins=bad)
        with pytest.raises(ValueError, match="builtins"):
            renderer.Renderer(None, 64, 36, builtins=bad)
    assert [W.builtins_value(n) for n in (None, "ieee", "reference")] == [0, 1, 2]
