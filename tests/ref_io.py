"""TEST INFRASTRUCTURE: ctypes binding of oracle/_ref/libref_io.so - the reference's own asset readers (its vendored stb_image,
stb_image_write and tinyobjloader headers compiled where they lie by oracle/build_ref.sh behind oracle/ref_io_runner.cpp).

Where that library is not built, every call is answered from tests/golden/io_replay.npz: what the library returned for the same
input, keyed by a hash of the input files' bytes and the arguments (tests/golden/make_io_replay.py records it by running the tests
with the library present).  An input the fixture does not hold is an error, not a skip."""
import atexit
import ctypes as C
import hashlib
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_io.so")
_REPLAY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io_replay.npz")
_RECORD = os.environ.get("REF_IO_RECORD")      # make_io_replay.py: write every answer of the library to this npz at exit
_lib = None
_replay = None
_recorded = {}


def available():
    return live() or os.path.exists(_REPLAY)


def live():
    return os.path.exists(_PATH)


def _key(fn, files, *args):
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(str(f)).encode() + b"\0" + open(f, "rb").read() + b"\0")
    return f"{fn}|{h.hexdigest()[:32]}|{args!r}"


def _dir_files(path):
    d = os.path.dirname(str(path))
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))]


def _answer(key, call):
    """call() -> {name: array} through the library (recorded when asked), or the stored answer for `key`; a stored RuntimeError
    is raised again."""
    global _replay
    if live():
        try:
            out = call()
        except RuntimeError as e:
            out = {"error": np.array(str(e))}
        if _RECORD:
            _recorded.update({f"{key}|{k}": v for k, v in out.items()})
    else:
        if _replay is None:
            _replay = np.load(_REPLAY)
        out = {k[len(key) + 1:]: _replay[k] for k in _replay.files if k.startswith(key + "|")}
        if not out:
            raise AssertionError(f"{key}: no stored answer of the reference readers for this input (regenerate "
                                 "tests/golden/io_replay.npz with tests/golden/make_io_replay.py)")
    if "error" in out:
        raise RuntimeError(str(out["error"]))
    return out


@atexit.register
def _save_record():
    if _RECORD and _recorded:
        np.savez_compressed(_RECORD, **_recorded)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_PATH)
        L.ref_io_last_error.restype = C.c_char_p
        ip = C.POINTER(C.c_int)
        L.ref_load_image_f.argtypes = [C.c_char_p, ip, ip, ip, C.c_void_p]
        L.ref_load_image_u8.argtypes = [C.c_char_p, ip, ip, ip, C.c_void_p]
        L.ref_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        L.ref_obj_load.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_float, C.c_float, C.c_int]
        L.ref_obj_faces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        for f in (L.ref_obj_tex_name, L.ref_obj_material_name, L.ref_obj_material_diffuse):
            f.restype, f.argtypes = C.c_char_p, [C.c_int]
        _lib = L
    return _lib


def _err():
    return lib().ref_io_last_error().decode()


def load_image_f(path):
    """The reference's LoadImageF (template/template.cpp:1613-1627): (h, w, 3) float32 and stb's channel count."""
    out = _answer(_key("load_image_f", [path]), lambda: dict(zip(("texels", "channels"), _load_image_f(path))))
    return out["texels"], int(out["channels"])


def _load_image_f(path):
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    if lib().ref_load_image_f(str(path).encode(), w, h, c, None) != 0:
        raise RuntimeError(_err())
    out = np.zeros((h.value, w.value, 3), np.float32)
    if lib().ref_load_image_f(str(path).encode(), w, h, c, out.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError(_err())
    return out, c.value


def load_image_u8(path):
    return _answer(_key("load_image_u8", [path]), lambda: {"pixels": _load_image_u8(path)})["pixels"]


def _load_image_u8(path):
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    if lib().ref_load_image_u8(str(path).encode(), w, h, c, None) != 0:
        raise RuntimeError(_err())
    out = np.zeros((h.value, w.value, c.value), np.uint8)
    if lib().ref_load_image_u8(str(path).encode(), w, h, c, out.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError(_err())
    return out


def write_png(path, rgb8):
    a = np.ascontiguousarray(rgb8, np.uint8)
    key = f"write_png|{hashlib.sha256(a.tobytes()).hexdigest()[:32]}|{a.shape!r}"
    data = _answer(key, lambda: {"file": _write_png(path, a)})["file"]
    with open(path, "wb") as f:
        f.write(data.tobytes())


def _write_png(path, a):
    if lib().ref_write_png(str(path).encode(), a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError("stbi_write_png failed")
    return np.fromfile(path, np.uint8)


def obj_load(path, default_mat="white", pos=(0.0, 0.0, 0.0), force_default=False):
    """Scene::LoadModel (src/scene.cpp:178-243) up to the AddTriangle calls: per triangle the face's `vertices` list after
    std::reverse (+ pos) as (n, 3, 3), its `texcoords` list as (n, 3, 2), the `tex` string as an index into `tex_names`; plus the
    MTL materials (name, diffuse_texname) whose images LoadModel loads first."""
    key = _key("obj_load", _dir_files(path), os.path.basename(str(path)), default_mat, tuple(float(x) for x in pos), bool(force_default))
    out = _answer(key, lambda: _pack_obj(_obj_load(path, default_mat, pos, force_default)))
    return dict(verts=out["verts"], uvs=out["uvs"], tex=out["tex"], tex_names=[str(x) for x in out["tex_names"]],
                materials=[(str(a), str(b)) for a, b in out["materials"].reshape(-1, 2)])


def _pack_obj(r):
    return dict(verts=r["verts"], uvs=r["uvs"], tex=r["tex"], tex_names=np.array(r["tex_names"], dtype=str),
                materials=np.array(r["materials"], dtype=str).reshape(-1, 2))


def _obj_load(path, default_mat, pos, force_default):
    L = lib()
    n = L.ref_obj_load(str(path).encode(), default_mat.encode(), pos[0], pos[1], pos[2], int(force_default))
    if n < 0:
        raise RuntimeError(_err())
    v, uv, tex = np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32)
    L.ref_obj_faces(v.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p))
    names = [L.ref_obj_tex_name(i).decode() for i in range(L.ref_obj_tex_count())]
    mtl = [(L.ref_obj_material_name(i).decode(), L.ref_obj_material_diffuse(i).decode()) for i in range(L.ref_obj_material_count())]
    return dict(verts=v, uvs=uv, tex=tex, tex_names=names, materials=mtl)
