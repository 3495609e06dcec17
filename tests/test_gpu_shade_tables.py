"""k_shade reads the light records and the materials from tables its workgroups copy into LDS at the start of a launch, when ALL lights
(six 16-byte rows each) and ALL materials (three rows each) of the scene fit the rows reserved for them (rt_shade_tables), and from global
memory as before when they do not, or when RT355_SHADE_TABLES=0.  The rows are the same bits, so nothing the kernel writes may change.
What can go wrong is a row taken from the wrong place (a light's row for a material's, the wrong word of the 80-byte Material), a table
read before it is complete, a table of the previous upload, and the rule itself - so:

  every material kind   a scene small enough to be staged that reaches every branch of shade_hit (asserted from the oracle's own rays):
                        light hits with and without lastSpecular, a dielectric entered and left (absorption), a mirror, a textured triangle
                        and a textured sphere, a sphere light and a triangle light; under NEE and under Kajiya, for both tile sizes, on
                        frames of one tile, two tiles and a partial last tile - every exported queue, shadow record, seed and the
                        accumulator against the oracle, bit for bit.  The suite's branch scene (four lights, thirteen materials: too
                        many) runs the same comparison through the fallback.
  the capacity          the same geometry with exactly as many rows as fit, with one more material, and with RT355_SHADE_TABLES=0 in a
                        fresh process: one image.  One more LIGHT cannot give the same image under NEE (the light is drawn from nLights),
                        so that scene is held to the oracle under NEE and to the image of the others under Kajiya, where no light is drawn.
  no light at all under NEE, and a scene whose only material is a light.
  freshness             a second upload with other colours and specular values renders the oracle's frames for the new table.
  the footprint         beside the 256-slot kernel a CU still holds six traversal workgroups with 22-entry columns."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from hand_trees import hand_scene, ladder
from helpers import DEFAULT, assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group
from magr_ray_tracer_amd.scene import Scene, material
from magr_ray_tracer_amd.scenes import box_tris
from oracle.oracle_py import seed_stream

pytestmark = pytest.mark.gpu

FRAMES = 2
EPS = np.float32(1e-4)            # kEps
LIGHT_ROWS, MAT_ROWS = 6, 3       # 16-byte rows of the staged tables per light record / per material
KAJIYA = dict(DEFAULT, shading=0)
VARIANTS = {"nee": DEFAULT, "kajiya": KAJIYA}
# (width, height) per tile size: one tile exactly, two tiles, a partial last tile
SHAPES = {256: [(64, 4), (64, 8), (40, 13)], 512: [(64, 8), (64, 16), (40, 13)]}
VIEW = dict(origin=(0.0, 1.0, 5.6), forward=(0.0, 0.0, 1.0), fov=80.0, aperture=0.03)


def _textures(s):
    yy, xx = np.mgrid[0:16, 0:16]
    tex = np.zeros((16, 16, 4), dtype=np.float32)
    tex[..., 0] = 0.25 + 0.6 * ((xx // 2 + yy // 2) % 2)
    tex[..., 1] = 0.3 + 0.04 * xx
    tex[..., 2] = 0.85 - 0.04 * yy
    s.AddTexture("checker", tex)


def kinds_scene(extra_materials=0, extra_light=False):
    """scenes.branch_scene with what the tables have room for: six materials (diffuse, mirror, absorbing glass, a texture, two lights) and
    two lights, a sphere and an upright triangle, in a closed room with a textured floor.  extra_materials: unused materials behind
    the used ones; extra_light: a third light outside the room, which no ray reaches (but NEE draws it)."""
    s = Scene()
    s.AddMaterial("white", material(color=(0.8, 0.8, 0.8)))
    s.AddMaterial("mirror", material(color=(0.1, 0.1, 0.9), specular=0.5))
    s.AddMaterial("thick-glass", material(color=(1, 1, 1), dielectric=True, n1=1.0, n2=1.5, specular=0.04, absorption=(0.9, 0.25, 0.1)))
    s.AddMaterial("green-light", material(color=(0.1, 1.0, 0.1), light=True, emittance=(4, 40, 4)))
    s.AddMaterial("red-light", material(color=(1.0, 0.1, 0.1), light=True, emittance=(100, 10, 10)))
    _textures(s)
    for k in range(extra_materials):
        s.AddMaterial(f"unused-{k}", material(color=(0.9 - 0.01 * k, 0.5, 0.01 * k), specular=0.25))
    s.AddTriangle((-6, 0, -5), (-6, 0, 6), (6, 0, 6), "checker", uv0=(0, 0), uv1=(0, 4), uv2=(4, 4))
    s.AddTriangle((6, 0, 6), (6, 0, -5), (-6, 0, -5), "checker", uv0=(4, 4), uv1=(4, 0), uv2=(0, 0))
    s.AddQuad((-6, 0, -5), (6, 0, -5), (6, 4, -5), (-6, 4, -5), "white")
    s.AddQuad((-6, 0, -5), (-6, 4, -5), (-6, 4, 6), (-6, 0, 6), "white")
    s.AddQuad((6, 0, -5), (6, 0, 6), (6, 4, 6), (6, 4, -5), "white")
    s.AddQuad((-6, 4, -5), (6, 4, -5), (6, 4, 6), (-6, 4, 6), "white")
    s.AddQuad((-6, 0, 6), (-6, 4, 6), (6, 4, 6), (6, 0, 6), "white")
    s.AddTriangles(box_tris((-4.6, 0.3, -0.7), (-3.2, 1.7, 0.7)), "thick-glass")
    s.AddSphere((-2.2, 1.0, 0.0), 0.7, "checker")
    s.AddSphere((-0.6, 1.0, 0.2), 0.7, "mirror")
    s.AddSphere((0.7, 1.0, -0.3), 0.35, "green-light")
    s.AddTriangle((1.4, 0.5, -1.0), (2.4, 0.5, -1.0), (1.9, 1.6, -1.0), "red-light")          # upright, faces +z (the camera)
    s.AddSphere((3.0, 1.0, 0.1), 0.65, "thick-glass")
    s.AddSphere((4.5, 1.0, 0.0), 0.7, "white")
    if extra_light:
        s.AddTriangle((20, 0.5, -1.0), (21, 0.5, -1.0), (20.5, 1.6, -1.0), "red-light")
    s.BuildBLAS(0, 1.0)
    return s, VIEW


def open_scene():
    """No light at all: a floor and two spheres under the sky (NEE finds nLights == 0 at every diffuse hit)."""
    s = Scene()
    s.AddMaterial("sand", material(color=(0.72, 0.62, 0.45)))
    s.AddMaterial("mirror", material(color=(0.1, 0.1, 0.9), specular=0.5))
    s.AddQuad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), "sand")
    s.AddSphere((-0.8, 0.7, 0.0), 0.7, "mirror")
    s.AddSphere((0.9, 0.6, 0.5), 0.6, "sand")
    s.BuildBLAS(0, 1.0)
    return s, dict(origin=(0.0, 1.2, 4.0), forward=(0.0, 0.1, 1.0), fov=70.0, aperture=0.0)


def lights_only_scene():
    """The only material is a light: every hit is an emissive hit of a primary ray, everything else is sky."""
    s = Scene()
    s.AddMaterial("white-light", material(color=(1.0, 0.7, 0.1), light=True, emittance=(3, 2, 1)))
    s.AddQuad((-1, 0, -1), (1, 0, -1), (1, 2, -1), (-1, 2, -1), "white-light")
    s.AddSphere((1.8, 1.0, -0.5), 0.5, "white-light")
    s.BuildBLAS(0, 1.0)
    return s, dict(origin=(0.5, 1.0, 1.5), forward=(0.0, 0.0, 1.0), fov=80.0, aperture=0.0)


_SC = {}


def _scene(name):
    """(scene arrays, view) of a named scene, built once; the Scene object is kept because the arrays are views of its memory."""
    if name not in _SC:
        if name.startswith("kinds"):      # "kinds+<extra materials>[+light]"
            parts = name.split("+")
            s, view = kinds_scene(int(parts[1]) if len(parts) > 1 else 0, "light" in parts[2:])
        else:
            s, view = {"branch": scenes.branch_scene, "open": open_scene, "lights-only": lights_only_scene, "cube": scenes.cube_scene}[name]()
        _SC[name] = (s, s.arrays(), view)
    return _SC[name][1], _SC[name][2]


def rows_of(sa):
    return LIGHT_ROWS * len(sa.lights) + MAT_ROWS * len(sa.mats)


_REF = {}


def _reference(key, sa, view, Wd, Hd, variant):
    """The oracle's frames, stage by stage: per frame and bounce the rays extend leaves, the queue shade leaves and its shadow records,
    and per frame the accumulator and the RNG states after connect.  Computed once per key."""
    if key not in _REF:
        cam = scenes.camera_for(view, Wd, Hd)
        n = Wd * Hd
        o = oracle_for(sa, Wd, Hd, **variant)
        seeds = seed_stream(0, n)
        acc = np.zeros((n, 4), np.float32)
        frames = []
        for _ in range(FRAMES):
            rays = o.generate(cam, 0, n, seeds)
            ins, outs, shadows = [], [], []
            for b in range(W.MAX_BOUNCES):
                o.extend(rays)
                ins.append(rays.copy())
                rays, sh = o.shade(rays, acc, seeds)
                outs.append(rays.copy())
                shadows.append(sh)
            if variant["shading"] == 1:
                o.connect(np.concatenate(shadows), acc)
            frames.append(dict(ins=ins, outs=outs, shadows=shadows, acc=acc.copy(), seeds=seeds.copy()))
        _REF[key] = (cam, frames)
    return _REF[key]


def _same_frames(d, ref, Wd, Hd, what):
    cam, frames = ref
    n = Wd * Hd
    d.set_seeds(seed_stream(0, n))
    d.reset()
    for f, want_f in enumerate(frames):
        d.stage_begin_frame()
        d.stage_generate(cam)
        for b in range(W.MAX_BOUNCES):
            w = f"{what}: frame {f} bounce {b}"
            d.stage_extend(b)
            d.stage_shade(b)
            out, want = d.get_rays(b + 1), want_f["outs"][b]
            assert len(out) == len(want), f"{w}: nRays {len(out)}, oracle {len(want)}"
            for k in ("pixelIdx", "bounces", "inside", "lastSpecular"):
                assert np.array_equal(out[k], want[k]), f"{w}: extension rays differ in {k}"
            for k in ("O", "D", "intensity"):
                assert_bits(out[k], want[k], f"{w}: extension rays {k}")
            rec, sh = d.get_shadow(b, b), want_f["shadows"][b]
            assert len(rec) == len(sh), f"{w}: nShadow grows by {len(rec)}, oracle {len(sh)}"
            if len(sh):
                assert np.array_equal(rec["pixelIdx"], sh["pixelIdx"]), f"{w}: shadow records differ in pixelIdx"
                assert_bits(rec["tmax"], sh["dist"] - np.float32(2) * EPS, f"{w}: shadow records tmax")
                assert_bits(rec["l"], sh["L"][:, :3], f"{w}: shadow records l")
                assert_bits(rec["o"], (sh["I"] + sh["L"] * EPS)[:, :3], f"{w}: shadow records o")
        if int(d.cfg["shading"]) == W.SHADING_NEE:
            d.stage_connect(0, W.MAX_BOUNCES - 1)
        assert_bits(d.read_accum().reshape(-1, 4), want_f["acc"], f"{what}: accumulator after frame {f}")
        assert np.array_equal(d.get_seeds(), want_f["seeds"]), f"{what}: seeds after frame {f}"


class _Ctx:
    """A context with 256-slot tiles (lane 0 of a group of two) or with 512-slot tiles (a context alone), the scene uploaded."""

    def __init__(self, tile, Wd, Hd, sa, variant):
        self.g = Group(Wd, Hd, lanes=2, **variant) if tile == 256 else None
        self.d = None
        try:
            if self.g is not None:
                self.g.upload(sa)
                self.d = self.g.devs[0]
            else:
                self.d = Device(Wd, Hd, **variant)
                self.d.upload(sa)
        except Exception:
            self.close()
            raise

    def __enter__(self):
        return self.d

    def close(self):
        if self.g is not None:
            self.g.close()
        elif self.d is not None:
            self.d.close()

    def __exit__(self, *exc):
        self.close()


def branches(sa, frames):
    """How often the oracle's own rays took each branch of shade_hit."""
    c = dict(light_spec=0, light_nospec=0, inside_dielectric=0, mirror=0, tex_tri=0, tex_sphere=0, sphere_light_shadow=0, tri_light_shadow=0)
    for fr in frames:
        for rays in fr["ins"]:
            hit = rays["primIdx"] != -1
            p = sa.prims[np.where(hit, rays["primIdx"], 0)]
            m = sa.mats[p["matIdx"]]
            light = hit & (m["isLight"] != 0)
            c["light_spec"] += int((light & (rays["lastSpecular"] != 0)).sum())
            c["light_nospec"] += int((light & (rays["lastSpecular"] == 0)).sum())
            c["inside_dielectric"] += int((hit & (rays["inside"] != 0) & (m["isDielectric"] != 0)).sum())
            c["mirror"] += int((hit & ~light & (m["isDielectric"] == 0) & (m["specular"] > 0)).sum())
            tex = hit & (m["texIdx"] != -1) & ~light
            c["tex_tri"] += int((tex & (p["objType"] == W.PRIM_TRIANGLE)).sum())
            c["tex_sphere"] += int((tex & (p["objType"] == W.PRIM_SPHERE)).sum())
        for sh in fr["shadows"]:
            if len(sh):
                t = sa.prims["objType"][sh["lightIdx"]]
                c["sphere_light_shadow"] += int((t == W.PRIM_SPHERE).sum())
                c["tri_light_shadow"] += int((t == W.PRIM_TRIANGLE).sum())
    return c


# ---- every material kind ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shading", list(VARIANTS))
@pytest.mark.parametrize("tile,Wd,Hd", [(t, w, h) for t in SHAPES for (w, h) in SHAPES[t]])
def test_every_material_kind_from_the_staged_tables(tile, Wd, Hd, shading):
    variant = VARIANTS[shading]
    sa, view = _scene("kinds")
    ref = _reference(("kinds", Wd, Hd, shading), sa, view, Wd, Hd, variant)
    # the frames of this tile size together reach every branch (a primary ray meets a light in a few pixels only)
    c = {}
    for w, h in SHAPES[tile]:
        for k, v in branches(sa, _reference(("kinds", w, h, shading), sa, view, w, h, variant)[1]).items():
            c[k] = c.get(k, 0) + v
    if shading == "kajiya":
        assert c.pop("sphere_light_shadow") == c.pop("tri_light_shadow") == 0
    assert all(v > 0 for v in c.values()), (c, "the frames do not reach every branch")
    with _Ctx(tile, Wd, Hd, sa, variant) as d:
        cap, staged = d.shade_tables()
        assert rows_of(sa) <= cap and staged
        _same_frames(d, ref, Wd, Hd, f"kinds {Wd}x{Hd}, {tile}-slot tiles, {shading}")


@pytest.mark.parametrize("shading", list(VARIANTS))
@pytest.mark.parametrize("tile", [256, 512])
def test_a_scene_too_large_for_the_tables_reads_global_memory_as_before(tile, shading):
    Wd, Hd = 40, 13
    variant = VARIANTS[shading]
    sa, view = _scene("branch")
    ref = _reference(("branch", Wd, Hd, shading), sa, view, Wd, Hd, variant)
    with _Ctx(tile, Wd, Hd, sa, variant) as d:
        cap, staged = d.shade_tables()
        assert rows_of(sa) > cap and not staged
        _same_frames(d, ref, Wd, Hd, f"branch {Wd}x{Hd}, {tile}-slot tiles, {shading}")


# ---- the capacity -------------------------------------------------------------------------------------------------------------------------
def _render(d, cam, n):
    d.set_seeds(seed_stream(0, n))
    d.reset()
    d.render(cam, FRAMES)
    d.synchronize()
    return d.read_accum().reshape(-1, 4).copy()


def _padding(cap):
    """Unused materials that fill the rows exactly beside the two lights and six materials of kinds_scene."""
    sa, _ = _scene("kinds")
    spare = cap - rows_of(sa)
    assert spare >= 0 and spare % MAT_ROWS == 0, (cap, rows_of(sa))
    return spare // MAT_ROWS


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {tests!r})
import test_gpu_shade_tables as T
sa, view = T._scene({name!r})
with T._Ctx({tile}, {Wd}, {Hd}, sa, T.VARIANTS[{shading!r}]) as d:
    staged = d.shade_tables()[1]
    acc = T._render(d, T.scenes.camera_for(view, {Wd}, {Hd}), {Wd} * {Hd})
np.savez({out!r}, acc=acc, staged=staged)
"""


@pytest.mark.parametrize("tile", [256, 512])
def test_at_the_capacity_and_one_past_it_the_image_is_the_same(tile, tmp_path):
    Wd, Hd = 40, 13
    n = Wd * Hd
    with _Ctx(tile, Wd, Hd, _scene("kinds")[0], DEFAULT) as d:
        cap = d.shade_tables()[0]
    pad = _padding(cap)
    full, more_mats, more_lights = f"kinds+{pad}", f"kinds+{pad + 1}", f"kinds+{pad}+light"
    assert rows_of(_scene(full)[0]) == cap
    assert rows_of(_scene(more_mats)[0]) == cap + MAT_ROWS and rows_of(_scene(more_lights)[0]) == cap + LIGHT_ROWS
    img = {}
    for shading, variant in VARIANTS.items():
        for name, fits in ((full, True), (more_mats, False), (more_lights, False)):
            sa, view = _scene(name)
            with _Ctx(tile, Wd, Hd, sa, variant) as d:
                assert d.shade_tables() == (cap, fits), (name, d.shade_tables())
                if name == more_lights and shading == "nee":      # NEE draws among three lights: another image, the oracle's
                    _same_frames(d, _reference((name, Wd, Hd, shading), sa, view, Wd, Hd, variant), Wd, Hd, f"{name}, {tile}-slot tiles")
                else:
                    img[shading, name] = _render(d, scenes.camera_for(view, Wd, Hd), n)
        sa, view = _scene(full)
        assert_bits(img[shading, full], _reference((full, Wd, Hd, shading), sa, view, Wd, Hd, variant)[1][-1]["acc"], f"{shading}: at the capacity, oracle")
        assert img[shading, full][:, :3].sum() > 0
        assert_bits(img[shading, more_mats], img[shading, full], f"{shading}: one more material")
    assert_bits(img["kajiya", more_lights], img["kajiya", full], "kajiya: one more light")
    # the same scene with the knob, in a fresh process
    out = str(tmp_path / "child.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD.format(tests=here, name=full, tile=tile, Wd=Wd, Hd=Hd, shading="nee", out=out)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, cwd=os.path.dirname(here), env=dict(os.environ, RT355_SHADE_TABLES="0"))
    child = np.load(out)
    assert not bool(child["staged"])
    assert_bits(child["acc"], img["nee", full], "RT355_SHADE_TABLES=0")


# ---- no light, nothing but lights -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["open", "lights-only"])
@pytest.mark.parametrize("tile", [256, 512])
def test_no_light_at_all_and_nothing_but_lights(tile, name):
    Wd, Hd = 40, 13
    sa, view = _scene(name)
    assert len(sa.lights) == (0 if name == "open" else 3) and len(sa.mats) == (2 if name == "open" else 1)
    ref = _reference((name, Wd, Hd, "nee"), sa, view, Wd, Hd, DEFAULT)
    assert ref[1][-1]["acc"][:, :3].sum() > 0
    if name == "lights-only":
        assert branches(sa, ref[1])["light_spec"] > 0
    with _Ctx(tile, Wd, Hd, sa, DEFAULT) as d:
        assert d.shade_tables()[1]
        _same_frames(d, ref, Wd, Hd, f"{name}, {tile}-slot tiles")


# ---- freshness --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [256, 512])
def test_a_second_upload_with_another_material_table_is_what_the_next_frame_reads(tile):
    Wd, Hd = 40, 13
    sa, view = _scene("kinds")
    mats = sa.mats.copy()
    plain = (mats["isLight"] == 0) & (mats["isDielectric"] == 0)
    mats["color"][plain, :3] = (np.float32(1.0) - mats["color"][plain, :3]) * np.float32(0.9)
    mats["specular"][plain] = np.where(mats["specular"][plain] > 0, np.float32(0.125), np.float32(0.375))
    sb = dataclasses.replace(sa, mats=mats)
    first = _reference(("kinds", Wd, Hd, "nee"), sa, view, Wd, Hd, DEFAULT)
    second = _reference(("kinds-recoloured", Wd, Hd, "nee"), sb, view, Wd, Hd, DEFAULT)
    assert not np.array_equal(first[1][-1]["acc"], second[1][-1]["acc"])
    with _Ctx(tile, Wd, Hd, sa, DEFAULT) as d:
        _same_frames(d, first, Wd, Hd, f"first table, {tile}-slot tiles")
        d.upload(sb)
        assert d.shade_tables()[1]
        _same_frames(d, second, Wd, Hd, f"second table, {tile}-slot tiles")
        d.upload(sa)
        _same_frames(d, first, Wd, Hd, f"first table again, {tile}-slot tiles")


# ---- the footprint ----------------------------------------------------------------------------------------------------------------------
def test_six_traversal_workgroups_still_fit_beside_the_256_slot_kernel(monkeypatch):
    """22-entry columns are 22,528 B = eighteen 1,280-B blocks; six of them leave twenty blocks, 25,600 B, of a CU's 163,840."""
    monkeypatch.delenv("RT355_TOP_LEVELS", raising=False)
    monkeypatch.delenv("RT355_TUNE", raising=False)
    g = Group(64, 48, lanes=2, **DEFAULT)
    try:
        g.upload(hand_scene(22, ladder(list(range(22)))))
        lane = g.devs[0]
        assert lane.kernel_info()["stack_entries"] == 22 and lane.kernel_info()["persist"] == 1
        lds, beside = lane.shade_footprint()
        assert 0 < lds <= 25600 and beside == 6
    finally:
        g.close()
    # the bench scene's tables - ten materials, one emissive quad - are what the rows were sized for
    sa, _ = _scene("cube")
    with _Ctx(256, 64, 48, sa, DEFAULT) as d:
        cap, staged = d.shade_tables()
        assert (len(sa.lights), len(sa.mats)) == (2, 10) and rows_of(sa) <= cap and staged
