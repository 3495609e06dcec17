"""Cost of an in-place material update (rt_update_materials) against the full upload it removes, on one GPU.

    python tools/materials_bench.py [--reps 10]

For sponza-class and config 5, three changes are timed in one process, each alternating between two states (min / median / max of --reps
after a warm-up that visits both states three times, after which an update allocates nothing), against rt_upload_scene of the same final
scene into a second context - host validation, derivation and upload of every array, the only way before this call existed:
  table    the whole material table, with the emittance of every light and a colour changed and one light material switched off and on
           (so the light list and the light records are derived anew on the device);
  texels   a 1024 x 1024 texture written from a torch tensor on the GPU into an atlas that holds it (bound once, before the timing, by
           an update that lengthens the atlas and points a material at the window); the upload's column includes bringing the tensor to
           the host (texels_to_host_ms says how much of it that is);
  primMat  the matIdx of the first tenth of the primitives, as a numpy array.
The first repetition of each checks that the second context's device arrays - table, atlas and light list included - equal the
updated context's.  One JSON line per scene and change.  No ratio is promised: the line holds both columns."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rebuild_bench as RBB  # noqa: E402
from magr_ray_tracer_amd import _lib as W, scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Device  # noqa: E402
from magr_ray_tracer_amd.scene import light_list  # noqa: E402

RW, RH = 1280, 720
ARRAYS = list(W.SCENE_ARRAYS) + list(W.SCENE_ARRAYS_RESIZE) + list(W.SCENE_ARRAYS_MATERIALS)
TEX = 1024


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, what, dA, d2, states, reps, upload_of):
    """states: two keyword sets of Device.update_materials; upload_of(k): (SceneArrays after state k, ms spent bringing data to the host)."""
    allocs = []
    for k in range(6):
        dA.update_materials(**states[(k + 1) % 2])
        allocs.append(dA.rebuild_allocations())
    d2.upload(upload_of(1)[0])
    A, Ag, B, H = [], [], [], []
    same = None
    for r in range(reps):
        k = (r + 1) % 2
        ms, st = timed(lambda: dA.update_materials(**states[k]))
        A.append(ms)
        Ag.append(st["gpu_ms"])

        def full():
            sa, host_ms = upload_of(k)
            d2.upload(sa)
            return host_ms
        ms, host_ms = timed(full)
        B.append(ms)
        H.append(host_ms)
        if r == 0:
            same = all(np.array_equal(dA.scene_array(a), d2.scene_array(a)) for a in ARRAYS)
    print(json.dumps({"scene": name, "change": what, "update_wall_ms": RBB.mmm(A), "update_gpu_ms": RBB.mmm(Ag), "upload_wall_ms": RBB.mmm(B),
                      "texels_to_host_ms": RBB.mmm(H), "lights": st["lights"], "arrays_equal": same, "allocations_warm_up": allocs,
                      "allocations_measured": dA.rebuild_allocations() - allocs[-1]}), flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    for name, make in (("sponza_class", lambda: scenes.sponza_class(1.0)), ("config5", lambda: scenes.config5_scene(0.0))):
        s, _ = make()
        sa = s.arrays(bvh4=False)
        n, lit = len(sa.prims), np.flatnonzero(sa.mats["isLight"] != 0)
        dA, d2 = Device(RW, RH), Device(320, 240)
        dA.upload(sa)
        # ---- the table
        tables = [sa.mats.copy(), sa.mats.copy()]
        tables[1]["emittance"][lit] *= np.float32(0.5)
        tables[1]["color"][0] = (0.9, 0.2, 0.2, 0.0)
        if len(lit) > 1:
            tables[1]["isLight"][lit[-1]] = 0
        after = [dataclasses.replace(sa, mats=t, lights=light_list(sa.prims, t)) for t in tables]
        measure(name, "table", dA, d2, [dict(mats=t) for t in tables], a.reps, lambda k: (after[k], 0.0))
        # ---- a 1024 x 1024 texture from a torch tensor
        base = len(sa.tex)
        mats = sa.mats.copy()
        plain = int(np.flatnonzero((mats["texIdx"] == -1) & (mats["isLight"] == 0))[0])
        mats["texIdx"][plain], mats["texW"][plain], mats["texH"][plain] = base, TEX, TEX
        dA.update_materials(mats=mats, n_texels=base + TEX * TEX)
        rng = np.random.default_rng(1)
        frames = [torch.from_numpy(rng.uniform(0, 1, (TEX * TEX, 4)).astype(np.float32)).to("cuda:0") for _ in range(2)]
        old = np.asarray(sa.tex, np.float32).reshape(-1, 4)

        def with_frame(k):
            ms, host = timed(lambda: frames[k].cpu().numpy())
            return dataclasses.replace(after[0], mats=mats, tex=np.concatenate([old, host])), ms
        measure(name, "texels 1024x1024 (torch)", dA, d2, [dict(texels=f, tex_first=base) for f in frames], a.reps, with_frame)
        # ---- the matIdx of a tenth of the primitives
        dA.update_materials(mats=sa.mats, n_texels=base)
        tenth = max(n // 10, 1)
        assign = [sa.prims["matIdx"][:tenth].copy(), np.roll(sa.prims["matIdx"][:tenth], 1) if len(lit) == 0 else np.full(tenth, plain, np.int32)]
        assign[1][::97] = lit[0] if len(lit) else assign[1][::97]         # some of them become lights
        prims = [sa.prims.copy(), sa.prims.copy()]
        prims[1]["matIdx"][:tenth] = assign[1]
        painted = [dataclasses.replace(sa, prims=p, lights=light_list(p, sa.mats)) for p in prims]
        measure(name, f"primMat of {tenth} primitives", dA, d2, [dict(prim_mat=m, prim_first=0) for m in assign], a.reps, lambda k: (painted[k], 0.0))
        dA.close()
        d2.close()
        s.close()


if __name__ == "__main__":
    main()
