"""Cost of an in-place scene update (rt_update_scene) against a rebuild + re-upload, on one GPU.

    python tools/refit_bench.py [--reps 10]

For sponza-class (BASELINE config 3) and config 5 (two SBVH BLAS under a TLAS), every primitive moves (a small jitter of every
vertex).  Three ways to bring the bound scene up to date are timed, alternating in the same run (median of --reps each):
  update       Device.update_scene(prims): BLAS refit, derived records and TLAS rebuild on the GPU (wall ms and its gpu_ms);
  sah+upload   the scene made and built again on the host (SAH / SBVH builder) + TLAS + rt_upload_scene;
  lbvh+upload  the same with rt_build_bvh2 on the GPU.
(The rebuilds build the unmoved geometry: a millimetre jitter does not change what a build costs.)
One JSON line per scene."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magr_ray_tracer_amd import scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Device  # noqa: E402


def med(xs):
    return round(statistics.median(xs), 3)


def jittered(prims, seed):
    rng = np.random.default_rng(seed)
    p = prims.copy()
    for f in ("v0", "v1", "v2"):
        p[f][:, :3] += rng.normal(scale=1e-3, size=(len(p), 3)).astype(np.float32)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    cases = {
        "sponza_class": lambda b: scenes.sponza_class(1.0) if b is None else scenes.sponza_class(1.0, builder="lbvh", device=0),
        "config5": lambda b: scenes.config5_scene(0.0) if b is None else scenes.config5_scene(0.0, builder="lbvh", device=0),
    }
    for name, make in cases.items():
        s, _ = make(None)
        sa = s.arrays(bvh4=False)
        d = Device(320, 240)
        d.upload(sa)
        d2 = Device(320, 240)   # the rebuilds upload here: d keeps the scene the updates refit
        out = {"scene": name, "prims": int(len(sa.prims)), "nodes": int(len(sa.bvh2)), "instances": int(len(sa.blas))}
        t_upd, g_upd, t_sah, t_lbvh = [], [], [], []
        d.update_scene(jittered(sa.prims, 0))   # first update: allocates the staging buffers
        for r in range(a.reps):
            p = jittered(sa.prims, r + 1)
            t0 = time.perf_counter()
            st = d.update_scene(p)
            t_upd.append((time.perf_counter() - t0) * 1e3)
            g_upd.append(st["gpu_ms"])
            for builder, acc in ((None, t_sah), ("lbvh", t_lbvh)):
                t0 = time.perf_counter()
                s2, _ = make(builder)
                d2.upload(s2.arrays(bvh4=False))
                acc.append((time.perf_counter() - t0) * 1e3)
                s2.close()
        out.update(update_wall_ms=med(t_upd), update_gpu_ms=med(g_upd), sah_upload_ms=med(t_sah), lbvh_upload_ms=med(t_lbvh),
                   tlas_depth=st["tlas_depth"], nodes_refit=st["nodes"])
        print(json.dumps(out), flush=True)
        d2.close()
        d.close()
        s.close()


if __name__ == "__main__":
    main()
