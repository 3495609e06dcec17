"""Build time and trace cost of the linear BVH builder (rt_build_bvh2) against the SAH builder, on one GPU.

    python tools/lbvh_bench.py [--frames 64] [--sweep]

Build: device ms (GPU time of the kernels, median of 10 after a warm-up), wall ms (the whole call: transfers and allocations
included), the host restatement and the host SAH builder at 1 and 16 threads, on the sponza-class atrium (BASELINE config 3), the
two BLAS of config 5 and a 1M-triangle soup.  Trace: config 3 (1920x1080, one sample per pixel per frame) rendered over the SAH tree
and over the LBVH tree, one context and four lanes, in M samples/s, with the LDS stack entries kernel_info reports for each tree.
--sweep also times the LBVH options (max_leaf, C_t) on four lanes."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magr_ray_tracer_amd import scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Group  # noqa: E402
from magr_ray_tracer_amd.scene import _view, build_lbvh  # noqa: E402
from magr_ray_tracer_amd import _lib as W  # noqa: E402


def prims_of(s):
    return _view(s._lib.rth_primitives, s._h, W.Primitive)


def soup(n, seed=12):
    rng = np.random.default_rng(seed)
    s = scenes.Scene()
    scenes._std_materials(s)
    c = rng.uniform(-4, 4, (n, 1, 3))
    s.AddTriangles((c + 0.45 * rng.normal(size=(n, 3, 3))).astype(np.float32), "sand")
    return s


def med(xs):
    return round(statistics.median(xs), 3)


def sah_ms(s, threads):
    """Host SAH build of the whole primitive array, appended to the scene (its statistics accumulate build ms)."""
    before = s.stats()["build_ms"]
    s.BuildBLAS(0, threads=threads)
    return round(s.stats()["build_ms"] - before, 1)


def build_rows():
    rows = []
    s3, _ = scenes.sponza_class(1.0, builder="lbvh", device=None)
    s1m = soup(1 << 20)
    s5, _ = scenes.config5_scene(0.0)
    sbvh5 = s5.stats()["build_ms"]
    sa5 = s5.arrays(bvh4=False)
    # config 5's second BLAS starts at its node block's lowest primIdx
    lo = len(sa5.prims)
    b1 = int(sa5.blas["bvhIdx"][1])
    for i in range(b1, len(sa5.bvh2)):
        if sa5.bvh2["count"][i]:
            f, c = int(sa5.bvh2["first"][i]), int(sa5.bvh2["count"][i])
            lo = min(lo, int(sa5.primIdx[f:f + c].min()))
    first1 = lo
    p3 = prims_of(s3)
    cases = [("config3 sponza_class", p3, [(0, len(p3))], s3),
             ("config5 BLAS 0 (robo-orb)", sa5.prims, [(0, first1)], None),
             ("config5 BLAS 1 (terrarium)", sa5.prims, [(first1, len(sa5.prims) - first1)], None),
             ("soup 1M", prims_of(s1m), [(0, 1 << 20)], s1m)]
    for name, p, ranges, scene in cases:
        for first, count in ranges:
            build_lbvh(p, first, count, device=0)                      # warm-up (module load, first allocation)
            dev = [build_lbvh(p, first, count, device=0)[2] for _ in range(10)]
            host = [build_lbvh(p, first, count, device=None)[2] for _ in range(3)]
            r = dict(case=name, prims=count, nodes=dev[0]["nodes"], leaves=dev[0]["leaves"], depth=dev[0]["depth"],
                     morton_bits=dev[0]["morton_bits"], device_ms=med([d["device_ms"] for d in dev]),
                     wall_ms=med([d["wall_ms"] for d in dev]), host_restatement_ms=med([h["wall_ms"] for h in host]))
            if scene is not None:
                r["host_sah_1t_ms"] = sah_ms(scene, 1)
                r["host_sah_16t_ms"] = sah_ms(scene, 16)
                r["sah_over_wall_16t"] = round(r["host_sah_16t_ms"] / r["wall_ms"], 1)
            rows.append(r)
            print(r, flush=True)
    print({"config5 host SBVH alpha 0, 1 thread, both BLAS (factory build) ms": round(sbvh5, 1)}, flush=True)
    return rows


def trace(sa, view, lanes, frames, W_=1920, H_=1080):
    g = Group(W_, H_, lanes=lanes, **dict(shading=1, sampling=1, accel=0, russian_roulette=True, filter_fireflies=True))
    try:
        g.upload(sa)
        info = g.devs[0].kernel_info()
        cam = scenes.camera_for(view, W_, H_)
        g.seed(0)
        g.render(cam, 2 * lanes)
        g.synchronize()
        g.reset()
        t = time.perf_counter()
        g.render(cam, frames)
        g.synchronize()
        dt = time.perf_counter() - t
        return round(W_ * H_ * frames / dt / 1e6, 1), info["stack_entries"]
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-build", action="store_true")
    a = ap.parse_args()
    if not a.skip_build:
        build_rows()
    s_sah, view = scenes.sponza_class(1.0)
    s_lb, _ = scenes.sponza_class(1.0, builder="lbvh", device=0)
    assert s_lb.lbvh_stats()["device_ms"] > 0
    trees = {"sah": s_sah.arrays(bvh4=False), "lbvh": s_lb.arrays(bvh4=False)}
    for rep in range(2):                                                   # alternated: SAH, LBVH, SAH, LBVH
        for lanes in (1, 4):
            for name, sa in trees.items():
                ms, stack = trace(sa, view, lanes, a.frames)
                print(dict(trace="config3 1920x1080", tree=name, lanes=lanes, rep=rep, M_samples_per_s=ms, stack_entries=stack), flush=True)
    if a.sweep:
        # options on the same primitives: a single-BLAS scene's TLAS only holds the root box, which every option shares
        sa = trees["lbvh"]
        for ml, ct in [(4, 1.0), (8, 1.0), (16, 1.0), (8, 0.5), (8, 2.0)]:
            nodes, idx, st = build_lbvh(sa.prims, device=0, max_leaf=ml, cost_traverse=ct)
            ms, stack = trace(dataclasses.replace(sa, bvh2=nodes, primIdx=idx), view, 4, a.frames)
            print(dict(sweep="config3 4 lanes", max_leaf=ml, cost_traverse=ct, M_samples_per_s=ms, stack_entries=stack,
                       depth=st["depth"], sah_cost=round(st["sah_cost"], 1)), flush=True)


if __name__ == "__main__":
    main()
