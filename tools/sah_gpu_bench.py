"""Build time of the GPU SAH build (rt_build_bvh2_sah) against the host SAH builder and the LBVH builder, on one GPU.

    python tools/sah_gpu_bench.py

Per input (sponza-class, both BLAS of config 5 at alpha 1, a 1M-triangle soup): device_ms (GPU time from the first kernel to the last)
and wall_ms (the whole call: allocation, transfers, level read-backs), median of 10 after a warm-up; the phase split of the median
call (allocation + upload, level passes, numbering + emit, download; rt_debug_sah_phases) and its level count; rt_build_bvh2 (LBVH)
wall ms; the host SAH builder (BVH2::BuildBLAS, alpha 1) at 1 and 16 threads."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magr_ray_tracer_amd import _lib as W, scenes  # noqa: E402
from magr_ray_tracer_amd.scene import _view, build_lbvh, build_sah_gpu  # noqa: E402


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


def host_sah_ms(p, first, count, threads):
    """BuildBLAS(alpha 1) over [first, first + count) of a scene holding exactly p[:first + count]."""
    s = scenes.Scene()
    scenes._std_materials(s)
    q = p[:first + count]
    tri = q["objType"] == W.PRIM_TRIANGLE
    assert tri.all(), "host timing rows use triangle-only inputs"
    s.AddTriangles(np.stack([q["v0"][:, :3], q["v1"][:, :3], q["v2"][:, :3]], 1), "sand")
    t = time.perf_counter()
    s.BuildBLAS(first, threads=threads)
    return round((time.perf_counter() - t) * 1e3, 1)


def config5_split(sa):
    nodes, root = sa.bvh2, int(sa.blas["bvhIdx"][1])
    st, lo = [root], len(sa.prims)
    while st:
        i = st.pop()
        if nodes["count"][i]:
            f, c = int(nodes["first"][i]), int(nodes["count"][i])
            lo = min(lo, int(sa.primIdx[f:f + c].min()))
        else:
            st += [int(nodes["first"][i]), int(nodes["first"][i]) + 1]
    return lo


def main():
    p3 = prims_of(scenes.sponza_class(1.0)[0])
    sa5 = scenes.config5_scene(1.0)[0].arrays(bvh4=False)
    f1 = config5_split(sa5)
    p1m = prims_of(soup(1 << 20))
    cases = [("config3 sponza_class", p3, 0, len(p3)), ("config5 BLAS 0 (robo-orb), alpha 1", sa5.prims, 0, f1),
             ("config5 BLAS 1 (terrarium), alpha 1", sa5.prims, f1, len(sa5.prims) - f1), ("soup 1M", p1m, 0, len(p1m))]
    L = W.device_lib()
    ph = np.zeros(5, np.float32)
    for name, p, first, count in cases:
        build_sah_gpu(p, first, count, device=0)                          # warm-up (module load, first allocation)
        runs = []
        for _ in range(10):
            st = build_sah_gpu(p, first, count, device=0)[2]
            L.rt_debug_sah_phases(W.ptr(ph))
            runs.append((st["wall_ms"], st, ph.copy()))
        runs.sort(key=lambda r: r[0])
        st, phases = runs[5][1], runs[5][2]
        build_lbvh(p, first, count, device=0)
        lb = [build_lbvh(p, first, count, device=0)[2]["wall_ms"] for _ in range(10)]
        r = dict(case=name, prims=count, nodes=st["nodes"], depth=st["depth"], device_ms=med([x[1]["device_ms"] for x in runs]),
                 wall_ms=med([x[0] for x in runs]),
                 phases_ms=dict(alloc_upload=round(float(phases[0]), 3), levels=round(float(phases[1]), 3),
                                numbering_emit=round(float(phases[2]), 3), download=round(float(phases[3]), 3)),
                 level_passes=int(phases[4]), lbvh_wall_ms=med(lb))
        if p["objType"][first:first + count].tolist().count(W.PRIM_TRIANGLE) == count and first == 0:
            r["host_sah_1t_ms"] = host_sah_ms(p, first, count, 1)
            r["host_sah_16t_ms"] = host_sah_ms(p, first, count, 16)
            r["host16_over_wall"] = round(r["host_sah_16t_ms"] / r["wall_ms"], 1)
        print(r, flush=True)


if __name__ == "__main__":
    main()
