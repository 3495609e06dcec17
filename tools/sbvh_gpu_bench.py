"""Build time of the GPU SBVH build (rt_build_bvh2_sbvh) against the host builder (BVH2::BuildBLAS) on the same machine, one GPU.

    python tools/sbvh_gpu_bench.py [--runs 5] [--host-threads 1,16]

Per input (both BLAS of config5_scene(0.0); sponza_class(1.0) at alpha 0 and 1e-5; the 50k soup at alpha 0): the tree (refs, nodes,
depth, spatial splits, clipped primitives, peak_refs, level passes); device_ms (GPU time from the first kernel to the last) and
wall_ms (the whole call: allocation, transfers, the two read-backs per level) of a call whose arrays are large enough, median of
--runs after a warm-up; wall_ms of the two calls the capacity protocol makes when the caller starts from 2n - 1 nodes and n indices;
the phase split of the median call (rt_debug_sbvh_phases); BuildBLAS at 1 and 16 host threads in the same run; the clip kernels'
scratch bytes per work-item."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magr_ray_tracer_amd import _lib as W, scenes  # noqa: E402
from magr_ray_tracer_amd.scene import _view, build_sbvh_gpu  # noqa: E402


def prims_of(s):
    return _view(s._lib.rth_primitives, s._h, W.Primitive)


def soup(n, seed=1):
    rng = np.random.default_rng(seed)            # tests/lbvh_check.py soup(50000): "soup-50k"
    c = rng.uniform(-4.0, 4.0, (n, 1, 3))
    return (c + 0.45 * rng.normal(size=(n, 3, 3))).astype(np.float32)


def timed_factory(factory, threads):
    """The factory's scene with every BuildBLAS at `threads` host threads; returns (scene, [ms per BuildBLAS call])."""
    orig, ms = scenes.Scene.BuildBLAS, []

    def timed(self, *a, **kw):
        kw.setdefault("threads", threads)
        t = time.perf_counter()
        r = orig(self, *a, **kw)
        ms.append(round((time.perf_counter() - t) * 1e3, 1))
        return r
    scenes.Scene.BuildBLAS = timed
    try:
        return factory(), ms
    finally:
        scenes.Scene.BuildBLAS = orig


def soup_scene(alpha):
    s = scenes.Scene()
    scenes._std_materials(s)
    s.AddTriangles(soup(50000), "sand")
    s.BuildBLAS(0, alpha)
    return s


def blocks_of(s):
    """(first, count, nodeBase, idxBase) per BLAS of a built scene."""
    n = len(prims_of(s))
    nodes = _view(s._lib.rth_bvh2_nodes, s._h, W.BVHNode2)
    idx = _view(s._lib.rth_prim_idx, s._h, np.dtype("<u4"))
    roots = [int(r) for r in _view(s._lib.rth_blas_nodes, s._h, W.BVHInstance)["bvhIdx"]] + [len(nodes)]
    out, ib = [], 0
    for k in range(len(roots) - 1):
        cnt = int(nodes["count"][roots[k]:roots[k + 1]].sum())
        first = int(idx[ib:ib + cnt].min())
        out.append((first, roots[k], ib, cnt))
        ib += cnt
    return [(f, (out[k + 1][0] if k + 1 < len(out) else n) - f, nb, i) for k, (f, nb, i, _) in enumerate(out)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-threads", default="1,16")
    args = ap.parse_args()
    threads = [int(t) for t in args.host_threads.split(",") if t]
    cases = [("config5_scene(0.0)", 0.0, lambda: scenes.config5_scene(0.0)[0]),
             ("sponza_class(1.0), alpha 0", 0.0, lambda: scenes.sponza_class(1.0, alpha=0.0)[0]),
             ("sponza_class(1.0), alpha 1e-5", 1e-5, lambda: scenes.sponza_class(1.0, alpha=1e-5)[0]),
             ("soup-50k, alpha 0", 0.0, lambda: soup_scene(0.0))]
    L = W.device_lib()
    ph = np.zeros(8, np.float32)
    for name, alpha, factory in cases:
        host = {}
        for t in threads:
            s, host[t] = timed_factory(factory, t)
        p, blocks = prims_of(s), blocks_of(s)
        hstats = s.stats()
        for k, (first, count, nb, ib) in enumerate(blocks):
            nodes, idx, st = build_sbvh_gpu(p, alpha, first, count, device=0, node_base=nb, idx_base=ib)     # warm-up; the sizes
            bn, bi = np.zeros(len(nodes), W.BVHNode2), np.zeros(len(idx), np.uint32)
            runs = []
            for _ in range(args.runs):
                st = build_sbvh_gpu(p, alpha, first, count, device=0, node_base=nb, idx_base=ib, nodes=bn, idx=bi)[2]
                L.rt_debug_sbvh_phases(W.ptr(ph))
                runs.append((st["wall_ms"], st, ph.copy()))
            two = []
            for _ in range(args.runs):
                t = time.perf_counter()
                build_sbvh_gpu(p, alpha, first, count, device=0, node_base=nb, idx_base=ib)
                two.append((time.perf_counter() - t) * 1e3)
            runs.sort(key=lambda r: r[0])
            st, phases = runs[len(runs) // 2][1], runs[len(runs) // 2][2]
            r = dict(case=f"{name}, BLAS {k}", prims=count, refs=st["n_idx"], nodes=st["nodes"], depth=st["depth"],
                     spatial_splits=st["spatial_splits"], prims_clipped=st["prims_clipped"], peak_refs=st["peak_refs"],
                     level_passes=st["levels"], device_ms=round(statistics.median(x[1]["device_ms"] for x in runs), 3),
                     wall_ms=round(statistics.median(x[0] for x in runs), 3), wall_ms_two_calls=round(statistics.median(two), 3),
                     phases_ms=dict(alloc_upload=round(float(phases[0]), 3), levels=round(float(phases[1]), 3),
                                    numbering_emit=round(float(phases[2]), 3), download=round(float(phases[3]), 3)),
                     clip_kernel_scratch_bytes=dict(sbins=int(phases[5]), flag=int(phases[6]), scatter=int(phases[7])))
            for t in threads:
                r[f"host_{t}t_ms"] = host[t][k]
                r[f"host{t}_over_wall"] = round(host[t][k] / r["wall_ms"], 1)
            print(r, flush=True)
        print(dict(case=name, host_stats={k: hstats[k] for k in ("depth", "nodes", "spatial_splits", "prims_clipped")}), flush=True)


if __name__ == "__main__":
    main()
