"""Cost of feeding an in-place update from where the geometry lies (rt_update_geometry / rt_rebuild_geometry_ranges) against the
host-records door (rt_update_scene / rt_rebuild_ranges), on one GPU.

    python tools/geometry_bench.py [--reps 15] [--warmup 3] [--scenes sponza,config5] [--out FILE]

Two scenes: sponza-class with every vertex moved (one BLAS: the range plan is ["refit"]), and config 5 with its moving BLAS (the
second; the plan is ["keep", "refit"]).  The vertices are jittered anew for every repetition.  Per scene and call (update: the refit
of the whole scene; ranges: the range plan), each source on a context of its own, alternating within a repetition:
  a  host       the host-records path: numpy records + Device.update_scene / Device.rebuild_ranges.  The records are made from the
                moved vertices on the host with numpy (normal, centroid, Heron's area: float32, not held to AddTriangle's bits, which
                a measurement does not need); records_ms is that time, and wall_with_records_ms the call's wall time plus it
  b  records    the same records in a torch tensor on the GPU, through update_geometry / rebuild_geometry_ranges
  c  packed     the moved vertices as a (count, 3, 3) torch tensor on the GPU
  d  indexed    the moved vertices as a vertex buffer without duplicates and an index tensor on the GPU
Reported per row: wall ms of the call (min / median / max over --reps), the spread (max - min) / median and the median gpu_ms.  One
JSON line per row and one verdict line per scene and call: whether b, c and d are slower than a beyond a's own run-to-run range
(median above a's max), to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magr_ray_tracer_amd import _lib as W, scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scenes", default="sponza,config5")
ap.add_argument("--out", default=None)
args = ap.parse_args()

RW, RH = 1280, 720
SOURCES = ("host", "records", "packed", "indexed")


def mmm(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3), round(max(xs), 3)]


def records_from(base, v):
    """The records `base` moved to the vertices v (count, 3, 3) float32, with numpy: what a caller of the host-records door computes."""
    p = base.copy()
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    p["v0"][:, :3], p["v1"][:, :3], p["v2"][:, :3] = a, b, c
    n = np.cross(b - a, c - a)
    flip = np.einsum("ij,ij->i", n, base["N"][:, :3]) < 0
    n = n * (np.float32(1) / np.sqrt(np.einsum("ij,ij->i", n, n)))[:, None]
    n[flip] *= -1
    p["N"][:, :3] = n
    p["centroid"][:, :3] = (a + b + c) * np.float32(1 / 3)
    la, lb, lc = (np.sqrt(np.einsum("ij,ij->i", e, e)) for e in (b - a, b - c, c - a))
    s = np.float32(0.5) * (la + lb + lc)
    p["area"] = np.sqrt(s * (s - la) * (s - lb) * (s - lc))
    return p


def last_range(d):
    blocks = d.blas_blocks()
    return blocks[-1]["prim_first"], blocks[-1]["prim_count"], ["keep"] * (len(blocks) - 1) + ["refit"]


def run(name, sa, emit):
    devs = {(call, src): Device(RW, RH) for call in ("update", "ranges") for src in SOURCES}
    try:
        for d in devs.values():
            d.upload(sa)
        first, count, plan = last_range(next(iter(devs.values())))
        base = sa.prims[first:first + count]
        assert np.all(base["objType"] == W.PRIM_TRIANGLE), "the moving range holds triangles only"
        v0 = np.stack([base["v0"][:, :3], base["v1"][:, :3], base["v2"][:, :3]], axis=1)
        words, inv = np.unique(v0.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
        idx = torch.from_numpy(inv.ravel().astype(np.int32)).cuda()
        shared = np.ascontiguousarray(words).view(np.float32)                     # the vertex buffer without duplicates
        wall = {k: [] for k in devs}
        gpu = {k: [] for k in devs}
        made = []
        for rep in range(args.warmup + args.reps):
            rng = np.random.default_rng(100 + rep)
            vb = (shared + rng.normal(scale=1e-3, size=shared.shape)).astype(np.float32)
            v = vb[inv.ravel()].reshape(-1, 3, 3)                                 # shared vertices move together
            t0 = time.perf_counter()
            recs = records_from(base, v)
            ms_records = (time.perf_counter() - t0) * 1e3
            src = {"host": dict(prims=recs), "records": dict(prims=torch.from_numpy(recs.view(np.uint8).reshape(-1, 128)).cuda()),
                   "packed": dict(positions=torch.from_numpy(v).cuda()), "indexed": dict(positions=torch.from_numpy(vb).cuda(), indices=idx)}
            torch.cuda.synchronize()
            for (call, s), d in devs.items():
                t0 = time.perf_counter()
                if s == "host":
                    st = d.update_scene(recs, first) if call == "update" else d.rebuild_ranges(plan, recs, first)
                else:
                    st = d.update_geometry(first, **src[s]) if call == "update" else d.rebuild_geometry_ranges(plan, first, **src[s])
                ms = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    wall[(call, s)].append(ms)
                    gpu[(call, s)].append(st["gpu_ms"])
            if rep >= args.warmup:
                made.append(ms_records)
    finally:
        for d in devs.values():
            d.close()
    for call in ("update", "ranges"):
        rows = {}
        for s in SOURCES:
            lo, med, hi = mmm(wall[(call, s)])
            r = {"scene": name, "call": call, "source": s, "prims": len(sa.prims), "moving_prims": count, "vertices": len(shared), "reps": args.reps,
                 "wall_ms": [lo, med, hi], "spread": round((hi - lo) / med, 3), "gpu_ms": round(statistics.median(gpu[(call, s)]), 3)}
            if s == "host":
                r["records_ms"] = mmm(made)
                r["wall_with_records_ms"] = round(med + statistics.median(made), 3)
            rows[s] = r
            emit(r)
        a = rows["host"]["wall_ms"]
        emit({"scene": name, "call": call, "plan": plan if call == "ranges" else None,
              **{f"{s}_over_host": round(rows[s]["wall_ms"][1] / a[1], 3) for s in SOURCES[1:]},
              **{f"{s}_slower_than_hosts_range": bool(rows[s]["wall_ms"][1] > a[2]) for s in SOURCES[1:]}})


def main():
    out = open(args.out, "w") if args.out else None

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name, make in (("sponza", lambda: scenes.sponza_class(1.0)[0]), ("config5", lambda: scenes.config5_scene(0.0)[0])):
        if name in args.scenes.split(","):
            run(name, make().arrays(bvh4=False), emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
