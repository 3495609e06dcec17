"""Cost of rebuilding only the BLAS that changed (rt_rebuild_ranges) against rebuilding every BLAS (rt_rebuild_scene), on one GPU.

    python tools/ranges_bench.py [--reps 15] [--warmup 3] [--builders lbvh,sah] [--scenes config5,sponza+5k] [--root DIR] [--baseline FILE]
                                 [--out FILE] [--frames 8] [--rounds 5]

Two scenes, each with one BLAS that moves (its vertices jittered anew for every call, only its primitives handed over) beside one that
does not:
  config5      config 5's two SBVH BLAS; the second (terrarium_bot) moves;
  sponza+5k    sponza-class (~262k triangles) plus a second BLAS of 5,000 triangles, which moves.
Per scene and builder X, alternating within each repetition after --warmup repetitions, each on a context of its own:
  full    Device.rebuild_scene(window, first, builder=X): every BLAS built by X;
  ranges  Device.rebuild_ranges(["keep", X], window, first): the static BLAS keeps its tree, the moving one is built by X;
and, builder "-" (no builder runs), once per scene:
  refit   Device.rebuild_ranges(["keep", "refit"], window, first): the static BLAS keeps its tree and its derived records, the moving
          one is refit alone (a build that has the plan word only);
  update  Device.update_scene(window, first): rt_update_scene, the refit of the whole scene.
Reported per row: wall ms of the call (min / median / max over --reps), the spread (max - min) / median, and the medians of the
call's own split (stage, build, derive, tlas, commit ms; gpu_ms; update: gpu_ms alone); a `ranges` / `refit` row of a build that has
Device.ranges_info adds what the last call derived and what it relocated.  After their last call the `refit` and `update` contexts of
config 5 render --frames frames each, in turn, --rounds times: frame_ms (min / median / max of the per-round ms per frame) is the trace
rate of the scene whose static SBVH tree kept its clipped boxes (refit) against the scene a whole-scene refit leaves (update).  One
JSON line per row, to stdout and to --out.

--root DIR runs the same measurement on another checkout of this package (one that may predate rt_rebuild_ranges: only the `full`
and `update` rows, and `ranges` where it has the call, are measured there); --baseline FILE reads the JSON lines such a run wrote and
adds, per scene and builder: the ratio of this build's medians to the baseline's `full` median, for a mode the baseline measured too
the ratio to its own median there (wall and derive_ms: vs_baseline_same_mode, derive_vs_baseline), and the verdict whether this build's
`full` median lies within the baseline's measured run-to-run spread (its min .. max)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--builders", default="lbvh,sah")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--baseline", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--scenes", default="config5,sponza+5k")
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
from magr_ray_tracer_amd import scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Device  # noqa: E402

RW, RH = 1280, 720
SPLIT = ("stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms", "gpu_ms")


def mmm(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3), round(max(xs), 3)]


def jittered(prims, seed):
    rng = np.random.default_rng(seed)
    p = prims.copy()
    for f in ("v0", "v1", "v2"):
        p[f][:, :3] += rng.normal(scale=1e-3, size=(len(p), 3)).astype(np.float32)
    return p


def config5():
    s = scenes.config5_scene(0.0)[0]
    return s.arrays(bvh4=False)


def sponza_plus():
    s = scenes.sponza_class(1.0)[0]
    first = s.num_prims
    rng = np.random.default_rng(7)
    c = rng.uniform((-2.0, 1.0, -2.0), (2.0, 4.0, 2.0), (5000, 1, 3))
    s.AddTriangles((c + 0.05 * rng.normal(size=(5000, 3, 3))).astype(np.float32), "red")
    s.BuildBLAS(first)
    return s.arrays(bvh4=False)


def moving_range(sa):
    """(first, count) of the BLAS with the larger primitive ids: the second of the scene's two."""
    roots = [int(r) for r in sa.blas["bvhIdx"]]
    assert len(roots) == 2 and roots[0] < roots[1]
    n, st, ids = sa.bvh2, [roots[1]], []
    while st:
        i = st.pop()
        if n["count"][i] > 0:
            ids.append(sa.primIdx[n["first"][i]:n["first"][i] + n["count"][i]])
        else:
            st += [int(n["first"][i]), int(n["first"][i]) + 1]
    ids = np.concatenate(ids)
    return int(ids.min()), int(ids.max() - ids.min() + 1)


def frame_ms(devs, view):
    """ms per frame of each context, alternating, after one untimed round: {mode: [min, median, max]}."""
    cam = scenes.camera_for(view, RW, RH)
    ms = {m: [] for m in devs}
    for rnd in range(args.rounds + 1):
        for m, d in devs.items():
            d.seed_default()
            d.reset()
            d.synchronize()
            t0 = time.perf_counter()
            d.render(cam, args.frames)
            d.synchronize()
            if rnd:
                ms[m].append((time.perf_counter() - t0) * 1e3 / args.frames)
    return {m: mmm(v) for m, v in ms.items()}


def run(name, sa, builder, modes, view=None):
    first, count = moving_range(sa)
    base = sa.prims[first:first + count]
    devs = {m: Device(RW, RH) for m in modes}
    wall = {m: [] for m in modes}
    split = {m: {k: [] for k in SPLIT} for m in modes}
    built = {}
    try:
        for d in devs.values():
            d.upload(sa)
        for rep in range(args.warmup + args.reps):
            window = jittered(base, 100 + rep)
            for m in modes:
                t0 = time.perf_counter()
                if m == "full":
                    st = devs[m].rebuild_scene(window, first, None, builder=builder)
                elif m == "update":
                    st = devs[m].update_scene(window, first)
                else:
                    st = devs[m].rebuild_ranges(["keep", "refit" if m == "refit" else builder], window, first)
                ms = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    wall[m].append(ms)
                    for k in SPLIT:
                        split[m][k].append(st.get(k, 0.0))
                    built[m] = st.get("blas_built", 0)
        info = {m: devs[m].ranges_info() for m in modes if m in ("ranges", "refit") and hasattr(Device, "ranges_info")}
        frames = frame_ms({m: devs[m] for m in modes}, view) if view is not None else {}
    finally:
        for d in devs.values():
            d.close()
    rows = []
    for m in modes:
        lo, med, hi = mmm(wall[m])
        rows.append({"scene": name, "builder": builder, "mode": m, "prims": len(sa.prims), "moving_prims": count, "blas_built": built[m], "reps": args.reps,
                     "wall_ms": [lo, med, hi], "spread": round((hi - lo) / med, 3), **{k: round(statistics.median(v), 3) for k, v in split[m].items()}})
        if m in info:
            rows[-1]["ranges_info"] = info[m]
        if m in frames:
            rows[-1]["frame_ms"] = frames[m]
    return rows


def main():
    from magr_ray_tracer_amd import scene as SC
    have_ranges = hasattr(Device, "rebuild_ranges")
    have_refit = have_ranges and "refit" in getattr(SC, "PLAN_WORDS", {})
    base, same = {}, {}
    if args.baseline:
        with open(args.baseline) as f:
            for line in f:
                if line.startswith("{"):
                    r = json.loads(line)
                    if r.get("mode") == "full":
                        base[(r["scene"], r["builder"])] = r
                    if "mode" in r:
                        same[(r["scene"], r["builder"], r["mode"])] = r
    out = open(args.out, "w") if args.out else None

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def against_baseline(r, b):
        o = same.get((r["scene"], r["builder"], r["mode"]))
        if b:
            r["vs_baseline_full"] = round(r["wall_ms"][1] / b["wall_ms"][1], 3)
            if r["mode"] == "full":
                r["baseline_full_ms"] = b["wall_ms"]
                r["within_baseline_spread"] = bool(b["wall_ms"][0] <= r["wall_ms"][1] <= b["wall_ms"][2])
        if o and r["mode"] != "full":
            r["vs_baseline_same_mode"] = round(r["wall_ms"][1] / o["wall_ms"][1], 3)
            if o.get("derive_ms"):
                r["baseline_derive_ms"] = o["derive_ms"]
                r["derive_vs_baseline"] = round(r["derive_ms"] / o["derive_ms"], 3)

    for name, make in (("config5", config5), ("sponza+5k", sponza_plus)):
        if name not in args.scenes.split(","):
            continue
        sa = make()
        view = scenes.config5_scene(0.0)[1] if name == "config5" else None
        rows = run(name, sa, "-", (["refit"] if have_refit else []) + ["update"], view)
        for r in rows:
            against_baseline(r, None)
            emit(r)
        if len(rows) == 2:
            v = {"scene": name, "refit_over_update": round(rows[0]["wall_ms"][1] / rows[1]["wall_ms"][1], 3)}
            if "frame_ms" in rows[0]:
                v["frame_ms_refit_over_update"] = round(rows[0]["frame_ms"][1] / rows[1]["frame_ms"][1], 3)
            emit(v)
        for builder in args.builders.split(","):
            rows = run(name, sa, builder, ["full"] + (["ranges"] if have_ranges else []))
            b = base.get((name, builder))
            for r in rows:
                against_baseline(r, b)
                emit(r)
            if len(rows) == 2:
                full, rng_ = rows
                v = {"scene": name, "builder": builder, "ranges_over_full": round(rng_["wall_ms"][1] / full["wall_ms"][1], 3)}
                if rng_["wall_ms"][1] >= full["wall_ms"][1]:   # not faster: say which stage dominates the selective call
                    v["dominant_stage"] = max(SPLIT[:5], key=lambda k: rng_[k])
                emit(v)
    if out:
        out.close()


if __name__ == "__main__":
    main()
