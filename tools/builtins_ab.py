#!/usr/bin/env python3
"""What RtConfig.builtins costs: IEEE against REFERENCE on BASELINE config 3 (sponza-class atrium, 1920x1080, NEE), in ONE process, the
two modes alternating, all contexts rendering from one device copy of the scene.

    python tools/builtins_ab.py [--steps 256] [--warmup 4] [--rounds 3] [--lanes 4] [--detail 1.0]

Per round and mode, bench.py's timed regions: a group of `--lanes` sample streams renders `--steps` frames between synchronise brackets
(+ the lane sum), timed once -> M samples/s; one context with the GPU to itself renders max(16, min(steps, 64)) frames -> M samples/s.
Then, per mode, 16 frames of the single context with every stage launch bracketed (profile 2): k_generate and k_shade in ms per frame.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()

    import numpy as np
    from magr_ray_tracer_amd import _lib
    import torch                     # the import order of bench.py (the HIP runtime the process runs on)
    _lib.device_lib()
    from magr_ray_tracer_amd import scenes
    from magr_ray_tracer_amd.renderer import Device, Group

    W, H = a.width, a.height
    s, view = scenes.sponza_class(a.detail)
    sa = s.arrays(bvh4=False)
    cam = scenes.camera_for(view, W, H)
    modes = ("ieee", "reference")
    groups, solos = {}, {}
    for m in modes:
        g = Group(W, H, lanes=a.lanes, builtins=m)
        if groups:
            g.share_scene(groups[modes[0]])
        else:
            g.upload(sa)
        g.seed(0)
        groups[m] = g
    cam["focalLength"] = groups[modes[0]].devs[0].focus(W // 2, H // 2, cam)
    for m in modes:
        d = Device(W, H, builtins=m)
        d.share_scene(groups[modes[0]].devs[0])
        d.seed_default()
        solos[m] = d
    reduced = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")

    def group_pass(g, steps):
        g.render(cam, steps)
        g.synchronize()
        g.sum_into(reduced)
        g.synchronize()
        torch.cuda.synchronize()

    n1 = max(16, min(a.steps, 64))
    for m in modes:                                   # warm-up of every kernel and shape the timed windows use
        group_pass(groups[m], max(a.warmup, 1) * a.lanes)
        groups[m].reset()
        groups[m].synchronize()
        solos[m].render(cam, 2)
        solos[m].synchronize()
    out = {m: {"group_msamples_s": [], "single_msamples_s": []} for m in modes}
    for r in range(a.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):      # alternate, and alternate who goes first
            g = groups[m]
            g.reset()
            g.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            group_pass(g, a.steps)
            dt = time.perf_counter() - t0
            out[m]["group_msamples_s"].append(round(W * H * a.steps / dt / 1e6, 2))
        for m in (modes if r % 2 == 0 else modes[::-1]):
            d = solos[m]
            d.synchronize()
            t0 = time.perf_counter()
            d.render(cam, n1)
            d.synchronize()
            dt = time.perf_counter() - t0
            out[m]["single_msamples_s"].append(round(W * H * n1 / dt / 1e6, 2))
    for m in modes:                                   # per-stage times, one context, every stage bracketed
        d = solos[m]
        d.set_profile(2)
        d.reset_stage_times()
        d.render(cam, 16)
        d.synchronize()
        st = d.stage_times()
        out[m]["stage_ms_per_frame"] = {k[:-3]: round(st[k] / 16, 4) for k in st if k.endswith("_ms") and k != "compact_ms"}
        d.set_profile(0)
        out[m]["builtins"] = d.builtins
    for m in modes:
        for k in ("group_msamples_s", "single_msamples_s"):
            v = out[m][k]
            out[m][k + "_range"] = [min(v), max(v)]
    line = {"tool": "tools/builtins_ab.py", "config": f"BASELINE config 3: sponza_class({a.detail}) {len(sa.prims)} prims {W}x{H} NEE+cosine+RR+firefly, BVH2",
            "steps": a.steps, "single_steps": n1, "warmup": a.warmup, "rounds": a.rounds, "lanes": a.lanes,
            "streams_concurrent": groups[modes[0]].concurrency(), "modes": out,
            "reference_over_ieee": {"group": round(float(np.median(out["reference"]["group_msamples_s"]) / np.median(out["ieee"]["group_msamples_s"])), 4),
                                    "single": round(float(np.median(out["reference"]["single_msamples_s"]) / np.median(out["ieee"]["single_msamples_s"])), 4)}}
    print(json.dumps(line), flush=True)
    for m in modes:
        solos[m].close()
        groups[m].close()


if __name__ == "__main__":
    main()
