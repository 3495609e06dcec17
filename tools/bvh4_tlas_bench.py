"""extend_variant 0 (nested loops) against 6 (k_trace_persist4_tlas) on config 5's two-BLAS scene under accel = BVH4, at config 5's own
resolution: per-bounce extend / connect times (profile = 2, a run of its own) and M primary samples/s (warm-up, alternating repeats,
median and spread), for one context and for the lane count bench.py uses for config 5.  Both variants run in this one process and
must leave a bit-identical accumulator.

    python tools/bvh4_tlas_bench.py [--frames 8] [--repeats 5] [--lanes 8] [--size 3840 2160] [--out profiles/r12_bvh4_tlas.txt]

If the alpha-0 collapse needs more than RT_BVH4_STACK entries and the upload refuses, the same geometry built at alpha 1 is used and the
output says so.  The resource table (VGPRs, SGPRs, scratch, LDS, occupancy) of the new instantiations comes from
`hipcc -Rpass-analysis=kernel-resource-usage` where hipcc is found; it needs no GPU."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magr_ray_tracer_amd import _lib as W, build, scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Device, Group, RtError  # noqa: E402

KERNELS = ("k_trace_persist4_tlas", "k_trace_persist4I", "k_trace_persist_tlas")


def resources():
    """name -> (VGPRs, SGPRs, scratch bytes per lane, static LDS, waves per SIMD) of the persistent traversal kernels, from a gfx950 compile."""
    src = os.path.join(build.CSRC, "rt355.hip")
    flags = [f for f in build.DEVICE_FLAGS if f not in ("-shared",)]
    cmd = [build.HIPCC] + flags + ["--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    try:
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=1800).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return None, f"not compiled here ({e})"
    out = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", err)[1:]:
        name = blk.split()[0]
        if not any(k in name for k in KERNELS):
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        try:
            name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0] or name
        except OSError:
            pass
        out[name.replace("rt355dev::", "").replace("void ", "")] = (g("VGPRs"), g("TotalSGPRs"), g(r"ScratchSize \[bytes/lane\]"), g(r"LDS Size \[bytes/block\]"),
                                                                    g(r"Occupancy \[waves/SIMD\]"))
    return out, None


def scene_arrays():
    note = "alpha 0 (config 5 as bench.py builds it)"
    s, view = scenes.config5_scene(0.0)
    sa = s.arrays()
    d = Device(64, 48, accel=W.ACCEL_BVH4)
    try:
        d.upload(sa)
    except RtError as e:
        note = f"alpha 1: the alpha-0 collapse was refused ({e})"
        s, view = scenes.config5_scene(1.0)
        sa = s.arrays()
    finally:
        d.close()
    return sa, view, note, s.stats()


def per_bounce(sa, cam, Wd, Hd, variant, frames):
    """Mean time of every extend / connect launch of a frame, by bounce: one stage_* call per measurement, profile = 2."""
    d = Device(Wd, Hd, accel=W.ACCEL_BVH4, profile=2, extend_variant=variant)
    try:
        d.upload(sa)
        info = d.kernel_info()
        d.seed_default()
        d.render(cam, 2)
        d.synchronize()
        ext, con = np.zeros(W.MAX_BOUNCES), np.zeros(W.MAX_BOUNCES)
        for f in range(frames):
            d.stage_begin_frame()
            d.stage_generate(cam)
            for b in range(W.MAX_BOUNCES):
                for stage, acc, key in ((lambda: d.stage_extend(b), ext, "extend_ms"), (None, None, None), (lambda: d.stage_connect(b, b), con, "connect_ms")):
                    if stage is None:
                        d.stage_shade(b)
                        continue
                    d.synchronize()
                    d.reset_stage_times()
                    stage()
                    d.synchronize()
                    acc[b] += d.stage_times()[key] * 1e3
            c = d.counters()
        return info, ext / frames, con / frames, c
    finally:
        d.close()


def rate(make, cam, frames, lanes):
    """One timed window: `frames` frames per lane after a 2-frame warm-up, ending in a synchronise.  Returns (handle, seconds)."""
    h = make()
    h.render(cam, 2 * lanes)
    h.synchronize()
    h.reset()
    t = time.perf_counter()
    h.render(cam, frames * lanes)
    h.synchronize()
    return h, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=8, help="bench.py's lane count for config 5")
    ap.add_argument("--size", type=int, nargs=2, default=[3840, 2160])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    Wd, Hd = args.size
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    sa, view, note, stats = scene_arrays()
    cam = scenes.camera_for(view, Wd, Hd)
    say(f"# tools/bvh4_tlas_bench.py: config 5's scene, accel = BVH4, {Wd}x{Hd}, {note}")
    say(f"# scene: {stats}")
    probe = Device(Wd, Hd, accel=W.ACCEL_BVH4)
    probe.upload(sa)
    cam["focalLength"] = probe.focus(Wd // 2, Hd // 2, cam)
    probe.close()

    say("\n## per bounce, one context, profile = 2 (us per launch, mean of %d frames)" % args.frames)
    pb = {}
    for v in (0, 6):
        info, ext, con, c = per_bounce(sa, cam, Wd, Hd, v, args.frames)
        pb[v] = (ext, con)
        mode = {0: "nested loops", 2: "k_trace_persist4_tlas, column in LDS", 3: "k_trace_persist4_tlas, spill"}[info["persist4"]]
        say(f"variant {v}: {mode}; kernel_info {info}; RT355_TLAS_FLAT {os.environ.get('RT355_TLAS_FLAT', 'default (extend flat, connect event loop)')}")
        say("  extend  " + " ".join(f"{x:8.1f}" for x in ext) + f"   sum {ext.sum():9.1f}")
        say("  connect " + " ".join(f"{x:8.1f}" for x in con) + f"   sum {con.sum():9.1f}")
    say("  ratio 6/0 extend  " + " ".join(f"{a / b:8.3f}" for a, b in zip(pb[6][0], pb[0][0]) if b > 0))
    say("  ratio 6/0 connect " + " ".join(f"{a / b:8.3f}" for a, b in zip(pb[6][1], pb[0][1]) if b > 0))

    say(f"\n## M primary samples/s: {args.repeats} alternating repeats of {args.frames} frames per lane after a 2-frame warm-up, profiler off")
    for lanes in (1, args.lanes):
        res, acc = {0: [], 6: []}, {}
        for r in range(args.repeats):
            for v in (0, 6):
                def make():
                    if lanes == 1:
                        d = Device(Wd, Hd, accel=W.ACCEL_BVH4, extend_variant=v)
                        d.upload(sa)
                        d.seed_default()
                        return d
                    g = Group(Wd, Hd, lanes=lanes, accel=W.ACCEL_BVH4, extend_variant=v)
                    g.upload(sa)
                    g.seed(0)
                    return g
                h, dt = rate(make, cam, args.frames, lanes)
                res[v].append(Wd * Hd * args.frames * lanes / dt / 1e6)
                if r == 0:
                    acc[v] = h.read_accum()
                h.close()
        same = np.array_equal(acc[0].view(np.uint32), acc[6].view(np.uint32))
        for v in (0, 6):
            x = res[v]
            say(f"  {lanes} lane(s), variant {v}: median {statistics.median(x):8.1f}  min {min(x):8.1f}  max {max(x):8.1f}  ({' '.join('%.0f' % y for y in x)})")
        say(f"  {lanes} lane(s): variant 6 / variant 0 = {statistics.median(res[6]) / statistics.median(res[0]):.3f}; accumulators bit-identical: {same}")

    if not args.no_resources:
        say("\n## resources of the persistent traversal kernels (gfx950 compile, -Rpass-analysis=kernel-resource-usage; dynamic LDS is set at launch)")
        table, why = resources()
        if table is None:
            say("  " + why)
        else:
            say("  %-64s %5s %5s %8s %5s %10s" % ("kernel", "VGPR", "SGPR", "scratch", "LDS", "waves/SIMD"))
            for k in sorted(table):
                say("  %-64s %5d %5d %8d %5d %10d" % ((k,) + table[k]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
