"""Rate of rt_trace (Device.trace_raw) against the frame's own traversal launches for the same queue, on one GPU.

    python tools/trace_bench.py [--reps 20] [--width 1920 --height 1080] [--detail 1.0] [--out FILE]

On the bench scene (bench.py config 3, sponza-class) one frame is run stage by stage up to shade(0).  The rays of bounce 1
(Device.get_rays) and the shadow records of bounce 0 (Device.get_shadow) are then traced as caller rays, three ways:
  in place   16-byte origins and directions, nothing but the hit record wanted: the traversal launch reads and writes the caller's arrays;
  strided    packed float3 origins and directions, hit + point + normal: the load and store passes stream 152 B per ray
             (24 in, 32 to the query's arrays; 48 back, 48 out);
  any        the frame's shadow records (packed float3 origin and direction, tmax): 93 B per ray (28 in, 48 to the query's arrays; 16
             back, 1 out).
Each figure stands beside the launch time of rt_stage_extend(1) resp. rt_stage_connect(0, 0) on the very same queue, from the kernels'
own begin / end timestamps (rt_read_stage_times, profile = 2), and the strided forms beside the allowance for their two passes: their
bytes at the 4.3 TB/s k_generate reaches.  The query's figures are wall-clock per call including the final
rt_synchronize (min / median / max of --reps after a warm-up), so they carry the host's launch and synchronisation cost (a few tens
of microseconds) that the kernel timestamps do not.  One JSON line; no threshold."""
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

STREAM_TBS = 4.3          # what k_generate reaches
BYTES = {"strided": 24 + 32 + 48 + 48, "any": 28 + 48 + 16 + 1}


def mmm(xs):
    return [round(min(xs), 4), round(statistics.median(xs), 4), round(max(xs), 4)]


def timed(d, reps, call):
    call()
    d.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        d.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stage_ms(d, reps, stage, key):
    """Mean kernel time of `reps` launches of one stage on the queue as it stands (the first, untimed one warms the caches)."""
    stage()
    d.synchronize()
    d.reset_stage_times()
    for _ in range(reps):
        stage()
    d.synchronize()
    t = d.stage_times()
    assert t[key + "_launches"] == reps, t
    return t[key + "_ms"] / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    s, view = scenes.sponza_class(a.detail)
    sa = s.arrays()
    cam = scenes.camera_for(view, a.width, a.height)
    d = Device(a.width, a.height, profile=2, russian_roulette=False)
    d.upload(sa)
    cam["focalLength"] = d.focus(a.width // 2, a.height // 2, cam)
    d.seed_default()
    d.reset()
    d.stage_begin_frame()
    d.stage_generate(cam)
    d.stage_extend(0)
    d.stage_shade(0)
    rays, rec = d.get_rays(1), d.get_shadow(0, 0)
    n, ns = len(rays), len(rec)
    res = dict(scene="sponza-class", detail=a.detail, width=a.width, height=a.height, reps=a.reps, kernel_info=d.kernel_info(),
               window=d.trace_window(), rays_bounce_1=n, shadow_records_bounce_0=ns)
    res["stage_extend_1_ms"] = round(stage_ms(d, a.reps, lambda: d.stage_extend(1), "extend"), 4)
    res["stage_connect_0_ms"] = round(stage_ms(d, a.reps, lambda: d.stage_connect(0, 0), "connect"), 4)

    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    o4, d4, o3, d3 = T(rays["O"]), T(rays["D"]), T(rays["O"][:, :3]), T(rays["D"][:, :3])
    so, sl, st = T(rec["o"]), T(rec["l"]), T(rec["tmax"])
    hit, pt, nm = (torch.empty((n, 4), device=dev) for _ in range(3))
    occ = torch.empty(ns, dtype=torch.uint8, device=dev)
    P = lambda x: x.data_ptr()   # noqa: E731
    torch.cuda.synchronize()
    forms = {
        "in_place": (n, lambda: d.trace_raw(W.TRACE_CLOSEST, P(o4), P(d4), 16, 16, 0, n, hit=P(hit)), "stage_extend_1_ms"),
        "strided": (n, lambda: d.trace_raw(W.TRACE_CLOSEST, P(o3), P(d3), 12, 12, 0, n, hit=P(hit), point=P(pt), normal=P(nm)), "stage_extend_1_ms"),
        "any": (ns, lambda: d.trace_raw(W.TRACE_ANY, P(so), P(sl), 12, 12, P(st), ns, occluded=P(occ)), "stage_connect_0_ms"),
    }
    for name, (m, call, base) in forms.items():
        ms = timed(d, a.reps, call)
        r = dict(ms=mmm(ms), mrays_per_s=round(m / statistics.median(ms) / 1e3, 1), stage_ms=res[base],
                 over_stage_ms=round(statistics.median(ms) - res[base], 4))
        if name in BYTES:
            r["stream_bytes_per_ray"] = BYTES[name]
            r["stream_allowance_ms"] = round(m * BYTES[name] / (STREAM_TBS * 1e12) * 1e3, 4)
        res[name] = r
    # the same hits as the frame's own launch left
    d.stage_extend(1)
    ref = d.get_rays(1)
    forms["in_place"][1]()
    d.synchronize()
    h = hit.cpu().numpy().view(W.Hit).reshape(-1)
    res["in_place_equals_stage_extend"] = bool(np.array_equal(h["primIdx"], ref["primIdx"]) and h["t"].tobytes() == ref["t"].tobytes())
    res["occluded_fraction"] = round(float(occ.float().mean()), 4)
    d.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
