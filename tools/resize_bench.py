"""Cost of an in-place resize (rt_resize_scene) against the round trip it removes, on one GPU.

    python tools/resize_bench.py [--reps 10] [--builders sah,lbvh,sbvh] [--device-input]

For sponza-class and config 5, a bound scene alternates between its full primitive array and the array without the last tenth of every
BLAS's primitives (so a repetition removes a tenth and the next adds it again; the BLAS and instance counts stay, the light list
follows the primitives).  Two ways to get there are timed in one process, alternating within each repetition (min / median / max of
--reps after a warm-up that visits both shapes three times, after which a resize allocates nothing):
  A  Device.resize_scene(prims, range_counts, inst_range, instances, builder): wall ms, gpu_ms and the split of RtRebuildStats (stage -
     which holds the copy of the primitives, the record checks and the light list -, builds, derive, TLAS, commit); with
     --device-input the primitives are a torch tensor on the GPU and do not cross the bus;
  B  what the parent commit needs for the same change, minus the scene generator: rt_build_bvh2_sah / rt_build_bvh2 /
     rt_build_bvh2_sbvh per BLAS on caller arrays (the tree comes back to the host), the light list and the TLAS on the host, and a full
     rt_upload_scene with materials and the texture atlas into a second context (the first repetition checks that B's device arrays,
     the light list included, equal A's).
One JSON line per scene and builder.  No ratio is promised: the line holds both columns."""
import argparse
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
from magr_ray_tracer_amd.scene import SceneArrays, blas_ranges, build_lbvh, build_sah_gpu, build_sbvh_gpu, light_list  # noqa: E402

RW, RH = 1280, 720
ARRAYS = list(W.SCENE_ARRAYS) + list(W.SCENE_ARRAYS_RESIZE)
RESIZE = {"sah": dict(builder="sah"), "lbvh": dict(builder="lbvh"), "sbvh": dict(builder="sbvh_gpu", alpha=0.0)}


def shapes(sa):
    """The full scene and the one without the last tenth of every BLAS: (prims, range counts, instance -> range) each."""
    per_inst = blas_ranges(sa)
    ranges = sorted(set(per_inst))
    inst_range = np.array([ranges.index(r) for r in per_inst], np.int32)
    assert ranges[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and sum(c for _, c in ranges) == len(sa.prims)
    full = (sa.prims, np.array([c for _, c in ranges], np.int32), inst_range)
    keep = [max(c - c // 10, 1) for _, c in ranges]
    less = np.concatenate([sa.prims[f:f + k] for (f, _), k in zip(ranges, keep)])
    return full, (less, np.array(keep, np.int32), inst_range)


def round_trip(sa, prims, counts, inst_range, builder, d2):
    """B: per-BLAS GPU builds on caller arrays, host light list and TLAS, a full upload.  Returns wall ms."""
    t0 = time.perf_counter()
    nodes, idx, roots = [], [], []
    nb = ib = first = 0
    for count in counts:
        if builder == "sbvh":
            n, i, _ = build_sbvh_gpu(prims, 0.0, first=first, count=int(count), device=0, node_base=nb, idx_base=ib)
        else:
            n, i, _ = (build_sah_gpu if builder == "sah" else build_lbvh)(prims, first=first, count=int(count), device=0, node_base=nb, idx_base=ib)
        roots.append(nb)
        nodes.append(n)
        idx.append(i)
        nb += len(n)
        ib += len(i)
        first += int(count)
    nodes, idx = np.concatenate(nodes), np.concatenate(idx)
    inst = sa.blas.copy()
    inst["bvhIdx"] = [roots[r] for r in inst_range]
    new = SceneArrays(prims=prims, mats=sa.mats, tex=sa.tex, lights=light_list(prims, sa.mats), bvh2=nodes, bvh4=sa.bvh4, primIdx=idx,
                      tlas=RBB.small_tlas(nodes, inst), blas=inst)
    d2.upload(new)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--builders", default="sah,lbvh,sbvh")
    ap.add_argument("--device-input", action="store_true")
    a = ap.parse_args()
    for name, make in (("sponza_class", lambda: scenes.sponza_class(1.0)), ("config5", lambda: scenes.config5_scene(0.0))):
        s, _ = make()
        sa = s.arrays(bvh4=False)
        both = shapes(sa)
        given = both
        if a.device_input:
            import torch
            given = [(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).copy()).to("cuda:0"), c, ir) for p, c, ir in both]
        for builder in a.builders.split(","):
            dA, d2 = Device(RW, RH), Device(320, 240)
            dA.upload(sa)
            allocs = []
            for k in range(6):                        # warm-up: three visits to each shape
                p, c, ir = given[(k + 1) % 2]
                dA.resize_scene(p, c, ir, sa.blas, **RESIZE[builder])
                allocs.append(dA.rebuild_allocations())
            round_trip(sa, *both[1], builder, d2)
            A, Ag, B = [], [], []
            split = {k: [] for k in ("stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms")}
            same = None
            for r in range(a.reps):
                p, c, ir = given[(r + 1) % 2]
                t0 = time.perf_counter()
                st = dA.resize_scene(p, c, ir, sa.blas, **RESIZE[builder])
                A.append((time.perf_counter() - t0) * 1e3)
                Ag.append(st["gpu_ms"])
                for k in split:
                    split[k].append(st[k])
                B.append(round_trip(sa, *both[(r + 1) % 2], builder, d2))
                if r == 0:
                    same = all(np.array_equal(dA.scene_array(k), d2.scene_array(k)) for k in ARRAYS)
            print(json.dumps({"scene": name, "builder": builder, "prims": [len(both[0][0]), len(both[1][0])], "device_input": bool(a.device_input),
                              "resize_wall_ms": RBB.mmm(A), "resize_gpu_ms": RBB.mmm(Ag), "split_ms": {k: RBB.mmm(v) for k, v in split.items()},
                              "round_trip_wall_ms": RBB.mmm(B), "arrays_equal": same, "allocations_warm_up": allocs,
                              "allocations_measured": dA.rebuild_allocations() - allocs[-1]}), flush=True)
            dA.close()
            d2.close()
        s.close()


if __name__ == "__main__":
    main()
