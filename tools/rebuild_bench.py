"""Cost of an in-place BLAS rebuild (rt_rebuild_scene) against the round trip it removes, on one GPU.

    python tools/rebuild_bench.py [--reps 10] [--frames 20] [--builders sah,lbvh,sbvh,refit] [--host-reps 1] [--accel bvh2|bvh4]

For sponza-class (every vertex scrambled across the triangles) and config 5 (every vertex jittered), three ways to bring a bound scene
up to date are timed in one process, alternating within each repetition (min / median / max of --reps after a warm-up):
  A  Device.rebuild_scene(prims, builder="sah" | "lbvh"): wall ms, gpu_ms and its split (stage, builds, derive, TLAS, commit);
  B  the way to the same arrays without it, minus the scene generator: rt_build_bvh2_sah (resp. rt_build_bvh2) per BLAS on caller
     arrays, the TLAS on the host, rt_upload_scene into a second context (the first repetition checks that B's eleven device arrays
     equal A's);
  C  Device.update_scene(prims) of the same records, for scale.
Then the trace rate (M samples/s over --frames frames) on sponza-class with the vertices scrambled among every 64 consecutive
triangles (a deformation that leaves a tree something to cull): the scene as built, after the refit alone, after the rebuild.
One JSON line per scene and builder.

--builders sbvh: the SBVH rebuild (builder="sbvh_gpu"), sponza-class at alpha 0.5 and 0 and config 5 at alpha 0 (the alpha both its
BLAS are built with), against the two ways to the same trees that exist without it, in the same run:
  a  rt_build_bvh2_sbvh per BLAS (the tree comes back to the host), the TLAS on the host, rt_upload_scene into a second context (the
     first repetition checks that its eleven device arrays equal the rebuild's);
  b  the same triangles built from scratch on the host by BuildBLAS(alpha) at 16 threads, BuildTLAS, rt_upload_scene (--host-reps times).
For config 5 also what the feature is for, the trace rate of the jittered scene in three states: refit alone (the SBVH leaves have
lost their clipped boxes), rebuilt with "sah" (no spatial splits), rebuilt with "sbvh_gpu" at alpha 0.

--accel bvh4: a BVH4 context bound with its BVH2 (Device.upload(sa, from_bvh2=True)), builders "sah" and "lbvh" of --builders, on the
same two scenes and deformations, alternating within each repetition:
  A  Device.rebuild_scene(prims, builder) in place: the BLAS builds, the BVH2 -> BVH4 collapse, quad records and TLAS on the device;
  H  the only way there was: Scene.SetPrimitives + Scene.Rebuild (the builder's host restatement, rth_rebuild), Scene.BuildBVH4
     (BVH4::Convert / Collapse, sequential), BuildTLAS and rt_upload_scene of everything into a second context, each part timed (the
     first repetition checks that H's thirteen device arrays equal A's);
and the collapse alone on the rebuilt BVH2 of the last repetition: rt_build_bvh4 (wall with both transfers, and its device_ms)
against Scene.BuildBVH4.  One JSON line per scene and builder.

--builders refit (with either --accel; name it alone or with "sah" / "lbvh", which then only serve as yardsticks): the refit of every
primitive, rebuild_scene(prims, builder="refit"), on both scenes with every vertex jittered, alternating within each repetition with
  a  what a BVH4 copy had before: rebuild_scene(prims, builder) with the "lbvh" and "sah" of --builders, on contexts of their own;
  b  Device.update_scene(prims) of the same records on a BVH2 context (--accel bvh2: the first repetition checks that its eleven
     device arrays equal the refit's);
  c  --accel bvh4: the refit itself with RT355_REFIT_RECOLLAPSE=1, the level-by-level collapse forced, on a context of its own (the
     first repetition checks that its thirteen device arrays equal the in-place ones);
and how many of the repetitions, each a new jitter of the scene as built and so two jitters away from the frame before, stayed in
place (refit_info path 1) and how many re-collapsed, with the changed nodes of those; --accel bvh4: then the last records handed over
again --reps times, which is in place by construction (identical boxes): what the in-place path costs when it applies.  One JSON line
per scene."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magr_ray_tracer_amd import _lib as W, scenes  # noqa: E402
from magr_ray_tracer_amd.renderer import Device  # noqa: E402
from magr_ray_tracer_amd.scene import SceneArrays, blas_ranges, build_lbvh, build_sah_gpu, build_sbvh_gpu  # noqa: E402
from magr_ray_tracer_amd.scenes import Scene, _std_materials  # noqa: E402

RW, RH = 1280, 720


def mmm(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3), round(max(xs), 3)]


def scrambled(prims, seed):
    rng = np.random.default_rng(seed)
    p = prims.copy()
    tri = np.where(p["objType"] == W.PRIM_TRIANGLE)[0]
    v = np.stack([p["v0"][tri], p["v1"][tri], p["v2"][tri]], axis=1).reshape(-1, 4)
    v = v[rng.permutation(len(v))].reshape(-1, 3, 4)
    p["v0"][tri], p["v1"][tri], p["v2"][tri] = v[:, 0], v[:, 1], v[:, 2]
    return p


def scrambled_locally(prims, seed, block=64):
    """Vertices scrambled among each run of `block` consecutive triangles: triangles several times their size that stay where they were,
    which a refit follows badly and a tree can still cull."""
    rng = np.random.default_rng(seed)
    p = prims.copy()
    tri = np.where(p["objType"] == W.PRIM_TRIANGLE)[0]
    v = np.stack([p["v0"][tri], p["v1"][tri], p["v2"][tri]], axis=1)
    for a in range(0, len(v), block):
        w = v[a:a + block].reshape(-1, 4)
        v[a:a + block] = w[rng.permutation(len(w))].reshape(-1, 3, 4)
    p["v0"][tri], p["v1"][tri], p["v2"][tri] = v[:, 0], v[:, 1], v[:, 2]
    return p


def jittered(prims, seed):
    rng = np.random.default_rng(seed)
    p = prims.copy()
    for f in ("v0", "v1", "v2"):
        p[f][:, :3] += rng.normal(scale=1e-3, size=(len(p), 3)).astype(np.float32)
    return p


def small_tlas(nodes, inst):
    """TLAS::Build for one or two identity instances (what the two scenes have): leaves at 1 + i, the join behind them, node 0 = root."""
    n = len(inst)
    assert n in (1, 2) and all(np.array_equal(i["invT"], np.eye(4, dtype=np.float32).ravel()) for i in inst)
    t = np.zeros(2 * n, W.TLASNode)
    for i in range(n):
        r = nodes[int(inst["bvhIdx"][i])]
        t["aabbMin"][1 + i], t["aabbMax"][1 + i], t["BLASidx"][1 + i] = r["aabbMin"], r["aabbMax"], i
    if n == 2:
        t["aabbMin"][3], t["aabbMax"][3] = np.minimum(t["aabbMin"][1], t["aabbMin"][2]), np.maximum(t["aabbMax"][1], t["aabbMax"][2])
        t["leftRight"][3] = 1 + (2 << 16)
    t[0] = t[2 * n - 1]
    return t


def round_trip(sa, prims, ranges, builder, d2, alpha=None):
    """B: per-BLAS GPU builds on caller arrays, host TLAS, upload.  Returns (wall ms, sum of the builders' device_ms)."""
    t0 = time.perf_counter()
    nodes, idx, roots, dev = [], [], {}, 0.0
    nb = ib = 0
    for first, count in sorted(set(ranges)):
        if builder == "sbvh":
            n, i, st = build_sbvh_gpu(prims, alpha, first=first, count=count, device=0, node_base=nb, idx_base=ib)
        else:
            fn = build_sah_gpu if builder == "sah" else build_lbvh
            n, i, st = fn(prims, first=first, count=count, device=0, node_base=nb, idx_base=ib)
        roots[(first, count)] = nb
        nodes.append(n)
        idx.append(i)
        nb += len(n)
        ib += len(i)
        dev += st["device_ms"]
    nodes, idx = np.concatenate(nodes), np.concatenate(idx)
    inst = sa.blas.copy()
    inst["bvhIdx"] = [roots[r] for r in ranges]
    new = SceneArrays(prims=prims, mats=sa.mats, tex=sa.tex, lights=sa.lights, bvh2=nodes, bvh4=sa.bvh4, primIdx=idx,
                      tlas=small_tlas(nodes, inst), blas=inst)
    d2.upload(new)
    return (time.perf_counter() - t0) * 1e3, dev


def trace_rate(d, cam, frames):
    d.seed_default()
    d.reset()
    d.render(cam, 2)
    d.synchronize()
    t0 = time.perf_counter()
    d.render(cam, frames)
    d.synchronize()
    return round(RW * RH * frames / (time.perf_counter() - t0) / 1e6, 3)


def host_from_scratch(prims, ranges, alpha, d2):
    """b: the triangles built from scratch on the host, BLAS after BLAS, by BuildBLAS(alpha) at 16 threads, BuildTLAS, upload.
    Returns (wall ms of the builds, TLAS and upload; of the BuildBLAS calls alone)."""
    assert np.all(prims["objType"] == W.PRIM_TRIANGLE)
    s = Scene()
    _std_materials(s)
    wall = build = 0.0
    for first, count in sorted(set(ranges)):
        q = prims[first:first + count]
        s.AddTriangles(np.stack([q["v0"][:, :3], q["v1"][:, :3], q["v2"][:, :3]], axis=1), "white")   # (not timed: the caller has its records)
        t0 = time.perf_counter()
        s.BuildBLAS(first, alpha=alpha, threads=16)
        build += (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    d2.upload(s.arrays(bvh4=False))
    wall = build + (time.perf_counter() - t0) * 1e3
    s.close()
    return wall, build


def sbvh_cases(a):
    """The SBVH rebuild against routes a and b; config 5's trace rate refit / rebuilt without / rebuilt with spatial splits."""
    # (the rebuild does not depend on how the scene was first built: sponza-class is bound as the plain SAH tree, which builds fast;
    # config 5 as what the benchmark measures, both BLAS at alpha 0, built by the GPU builder - the same arrays as the host's)
    cases = (("sponza_class", 0.5, lambda: scenes.sponza_class(1.0), scrambled), ("sponza_class", 0.0, lambda: scenes.sponza_class(1.0), scrambled),
             ("config5", 0.0, lambda: scenes.config5_scene(0.0, builder="sbvh_gpu", device=0), jittered))
    for name, alpha, make, move in cases:
        s, view = make()
        sa = s.arrays(bvh4=False)
        ranges = blas_ranges(sa)
        cam = scenes.camera_for(view, RW, RH)
        d2 = Device(320, 240)
        dA = Device(RW, RH)
        dA.upload(sa)
        allocs = []
        for k in range(3):                            # warm-up: both sets grown, the builder's blocks pooled
            dA.rebuild_scene(move(sa.prims, 100 + k), builder="sbvh_gpu", alpha=alpha)
            allocs.append(dA.rebuild_allocations())
        round_trip(sa, move(sa.prims, 100), ranges, "sbvh", d2, alpha)
        A, Ag, Ra, Rad = [], [], [], []
        split = {k: [] for k in ("stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms")}
        for r in range(a.reps):
            p = move(sa.prims, r + 1)
            t0 = time.perf_counter()
            st = dA.rebuild_scene(p, builder="sbvh_gpu", alpha=alpha)
            A.append((time.perf_counter() - t0) * 1e3)
            Ag.append(st["gpu_ms"])
            for k in split:
                split[k].append(st[k])
            w, dev = round_trip(sa, p, ranges, "sbvh", d2, alpha)
            Ra.append(w)
            Rad.append(dev)
            if r == 0:
                for k in W.SCENE_ARRAYS:
                    assert np.array_equal(dA.scene_array(k), d2.scene_array(k)), f"{name} / sbvh alpha {alpha}: route a's {k} differs from the rebuild's"
        allocs.append(dA.rebuild_allocations())
        Rb, Rbb = [], []
        for r in range(a.host_reps):
            w, bw = host_from_scratch(move(sa.prims, r + 1), ranges, alpha, d2)
            Rb.append(w)
            Rbb.append(bw)
        mA = statistics.median(A)
        out = {"scene": name, "builder": "sbvh_gpu", "alpha": alpha, "prims": int(len(sa.prims)), "nodes": st["nodes"], "n_idx": st["n_idx"],
               "max_depth": st["max_depth"], "spatial_splits": st["spatial_splits"], "prims_clipped": st["prims_clipped"],
               "A_wall_ms": mmm(A), "A_gpu_ms": mmm(Ag), "A_split_ms": {k: round(statistics.median(v), 3) for k, v in split.items()},
               "a_wall_ms": mmm(Ra), "a_builders_device_ms": mmm(Rad), "A_over_a": round(mA / statistics.median(Ra), 3),
               "allocations_after_warmups_and_reps": allocs}
        if Rb:
            out.update({"b_wall_ms": mmm(Rb), "b_buildblas_ms": mmm(Rbb), "A_over_b": round(mA / statistics.median(Rb), 4)})
        if name == "config5":
            dT = Device(RW, RH)
            dT.upload(sa)
            out["trace_built_Msps"] = trace_rate(dT, cam, a.frames)           # the scene as built, for scale
            p = move(sa.prims, 7)
            dT.update_scene(p)
            out["trace_refit_only_Msps"] = trace_rate(dT, cam, a.frames)
            dT.rebuild_scene(p, builder="sah")
            out["trace_rebuilt_sah_Msps"] = trace_rate(dT, cam, a.frames)
            dA.rebuild_scene(p, builder="sbvh_gpu", alpha=alpha)
            out["trace_rebuilt_sbvh_Msps"] = trace_rate(dA, cam, a.frames)
            dT.close()
        print(json.dumps(out), flush=True)
        dA.close()
        d2.close()
        s.close()


def bvh4_cases(a, which):
    """--accel bvh4: the in-place rebuild of a BVH4 copy against rebuild + collapse on the host + upload; the collapse alone."""
    from magr_ray_tracer_amd.scene import build_bvh4_gpu
    b4 = dict(accel=W.ACCEL_BVH4)
    arrays = [k for k in list(W.SCENE_ARRAYS) + list(W.SCENE_ARRAYS_BVH4) if k != "bvh2Kept"]
    cases = {"sponza_class": (lambda: scenes.sponza_class(1.0), scrambled), "config5": (lambda: scenes.config5_scene(0.0), jittered)}
    for name, (make, move) in cases.items():
        s, view = make()
        sa = s.arrays()
        d2 = Device(320, 240, **b4)
        for builder in [b for b in which if b in ("sah", "lbvh")]:
            dA = Device(RW, RH, **b4)
            dA.upload(sa, from_bvh2=True)
            for k in range(2):                        # warm-up: both sets of arrays, the builders' workspace, the collapse's scratch
                dA.rebuild_scene(move(sa.prims, 100 + k), builder=builder)
            A, Ag, H = [], [], {k: [] for k in ("wall", "rebuild", "collapse", "tlas_and_views", "upload")}
            split = {k: [] for k in ("stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms")}
            for r in range(a.reps):
                p = move(sa.prims, r + 1)
                t0 = time.perf_counter()
                st = dA.rebuild_scene(p, builder=builder)
                A.append((time.perf_counter() - t0) * 1e3)
                Ag.append(st["gpu_ms"])
                for k in split:
                    split[k].append(st[k])
                t0 = time.perf_counter()
                s.SetPrimitives(0, p)
                s.Rebuild(builder)
                t1 = time.perf_counter()
                s.BuildBVH4()
                t2 = time.perf_counter()
                new = s.arrays(bvh4=False)            # BuildTLAS and the copies out of the host library
                new.bvh4 = K_view(s)
                t3 = time.perf_counter()
                d2.upload(new)
                t4 = time.perf_counter()
                for k, v in zip(H, (t4 - t0, t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    H[k].append(v * 1e3)
                if r == 0:
                    for k in arrays:
                        assert np.array_equal(dA.scene_array(k), d2.scene_array(k)), f"{name} / {builder}: H's {k} differs from A's"
            roots = new.blas["bvhIdx"].astype(np.uint32)
            Cw, Cd, Ch = [], [], []
            for r in range(a.reps):
                t0 = time.perf_counter()
                n4, cs = build_bvh4_gpu(new.bvh2, roots, len(new.primIdx), device=0)
                Cw.append((time.perf_counter() - t0) * 1e3)
                Cd.append(cs["device_ms"])
                t0 = time.perf_counter()
                s.BuildBVH4()
                Ch.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(n4.view(np.uint8), K_view(s).view(np.uint8)), f"{name} / {builder}: rt_build_bvh4 differs from BuildBVH4"
            out = {"scene": name, "accel": "bvh4", "builder": builder, "prims": int(len(sa.prims)), "nodes": st["nodes"], "max_depth": st["max_depth"],
                   "live_nodes": cs["live_nodes"], "bvh4_levels": cs["levels"], "stack_need": cs["stack_need"],
                   "A_wall_ms": mmm(A), "A_gpu_ms": mmm(Ag), "A_split_ms": {k: round(statistics.median(v), 3) for k, v in split.items()},
                   "H_wall_ms": mmm(H["wall"]), "H_split_ms": {k: round(statistics.median(v), 3) for k, v in H.items() if k != "wall"},
                   "A_over_H": round(statistics.median(A) / statistics.median(H["wall"]), 4),
                   "collapse_gpu_wall_ms": mmm(Cw), "collapse_gpu_device_ms": mmm(Cd), "collapse_host_ms": mmm(Ch)}
            print(json.dumps(out), flush=True)
            dA.close()
        d2.close()
        s.close()


def refit_cases(a, which):
    """--builders refit: the refit against the rebuilds, rt_update_scene and its own forced fallback; how often it stays in place."""
    bvh4 = a.accel == "bvh4"
    kw = dict(accel=W.ACCEL_BVH4) if bvh4 else {}
    arrays = list(W.SCENE_ARRAYS) + ([k for k in W.SCENE_ARRAYS_BVH4 if k != "bvh2Kept"] if bvh4 else [])
    split_keys = ("stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms")

    def timed(fn):
        t0 = time.perf_counter()
        st = fn()
        return (time.perf_counter() - t0) * 1e3, st

    def forced(dev, p):
        os.environ["RT355_REFIT_RECOLLAPSE"] = "1"                  # (read per call)
        try:
            return dev.rebuild_scene(p, builder="refit")
        finally:
            del os.environ["RT355_REFIT_RECOLLAPSE"]

    for name, make in (("sponza_class", lambda: scenes.sponza_class(1.0)), ("config5", lambda: scenes.config5_scene(0.0))):
        s, view = make()
        sa = s.arrays()
        dR, dC = Device(RW, RH, **kw), Device(RW, RH)
        dR.upload(sa, from_bvh2=True)
        dC.upload(sa)
        dF = Device(RW, RH, **kw) if bvh4 else None
        if dF:
            dF.upload(sa, from_bvh2=True)
        others = {b: Device(RW, RH, **kw) for b in which if b in ("sah", "lbvh")}
        for dv in others.values():
            dv.upload(sa, from_bvh2=True)
        for k in range(3):                                            # warm-up: both sets, the staging buffers, the workspaces
            p = jittered(sa.prims, 100 + k)
            dR.rebuild_scene(p, builder="refit")
            dC.update_scene(p)
            if dF:
                forced(dF, p)
            for b, dv in others.items():
                dv.rebuild_scene(p, builder=b)
        allocs = dR.rebuild_allocations()
        R, Rg, F, Fg, U, Ug, paths, changed = [], [], [], [], [], [], [], []
        O = {b: ([], []) for b in others}
        split = {k: [] for k in split_keys}
        for r in range(a.reps):
            p = jittered(sa.prims, r + 1)
            w, st = timed(lambda: dR.rebuild_scene(p, builder="refit"))
            R.append(w)
            Rg.append(st["gpu_ms"])
            for k in split:
                split[k].append(st[k])
            info = dR.refit_info()
            paths.append(info["path"])
            changed.append(info["changed_nodes"])
            if dF:
                w, st = timed(lambda: forced(dF, p))
                F.append(w)
                Fg.append(st["gpu_ms"])
                assert dF.refit_info()["path"] == 3
            w, su = timed(lambda: dC.update_scene(p))
            U.append(w)
            Ug.append(su["gpu_ms"])
            for b, dv in others.items():
                w, so = timed(lambda: dv.rebuild_scene(p, builder=b))
                O[b][0].append(w)
                O[b][1].append(so["gpu_ms"])
            if r == 0:
                for k in arrays:
                    other = dF if bvh4 else dC
                    assert np.array_equal(dR.scene_array(k), other.scene_array(k)), f"{name}: {k} differs between the refit and its yardstick"
        S, Sg = [], []                                                # the last records again: identical boxes, in place by construction
        for r in range(a.reps if bvh4 else 0):
            w, ss = timed(lambda: dR.rebuild_scene(p, builder="refit"))
            S.append(w)
            Sg.append(ss["gpu_ms"])
            assert dR.refit_info()["path"] == 1
        assert dR.rebuild_allocations() == allocs, "a refit of a stable scene allocated"
        mR = statistics.median(R)
        out = {"scene": name, "accel": a.accel, "builder": "refit", "prims": int(len(sa.prims)), "nodes": st["nodes"], "live_quads": info["live_quads"],
               "stack_need": info["stack_need"], "refit_wall_ms": mmm(R), "refit_gpu_ms": mmm(Rg),
               "refit_split_ms": {k: round(statistics.median(v), 3) for k, v in split.items()},
               "in_place": paths.count(1), "recollapsed": paths.count(2), "changed_nodes_when_recollapsed": [c for c in changed if c],
               "update_bvh2_wall_ms": mmm(U), "update_bvh2_gpu_ms": mmm(Ug), "refit_over_update": round(mR / statistics.median(U), 3)}
        if dF:
            out.update({"forced_wall_ms": mmm(F), "forced_gpu_ms": mmm(Fg), "refit_over_forced": round(mR / statistics.median(F), 3),
                        "same_records_in_place_wall_ms": mmm(S), "same_records_in_place_gpu_ms": mmm(Sg),
                        "in_place_over_forced": round(statistics.median(S) / statistics.median(F), 3)})
        for b, (w, g) in O.items():
            out.update({f"{b}_wall_ms": mmm(w), f"{b}_gpu_ms": mmm(g), f"refit_over_{b}": round(mR / statistics.median(w), 4)})
        print(json.dumps(out), flush=True)
        for dv in [dR, dC] + ([dF] if dF else []) + list(others.values()):
            dv.close()
        s.close()


def K_view(s):
    """The Scene's BVH4 array as a copy."""
    from magr_ray_tracer_amd.scene import _view
    return _view(s._lib.rth_bvh4_nodes, s._h, W.BVHNode4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--builders", default="sah,lbvh,sbvh")
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--accel", default="bvh2", choices=["bvh2", "bvh4"])
    a = ap.parse_args()
    which = a.builders.split(",")
    if "refit" in which:
        return refit_cases(a, which)
    if a.accel == "bvh4":
        return bvh4_cases(a, which)
    cases = {"sponza_class": (lambda: scenes.sponza_class(1.0), scrambled), "config5": (lambda: scenes.config5_scene(0.0), jittered)}
    if not [b for b in which if b in ("sah", "lbvh")]:
        cases = {}
    for name, (make, move) in cases.items():
        s, view = make()
        sa = s.arrays(bvh4=False)
        ranges = blas_ranges(sa)
        cam = scenes.camera_for(view, RW, RH)
        dC = Device(RW, RH)
        dC.upload(sa)
        dC.update_scene(move(sa.prims, 0))            # warm-up: allocates the staging buffers
        d2 = Device(320, 240)
        for builder in [b for b in which if b in ("sah", "lbvh")]:
            dA = Device(RW, RH)
            dA.upload(sa)
            for k in range(2):                        # warm-up: both sets of arrays and the builders' workspace
                dA.rebuild_scene(move(sa.prims, 100 + k), builder=builder)
            round_trip(sa, move(sa.prims, 100), ranges, builder, d2)
            A, Ag, B, Bd, Cw, Cg = [], [], [], [], [], []
            split = {k: [] for k in ("stage_ms", "build_ms", "derive_ms", "tlas_ms", "commit_ms")}
            for r in range(a.reps):
                p = move(sa.prims, r + 1)
                t0 = time.perf_counter()
                st = dA.rebuild_scene(p, builder=builder)
                A.append((time.perf_counter() - t0) * 1e3)
                Ag.append(st["gpu_ms"])
                for k in split:
                    split[k].append(st[k])
                w, dev = round_trip(sa, p, ranges, builder, d2)
                B.append(w)
                Bd.append(dev)
                if r == 0:
                    for k in W.SCENE_ARRAYS:
                        assert np.array_equal(dA.scene_array(k), d2.scene_array(k)), f"{name} / {builder}: B's {k} differs from A's"
                t0 = time.perf_counter()
                su = dC.update_scene(p)
                Cw.append((time.perf_counter() - t0) * 1e3)
                Cg.append(su["gpu_ms"])
            mA, mB = statistics.median(A), statistics.median(B)
            out = {"scene": name, "builder": builder, "prims": int(len(sa.prims)), "nodes": st["nodes"], "max_depth": st["max_depth"],
                   "A_wall_ms": mmm(A), "A_gpu_ms": mmm(Ag), "A_split_ms": {k: round(statistics.median(v), 3) for k, v in split.items()},
                   "B_wall_ms": mmm(B), "B_builders_device_ms": mmm(Bd), "C_wall_ms": mmm(Cw), "C_gpu_ms": mmm(Cg),
                   "A_over_B": round(mA / mB, 3), "B_spread_ms": round(max(B) - min(B), 3), "A_below_B_by_ms": round(mB - mA, 3),
                   "gpu_budget_ms": round(statistics.median(Bd) + statistics.median(Cg) + statistics.median(split["derive_ms"]), 3)}
            if name == "sponza_class":   # the number that tells when to call which: the same locally scrambled scene, refit and rebuilt
                dT = Device(RW, RH)
                dT.upload(sa)
                out["trace_built_Msps"] = trace_rate(dT, cam, a.frames)           # the scene as built, for scale
                p = scrambled_locally(sa.prims, 7)
                dT.update_scene(p)
                out["trace_refit_only_Msps"] = trace_rate(dT, cam, a.frames)
                dA.rebuild_scene(p, builder=builder)
                out["trace_rebuilt_Msps"] = trace_rate(dA, cam, a.frames)
                dT.close()
            print(json.dumps(out), flush=True)
            dA.close()
        d2.close()
        dC.close()
        s.close()
    if "sbvh" in which:
        sbvh_cases(a)


if __name__ == "__main__":
    main()
