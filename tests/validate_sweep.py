"""The mutation sweep and fuzz of rt_validate_scene (test_validate_cpu.py runs this file in a child process).

Every mutant of a valid scene goes to rt_validate_scene; whatever it accepts must have an empty access audit (wire_audit.py) under
both layouts, whatever it refuses must be refused with RT_E_INVALID or RT_E_UNSUPPORTED and a message.  The same mutants go to the
other host entry points that read wire arrays without a device (rt_blas_ranges, rth_bvh4_from_nodes): those only have to return.

A mutant's description is appended to the log file BEFORE the library sees it, so a crash of the library names its mutant: the
parent reads the last line.  Run as   python validate_sweep.py LOG RESULT.json"""
import dataclasses
import itertools
import json
import sys
import time

import numpy as np

import wire_audit as A
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.scenes import Scene, _std_materials

I32_MIN = -(1 << 31)
SEEDS = (20260, 20261)           # fuzz: fixed seeds
FUZZ_PER_PAIR = 6                # draws for every field pair of a record, per seed and scene
FUZZ_TRIPLES = 150               # three fields anywhere in the scene, per seed and scene

# record types: array -> [(field, sub-index or half, signed)]
FIELDS = {
    "bvh2": [("first", None, False), ("count", None, False)],
    "bvh4": [(f, k, True) for k in range(4) for f in ("first", "count")],
    "tlas": [("leftRight", "lo", False), ("leftRight", "hi", False), ("BLASidx", None, False)],
    "blas": [("bvhIdx", None, False)],
    "primIdx": [(None, None, False)],
    "lights": [(None, None, False)],
    "prims": [("objType", None, True), ("matIdx", None, True)],
    "mats": [("texIdx", None, True), ("texW", None, True), ("texH", None, True)],
}


# ---- base scenes ------------------------------------------------------------------------------------------------------------------------
def _tiny(builder="sah", leaf_root=False):
    s = Scene()
    _std_materials(s)
    s.AddTriangles(scenes.box_tris((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5)), "red")
    s.AddQuad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), "grey")
    s.AddQuad((-1, 3, -1), (1, 3, -1), (1, 3, 1), (-1, 3, 1), "white-light")
    if builder == "lbvh":
        s.BuildBLAS(0, 1.0, builder="lbvh", device=None, max_leaf=2)
    else:
        s.BuildBLAS(0, 1.0)
    if leaf_root:                # a second BLAS of one triangle: its root is a leaf
        st = s.num_prims
        s.AddTriangle((2, 0, 0), (3, 0, 0), (2, 1, 0), "green")
        s.BuildBLAS(st, 1.0)
    return s.arrays()


def base_scenes():
    """name -> (arrays, accels, exhaustive).  All from the repository's builders, all small."""
    import test_groundtruth_cpu as C
    out = {"one-blas": (_tiny(), (0, 1), True)}
    out["two-blas-alpha0"] = (scenes.two_blas_scene(0.0, 8)[0].arrays(), (0, 1), False)
    out["two-blas-alpha1"] = (scenes.two_blas_scene(1.0, 8)[0].arrays(), (0, 1), False)
    out["tlas-four-instances"] = (C.tlas_scene(0.0)[1], (0, 1), False)
    tex = scenes.mixed_scene(1.0, True)[0].arrays()
    m = tex.mats[tex.mats["texIdx"] != -1]
    assert len(m) and int((m["texIdx"].astype(np.int64) + m["texW"].astype(np.int64) * m["texH"]).max()) == len(tex.tex), \
        "the textured base scene must have a window that ends exactly at nTexels"
    out["textured"] = (tex, (0, 1), False)
    out["lbvh"] = (_tiny("lbvh"), (0, 1), False)
    out["leaf-root"] = (_tiny(leaf_root=True), (0, 1), False)
    assert int(out["leaf-root"][0].bvh2["count"][out["leaf-root"][0].blas["bvhIdx"][1]]) > 0
    return out


def limit_scenes():
    """Scenes on either side of every limit no single-field mutant of a small scene can reach: (name, arrays, accel, accepted).  The
    trees at the limit are those of capacity_check; one step beyond, validation must refuse and - should it ever not - the audit
    reports the stack or the 15-bit id."""
    import capacity_check as CC
    out = []
    for h, ok in ((64, True), (65, False)):
        out.append((f"chain({h})", CC.chain(h).sa, 0, ok))                    # BVH2 height against RT_BVH4_STACK
    for levels, ok in ((21, True), (22, False)):
        out.append((f"comb({levels})", CC.comb(levels).sa, 1, ok))            # BVH4 pending entries: 64 / 67
    for d, ok in ((32, True), (33, False)):
        out.append((f"tlas_chain({d}, 1)", CC.tlas_chain(d, 1).sa, 0, ok))    # TLAS depth against RT_TLAS_STACK
    sa = _tiny()
    for n, ok in ((0x8000, True), (0x8001, False)):                           # ids on the 16-bit TLAS stack entries: bit 15 is the leaf bit
        t = np.zeros(n, W.TLASNode)
        t["aabbMin"][:], t["aabbMax"][:] = sa.tlas["aabbMin"][0], sa.tlas["aabbMax"][0]
        t["leftRight"][0] = 1 | ((n - 1) << 16)
        out.append((f"tlas of {n} nodes, node {n - 1} reachable", dataclasses.replace(sa, tlas=t), 0, ok))
        leaf = sa.tlas[:1].copy()
        leaf["leftRight"], leaf["BLASidx"] = 0, n - 1
        out.append((f"{n} instances, instance {n - 1} named", dataclasses.replace(sa, tlas=leaf, blas=np.repeat(sa.blas[:1], n)), 0, ok))
    return out


# ---- calling the library ----------------------------------------------------------------------------------------------------------------
def validate(sa, accel, counts=None):
    """(code, message) of rt_validate_scene; counts override the arrays' lengths."""
    lib, P = W.device_lib(), W.ptr
    n = A.counts_of(sa, accel)
    n.update(counts or {})
    nodes = sa.nodes(accel)
    rc = lib.rt_validate_scene(accel, P(sa.prims), n["nPrims"], P(sa.mats), n["nMats"], P(sa.tex) if len(sa.tex) else None, n["nTexels"],
                               P(sa.lights) if len(sa.lights) else None, n["nLights"], P(nodes), n["nNodes"], P(sa.primIdx), n["nIdx"],
                               P(sa.tlas), n["nTlas"], P(sa.blas), n["nBlas"])
    return rc, (lib.rt_last_error() or b"").decode(errors="replace") if rc != 0 else ""


def other_entry_points(sa, counts=None):
    """rt_blas_ranges and rth_bvh4_from_nodes on the BVH2 arrays: any code, but they must return.  (The refit / rebuild restatements of
    rt355_host.h take a scene handle or primitives, never caller-made index arrays.)"""
    n = A.counts_of(sa, 0)
    n.update(counts or {})
    P = W.ptr
    first, count = np.zeros(max(n["nBlas"], 1), np.int32), np.zeros(max(n["nBlas"], 1), np.int32)
    W.device_lib().rt_blas_ranges(P(sa.bvh2), n["nNodes"], P(sa.primIdx), n["nIdx"], n["nPrims"], P(sa.blas), n["nBlas"], P(first), P(count))
    out = np.zeros(len(sa.bvh2), W.BVHNode4)
    W.host_lib().rth_bvh4_from_nodes(P(sa.bvh2), n["nNodes"], P(out))


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
def apply(sa, muts):
    """A copy of the scene with (array, index, field, sub, value) applied; value is the bit pattern's value in the field's signedness."""
    new = {}
    for arr, i, field, sub, val in muts:
        a = new.setdefault(arr, getattr(sa, arr).copy())
        if field is None:
            a[i] = val
        elif arr == "bvh4":
            a[field][i][sub] = val
        elif sub in ("lo", "hi"):
            lr = int(a[field][i])
            a[field][i] = (lr & 0xffff0000) | val if sub == "lo" else (lr & 0xffff) | (val << 16)
        else:
            a[field][i] = val
    return dataclasses.replace(sa, **new)


def _wrap(v, signed, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >= 1 << (bits - 1) else v


def boundary_values(ns, signed, related=(), bits=32):
    """The issue's value list in the field's own signedness (a value the field cannot hold is taken as its bit pattern); ns: the
    lengths of the arrays the field indexes; related: the node's own index, its parent's and its sibling's."""
    vals = [0, 1, (1 << 15) - 1, 1 << 15, (1 << 16) - 1, 1 << 16, (1 << 24) - 1, 1 << 24, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1,
            -1, -2, I32_MIN, 127, 128]
    for n in ns:
        vals += [n - 2, n - 1, n, n + 1]
    vals += [r for r in related if r is not None]
    return sorted({_wrap(int(v), signed, bits) for v in vals})


def _indexed(arr, field, n):
    """The lengths of the arrays a field can index."""
    return {("bvh2", "first"): (n["nNodes"], n["nIdx"]), ("bvh2", "count"): (n["nIdx"],), ("bvh4", "first"): (n["nNodes"], n["nIdx"]),
            ("bvh4", "count"): (n["nIdx"],), ("tlas", "leftRight"): (n["nTlas"],), ("tlas", "BLASidx"): (n["nBlas"],),
            ("blas", "bvhIdx"): (n["nNodes"],), ("primIdx", None): (n["nPrims"],), ("lights", None): (n["nPrims"],),
            ("prims", "objType"): (3,), ("prims", "matIdx"): (n["nMats"],), ("mats", "texIdx"): (n["nTexels"],),
            ("mats", "texW"): (n["nTexels"],), ("mats", "texH"): (n["nTexels"],)}[(arr, field)]


def topology(sa, accel):
    """Of the unmutated scene: per tree array {node: (parent, sibling)} of the reachable nodes, by the builders' own rules."""
    out = {}
    nodes = sa.nodes(accel)
    rel, todo = {}, [(int(r), None, None) for r in sa.blas["bvhIdx"]]
    while todo:
        i, p, s = todo.pop()
        if i in rel:
            continue
        rel[i] = (p, s)
        if accel == 0:
            if nodes["count"][i] == 0:
                f = int(nodes["first"][i])
                todo += [(f, i, f + 1), (f + 1, i, f)]
        else:
            kids = [int(nodes["first"][i][k]) for k in range(4) if nodes["first"][i][k] != -1 and nodes["count"][i][k] == 0]
            todo += [(c, i, next((d for d in kids if d != c), None)) for c in kids]
    out["bvh4" if accel else "bvh2"] = rel
    rel, todo = {}, [(0, None, None)]
    while todo:
        i, p, s = todo.pop()
        rel[i] = (p, s)
        lr = int(sa.tlas["leftRight"][i])
        if lr:
            todo += [(lr & 0xffff, i, lr >> 16), (lr >> 16, i, lr & 0xffff)]
    out["tlas"] = rel
    return out


def sample(sa, accel, arr, topo, exhaustive):
    """Deterministic record sample: for trees the roots, two interior nodes, two leaves, the last node and one unreachable node; for
    flat arrays the first, a middle and the last record.  Every record on the exhaustive scene."""
    n = len(sa.nodes(accel) if arr in ("bvh2", "bvh4") else getattr(sa, arr))
    if n == 0:
        return []
    if exhaustive:
        return list(range(n))
    if arr not in topo:
        return sorted({0, n // 2, n - 1})
    rel, nodes = topo[arr], sa.nodes(accel) if arr != "tlas" else sa.tlas
    reach = sorted(rel)
    if arr == "tlas":
        leaf = [i for i in reach if nodes["leftRight"][i] == 0]
    elif arr == "bvh2":
        leaf = [i for i in reach if nodes["count"][i] > 0]
    else:
        leaf = [i for i in reach if not ((nodes["first"][i] != -1) & (nodes["count"][i] == 0)).any()]
    inner = [i for i in reach if i not in set(leaf) and rel[i][0] is not None]
    roots = [i for i in reach if rel[i][0] is None]
    unreach = [i for i in range(n) if i not in rel]
    return sorted(set(roots[:2] + inner[:1] + inner[-1:] + leaf[:1] + leaf[-1:] + [n - 1] + unreach[:1]))


def sweep_mutants(sa, accel, exhaustive):
    """Every (field, boundary value) on the sampled records of every array, one field at a time."""
    n, topo = A.counts_of(sa, accel), topology(sa, accel)
    for arr, fields in FIELDS.items():
        if arr == ("bvh4", "bvh2")[accel]:
            continue
        for i in sample(sa, accel, arr, topo, exhaustive):
            related = (i,) + tuple(topo[arr].get(i, (None, None))) if arr in topo else ()
            for field, sub, signed in fields:
                bits = 16 if sub in ("lo", "hi") else 32
                for v in boundary_values(_indexed(arr, field, n), signed, related, bits):
                    yield [(arr, i, field, sub, v)]


def fuzz_mutants(sa, accel, seed):
    """Two fields of one record at once - every pair of a record type, FUZZ_PER_PAIR draws each - and three fields anywhere."""
    rng = np.random.default_rng(seed)
    n, topo = A.counts_of(sa, accel), topology(sa, accel)

    def draw(arr, i, field, sub, signed):
        related = (i,) + tuple(topo[arr].get(i, (None, None))) if arr in topo else ()
        vals = boundary_values(_indexed(arr, field, n), signed, related, 16 if sub in ("lo", "hi") else 32)
        return (arr, i, field, sub, vals[int(rng.integers(len(vals)))])
    arrays = [a for a in FIELDS if a != ("bvh4", "bvh2")[accel] and len(sa.nodes(accel) if a in ("bvh2", "bvh4") else getattr(sa, a))]
    size = lambda a: len(sa.nodes(accel) if a in ("bvh2", "bvh4") else getattr(sa, a))
    for arr in arrays:
        for fa, fb in itertools.combinations(FIELDS[arr], 2):
            for _ in range(FUZZ_PER_PAIR):
                i = int(rng.integers(size(arr)))
                yield [draw(arr, i, *fa), draw(arr, i, *fb)]
    flat = [(a, f) for a in arrays for f in FIELDS[a]]
    for _ in range(FUZZ_TRIPLES):
        picks = [flat[int(k)] for k in rng.choice(len(flat), 3, replace=False)]
        yield [draw(a, int(rng.integers(size(a))), *f) for a, f in picks]


def describe(name, accel, muts, counts=None):
    m = "; ".join(f"{a}[{i}]" + (f".{f}" if f else "") + (f"[{s}]" if s is not None else "") + f" = {v}" for a, i, f, s, v in muts)
    return f"{name} accel {accel}: {m or 'unmutated'}" + (f" counts {counts}" if counts else "")


# ---- the property -----------------------------------------------------------------------------------------------------------------------
class Tally:
    def __init__(self, log):
        self.log = log
        self.mutants = self.accepted = self.refused = self.over_refused = 0
        self.failures, self.over, self.messages = [], [], {}

    def check(self, name, sa, accel, muts, counts=None, must_accept=False):
        what = describe(name, accel, muts, counts)
        self.log.write(what + "\n")
        self.log.flush()
        m = apply(sa, muts) if muts else sa
        rc, msg = validate(m, accel, counts)
        if accel == 0:
            other_entry_points(m, counts)
        self.mutants += 1
        if rc == W.RT_OK:
            self.accepted += 1
            v = A.audit_both(m, accel, counts)
            if v:
                self.failures.append(f"ACCEPTED but unsafe: {what}: {v[0].array}[{v[0].index}] via {v[0].path}")
            return
        self.refused += 1
        key = "".join(c for c in msg if not c.isdigit())
        self.messages[key] = self.messages.get(key, 0) + 1
        if must_accept:
            self.failures.append(f"REFUSED a valid scene: {what}: {rc} {msg}")
        if rc not in (W.RT_E_INVALID, W.RT_E_UNSUPPORTED) or not msg:
            self.failures.append(f"refused with code {rc}, message {msg!r}: {what}")
        # layout 1's accesses include layout 0's wherever the derived layout is taken (and equal them elsewhere)
        if not A.audit(m, accel, 1, counts):
            self.over_refused += 1
            if len(self.over) < 40:
                self.over.append(f"{what}: {msg}")


def run(log_path):
    t0 = time.time()
    with open(log_path, "a") as log:
        T = Tally(log)
        per_scene = {}
        for name, (sa, accels, exhaustive) in base_scenes().items():
            before = T.mutants
            for accel in accels:
                T.check(name, sa, accel, [], must_accept=True)
                for c in A.COUNTS:                               # every count shortened by one, the arrays unchanged
                    T.check(name, sa, accel, [], {c: A.counts_of(sa, accel)[c] - 1})
                for muts in sweep_mutants(sa, accel, exhaustive):
                    T.check(name, sa, accel, muts)
                for seed in SEEDS:
                    for muts in fuzz_mutants(sa, accel, seed):
                        T.check(name, sa, accel, muts)
            per_scene[name] = T.mutants - before
        for name, sa, accel, ok in limit_scenes():
            T.check(name, sa, accel, [], must_accept=ok)         # (an over-limit scene, were it accepted, fails its audit there)
            per_scene["limits"] = per_scene.get("limits", 0) + 1
    return dict(mutants=T.mutants, accepted=T.accepted, refused=T.refused, over_refused=T.over_refused, failures=T.failures,
                over_refused_examples=T.over, refusal_messages=T.messages, per_scene=per_scene, seconds=round(time.time() - t0, 2))


if __name__ == "__main__":
    res = run(sys.argv[1])
    with open(sys.argv[2], "w") as f:
        json.dump(res, f, indent=1)
