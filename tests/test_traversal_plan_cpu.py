"""How a context chooses its traversal (csrc/trav_common.h: plan_traversal, read_trav_knobs), through rt_debug_traversal_plan; no GPU.
A table of literal cases: the facts, the RT355_* knobs in the environment, and EVERY field of the plan, worked out by hand from the
rules as the header's comments and INTEGRATION.md state them - not from a restatement of the conditions.

Column entries E = stackEntries + tlasDepth + 1.  A column with its ten backup words takes (E + 10) * 1024 bytes of LDS, so 64 KB hold
E <= 54 and a spill cap of at most 54; 160 KB hold all that is asked here."""
import pytest

from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.renderer import traversal_plan

KNOBS = ("RT355_SPILL_CAP", "RT355_NO_SPILL", "RT355_COHERENT", "RT355_TUNE", "RT355_FIXED_CHUNKS", "RT355_TUNE_CONNECT", "RT355_TOP_LEVELS",
         "RT355_TLAS_FLAT", "RT355_XCD_RAYS", "RT355_THIN", "RT355_CONNECT_BLOCKS")
NESTED, BVH2, TLAS, TLAS_SPILL, BVH4, BVH4_TLAS, BVH4_TLAS_SPILL = range(7)
XCD = 5


def one(**kw):
    """Facts of a single-BLAS scene in layout 1 on a BVH2 context that has the GPU to itself."""
    f = dict(accel=W.ACCEL_BVH2, extend_variant=0, persist_blocks_per_cu=0, layout=1, singleBlas=1, tlasDepth=0, nInterior=1000, nQuads=1000,
             stackEntries=20, sharedMemPerBlock=65536, xcdFirst=XCD)
    f.update(kw)
    return f


def many(E=20, **kw):
    """... of a scene of several BLAS under a TLAS of one level, with E column entries."""
    return one(**{**dict(singleBlas=0, tlasDepth=1, stackEntries=E - 2), **kw})


def many4(E=20, **kw):
    """... on a BVH4 context with extend_variant 6."""
    return many(E, **{**dict(accel=W.ACCEL_BVH4, extend_variant=6), **kw})


def want(trav, spillCap=12, coherent=1, topAuto=False, tuneBlocks=0, connectBlocks=0, tune=None, tuneConnect=None, tune4=None, every=None):
    """The plan of a context alone on the GPU with no knob set, except for what the arguments name (`every`: on all three tunes)."""
    p = dict(trav=trav, spillCap=spillCap, coherent=coherent, topAuto=topAuto, tuneBlocks=tuneBlocks, connectBlocks=connectBlocks,
             tune=dict(chunk=112, refill=24, inner=6, leafK=8, fixedChunks=1, flat=0, xcdRays=1024, xcdFirst=XCD, thin=16, topLevels=0, topBase=0),
             tuneConnect=dict(chunk=128, refill=32, inner=6, leafK=16, fixedChunks=1, flat=0, xcdRays=1024, xcdFirst=XCD, thin=16, topLevels=0, topBase=0),
             tune4=dict(chunk=64, refill=20, inner=6, leafK=8, fixedChunks=1, flat=0, xcdRays=1024, xcdFirst=XCD, thin=16, topLevels=0, topBase=0))
    for name, over in (("tune", tune), ("tuneConnect", tuneConnect), ("tune4", tune4)):
        p[name].update(every or {})
        p[name].update(over or {})
    return p


def bvh2(**kw):
    """TRAV_BVH2 takes top tables of 6 / 6 levels, to be fitted to the device."""
    kw = {**dict(topAuto=True, tune={}, tuneConnect={}), **kw}
    kw["tune"] = {"topLevels": 6, **kw["tune"]}
    kw["tuneConnect"] = {"topLevels": 6, **kw["tuneConnect"]}
    return want(BVH2, **kw)


def tlas(trav, **kw):
    """The four TLAS kinds run extend flat (tune and tune4) and connect through the event loop."""
    return want(trav, tune={"flat": 1}, tune4={"flat": 1}, **kw)


TUNED = dict(chunk=64, refill=20, inner=6, leafK=8, fixedChunks=0)   # RT355_TUNE=64,20,6,8: all three tunes, fixedChunks 0 with them

CASES = [
    # one BLAS
    ("one BLAS, BVH2", one(), {}, bvh2()),
    ("one BLAS, BVH4", one(accel=W.ACCEL_BVH4), {}, want(BVH4)),
    ("one BLAS, layout 0", one(layout=0), {}, want(NESTED)),
    ("one BLAS, extend_variant 2", one(extend_variant=2), {}, want(NESTED)),
    ("one BLAS, BVH4, extend_variant 6", one(accel=W.ACCEL_BVH4, extend_variant=6), {}, want(BVH4)),
    # several BLAS, BVH2
    ("tlasDepth 8", many(tlasDepth=8, stackEntries=10), {}, tlas(TLAS)),
    ("tlasDepth 9", many(tlasDepth=9, stackEntries=10), {}, want(NESTED)),
    ("2^29 - 1 pair records", many(nInterior=2**29 - 1), {}, tlas(TLAS)),
    ("2^29 pair records", many(nInterior=2**29), {}, want(NESTED)),
    ("several BLAS, extend_variant 4", many(extend_variant=4), {}, want(NESTED)),
    # several BLAS, BVH4
    ("BVH4, extend_variant 0", many4(extend_variant=0), {}, want(NESTED)),
    ("BVH4, extend_variant 6", many4(), {}, tlas(BVH4_TLAS)),
    ("BVH4, 2^29 quad records", many4(nQuads=2**29), {}, want(NESTED)),
    ("BVH4, tlasDepth 9", many4(tlasDepth=9, stackEntries=8), {}, want(NESTED)),
    # column depth
    ("E = 22", many(22), {}, tlas(TLAS)),
    ("E = 23", many(23), {}, tlas(TLAS_SPILL)),
    ("E = 23, NO_SPILL", many(23), {"RT355_NO_SPILL": "1"}, tlas(TLAS)),
    ("E = 73, NO_SPILL", many(73), {"RT355_NO_SPILL": "1"}, tlas(TLAS)),
    ("E = 74, NO_SPILL", many(74), {"RT355_NO_SPILL": "1"}, want(NESTED)),                      # flat stays 0 on all three
    ("E = 23, NO_SPILL=0", many(23), {"RT355_NO_SPILL": "0"}, tlas(TLAS_SPILL)),
    # RT355_SPILL_CAP
    ("SPILL_CAP=6, E = 10", many(10), {"RT355_SPILL_CAP": "6"}, tlas(TLAS_SPILL, spillCap=6)),
    ("SPILL_CAP=6, E = 6", many(6), {"RT355_SPILL_CAP": "6"}, tlas(TLAS, spillCap=6)),
    ("SPILL_CAP=5 is ignored", many(20), {"RT355_SPILL_CAP": "5"}, tlas(TLAS)),                  # (forced, E = 20 > 12 would spill)
    ("SPILL_CAP=65 is ignored", many(20), {"RT355_SPILL_CAP": "65"}, tlas(TLAS)),
    ("SPILL_CAP=64, E = 65", many(65), {"RT355_SPILL_CAP": "64"}, tlas(TLAS_SPILL, spillCap=64)),
    # BVH4 TLAS against the LDS a workgroup may ask for
    ("BVH4 E = 22", many4(22), {}, tlas(BVH4_TLAS)),
    ("BVH4 E = 23", many4(23), {}, tlas(BVH4_TLAS_SPILL)),
    ("BVH4 E = 55, NO_SPILL", many4(55), {"RT355_NO_SPILL": "1"}, want(NESTED)),
    ("BVH4 E = 54, NO_SPILL", many4(54), {"RT355_NO_SPILL": "1"}, tlas(BVH4_TLAS)),
    ("BVH4 E = 65, SPILL_CAP=64 does not fit", many4(65), {"RT355_SPILL_CAP": "64"}, want(NESTED, spillCap=64)),
    ("BVH4 E = 30, SPILL_CAP=64 does not fit", many4(30), {"RT355_SPILL_CAP": "64"}, tlas(BVH4_TLAS, spillCap=64)),
    ("BVH4 E = 55, 160 KB", many4(55, sharedMemPerBlock=163840), {}, tlas(BVH4_TLAS_SPILL)),
    ("BVH4 E = 55, 160 KB, NO_SPILL", many4(55, sharedMemPerBlock=163840), {"RT355_NO_SPILL": "1"}, tlas(BVH4_TLAS)),
    # the tunes
    ("shared", one(persist_blocks_per_cu=2), {}, bvh2(tune={"leafK": 16}, every={"fixedChunks": 0})),
    ("RT355_TUNE alone", one(), {"RT355_TUNE": "64,20,6,8,1"}, bvh2(tuneBlocks=1, every=TUNED)),
    ("RT355_TUNE shared", one(persist_blocks_per_cu=2), {"RT355_TUNE": "64,20,6,8,1"}, bvh2(tuneBlocks=1, every=TUNED)),
    ("RT355_TUNE, four fields", one(), {"RT355_TUNE": "64,20,6,8"}, bvh2(every=TUNED)),
    ("RT355_TUNE, refill 65 is ignored", one(), {"RT355_TUNE": "64,65,6,8"}, bvh2()),
    ("RT355_FIXED_CHUNKS", one(), {"RT355_FIXED_CHUNKS": "0,1"}, bvh2(tune={"fixedChunks": 0}, tune4={"fixedChunks": 0})),
    ("RT355_FIXED_CHUNKS shared", one(persist_blocks_per_cu=2), {"RT355_FIXED_CHUNKS": "0,1"},
     bvh2(tune={"leafK": 16, "fixedChunks": 0}, tune4={"fixedChunks": 0})),
    ("RT355_TUNE_CONNECT", one(), {"RT355_TUNE_CONNECT": "96,16,4,32"}, bvh2(tuneConnect=dict(chunk=96, refill=16, inner=4, leafK=32, fixedChunks=0))),
    ("RT355_TOP_LEVELS=3", one(), {"RT355_TOP_LEVELS": "3"}, bvh2(topAuto=False, tune={"topLevels": 3}, tuneConnect={"topLevels": 3})),
    ("RT355_TOP_LEVELS=2,5", one(), {"RT355_TOP_LEVELS": "2,5"}, bvh2(topAuto=False, tune={"topLevels": 2}, tuneConnect={"topLevels": 5})),
    ("RT355_TOP_LEVELS=0", one(), {"RT355_TOP_LEVELS": "0"}, bvh2(topAuto=False, tune={"topLevels": 0}, tuneConnect={"topLevels": 0})),
    ("RT355_TOP_LEVELS=7 is ignored", one(), {"RT355_TOP_LEVELS": "7"}, bvh2()),
    ("RT355_TOP_LEVELS under a TLAS", many(), {"RT355_TOP_LEVELS": "3"}, tlas(TLAS)),
    ("RT355_TOP_LEVELS on a BVH4", one(accel=W.ACCEL_BVH4), {"RT355_TOP_LEVELS": "3"}, want(BVH4)),
    ("RT355_TLAS_FLAT=0,1", many(), {"RT355_TLAS_FLAT": "0,1"}, want(TLAS, tuneConnect={"flat": 1})),
    ("RT355_TLAS_FLAT=1,1 on one BLAS", one(), {"RT355_TLAS_FLAT": "1,1"}, bvh2()),
    ("RT355_THIN=100", one(), {"RT355_THIN": "100"}, bvh2(every={"thin": 64})),
    ("RT355_THIN=0", one(), {"RT355_THIN": "0"}, bvh2(every={"thin": 0})),
    ("RT355_XCD_RAYS=-3", one(), {"RT355_XCD_RAYS": "-3"}, bvh2(every={"xcdRays": 0})),
    ("RT355_XCD_RAYS=4096", one(), {"RT355_XCD_RAYS": "4096"}, bvh2(every={"xcdRays": 4096})),
    ("RT355_COHERENT=0", one(), {"RT355_COHERENT": "0"}, bvh2(coherent=0)),
    ("RT355_COHERENT=2", many(), {"RT355_COHERENT": "2"}, tlas(TLAS, coherent=2)),
    ("RT355_CONNECT_BLOCKS=3", one(), {"RT355_CONNECT_BLOCKS": "3"}, bvh2(connectBlocks=3)),
    ("RT355_CONNECT_BLOCKS=0", one(), {"RT355_CONNECT_BLOCKS": "0"}, bvh2()),
    ("xcdFirst is passed through", one(xcdFirst=2), {}, bvh2(every={"xcdFirst": 2})),
]


@pytest.mark.parametrize("what,facts,env,plan", CASES, ids=[c[0] for c in CASES])
def test_the_plan(monkeypatch, what, facts, env, plan):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = traversal_plan(facts)
    assert got == plan, (what, {k: (got[k], plan[k]) for k in plan if got[k] != plan[k]})


def test_the_knobs_are_read_at_every_call(monkeypatch):
    """Tests set them between a context's uploads: nothing is cached."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert traversal_plan(many(23))["trav"] == TLAS_SPILL
    monkeypatch.setenv("RT355_NO_SPILL", "1")
    assert traversal_plan(many(23))["trav"] == TLAS
    monkeypatch.delenv("RT355_NO_SPILL")
    assert traversal_plan(many(23))["trav"] == TLAS_SPILL


def test_the_kinds_are_the_public_numbers():
    assert (NESTED, BVH2, TLAS, TLAS_SPILL, BVH4, BVH4_TLAS, BVH4_TLAS_SPILL) == (
        W.TRAV_NESTED, W.TRAV_BVH2, W.TRAV_TLAS, W.TRAV_TLAS_SPILL, W.TRAV_BVH4, W.TRAV_BVH4_TLAS, W.TRAV_BVH4_TLAS_SPILL)
