"""Generates tests/golden/io_replay.npz: every answer the REFERENCE's own asset readers (oracle/_ref/libref_io.so, see tests/ref_io.py)
give to the synthetic inputs of tests/test_ref_io_cpu.py, so that those tests run where the reference is not built.  It runs the tests
with the library present and records each call; the tests on the reference's own asset files are left out (they stay live only).

    python tests/golden/make_io_replay.py      # needs oracle/_ref/libref_io.so (built where the reference exists) and Pillow
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "io_replay.npz")

if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_io.so")):
    raise SystemExit("oracle/_ref/libref_io.so is not built: nothing to record")
tmp = OUT + ".new.npz"
env = dict(os.environ, REF_IO_RECORD=tmp)
rc = subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_ref_io_cpu.py"),
                      "-k", "not test_reference_ and not test_golden_"], cwd=ROOT, env=env)
if rc != 0 or not os.path.exists(tmp):
    raise SystemExit(f"recording run failed ({rc})")
os.replace(tmp, OUT)
print("wrote", OUT, os.path.getsize(OUT), "bytes")
