#!/usr/bin/env python3
"""Where the lanes' kernels ran, per hardware queue, in the timed region of a bench.py kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python bench.py --steps 64 --no-single --no-cpu-baseline
    python tools/queue_tail.py DIR/run_results.db --steps 64 [--kernels]

A frame starts with its k_generate launch or, on the fused primary path (rt_primary_fused), with its k_trace_primary launch.  The timed
region starts at the first launch of its first frame (the last `--steps` such launches) and ends at the k_sum_lanes that follows it.
Per queue: its frames, busy time (union of its kernels' intervals) and when its last kernel ended.  `tail_ms` is the stretch at the end
of the region during which only one queue still had frames to run (queues that ran no frame - a runtime fill on the null stream - do
not count).  --kernels: per kernel the launches inside the region, with k_shade's launches split into a frame's first (bounce 0) and
its later ones.
"""
import argparse
import sqlite3

FRAME_START = ("k_generate", "k_trace_primary")


def starts_frame(name):
    return any(k in name for k in FRAME_START)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    c = sqlite3.connect(a.db)
    rows = c.execute("select name, queue_id, start, end from kernels order by start").fetchall()
    gen = [r for r in rows if starts_frame(r[0])]
    t0 = gen[-a.steps][2]
    sums = [r for r in rows if "k_sum_lanes" in r[0] and r[2] > t0]
    t1 = sums[0][2] if sums else max(r[3] for r in rows)
    reg = [r for r in rows if r[2] >= t0 and r[3] <= t1 and not "k_sum_lanes" in r[0]]
    region_ms = (max(r[3] for r in reg) - t0) / 1e6
    per = {}
    for name, q, s, e in reg:
        d = per.setdefault(q, dict(frames=0, iv=[], last=0))
        d["frames"] += starts_frame(name)
        d["iv"].append((s, e)); d["last"] = max(d["last"], e)
    print(f"timed region {region_ms:.3f} ms, {len(reg)} kernels on {len(per)} queue(s)")
    for q, d in sorted(per.items(), key=lambda kv: kv[1]["last"]):
        busy, cur = 0, None
        for s, e in sorted(d["iv"]):
            if cur is None or s > cur[1]:
                if cur: busy += cur[1] - cur[0]
                cur = [s, e]
            else:
                cur[1] = max(cur[1], e)
        busy += cur[1] - cur[0]
        print(f"  queue {q}: {d['frames']:3d} frames, busy {busy / 1e6:8.3f} ms, last kernel ends at {(d['last'] - t0) / 1e6:8.3f} ms")
    lasts = sorted(d["last"] for d in per.values() if d["frames"])
    tail = (lasts[-1] - lasts[-2]) / 1e6 if len(lasts) > 1 else 0.0
    print(f"tail_ms {tail:.3f} ({100 * tail / region_ms:.1f} % of the region): only one queue runs")
    if a.kernels:
        tab, shades = {}, {}
        for name, q, s, e in reg:       # (in start order; a queue runs its frames one after the other)
            key = name
            if starts_frame(name):
                shades[q] = 0
            if "k_shade" in name:
                key = name + ("  [bounce 0]" if shades.get(q, 1) == 0 else "  [bounces 1..]")
                shades[q] = shades.get(q, 1) + 1
            t = tab.setdefault(key, [0, 0])
            t[0] += 1; t[1] += e - s
        for key, (n, ns) in sorted(tab.items(), key=lambda kv: -kv[1][1]):
            print(f"  {key:86s} {n:4d} launches, mean {ns / n / 1e3:8.1f} us, total {ns / 1e6:8.2f} ms")


if __name__ == "__main__":
    main()
