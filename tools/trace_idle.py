"""Dispatches per step and GPU idle time per step from a rocprofv3 kernel trace
of bench.py (config 2: every step starts with ksim_reset_cluster's
k_reset_copy, so the steps are the spans between those dispatches).
Usage: python tools/trace_idle.py <rocprofv3 output directory>/<name>_results.db

Per step: the time from its first dispatch's start to its last dispatch's end,
the sum of the dispatches' own durations, and the difference (idle: the device
had no kernel of this process running); and the dispatch counts of the blit
kernels (copyBuffer, fillBufferAligned), of the flush instantiations of
k_batch_top_commit (first template argument true) and of everything else."""
import json
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
rows = db.execute("select name, start, end from kernels order by start").fetchall()
cuts = [i for i, r in enumerate(rows) if "k_reset_copy" in r[0]]
steps = []
for a, b in zip(cuts, cuts[1:] + [len(rows)]):
    ks = rows[a:b]
    # the last span also holds whatever follows the last step: stop at its last batch kernel
    last = max(i for i, r in enumerate(ks) if "k_batch" in r[0] or "k_lazy_move" in r[0] or "rocclr" in r[0])
    ks = ks[:last + 1]
    span = ks[-1][2] - ks[0][1]
    busy = sum(e - s for _, s, e in ks)
    n = {"copyBuffer": 0, "fillBufferAligned": 0, "flush": 0, "k_lazy_move": 0, "other": 0}
    for name, _, _ in ks:
        if "copyBuffer" in name:
            n["copyBuffer"] += 1
        elif "fillBuffer" in name:
            n["fillBufferAligned"] += 1
        elif "k_batch_top_commit<true" in name or "k_adapt_mask_commit<true" in name:
            n["flush"] += 1
        elif "k_lazy_move" in name:
            n["k_lazy_move"] += 1
        else:
            n["other"] += 1
    steps.append({"span_us": span / 1e3, "busy_us": busy / 1e3, "idle_us": (span - busy) / 1e3, "dispatches": n})
out = {"steps": steps}
if steps:
    k = len(steps)
    out["mean"] = {f: sum(s[f] for s in steps) / k for f in ("span_us", "busy_us", "idle_us")}
    out["mean"]["dispatches"] = {f: sum(s["dispatches"][f] for s in steps) / k for f in steps[0]["dispatches"]}
print(json.dumps(out, indent=1))
