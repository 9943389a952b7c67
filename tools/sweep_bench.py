#!/usr/bin/env python3
"""Policy sweep (BASELINE config 5), packed against threaded, in one process.

On gen.config2(5000, 10000) with gen.config5_weights(V) it times

  threaded   bench.py's config-5 loop: 8 engines, one host thread each, every
             vector as set_profile / load_pods / reset_cluster / schedule_loaded;
  packed     sweep.run_sweep (ksim_sweep_loaded: the vectors packed into shared
             launches on one handle and one stream) at max_lanes 4, 8, 16, 32, 64

and prints one JSON line: per form the host wall time of each timed step
(every step ends with the placements on the host), their median, the time per
vector and the placement digest.  Every form is warmed up first (graph
captures, buffer allocation), then the forms' steps alternate so that drift on
a shared host falls on all of them alike.

    python tools/sweep_bench.py [--vectors 1024] [--steps 3] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "kube-scheduler-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from ksim import engine, gen, profile, sweep  # noqa: E402

LANES = (4, 8, 16, 32, 64)
STREAMS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--lanes", type=str, default=",".join(str(x) for x in LANES))
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    lanes = [int(x) for x in args.lanes.split(",") if x]

    cluster, pods = gen.config2(args.nodes, args.pods)
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    prof = profile.compile_profile(sp)
    weights = gen.config5_weights(args.vectors)
    names = [p.name for p in sp.score_plugins()]
    profs = [profile.compile_profile(sp.with_weights({n: int(x) for n, x in zip(names, w)})) for w in weights]

    def new_engine():
        e = engine.Engine(0)
        e.set_profile(prof)
        e.set_cluster(cluster)
        e.load_pods(pods)
        return e

    # ---- threaded: bench.py's config-5 step ----------------------------------
    engs = [new_engine() for _ in range(STREAMS)]
    pool = ThreadPoolExecutor(len(engs))

    def run_part(j):
        e, rows = engs[j], []
        for pr in profs[j::len(engs)]:
            e.set_profile(pr)
            e.load_pods(pods)
            e.reset_cluster()
            chosen, _ = e.schedule_loaded(0, pods.n_pods)
            rows.append(chosen)
        return rows

    def threaded():
        res = list(pool.map(run_part, range(len(engs))))
        return sweep.order_engine_results(res, len(profs))

    # ---- packed: one engine, one stream ---------------------------------------
    one = new_engine()

    def packed(n):
        def step():
            rows, _, was_packed = sweep.run_sweep(one, pods, profs, max_lanes=n)
            if not was_packed:
                raise SystemExit("sweep_bench: the packed path was refused (serial fallback ran)")
            return rows
        return step

    forms = [("threaded_8_engines", threaded)] + [(f"packed_lanes_{n}", packed(n)) for n in lanes]
    times = {name: [] for name, _ in forms}
    digest = {}
    for name, fn in forms:
        for _ in range(max(args.warmup, 1)):
            digest[name] = sweep.placement_digest(fn())
    for _ in range(args.steps):
        for name, fn in forms:                           # alternate the forms
            t0 = time.perf_counter()
            rows = fn()                                  # returns with the placements on the host
            times[name].append((time.perf_counter() - t0) * 1e3)
            d = sweep.placement_digest(rows)
            if d != digest[name]:
                raise SystemExit(f"sweep_bench: {name} digest changed between steps: {digest[name]} -> {d}")
    out = {"tool": "sweep_bench", "nodes": cluster.n_nodes, "pods": pods.n_pods, "vectors": args.vectors,
           "steps": args.steps, "warmup": max(args.warmup, 1), "forms": {}}
    for name, _ in forms:
        med = statistics.median(times[name])
        out["forms"][name] = {"step_ms": [round(x, 2) for x in times[name]], "median_ms": round(med, 2),
                              "ms_per_vector": round(med / args.vectors, 4), "digest": digest[name]}
    best = min((n for n, _ in forms if n.startswith("packed")), key=lambda n: out["forms"][n]["median_ms"])
    out["fastest_packed"] = best
    out["packed_over_threaded"] = round(out["forms"]["threaded_8_engines"]["median_ms"] /
                                        out["forms"][best]["median_ms"], 3)
    out["digests_equal"] = len(set(digest.values())) == 1
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
