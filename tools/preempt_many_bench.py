#!/usr/bin/env python3
"""A crowded cluster's pending pods through DefaultPreemption's dry run: a
host loop of ksim_preempt_full single calls against ksim_preempt_many.

Scene: 5,000 nodes (ksim.gen config 1's: 4 to 32 cores, three zones, a tenth
tainted NoSchedule), each filled to 97 % of its CPU by 20 bound pods over five
priorities (0, 10, 100, 500, 900), the first of them holding host port 8080 and
every fifth one a pod of app=web; 512 pending preemptors of 2 CPUs and
priorities 50 to 1,000 that fit nowhere: half Fit-only, a quarter with host
port 8080, a quarter app=web pods with a ScheduleAnyway zone constraint (a use
no Filter reads).

Forms timed, in one process, alternating, ``--repeats`` times after one
warm-up round, each on its own handle; a form's time is the host wall time to
answer all 512 pods, ending synchronized:
  loop_parent   Engine.preempt(..., full=True) per pod on the library flavor
                ``--parent`` (tools/build_ref_flavor.sh <rev> <tag>); left out
                when that library is not there
  loop          the same loop on this tree's library
  many_N        Engine.preempt_many in calls of N rows, N = 1, 8, 64, 512
The answers of ``loop`` and of every ``many_N`` must be identical (asserted).
Writes the medians, min to max and rows per second per form as JSON
(``--out``, default profiles/preempt_many/ab.json) and prints the same line.

    python tools/preempt_many_bench.py [--nodes 5000] [--pods 512] [--repeats 5] [--parent parent] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "kube-scheduler-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


from ksim import abi, engine, gen, profile  # noqa: E402
from ksim.encode import encode_cluster, encode_pods  # noqa: E402
from ksim.model import Container, ContainerPort, LabelSelector, Pod, TopologySpreadConstraint  # noqa: E402
from ksim.preemption import bound_table  # noqa: E402

ZONE = "topology.kubernetes.io/zone"
PER_NODE = 20
PRIOS = (0, 10, 100, 500, 900)
PENDING_PRIOS = (50, 200, 600, 1000)
GROUPS = (1, 8, 64, 512)


def build(n_nodes: int, n_pods: int):
    nodes, _ = gen.config1_objects(n_nodes, 0)
    r = gen.Rng(gen.SEEDS[1] ^ 0x9E3779)
    bound, start = [], {}
    for v, node in enumerate(nodes):
        milli = int(node.allocatable["cpu"]) * 1000 * 97 // 100 // PER_NODE
        for k in range(PER_NODE):
            p = Pod(f"b{v}-{k}", node_name=node.name, priority=PRIOS[r.below(len(PRIOS))],
                    labels={"app": "web"} if k % 5 == 4 else {},
                    containers=[Container({"cpu": f"{milli}m"}, [ContainerPort(8080)] if k == 0 else [])])
            bound.append(p)
            start[p.name] = r.below(1000)
    web = LabelSelector({"app": "web"})
    pending = []
    for j in range(n_pods):
        p = Pod(f"p{j}", priority=PENDING_PRIOS[r.below(len(PENDING_PRIOS))], containers=[Container({"cpu": "2000m"})])
        if j % 4 == 1:
            p.containers[0].ports = [ContainerPort(8080)]
        elif j % 4 == 3:
            p.labels = {"app": "web"}
            p.topology_spread = [TopologySpreadConstraint(1, ZONE, "ScheduleAnyway", web)]
        pending.append(p)
    cluster, _ = encode_cluster(nodes, bound)
    enc = encode_pods(cluster, pending)
    table = bound_table(cluster, bound, start, cluster.topo)
    kinds = [sorted({int(k) for k in enc.uses["kind"][int(q["use_first"]):int(q["use_first"]) + int(q["use_count"])]})
             for q in enc.pods]
    assert all(k == ([] if j % 2 == 0 else [abi.USE_NODE_PORT] if j % 4 == 1 else [abi.USE_PTS_SOFT])
               for j, k in enumerate(kinds)), "the pending pods' uses"
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof, [p.priority for p in pending]


def handle(variant, cluster, table, prof):
    eng = engine.Engine(0, variant=variant)
    eng.set_profile(prof)
    eng.set_cluster(cluster)
    eng.set_bound_pods(table)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default="parent", help="library flavor of the parent commit (tools/build_ref_flavor.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_many", "ab.json"))
    args = ap.parse_args()
    cluster, table, enc, prof, prios = build(args.nodes, args.pods)
    idx = list(range(args.pods))
    parent = None
    if os.path.exists(os.path.join(os.path.dirname(engine.LIB_PATH), f"libksim_engine_{args.parent}.so")):
        parent = args.parent

    def loop(eng):
        return [eng.preempt(enc, i, prios[i], full=True) for i in idx]

    def many(eng, n):
        out = []
        for a in range(0, args.pods, n):
            out += eng.preempt_many(enc, idx[a:a + n], prios[a:a + n])
        return out

    forms = {}
    if parent is not None:
        forms["loop_parent"] = (handle(parent, cluster, table, prof), loop)
    forms["loop"] = (handle(None, cluster, table, prof), loop)
    for n in GROUPS:
        forms[f"many_{n}"] = (handle(None, cluster, table, prof), lambda eng, n=n: many(eng, n))
    times = {k: [] for k in forms}
    answers = {}
    for rep in range(args.repeats + 1):                  # round 0: the warm-up
        for name, (eng, run) in forms.items():
            t0 = time.perf_counter()
            got = run(eng)
            dt = time.perf_counter() - t0
            if rep == 0:
                answers[name] = got
            else:
                assert got == answers[name], f"{name}: the answers moved between rounds"
                times[name].append(dt)
    for name in forms:
        assert answers[name] == answers["loop"], f"{name} differs from the loop of single calls"
    diag = forms["many_512"][0].diag()
    for eng, _ in forms.values():
        eng.close()
    nominated = sum(1 for a in answers["loop"] if a[0] >= 0)
    res = dict(bench="preempt_many", nodes=args.nodes, bound_pods=table.n, pods=args.pods, repeats=args.repeats,
               nominated=nominated, victims=sum(len(a[1]) for a in answers["loop"]),
               potential_mean=round(statistics.mean(a[2] for a in answers["loop"]), 1),
               rows_batched=diag["preempt_many_rows"], rows_single=diag["preempt_many_single"], forms={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res["forms"][name] = dict(median_ms=round(med * 1e3, 3), min_ms=round(min(ts) * 1e3, 3),
                                  max_ms=round(max(ts) * 1e3, 3), rows_per_s=round(args.pods / med, 1))
    base = "loop_parent" if parent is not None else "loop"
    res["baseline"] = base
    res["ratio_to_baseline"] = {name: round(f["median_ms"] / res["forms"][base]["median_ms"], 4)
                                for name, f in res["forms"].items()}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
