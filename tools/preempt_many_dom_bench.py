#!/usr/bin/env python3
"""A crowded cluster's pending pods that read domain tables through
DefaultPreemption's dry run: a host loop of ksim_preempt_full single calls and
ksim_preempt_many (which answers such rows by the same single launches inside
the call) against ksim_preempt_many_dom.

Scene: tools/preempt_many_bench.py's (5,000 nodes, each filled to 97 % of its
CPU by 20 bound pods over five priorities, every fifth one a pod of app=web),
with 512 pending preemptors of 2 CPUs that fit nowhere and all read domain
tables: a third with hostname anti-affinity against app=web, a third app=web
pods with a DoNotSchedule zone constraint, a third with both.

Forms timed, in one process, alternating, ``--repeats`` times after one
warm-up round, each on its own handle; a form's time is the host wall time to
answer all 512 pods, ending synchronized:
  loop_parent   Engine.preempt(..., full=True) per pod on the library flavor
                ``--parent`` (tools/build_ref_flavor.sh <rev> <tag>); left out
                when that library is not there
  loop          the same loop on this tree's library
  many_old      Engine.preempt_many, one call of 512 rows
  dom_N         Engine.preempt_many(domains=True) in calls of N rows, N = 1, 8, 64, 512
Every batched form writes into one preallocated victims array per row, as long
as the fullest node's pod list (no list is cut: the answers of every form must
be identical to the loop's, asserted).  Writes the medians,
min to max and rows per second per form, and the comparison of dom_64 with the
baseline loop and with many_old, as JSON (``--out``, default
profiles/preempt_many_dom/ab.json) and prints the same line.

    python tools/preempt_many_dom_bench.py [--nodes 5000] [--pods 512] [--repeats 5] [--parent parent] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "kube-scheduler-simulator_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


import preempt_many_bench as base  # noqa: E402
from ksim import abi, engine, gen, profile  # noqa: E402
from ksim.encode import encode_cluster, encode_pods  # noqa: E402
from ksim.model import Container, ContainerPort, LabelSelector, Pod, PodAffinityTerm, TopologySpreadConstraint  # noqa: E402
from ksim.preemption import bound_table  # noqa: E402

HOST = "kubernetes.io/hostname"
GROUPS = (1, 8, 64, 512)


def build(n_nodes: int, n_pods: int):
    nodes, _ = gen.config1_objects(n_nodes, 0)
    r = gen.Rng(gen.SEEDS[1] ^ 0x9E3779)
    bound, start = [], {}
    for v, node in enumerate(nodes):                     # preempt_many_bench's bound pods, draw for draw
        milli = int(node.allocatable["cpu"]) * 1000 * 97 // 100 // base.PER_NODE
        for k in range(base.PER_NODE):
            p = Pod(f"b{v}-{k}", node_name=node.name, priority=base.PRIOS[r.below(len(base.PRIOS))],
                    labels={"app": "web"} if k % 5 == 4 else {},
                    containers=[Container({"cpu": f"{milli}m"}, [ContainerPort(8080)] if k == 0 else [])])
            bound.append(p)
            start[p.name] = r.below(1000)
    web = LabelSelector({"app": "web"})
    pending = []
    for j in range(n_pods):
        p = Pod(f"p{j}", priority=base.PENDING_PRIOS[r.below(len(base.PENDING_PRIOS))],
                containers=[Container({"cpu": "2000m"})])
        if j % 3 != 1:
            p.pod_anti_affinity_required = [PodAffinityTerm(HOST, web)]
        if j % 3 != 0:
            p.labels = {"app": "web"}
            p.topology_spread = [TopologySpreadConstraint(1, base.ZONE, "DoNotSchedule", web)]
        pending.append(p)
    cluster, _ = encode_cluster(nodes, bound)
    enc = encode_pods(cluster, pending)
    table = bound_table(cluster, bound, start, cluster.topo, full_adds=True)
    dom = {abi.USE_IPA_ANTI, abi.USE_IPA_EXISTING_ANTI, abi.USE_PTS_HARD}
    for j, q in enumerate(enc.pods):
        kinds = {int(k) for k in enc.uses["kind"][int(q["use_first"]):int(q["use_first"]) + int(q["use_count"])]}
        assert kinds & dom and (abi.USE_IPA_ANTI in kinds) == (j % 3 != 1) and (abi.USE_PTS_HARD in kinds) == (j % 3 != 0), \
            "the pending pods' uses"
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof, [p.priority for p in pending]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default="parent", help="library flavor of the parent commit (tools/build_ref_flavor.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_many_dom", "ab.json"))
    args = ap.parse_args()
    cluster, table, enc, prof, prios = build(args.nodes, args.pods)
    idx = list(range(args.pods))
    parent = None
    if os.path.exists(os.path.join(os.path.dirname(engine.LIB_PATH), f"libksim_engine_{args.parent}.so")):
        parent = args.parent

    def loop(eng):
        return [eng.preempt(enc, i, prios[i], full=True) for i in idx]

    # one victims array per row, as long as the fullest node's pod list, allocated once: by default
    # Engine.preempt_many sizes every row's array for the whole table at every call, and the time of
    # a call is then the allocator's (page faults over rows x 400 KB), not the library's
    outs = [abi.PreemptOut(base.PER_NODE) for _ in idx]

    def many(eng, n, domains):
        out = []
        for a in range(0, args.pods, n):
            out += eng.preempt_many(enc, idx[a:a + n], prios[a:a + n], outs=outs[a:a + n], domains=domains)
        return out

    forms = {}
    if parent is not None:
        forms["loop_parent"] = (base.handle(parent, cluster, table, prof), loop)
    forms["loop"] = (base.handle(None, cluster, table, prof), loop)
    forms["many_old"] = (base.handle(None, cluster, table, prof), lambda eng: many(eng, args.pods, False))
    for n in GROUPS:
        forms[f"dom_{n}"] = (base.handle(None, cluster, table, prof), lambda eng, n=n: many(eng, n, True))
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
    diag = forms["dom_512"][0].diag()
    old = forms["many_old"][0].diag()
    for eng, _ in forms.values():
        eng.close()
    nominated = sum(1 for a in answers["loop"] if a[0] >= 0)
    res = dict(bench="preempt_many_dom", nodes=args.nodes, bound_pods=table.n, pods=args.pods, repeats=args.repeats,
               nominated=nominated, victims=sum(len(a[1]) for a in answers["loop"]),
               potential_mean=round(statistics.mean(a[2] for a in answers["loop"]), 1),
               rows_domain_batched=diag["preempt_many_dom"], rows_single=diag["preempt_many_single"],
               old_call_rows_single=old["preempt_many_single"], forms={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res["forms"][name] = dict(median_ms=round(med * 1e3, 3), min_ms=round(min(ts) * 1e3, 3),
                                  max_ms=round(max(ts) * 1e3, 3), rows_per_s=round(args.pods / med, 1))
    basef = "loop_parent" if parent is not None else "loop"
    res["baseline"] = basef
    res["ratio_to_baseline"] = {name: round(f["median_ms"] / res["forms"][basef]["median_ms"], 4)
                                for name, f in res["forms"].items()}
    # dom_64 below the other form by more than the larger min-to-max spread of the two
    f64 = res["forms"]["dom_64"]
    res["acceptance"] = {}
    for other in (basef, "many_old"):
        o = res["forms"][other]
        spread = max(f64["max_ms"] - f64["min_ms"], o["max_ms"] - o["min_ms"])
        res["acceptance"][other] = dict(gain_ms=round(o["median_ms"] - f64["median_ms"], 3), spread_ms=round(spread, 3),
                                        below=bool(o["median_ms"] - f64["median_ms"] > spread))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
