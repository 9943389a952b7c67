#!/usr/bin/env python3
"""A chain of preemptions on a crowded cluster: what making a dry run's
evictions real costs by ksim_preempt_commit and by the rebuild form.

Scene: ``--nodes`` nodes (gen.config1_objects), each filled to 97 % of its CPU
by ``--per-node`` bound pods over five priorities, every fifth one app=web; the
table carries every row's class adds and one budget over app=web.  ``--chain``
pending pods of 2 CPUs fit nowhere; every third has hostname anti-affinity
against app=web.

Each preemption is two steps: a dry run by ksim_preempt_full (Engine.preempt,
full=True, with the budgets), then the eviction of its victims, which is timed:
  commit    Engine.preempt_commit over the victims' rows
  rebuild   Engine.forget per victim, then set_bound_pods with the adds and the
            budgets over the survivors; the survivors' table is cut out of the
            full table's arrays with numpy beforehand (``construct``, reported
            on its own: a caller might keep it incrementally)
Both forms run in one process on handles of their own, alternating chain by
chain, ``--repeats`` times after a warm-up chain (the chains restart from a
fresh reset_cluster / set_bound_pods, not timed).  Both must give the same
answers at every step (the rebuild form's victims mapped through the
survivors) and the same final state (digests of the node state, the class
counts and the last answers).  One JSON line, also written to ``--out``.

    python tools/preempt_commit_bench.py [--nodes 5000] [--per-node 20] [--chain 64] [--repeats 5] [--out PATH]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "kube-scheduler-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ksim import abi, gen, profile  # noqa: E402
from ksim.encode import encode_cluster, encode_pods  # noqa: E402
from ksim.engine import Engine  # noqa: E402
from ksim.model import Container, LabelSelector, Pod, PodAffinityTerm, PodDisruptionBudget  # noqa: E402
from ksim.preemption import bound_table, commit_args  # noqa: E402

HOST = "kubernetes.io/hostname"
PRIOS = (0, 10, 100, 500, 900)


def build(n_nodes: int, per_node: int, chain: int):
    nodes, _ = gen.config1_objects(n_nodes, 0)
    r = gen.Rng(gen.SEEDS[1] ^ 0xC0117)
    bound, start, shape = [], {}, []
    for v, node in enumerate(nodes):
        milli = int(node.allocatable["cpu"]) * 1000 * 97 // 100 // per_node
        for k in range(per_node):
            web = k % 5 == 4
            bound.append(Pod(f"b{v}-{k}", node_name=node.name, priority=PRIOS[r.below(len(PRIOS))],
                             labels={"app": "web"} if web else {}, containers=[Container({"cpu": f"{milli}m"})]))
            start[bound[-1].name] = r.below(1000)
            shape.append((milli, web))
    web = LabelSelector({"app": "web"})
    pending = [Pod(f"p{j}", priority=1000 - j, containers=[Container({"cpu": "2000m"})],
                   pod_anti_affinity_required=[PodAffinityTerm(HOST, web)] if j % 3 == 0 else [])
               for j in range(chain)]
    cluster, _ = encode_cluster(nodes, bound)
    # a bound pod's record depends on its requests and labels alone: one record per shape
    kinds = sorted(set(shape))
    reps = [Pod(f"shape{i}", labels={"app": "web"} if w else {}, containers=[Container({"cpu": f"{m}m"})])
            for i, (m, w) in enumerate(kinds)]
    enc = encode_pods(cluster, pending + reps)
    pdbs = [PodDisruptionBudget("web", selector=web, disruptions_allowed=len(bound))]
    table = bound_table(cluster, bound, start, cluster.topo, full_adds=True, pdbs=pdbs)
    at = {k: chain + i for i, k in enumerate(kinds)}
    row_pod = np.array([at[s] for s in shape], np.int32)
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof, [p.priority for p in pending], row_pod


def cut(t, alive):
    """The table over the rows ``alive`` (ascending) of ``t``, its lists gathered with numpy."""
    def csr(off, ent):
        n = off[alive + 1] - off[alive]
        new = np.concatenate(([0], np.cumsum(n))).astype(np.int32)
        src = np.repeat(off[alive] - new[:-1], n) + np.arange(int(new[-1]))
        return new, ent[src]
    aoff, adds = csr(t.adds_off, t.adds)
    poff, pids = csr(t.pdb_off, t.pdb_ids)
    return abi.BoundPods(t.node[alive], t.priority[alive], t.start_time[alive], t.req[alive], aoff, adds,
                         t.pdb_allowed, poff, pids)


def digest(eng, last) -> str:
    h = hashlib.sha256()
    st = eng.node_state()
    for k in sorted(st):
        h.update(st[k].tobytes())
    h.update(eng.class_count().tobytes())
    h.update(repr(last).encode())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--per-node", type=int, default=20)
    ap.add_argument("--chain", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_commit", "ab.json"))
    args = ap.parse_args()
    t0 = time.perf_counter()
    cluster, table, enc, prof, prios, row_pod = build(args.nodes, args.per_node, args.chain)
    build_s = time.perf_counter() - t0
    engines = {}
    for form in ("commit", "rebuild"):
        engines[form] = Engine(0)
        engines[form].set_profile(prof)
        engines[form].set_cluster(cluster)

    def fresh(eng):
        eng.reset_cluster()
        eng.set_bound_pods(table)

    def dry(eng, k):
        return eng.preempt(enc, k, prios[k], full=True, with_pdb=True)

    def chain_commit(eng):
        evict, answers = [], []
        for k in range(args.chain):
            got = dry(eng, k)
            rows, idx = commit_args(got, row_pod)
            t = time.perf_counter()
            eng.preempt_commit(enc, rows, idx)
            evict.append(time.perf_counter() - t)
            answers.append(got)
        return answers, evict, [0.0] * args.chain

    def chain_rebuild(eng):
        evict, construct, answers = [], [], []
        alive = np.arange(table.n)
        for k in range(args.chain):
            got = dry(eng, k)
            got = (got[0], [int(alive[v]) for v in got[1]]) + tuple(got[2:])
            rows = np.array(got[1], np.int64)
            t = time.perf_counter()
            keep = np.ones(table.n, bool)
            keep[rows] = False
            alive = alive[keep[alive]]
            sub = cut(table, alive)
            tc = time.perf_counter()
            for r in rows:
                eng.forget(enc, int(row_pod[r]), int(table.node[r]))
            eng.set_bound_pods(sub)                         # (ends synchronized, as the commit does)
            te = time.perf_counter()
            construct.append(tc - t)
            evict.append(te - tc)
            answers.append(got)
        return answers, evict, construct

    runs = {"commit": chain_commit, "rebuild": chain_rebuild}
    times = {f: [] for f in runs}
    cons, digests, first = [], {}, None
    for rep in range(args.repeats + 1):                      # round 0: the warm-up
        for form, run in runs.items():
            fresh(engines[form])
            answers, evict, construct = run(engines[form])
            if first is None:
                first = answers
            assert answers == first, f"{form}: the answers differ (round {rep})"
            digests[form] = digest(engines[form], answers[-1])
            if rep:
                times[form].append(statistics.mean(evict))
                if form == "rebuild":
                    cons.append(statistics.mean(construct))
    assert digests["commit"] == digests["rebuild"], digests
    for e in engines.values():
        e.close()
    res = dict(bench="preempt_commit", nodes=args.nodes, bound_pods=table.n, chain=args.chain, repeats=args.repeats,
               victims=sum(len(a[1]) for a in first), nominated=sum(a[0] >= 0 for a in first),
               scene_build_s=round(build_s, 1), digest=digests["commit"], per_preemption_ms={})
    for form, ts in times.items():
        res["per_preemption_ms"][form] = dict(median=round(statistics.median(ts) * 1e3, 4), min=round(min(ts) * 1e3, 4),
                                              max=round(max(ts) * 1e3, 4))
    res["per_preemption_ms"]["rebuild_construct"] = dict(median=round(statistics.median(cons) * 1e3, 4),
                                                         min=round(min(cons) * 1e3, 4), max=round(max(cons) * 1e3, 4))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
