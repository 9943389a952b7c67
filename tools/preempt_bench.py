#!/usr/bin/env python3
"""Host wall time of one DefaultPreemption dry run (ksim_preempt) for a
use-free preemptor: 5,000 nodes of 10 CPUs, four bound pods each of mixed
priorities and start times filling 9.6 CPUs, a 2-CPU preemptor of priority
1,000, so every node is a potential node and a candidate.  Each timed call is
Engine.preempt: the pod's upload, the filter pass, the two preemption kernels
and the result copies, ending synchronized.

--ports: the same cluster where the first bound pod of every node holds host
port 8080, and a preemptor with that host port: every node is a potential node
(Fit fails first) and a candidate once the holder is a victim, and each runs
the ports form of the dry run.  The table carries the rows' port holdings.

--anti: the same cluster spread over 50 zones, one pod of app=x in each zone
(priority 10, on the zone's first node), and a preemptor with a required zone
anti-affinity term against app=x: every node is a potential node (Fit fails
first), each runs the domain form of the dry run, and the 50 holders' nodes are
the candidates.  The table carries every row's class contributions.

--spread: --anti's cluster (50 zones, an app=x pod of priority 10 on each
zone's first node) and a preemptor that is an x pod with one DoNotSchedule
constraint (maxSkew 1 on the zone over app=x): every node is a potential node
(Fit fails first), each runs the spread form of the dry run through
ksim_preempt_spread (one more small launch, k_preempt_spread_mins), and every
node is a candidate.

--volumes: the use-free cluster where every bound pod holds one EBS volume of
its own (limit 4 a node, so every node is full) and one bound pod in eight
shares a CSI volume with its neighbour on the node; the preemptor brings one
new EBS volume and mounts node 0's shared CSI volume.  Every node is a
potential node (Fit fails first) and a candidate, and each runs the volume
form of the dry run through ksim_preempt_volumes.  The table carries every
row's holdings.

--full: --volumes' cluster spread over 50 zones, and a preemptor (app=x) that
also carries a required hostname anti-affinity term against app=x and one
DoNotSchedule constraint (maxSkew 1 on the zone over app=x); no bound pod is an
x pod.  Every node is a potential node (Fit fails first) and a candidate, and
each runs the full form of the dry run through ksim_preempt_full.  The table
carries every row's class contributions and holdings.

--pdbs K: K PodDisruptionBudgets with disruptionsAllowed 1 over the table,
the bound pods of node v in budget v % K (ksim_set_bound_pod_pdbs), so all but
the most important lower-priority pod of a node violate: the call takes the
PDB form of the kernels.  With --ports, --anti, --spread, --volumes or --full too.

Prints one JSON line: the calls' median, min, max and the 10th / 90th
percentiles in microseconds, per repeat (a fresh handle each) and over all.
To compare two builds on one machine run it once per library
(KSIM_LIB_VARIANT=<tag> loads libksim_engine_<tag>.so, tools/build_ref_flavor.sh).

    python tools/preempt_bench.py [--nodes 5000] [--calls 200] [--warmup 20] [--repeats 3] [--ports | --anti | --spread | --volumes | --full] [--pdbs K]
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

import numpy as np  # noqa: E402

from ksim import abi, engine, profile  # noqa: E402
from ksim.encode import encode_cluster, encode_pods  # noqa: E402
from ksim.model import (Container, ContainerPort, LabelSelector, Node, PersistentVolume, PersistentVolumeClaim, Pod,  # noqa: E402
                        PodAffinityTerm, TopologySpreadConstraint)

ZONE, N_ZONES = "topology.kubernetes.io/zone", 50


def build(n_nodes: int):
    rng = np.random.default_rng(7)
    nodes = [Node(name=f"n{i:05d}", labels={"kubernetes.io/hostname": f"n{i:05d}"},
                  allocatable={"cpu": "10", "memory": "64Gi", "pods": "110"}) for i in range(n_nodes)]
    bound, node, prio, start = [], [], [], []
    for v in range(n_nodes):
        for k in range(4):
            bound.append(Pod(f"b{v}-{k}", node_name=nodes[v].name, containers=[Container({"cpu": "2400m"})]))
            node.append(v)
            prio.append(int(rng.choice([0, 10, 100, 500])))
            start.append(int(rng.integers(0, 1000)))
    cluster, _ = encode_cluster(nodes, bound)
    assert list(cluster.node_names) == [n.name for n in nodes]
    req = np.zeros((len(bound), abi.PREEMPT_REQ), np.int64)
    req[:, 0] = 2400
    table = abi.BoundPods(node, prio, start, req)
    enc = encode_pods(cluster, [Pod("preemptor", priority=1000, containers=[Container({"cpu": "2000m"})])])
    assert int(enc.pods[0]["use_count"]) == 0
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof


def build_ports(n_nodes: int):
    """build()'s load, host port 8080 on every node's first bound pod and on the preemptor."""
    from ksim.preemption import bound_table
    rng = np.random.default_rng(7)
    nodes = [Node(name=f"n{i:05d}", labels={"kubernetes.io/hostname": f"n{i:05d}"},
                  allocatable={"cpu": "10", "memory": "64Gi", "pods": "110"}) for i in range(n_nodes)]
    bound, start = [], {}
    for v in range(n_nodes):
        for k in range(4):
            ports = [ContainerPort(8080)] if k == 0 else []
            bound.append(Pod(f"b{v}-{k}", node_name=nodes[v].name, priority=int(rng.choice([0, 10, 100, 500])),
                             containers=[Container({"cpu": "2400m"}, ports)]))
            start[bound[-1].name] = int(rng.integers(0, 1000))
    cluster, _ = encode_cluster(nodes, bound)
    enc = encode_pods(cluster, [Pod("preemptor", priority=1000,
                                    containers=[Container({"cpu": "2000m"}, [ContainerPort(8080)])])])
    assert [int(k) for k in enc.uses["kind"][:int(enc.pods[0]["use_count"])]] == [abi.USE_NODE_PORT]
    table = bound_table(cluster, bound, start, cluster.topo)
    assert int(table.adds_off[-1]) == n_nodes
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof


def build_anti(n_nodes: int, spread: bool = False):
    """build()'s load on N_ZONES zones, an app=x pod per zone, the anti-affine
    preemptor (``spread``: the one with a DoNotSchedule zone constraint)."""
    from ksim.preemption import bound_table
    rng = np.random.default_rng(7)
    nodes = [Node(name=f"n{i:05d}", labels={"kubernetes.io/hostname": f"n{i:05d}", ZONE: f"z{i % N_ZONES:02d}"},
                  allocatable={"cpu": "10", "memory": "64Gi", "pods": "110"}) for i in range(n_nodes)]
    bound, start = [], {}
    for v in range(n_nodes):
        for k in range(4):
            holder = v < N_ZONES and k == 0
            bound.append(Pod(f"b{v}-{k}", node_name=nodes[v].name, labels={"app": "x"} if holder else {},
                             priority=10 if holder else int(rng.choice([0, 10, 100, 500])),
                             containers=[Container({"cpu": "2400m"})]))
            start[bound[-1].name] = int(rng.integers(0, 1000))
    cluster, _ = encode_cluster(nodes, bound)
    if spread:
        pod = Pod("preemptor", priority=1000, labels={"app": "x"}, containers=[Container({"cpu": "2000m"})],
                  topology_spread=[TopologySpreadConstraint(1, ZONE, "DoNotSchedule", LabelSelector({"app": "x"}))])
    else:
        pod = Pod("preemptor", priority=1000, containers=[Container({"cpu": "2000m"})],
                  pod_anti_affinity_required=[PodAffinityTerm(ZONE, LabelSelector({"app": "x"}))])
    enc = encode_pods(cluster, [pod])
    assert int(enc.pods[0]["use_count"]) == 1
    assert int(enc.uses["kind"][0]) == (abi.USE_PTS_HARD if spread else abi.USE_IPA_ANTI)
    table = bound_table(cluster, bound, start, cluster.topo, full_adds=True)
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof


def build_volumes(n_nodes: int, full: bool = False):
    """build()'s load with counted volumes on every bound pod and the preemptor
    (``full``: on N_ZONES zones, the preemptor with hostname anti-affinity and a
    DoNotSchedule zone constraint as well)."""
    from ksim.preemption import bound_table
    from ksim.volumes import VolumeIndex
    rng = np.random.default_rng(7)
    ebs, csi = "attachable-volumes-aws-ebs", "attachable-volumes-csi-x"
    nodes = [Node(name=f"n{i:05d}", labels={"kubernetes.io/hostname": f"n{i:05d}"},
                  allocatable={"cpu": "10", "memory": "64Gi", "pods": "110", ebs: "4", csi: "8"}) for i in range(n_nodes)]
    if full:
        for i, n in enumerate(nodes):
            n.labels[ZONE] = f"z{i % N_ZONES:02d}"
    pvs, pvcs = [], []

    def claim(name, **source):
        pv = PersistentVolume(name="pv-" + name, **source)
        pv.claim_ref = ("default", name)
        pvs.append(pv)
        pvcs.append(PersistentVolumeClaim(name=name, namespace="default", volume_name=pv.name))
        return name
    bound, start = [], {}
    for v in range(n_nodes):
        for k in range(4):
            g = 4 * v + k
            claims = [claim(f"e{g}", source="awsElasticBlockStore", source_id=f"vol-{g}")]
            if g % 8 == 0:                               # shared with the next pod of the node
                claim(f"s{g}", source="csi", source_id=f"h{g}", csi_driver="x")
            if g % 8 < 2:
                claims.append(f"s{g - g % 8}")
            bound.append(Pod(f"b{v}-{k}", node_name=nodes[v].name, priority=int(rng.choice([0, 10, 100, 500])),
                             containers=[Container({"cpu": "2400m"})], pvc_claims=claims))
            start[bound[-1].name] = int(rng.integers(0, 1000))
    pod = Pod("preemptor", priority=1000, containers=[Container({"cpu": "2000m"})],
              pvc_claims=[claim("mine", source="awsElasticBlockStore", source_id="vol-mine"), "s0"])
    if full:
        sel = LabelSelector({"app": "x"})
        pod.labels = {"app": "x"}
        pod.pod_anti_affinity_required = [PodAffinityTerm("kubernetes.io/hostname", sel)]
        pod.topology_spread = [TopologySpreadConstraint(1, ZONE, "DoNotSchedule", sel)]
    index = VolumeIndex.from_nodes(nodes, pvs, pvcs)
    cluster, _ = encode_cluster(nodes, bound)
    cluster.set_volume_limits(index.volume_limits(nodes, bound, [pod]))
    enc = encode_pods(cluster, [pod], volumes=index)
    kinds = [int(k) for k in enc.uses["kind"][:int(enc.pods[0]["use_count"])]]
    vol = [int(c) >= 0 for c, k in zip(enc.uses["cls"], kinds) if k == abi.USE_VOLUME]
    assert sorted(vol) == [False, True]
    assert {k for k in kinds if k != abi.USE_VOLUME} >= ({abi.USE_PTS_HARD, abi.USE_IPA_ANTI} if full else set())
    assert full or len(kinds) == 2
    table = bound_table(cluster, bound, start, cluster.topo, full_adds=full, vol_limits=cluster.vol_limits)
    assert int(table.vol_off[-1]) == len(bound) + 2 * ((len(bound) + 7) // 8)
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0))
    return cluster, table, enc, prof


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def summary(us):
    return dict(median_us=round(statistics.median(us), 1), min_us=round(min(us), 1), max_us=round(max(us), 1),
                p10_us=round(pct(us, 0.10), 1), p90_us=round(pct(us, 0.90), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ports", action="store_true", help="a preemptor with a host port one bound pod per node holds")
    ap.add_argument("--anti", action="store_true", help="a preemptor with a required zone anti-affinity term")
    ap.add_argument("--spread", action="store_true", help="a preemptor with a DoNotSchedule zone spread constraint")
    ap.add_argument("--volumes", action="store_true", help="counted volumes on every bound pod and the preemptor")
    ap.add_argument("--full", action="store_true", help="--volumes' load, and hostname anti-affinity and a zone spread "
                                                        "constraint on the preemptor (ksim_preempt_full)")
    ap.add_argument("--pdbs", type=int, default=0, help="this many budgets (disruptionsAllowed 1), each bound pod in one")
    args = ap.parse_args()
    if args.ports + args.anti + args.spread + args.volumes + args.full > 1:
        ap.error("--ports, --anti, --spread, --volumes or --full, not two of them")
    cluster, table, enc, prof = build_anti(args.nodes, args.spread) if args.anti or args.spread else \
        build_volumes(args.nodes, args.full) if args.volumes or args.full else \
        build_ports(args.nodes) if args.ports else build(args.nodes)
    kw = dict(hard_spread=True) if args.spread else dict(volumes=True) if args.volumes else \
        dict(full=True) if args.full else {}
    budgets = None
    if args.pdbs > 0:
        budgets = (np.ones(args.pdbs, np.int32), np.arange(table.n + 1, dtype=np.int32),
                   (np.asarray(table.node) % args.pdbs).astype(np.int32))
    runs, every, result = [], [], None
    for _ in range(args.repeats):
        eng = engine.Engine(0)
        eng.set_profile(prof)
        eng.set_cluster(cluster)
        eng.set_bound_pods(table)
        if budgets is not None:
            eng.set_bound_pod_pdbs(*budgets)
        for _ in range(args.warmup):
            result = eng.preempt(enc, 0, 1000, with_pdb=budgets is not None, **kw)
        us = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            eng.preempt(enc, 0, 1000, **kw)
            us.append((time.perf_counter() - t0) * 1e6)
        eng.close()
        runs.append(summary(us))
        every += us
    name = ("preempt_ports" if args.ports else "preempt_zone_anti" if args.anti else "preempt_zone_spread" if args.spread else
            "preempt_volumes" if args.volumes else "preempt_full" if args.full else "preempt_use_free") + ("_pdb" if budgets is not None else "")
    extra = dict(pdbs=args.pdbs, pdb_violations=result[4]) if budgets is not None else {}
    print(json.dumps(dict(bench=name, library=os.path.basename(engine.LIB_PATH), nodes=args.nodes,
                          bound_pods=table.n, calls=args.calls, repeats=args.repeats,
                          nominated=result[0], victims=len(result[1]), potential=result[2], candidates=result[3],
                          runs=runs, **extra, **summary(every))))


if __name__ == "__main__":
    main()
