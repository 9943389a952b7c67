"""The scenes of tests/preemptvolcases.py compiled for the engine, and a numpy
restatement of the volume form's *incremental* rule over the compiled tables
(ksim.volumes.VolumeLimits, ksim.preemption.bound_table(..., vol_limits=), the
encoded uses): what csrc/ksim_preempt.hip computes, written a second time so
that the compile and the reaches-0 rule are pinned to the object-level
reference (tests/preemptvolref.py) before any GPU run.

The model keeps the live count of every volume class per node (the second of
the two exact last-holder schemes; the device counts the rows that are out
against its class counts instead, so the two check each other).  It knows
NodeResourcesFit on cpu, memory and the pod count, NodePorts on the port
classes, and the four limit plugins: the filters the scenes' nodes can fail.
``wrap32``: the sums in 32 bits, the faulty reading no object scene can show."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.preemption import bound_table
from ksim.volumes import VolumeIndex

import preemptvolcases as cases

LIMIT_PLUGINS = {abi.PL_EBS_LIMITS: "EBSLimits", abi.PL_GCEPD_LIMITS: "GCEPDLimits",
                 abi.PL_NODE_VOLUME_LIMITS: "NodeVolumeLimits", abi.PL_AZURE_DISK_LIMITS: "AzureDiskLimits"}
I32_MAX = 2 ** 31 - 1


def sched_profile(order, args=(100, 0)):
    plugins = profile.convert_for_simulator({"filter": profile.PluginSet([profile.Plugin(n) for n in order],
                                                                         [profile.Plugin("*")])})
    return profile.SchedulerProfile(plugins=plugins, percentage_of_nodes_to_score=100,
                                    preemption=profile.PreemptionArgs(*args))


@dataclass
class Built:
    sc: object
    cluster: object
    vl: object
    enc: object
    table: object
    sp: object
    prof: object
    groups: Optional[List[Tuple[int, List[int]]]]
    nodes: list                                   # the scene's nodes in the cluster's order


def build(sc, extra_pods=(), order=None) -> Built:
    """The scene compiled: the limits compile over the bound pods and every
    pending pod (the preemptor, the nominated pods, ``extra_pods``), the pods'
    uses, and the bound-pod table with the rows' port and volume holdings."""
    pending = list(sc.pending) + list(extra_pods)
    index = VolumeIndex.from_nodes(sc.nodes, sc.pvs, sc.pvcs)
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    cluster.set_volume_limits(index.volume_limits(sc.nodes, sc.bound, pending))
    enc = encode_pods(cluster, pending, volumes=index)
    assert not (enc.pods["flags"] & abi.POD_HAS_VOLUMES).any()
    table = bound_table(cluster, sc.bound, sc.start, cluster.topo, vol_limits=cluster.vol_limits)
    sp = sched_profile(order or sc.filter_order, sc.args)
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    groups = [(pos[n], list(idx)) for n, idx in sc.nominated.items()] or None
    by_name = {n.name: n for n in sc.nodes}
    return Built(sc, cluster, cluster.vol_limits, enc, table, sp, profile.compile_profile(sp), groups,
                 [by_name[n] for n in cluster.node_names])


def patch_past_2_31(b: Built) -> None:
    """preemptvolcases.past_2_31's counts, written into the compiled tables."""
    assert b.vl.limit.shape == (1, 1) and b.table.vol_uses.size == 1 and int(b.table.vol_uses["cls"][0]) == -1
    b.vl.limit[0, 0] = cases.PAST_LIMIT
    b.vl.attached[0, 0] = cases.PAST_ATTACHED
    b.table.vol_uses["arg"][0] = cases.PAST_HELD
    p = b.enc.pods[0]
    u = b.enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
    at = int(p["use_first"]) + [int(k) for k in u["kind"]].index(abi.USE_VOLUME)
    assert int(b.enc.uses["cls"][at]) == -1
    b.enc.uses["arg"][at] = cases.PAST_ARG


def _uses(enc, i):
    p = enc.pods[i]
    return enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]


def _adds(enc, i):
    p = enc.pods[i]
    return enc.adds[int(p["add_first"]):int(p["add_first"]) + int(p["add_count"])]


def device_rule(b: Built, grouped: bool = True, wrap32: bool = False, index: int = 0,
                priority: int = cases.PRIO) -> tuple:
    """(nominated node or -1, victim rows in list order, potential nodes,
    candidates kept): ksim_preempt_volumes' result, from the compiled tables."""
    c, vl, t, enc = b.cluster, b.vl, b.table, b.enc
    order = b.sp.filter_order()
    N = c.n_nodes
    pod = enc.pods[index]
    fam_plugin = [LIMIT_PLUGINS[int(x)] for x in vl.family_plugin]
    uses = [u for u in _uses(enc, index)]
    vol_uses = [(int(u["col"]), int(u["cls"]), int(u["arg"])) for u in uses if int(u["kind"]) == abi.USE_VOLUME
                and fam_plugin[int(u["col"])] in order]
    port_cls = [int(u["cls"]) for u in uses if int(u["kind"]) == abi.USE_NODE_PORT] if "NodePorts" in order else []
    fams = sorted({f for f, _, _ in vol_uses})
    groups = dict(b.groups or []) if grouped else {}

    def wrap(x):
        return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31 if wrap32 else x

    class State:
        def __init__(self, n):
            self.n = n
            self.cpu, self.mem, self.pods = int(c.req_cpu[n]), int(c.req_mem[n]), int(c.num_pods[n])
            self.live: Dict[int, int] = {}                  # class -> pods on the node (ports and volumes)
            self.att = {f: int(vl.attached[f, n]) for f in fams}

        def count(self, cls):
            return self.live.setdefault(cls, int(c.class_count[cls, self.n]))

        def move(self, req, adds, vols, sign):
            self.cpu += sign * int(req[0])
            self.mem += sign * int(req[1])
            self.pods += sign
            for cls, k in adds:
                self.live[int(cls)] = self.count(int(cls)) + sign * int(k)
            for f, cls, arg in vols:
                if cls < 0:
                    if f in self.att:
                        self.att[f] += sign * arg
                    continue
                old = self.count(cls)
                self.live[cls] = old + sign
                if (old == 0 if sign > 0 else old == 1) and f in self.att:
                    self.att[f] += sign

        def first_failure(self) -> Optional[str]:
            bad = set()
            if self.cpu + int(pod["req_cpu"]) > int(c.alloc_cpu[self.n]) or \
                    self.mem + int(pod["req_mem"]) > int(c.alloc_mem[self.n]) or self.pods + 1 > int(c.alloc_pods[self.n]):
                bad.add("NodeResourcesFit")
            if any(self.count(x) > 0 for x in port_cls):
                bad.add("NodePorts")
            for f in fams:
                new = sum((1 if self.count(cls) == 0 else 0) if cls >= 0 else arg for g, cls, arg in vol_uses if g == f)
                lim = int(vl.limit[f, self.n])
                total = wrap(self.att[f] + new)
                csi = fam_plugin[f] == "NodeVolumeLimits"
                if lim != I32_MAX and total > lim and (not csi or new > 0):
                    bad.add(fam_plugin[f])
            hit = [pl for pl in order if pl in bad]
            return hit[0] if hit else None

    def pod_move(i):
        return ([int(enc.pods[i]["req_cpu"]), int(enc.pods[i]["req_mem"])], [(int(a["cls"]), int(a["count"])) for a in _adds(enc, i)],
                [(int(u["col"]), int(u["cls"]), int(u["arg"])) for u in _uses(enc, i) if int(u["kind"]) == abi.USE_VOLUME])

    def row_move(j):
        adds = t.adds[t.adds_off[j]:t.adds_off[j + 1]].tolist() if t.adds_off is not None else []
        v = t.vol_uses[t.vol_off[j]:t.vol_off[j + 1]]
        return (t.req[j], adds, [(int(u["col"]), int(u["cls"]), int(u["arg"])) for u in v])

    res = []
    for n in range(N):
        st = State(n)
        for i in groups.get(n, ()):
            st.move(*pod_move(i), 1)
        fail = st.first_failure()
        if fail is None and n in groups:                     # pass 2: the node as is
            fail = State(n).first_failure()
        if fail is None or not (fail in ("NodeResourcesFit", "NodePorts") or fail in LIMIT_PLUGINS.values()):
            continue
        rows = [j for j in range(t.n) if int(t.node[j]) == n]
        rows.sort(key=lambda j: (-int(t.priority[j]), int(t.start_time[j]), j))
        lower = [j for j in rows if int(t.priority[j]) < priority]
        for j in lower:
            st.move(*row_move(j), -1)
        if st.first_failure() is not None:
            res.append((n, None))
            continue
        victims = []
        for j in lower:
            st.move(*row_move(j), 1)
            if st.first_failure() is not None:
                st.move(*row_move(j), -1)
                victims.append(j)
        res.append((n, victims))
    n_pot = len(res)
    pa = b.sp.preemption
    want = min(max(n_pot * pa.min_candidate_nodes_percentage // 100, pa.min_candidate_nodes_absolute), n_pot)
    cands = [(n, v) for n, v in res if v is not None][:want]
    if not cands:
        return -1, [], n_pot, 0

    def criteria(cand):
        n, v = cand
        high = int(t.priority[v[0]]) if v else -(2 ** 31)
        total = sum(int(t.priority[j]) + 2 ** 31 for j in v)
        early = min((int(t.start_time[j]) for j in v if int(t.priority[j]) == high), default=2 ** 63)
        return (high, total, len(v), -early, n)
    n, v = min(cands, key=criteria)
    return n, list(v), n_pot, len(cands)
