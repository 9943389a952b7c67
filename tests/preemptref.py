"""DefaultPreemption's dry run restated in numpy, for preemptors the C oracle
refuses (it refuses every pod with a use): the reference of
tests/test_gpu_preempt_uses.py, pinned to the oracle on use-free pods by
tests/test_preempt_uses.py.  No code is shared with the engine or the oracle.

The dry run (include/ksim_engine.h, ksim_preempt):
  1. potential nodes: the per-node first failing filter is NodeResourcesFit
     or NodePorts (either may be absent from the profile);
  2. per potential node SelectVictimsOnNode: take out every bound pod of
     lower priority (its requests, and its count in each of the preemptor's
     port classes); the node is a candidate when the preemptor then fits and
     no port class has a pod left; add the pods back most important first
     (priority descending, start ascending, table row), keeping each one the
     preemptor still passes beside, the others are the victims;
  3. the first numCandidates = max(pct % of the potential nodes, abs)
     candidates in node order are kept;
  4. pickOneNodeForPreemption: lowest highest-victim priority, lowest sum of
     (priority + 2^31), fewest victims, latest earliest start among the
     highest-priority victims, then the first.
NodeResourcesFit is fitsRequest (v1.26): the pod count, then, unless the pod
requests nothing, each of cpu / memory / ephemeral-storage and each requested
scalar against allocatable minus requested."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ksim import abi

I32_MIN = -(2 ** 31)


def columns(cluster) -> dict:
    """The node columns the dry run reads, from an EncodedCluster."""
    n, s = cluster.n_nodes, cluster.n_scalar
    alloc = np.zeros((n, abi.PREEMPT_REQ), np.int64)
    req = np.zeros((n, abi.PREEMPT_REQ), np.int64)
    alloc[:, 0], alloc[:, 1], alloc[:, 2] = cluster.alloc_cpu, cluster.alloc_mem, cluster.alloc_eph
    req[:, 0], req[:, 1], req[:, 2] = cluster.req_cpu, cluster.req_mem, cluster.req_eph
    for k in range(s):
        alloc[:, 3 + k] = cluster.alloc_scalar[k]
        req[:, 3 + k] = cluster.req_scalar[k]
    cc = cluster.class_count if cluster.class_count is not None else np.zeros((0, n), np.int32)
    return dict(alloc=alloc, req=req, alloc_pods=np.asarray(cluster.alloc_pods, np.int64),
                num_pods=np.asarray(cluster.num_pods, np.int64), class_count=np.asarray(cc, np.int64))


def pod_inputs(enc, index: int) -> Tuple[np.ndarray, List[int]]:
    """(requests [PREEMPT_REQ], port classes) of pod ``index`` of an EncodedPods."""
    p = enc.pods[index]
    req = np.zeros(abi.PREEMPT_REQ, np.int64)
    req[0], req[1], req[2] = p["req_cpu"], p["req_mem"], p["req_eph"]
    req[3:] = p["scalar_req"]
    u = enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
    return req, [int(x["cls"]) for x in u if int(x["kind"]) == abi.USE_NODE_PORT]


def filter_positions(prof) -> Tuple[Optional[int], Optional[int]]:
    """(position of NodeResourcesFit, of NodePorts) in a compiled profile's filter list."""
    order = [int(prof.filter[i]) for i in range(prof.n_filter)]
    fit = order.index(abi.PL_NODE_RESOURCES_FIT) if abi.PL_NODE_RESOURCES_FIT in order else None
    port = order.index(abi.PL_NODE_PORTS) if abi.PL_NODE_PORTS in order else None
    return fit, port


def _row_adds(table, row: int) -> Dict[int, int]:
    if getattr(table, "adds_off", None) is None:
        return {}
    out: Dict[int, int] = {}
    for cls, cnt in table.adds[int(table.adds_off[row]):int(table.adds_off[row + 1])]:
        out[int(cls)] = out.get(int(cls), 0) + int(cnt)
    return out


def dry_run(fail: Sequence[int], cols: dict, table, priority: int, pod_req: np.ndarray, port_classes: Sequence[int],
            fit_pos: Optional[int], port_pos: Optional[int], min_pct: int, min_abs: int,
            groups: Sequence[Tuple[int, np.ndarray, int, Dict[int, int]]] = ()) -> tuple:
    """(nominated node or -1, victim rows in reprieve order, potential nodes,
    candidates kept).  ``fail``: per node the first failing filter's position
    (abi.PASSED: none).  ``table``: an abi.BoundPods (with adds when the pod
    has port classes).  ``groups``: (node, requests [PREEMPT_REQ], pods,
    {class: count}) of the nominated pods that stay on a node."""
    pod_req = np.asarray(pod_req, np.int64)
    ports = list(port_classes) if port_pos is not None else []    # no NodePorts filter: ports ignored
    n = len(fail)
    by_node: Dict[int, List[int]] = {}
    for i in range(table.n):
        by_node.setdefault(int(table.node[i]), []).append(i)
    group = {int(g[0]): g for g in groups}

    def passes(node, used, pods, held) -> bool:
        if fit_pos is not None:
            if pods + 1 > cols["alloc_pods"][node]:
                return False
            if pod_req.any() and (pod_req > cols["alloc"][node] - used)[(pod_req != 0) | (np.arange(pod_req.size) < 3)].any():
                return False
        return all(h <= 0 for h in held)

    potential = [v for v in range(n) if (fit_pos is not None and fail[v] == fit_pos) or
                 (ports and fail[v] == port_pos)]
    want = min(max(len(potential) * min_pct // 100, min_abs), len(potential))
    kept: List[Tuple[tuple, int, List[int]]] = []
    for node in potential:
        if len(kept) >= want:
            break
        used = cols["req"][node].copy()
        pods = int(cols["num_pods"][node])
        held = [int(cols["class_count"][c][node]) if c >= 0 else 0 for c in ports]
        if node in group:
            _, greq, gpods, gadds = group[node]
            used += np.asarray(greq, np.int64)
            pods += int(gpods)
            held = [h + int(gadds.get(c, 0)) for h, c in zip(held, ports)]
        lower = sorted((i for i in by_node.get(node, []) if int(table.priority[i]) < priority),
                       key=lambda i: (-int(table.priority[i]), int(table.start_time[i]), i))
        adds = {i: _row_adds(table, i) for i in lower} if ports else {i: {} for i in lower}
        for i in lower:
            used -= table.req[i]
            pods -= 1
            held = [h - adds[i].get(c, 0) for h, c in zip(held, ports)]
        if not passes(node, used, pods, held):
            continue
        victims = []
        for i in lower:
            used2 = used + table.req[i]
            held2 = [h + adds[i].get(c, 0) for h, c in zip(held, ports)]
            if passes(node, used2, pods + 1, held2):
                used, pods, held = used2, pods + 1, held2
            else:
                victims.append(i)
        high = int(table.priority[victims[0]]) if victims else I32_MIN
        total = sum(int(table.priority[i]) + 2 ** 31 for i in victims)
        early = min((int(table.start_time[i]) for i in victims if int(table.priority[i]) == high), default=2 ** 63 - 1)
        kept.append(((high, total, len(victims), -early, len(kept)), node, victims))
    if not kept:
        return -1, [], len(potential), 0
    _, node, victims = min(kept, key=lambda k: k[0])
    return node, victims, len(potential), len(kept)


def group_inputs(enc, indices: Sequence[int], node: int) -> Tuple[int, np.ndarray, int, Dict[int, int]]:
    """A ``groups`` entry of dry_run for the pods ``indices`` of ``enc`` nominated on ``node``."""
    req = np.zeros(abi.PREEMPT_REQ, np.int64)
    adds: Dict[int, int] = {}
    for i in indices:
        req += pod_inputs(enc, i)[0]
        p = enc.pods[i]
        for a in enc.adds[int(p["add_first"]):int(p["add_first"]) + int(p["add_count"])]:
            adds[int(a["cls"])] = adds.get(int(a["cls"]), 0) + int(a["count"])
    return node, req, len(indices), adds
