"""Host side of DefaultPreemption: the bound-pod table the
engine's PostFilter dry run reads (ksim_bound_pods), built from the pods bound
in a snapshot.  Requests follow NodeInfo's Requested (the same
computePodResourceRequest the encoder uses)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import abi
from .encode import pod_requests
from .model import Pod, PodDisruptionBudget


def pdb_matches(rows: Sequence[Pod], pdbs: Sequence[PodDisruptionBudget]) -> List[List[int]]:
    """Per pod of ``rows`` the positions in ``pdbs`` of the budgets that match it,
    ascending (filterPodsWithPDBViolation, v1.26): the pod has at least one
    label, the namespaces are equal, the selector is non-nil, non-empty and
    matches the labels, and the pod's name is no key of status.disruptedPods."""
    out = []
    for p in rows:
        hit = []
        if p.labels:
            for k, b in enumerate(pdbs):
                if b.namespace != p.namespace or b.selector is None or b.selector.empty():
                    continue
                if b.selector.matches(p.labels) and p.name not in b.disrupted_pods:
                    hit.append(k)
        out.append(hit)
    return out


COMMIT_TILE = 1024   # rows per scan tile of ksim_preempt_commit's compaction (csrc kCommitTile)


def commit_args(answer, row_pod):
    """A dry run's answer (``Engine.preempt`` / ``preempt_many``: nominated node,
    victims, ...) as ``Engine.preempt_commit``'s arrays: the victims' rows of the
    bound table, and per row the index of that bound pod's record in the pod
    set handed to the commit.  ``row_pod``: that index per row of
    ``bound_table`` (a sequence or a mapping; the table's rows are the bound
    pods on the cluster's nodes, in list order).  No nominated node: empty arrays."""
    victims = [int(r) for r in answer[1]] if answer[0] >= 0 else []
    return np.array(victims, np.int32), np.array([row_pod[r] for r in victims], np.int32)


def bound_table(cluster, bound: Sequence[Pod], start_time: Dict[str, int], topo=None,
                full_adds: bool = False, pdbs: Optional[Sequence[PodDisruptionBudget]] = None,
                vol_limits=None) -> abi.BoundPods:
    """ksim_bound_pods for ``bound`` (pods whose node is in ``cluster``), in list order.
    With ``topo`` (the cluster's ksim.topology.TopologyIndex) the table also
    carries each row's host-port holdings (``topo.port_adds``, over the port
    classes registered so far: build it after the preemptor is encoded), which
    the dry run of a pod with host ports reads (ksim_set_bound_pod_adds).
    ``full_adds``: every class the row counts into instead (``topo.adds``: its
    carried terms, the selector classes it matches and its ports), which the dry
    run of a pod with required pod (anti-)affinity reads.
    ``pdbs``: the cluster's PodDisruptionBudgets; the table then carries their
    disruptionsAllowed and the budgets each row matches (``pdb_matches``;
    ksim_set_bound_pod_pdbs).  None or empty: no budgets.
    ``vol_limits``: the cluster's ksim.volumes.VolumeLimits (``cluster.vol_limits``,
    with ``topo``); the table then carries the rows' counted volumes
    (``bound_uses``: families by index, class ids from ``topo.volume_class``),
    which the dry run of a pod with counted volumes reads
    (ksim_set_bound_pod_volumes)."""
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    rows = [p for p in bound if p.node_name in pos]
    node = np.array([pos[p.node_name] for p in rows], np.int32)
    prio = np.array([p.priority for p in rows], np.int32)
    start = np.array([start_time[p.name] for p in rows], np.int64)
    req = np.zeros((len(rows), abi.PREEMPT_REQ), np.int64)
    for i, p in enumerate(rows):
        r = pod_requests(p)
        req[i, 0] = r.get("cpu", 0)
        req[i, 1] = r.get("memory", 0)
        req[i, 2] = r.get("ephemeral-storage", 0)
        for k, name in enumerate(cluster.scalar_names):
            req[i, 3 + k] = r.get(name, 0)
    budgets = {}
    if pdbs:
        hits = pdb_matches(rows, pdbs)
        budgets = dict(pdb_allowed=np.array([b.disruptions_allowed for b in pdbs], np.int32),
                       pdb_off=np.cumsum([0] + [len(h) for h in hits]).astype(np.int32),
                       pdb_ids=np.array([k for h in hits for k in h], np.int32))
    if vol_limits is not None:
        if topo is None:
            raise ValueError("vol_limits needs topo (the shared volumes' classes)")
        voff, vols = [0], []
        for p in rows:
            for f, shared, count in vol_limits.bound_uses.get((p.namespace, p.name), ()):
                cls = -1 if shared is None else topo.volume_class(vol_limits.families[f], shared)
                vols.append((cls, count, f))
            voff.append(len(vols))
        budgets.update(vol_off=np.array(voff, np.int32), vols=np.array(vols, np.int32).reshape(-1, 3))
    if topo is None:
        return abi.BoundPods(node, prio, start, req, **budgets)
    off, adds = [0], []
    for p in rows:
        adds.extend(topo.adds(p) if full_adds else sorted(topo.port_adds(p).items()))
        off.append(len(adds))
    return abi.BoundPods(node, prio, start, req, np.array(off, np.int32), np.array(adds, np.int32).reshape(-1, 2),
                         **budgets)
