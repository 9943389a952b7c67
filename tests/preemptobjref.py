"""DefaultPreemption's dry run at the object level, for preemptors with required
pod (anti-)affinity, which the C oracle refuses: the reference of
tests/test_gpu_preempt_affinity.py, pinned by tests/test_preempt_affinity_ref.py
to oracle/objref.py ObjScheduler.preempt and to the C oracle on every use-free
case.  oracle/objref.py is imported unmodified; no code is shared with the
engine.

Upstream (v1.26 SelectVictimsOnNode) copies the cycle state per node and moves
it with PreFilterExtensions.RemovePod / AddPod.  The InterPodAffinity maps are
plain sums over the pods with delete-at-zero, so the moved state equals
PreFilter run from scratch over the cluster with the pods taken out.  That is
what ``dry_run`` does: for every trial state of a node (every lower-priority
pod out, then each put back in MoreImportantPod order) it rebuilds the node's
NodeInfo from the pods that stay plus the node's nominated pods, inside a
scheduler whose other NodeInfos are never touched (so they hold what a fresh
ObjScheduler over the same nodes and the remaining pods would), and calls
``ipa_prefilter``, ``pts_prefilter`` and ``filter_node``.

Potential nodes come from ``filter_node``'s (plugin, message) on the cluster as
it stands: NodeResourcesFit, NodePorts, and InterPodAffinity's two
anti-affinity messages (the affinity message is UnschedulableAndUnresolvable).
The cut and the pick follow ObjScheduler.preempt.

``flaw`` switches on one faulty variant of the dry run, for the test that the
scenes discriminate (FLAWS).  The variants move the maps incrementally, by each
pod's own contribution (PreFilter over that pod alone); with no flaw that
incremental form equals the recomputation, which ``dry_run(..., flaw="none")``
exposes so the test can check the machinery the variants are built on."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

from ksim import profile
from ksim.model import Node, Pod
from oracle.objref import IPA_AFF, IPA_ANTI, IPA_EXIST, LABEL_HOSTNAME, NodeInfo, ObjScheduler

FLAWS = ("stale_domains",          # domain counts never adjusted
         "node_local_only",        # only hostname-keyed (node-local) counts adjusted
         "multiplicity_one",       # a pod moves each pair by 1, not by its count
         "stale_emptiness",        # len(affinityCounts) as before the removals
         "no_ipa_in_reprieve",     # InterPodAffinity skipped while pods are put back
         "affinity_potential")     # nodes failing the affinity rule count as potential


def _carries_terms(p: Pod) -> bool:
    return bool(p.pod_affinity_required or p.pod_anti_affinity_required)


class _Run:
    def __init__(self, nodes, bound, pod, nominated, flaw, filter_order):
        self.nodes, self.bound, self.pod, self.nominated, self.flaw = nodes, list(bound), pod, nominated or {}, flaw
        self.s = ObjScheduler(nodes, self.bound, pct=100, seed=0)
        if filter_order is not None:
            self.s.filter_order = list(filter_order)
        everyone = self.bound + [q for qs in self.nominated.values() for q in qs]
        # no pod carries a term and the preemptor has no hard spread: PreFilter's
        # state does not depend on which pods are out (it is empty), computed once
        self.static = not _carries_terms(pod) and not any(_carries_terms(q) for q in everyone) and \
            not any(c.when_unsatisfiable == "DoNotSchedule" for c in pod.topology_spread)
        self.pts0, self.ipa0 = self.s.pts_prefilter(pod), self.s.ipa_prefilter(pod)
        self._contrib: Dict[str, tuple] = {}

    def staying(self, ni: NodeInfo):
        return ObjScheduler._nominated_for(self.pod, ni, self.nominated)

    # ---- the right dry run: PreFilter from scratch ---------------------------------------
    def passes_recomputed(self, ni: NodeInfo, pods_on: List[Pod]) -> bool:
        fresh = NodeInfo(ni.node)
        for q in pods_on + self.staying(ni):
            fresh.add_pod(q)
        s, at = self.s, self.s.nodes.index(ni)
        s.nodes[at] = s.by_name[ni.node.name] = fresh
        try:
            pts, ipa = (self.pts0, self.ipa0) if self.static else (s.pts_prefilter(self.pod), s.ipa_prefilter(self.pod))
            return s.filter_node(self.pod, fresh, pts, ipa)[0] is None
        finally:
            s.nodes[at] = s.by_name[ni.node.name] = ni

    # ---- the incremental form, with the flaws ---------------------------------------------
    def contrib(self, q: Pod, node: Node) -> tuple:
        """(existing, aff, anti) of ``q`` alone on ``node``: the maps are sums over pods."""
        if q.name not in self._contrib:
            one = ObjScheduler(self.nodes, [dataclasses.replace(q, node_name=node.name)], pct=100, seed=0)
            self._contrib[q.name] = one.ipa_prefilter(self.pod)[2:5]
        return self._contrib[q.name]

    def passes_incremental(self, ni: NodeInfo, pods_on: List[Pod], out: List[Pod], reprieving: bool) -> bool:
        flaw = self.flaw
        fresh = NodeInfo(ni.node)
        for q in pods_on + self.staying(ni):
            fresh.add_pod(q)
        req_aff, req_anti, ex0, aff0, anti0, self_match = self.ipa0
        maps = [dict(ex0), dict(aff0), dict(anti0)]
        moves = [(q, +1) for q in self.staying(ni)] + [(q, -1) for q in out]
        for q, sign in moves:
            if flaw == "stale_domains":
                continue
            for m, c in zip(maps, self.contrib(q, ni.node)):
                for pair, k in c.items():
                    if flaw == "node_local_only" and pair[0] != LABEL_HOSTNAME:
                        continue
                    m[pair] = m.get(pair, 0) + sign * (1 if flaw == "multiplicity_one" else k)
        for i, m in enumerate(maps):                     # delete at zero
            keep_zero = flaw == "stale_emptiness" and i == 1
            maps[i] = {pair: k for pair, k in m.items() if k > 0 or (keep_zero and pair in aff0)}
        ipa = (req_aff, req_anti, maps[0], maps[1], maps[2], self_match)
        s = self.s
        saved = s.filter_order
        if flaw == "no_ipa_in_reprieve" and reprieving:
            s.filter_order = [pl for pl in saved if pl != "InterPodAffinity"]
        try:
            return s.filter_node(self.pod, fresh, self.pts0, ipa)[0] is None
        finally:
            s.filter_order = saved


def dry_run(nodes: List[Node], bound: List[Pod], start: Dict[str, int], order: Dict[str, int], pod: Pod,
            priority: int, args=(10, 100), nominated: Optional[Dict[str, List[Pod]]] = None,
            flaw: Optional[str] = None, filter_order=None) -> Tuple[Optional[str], List[str], int, int]:
    """(nominated node name or None, victim names in reprieve order, potential
    nodes, candidates kept).  ``nominated``: {node name: pods nominated there};
    the ones of priority >= the pod's stay on their node through its dry run
    (pass 1 of RunFilterPluginsWithNominatedPods).  ``flaw``: None for the
    reference, "none" for its incremental form, or one of FLAWS."""
    assert flaw is None or flaw == "none" or flaw in FLAWS
    run = _Run(nodes, bound, pod, nominated, flaw, filter_order)
    s = run.s
    unresolvable_ok = flaw == "affinity_potential"
    potential = []
    for ni in s.nodes:
        pl, msg = s.filter_with_nominated(pod, ni, run.pts0, run.ipa0, run.nominated)
        if pl in ("NodeResourcesFit", "NodePorts") or \
                (pl == "InterPodAffinity" and (msg in (IPA_ANTI, IPA_EXIST) or (unresolvable_ok and msg == IPA_AFF))):
            potential.append(ni)
    pa = profile.PreemptionArgs(*args)
    want = min(max(len(potential) * pa.min_candidate_nodes_percentage // 100, pa.min_candidate_nodes_absolute),
               len(potential))

    def passes(ni, on, out, reprieving):
        if flaw is None:
            return run.passes_recomputed(ni, on)
        return run.passes_incremental(ni, on, out, reprieving)

    def select_victims(ni):
        here = [pi.pod for pi in ni.pods]
        lower = [q for q in here if q.priority < priority]
        lower.sort(key=lambda q: (-q.priority, start[q.name], order[q.name]))       # MoreImportantPod
        on = [q for q in here if q.priority >= priority]
        out = list(lower)
        if not passes(ni, on, out, False):
            return None
        victims = []
        for q in lower:                                    # reprievePod
            out.remove(q)
            if passes(ni, on + [q], out, True):
                on.append(q)
            else:
                out.append(q)
                victims.append(q)
        return victims

    cands = []
    for ni in potential:
        if len(cands) >= want:
            break
        v = select_victims(ni)
        if v is not None:
            cands.append((ni, v))
    if not cands:
        return None, [], len(potential), 0

    def criteria(c):                                       # pickOneNodeForPreemption (no PDBs)
        v = c[1]
        high = v[0].priority if v else -(2 ** 31)
        total = sum(q.priority + 2 ** 31 for q in v)
        early = min((start[q.name] for q in v if q.priority == high), default=2 ** 63)
        return (high, total, len(v), -early)
    best = min(range(len(cands)), key=lambda i: (criteria(cands[i]), i))
    return cands[best][0].node.name, [q.name for q in cands[best][1]], len(potential), len(cands)


def as_indices(result, node_names: List[str], order: Dict[str, int]) -> tuple:
    """The engine's 4-tuple: node position (-1: none) and bound-pod table rows."""
    name, victims, n_pot, n_cand = result
    return (list(node_names).index(name) if name is not None else -1), [order[v] for v in victims], n_pot, n_cand
