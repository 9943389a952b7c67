"""DefaultPreemption's dry run at the object level for preemptors with
DoNotSchedule topology spread (ksim_preempt_spread): the reference of
tests/test_gpu_preempt_spread.py, pinned by tests/test_preempt_spread_ref.py to
tests/preemptobjref.py on every scene without such a constraint.  No code is
shared with the engine.

The dry run is preemptobjref's recomputation, ``_Run.passes_recomputed``
imported unmodified: every trial state of a node rebuilds the node's NodeInfo
from the pods that stay plus its nominated pods and runs ``pts_prefilter``,
``ipa_prefilter`` and ``filter_node`` from scratch.  For PodTopologySpread that
is a legitimate reference because upstream's TpPairToMatchNum is a plain sum
over the eligible nodes (pairs kept at zero), moved by updateWithPod by exactly
the pods the sum would count, and TpKeyToCriticalPaths is its exact minimum as
long as one domain moves: in node n's dry run only n's pods move, so only the
pair of n's own domain changes, and the two-entry criticalPaths.update is exact
under moves of a single pair.

What this file adds is the potential-node rule: preemptobjref.dry_run's plus
PodTopologySpread with the skew message (Unschedulable; the missing-label
message is UnschedulableAndUnresolvable), and a ``filter_order``.

``flaw`` switches on one faulty reading (FLAWS), for the test that the scenes of
tests/preemptspreadcases.py discriminate.  The readings move the status pass's
pairs incrementally by the pods of the node under trial; with no flaw
(``flaw="none"``) that incremental form equals the recomputation."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import preemptobjref
from ksim import profile
from ksim.model import Node, Pod, selector_matches
from oracle.objref import IPA_ANTI, IPA_EXIST, PTS_MISSING, PTS_SKEW, NodeInfo

FLAWS = ("stale_domains",            # the own domain's count never moves
         "stale_min",                # the status pass's minimum is kept as is
         "ineligible_moves",         # pods of a node the inclusion policy excludes move the domain
         "missing_label_potential",  # nodes failing for a missing label count as potential
         "no_pts_in_reprieve",       # PodTopologySpread skipped while pods are put back
         "no_self_match",            # selfMatch taken as 0
         "other_namespace_counts",   # a pod with matching labels in another namespace moves the count
         "group_ignored")            # a nominated group's matching pods are not added

MAX_INT32 = 2 ** 31 - 1


class _Run(preemptobjref._Run):
    def passes_incremental(self, ni: NodeInfo, pods_on: List[Pod], out: List[Pod], reprieving: bool) -> bool:
        flaw, s, pod, node = self.flaw, self.s, self.pod, ni.node
        staying = self.staying(ni)
        fresh = NodeInfo(node)
        for q in pods_on + staying:
            fresh.add_pod(q)
        cons, pair0, crit0 = self.pts0
        pair = dict(pair0)
        moves = ([] if flaw == "group_ignored" else [(q, +1) for q in staying]) + [(q, -1) for q in out]
        if flaw != "stale_domains" and all(c.topology_key in node.labels for c in cons):     # updateWithPod
            for c in cons:
                if not (s._inclusion(c, pod, node) or flaw == "ineligible_moves"):
                    continue
                if c.label_selector is None or c.label_selector.empty():
                    continue
                key = (c.topology_key, node.labels[c.topology_key])
                for q, sign in moves:
                    same_ns = q.namespace == pod.namespace or flaw == "other_namespace_counts"
                    if same_ns and c.label_selector.matches(q.labels):
                        pair[key] = pair.get(key, 0) + sign
        crit = dict(crit0)
        if flaw != "stale_min":
            crit = {c.topology_key: MAX_INT32 for c in cons}
            for (k, _), num in pair.items():
                crit[k] = min(crit[k], num)
        if flaw == "no_self_match":                       # match + 0 - min > skew
            cons = [dataclasses.replace(c, max_skew=c.max_skew + (1 if selector_matches(c.label_selector, pod.labels)
                                                                  else 0)) for c in cons]
        at = s.nodes.index(ni)
        s.nodes[at] = s.by_name[node.name] = fresh
        saved = s.filter_order
        if flaw == "no_pts_in_reprieve" and reprieving:
            s.filter_order = [pl for pl in saved if pl != "PodTopologySpread"]
        try:
            return s.filter_node(pod, fresh, (cons, pair, crit), s.ipa_prefilter(pod))[0] is None
        finally:
            s.filter_order = saved
            s.nodes[at] = s.by_name[node.name] = ni


def dry_run(nodes: List[Node], bound: List[Pod], start: Dict[str, int], order: Dict[str, int], pod: Pod,
            priority: int, args=(10, 100), nominated: Optional[Dict[str, List[Pod]]] = None,
            flaw: Optional[str] = None, filter_order=None) -> Tuple[Optional[str], List[str], int, int]:
    """(nominated node name or None, victim names in reprieve order, potential
    nodes, candidates kept), as preemptobjref.dry_run.  ``flaw``: None for the
    reference, "none" for its incremental form, or one of FLAWS."""
    assert flaw is None or flaw == "none" or flaw in FLAWS
    run = _Run(nodes, bound, pod, nominated, flaw, filter_order)
    s = run.s
    potential = []
    for ni in s.nodes:
        pl, msg = s.filter_with_nominated(pod, ni, run.pts0, run.ipa0, run.nominated)
        if pl in ("NodeResourcesFit", "NodePorts") or (pl == "InterPodAffinity" and msg in (IPA_ANTI, IPA_EXIST)) or \
                (pl == "PodTopologySpread" and (msg == PTS_SKEW or
                                                (flaw == "missing_label_potential" and msg == PTS_MISSING))):
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


as_indices = preemptobjref.as_indices
