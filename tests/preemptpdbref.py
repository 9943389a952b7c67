"""DefaultPreemption's dry run with PodDisruptionBudgets at the object level:
the reference of tests/test_gpu_preempt_pdb.py, pinned by
tests/test_preempt_pdb_ref.py to oracle/objref.py ObjScheduler.preempt and to
the C oracle wherever no budget matches a lower-priority pod.  It is literal to
the upstream structure (v1.26.2, restated from memory):

  filterPodsWithPDBViolation   per node, over the lower-priority pods sorted by
      MoreImportantPod, from a fresh copy of every budget's
      status.disruptionsAllowed: each budget that matches the pod is decremented
      and the pod violates when one of them is then below zero;
  SelectVictimsOnNode          every lower-priority pod out, the filters, then
      two reprieve loops: the violating pods, then the others, each most
      important first; the victims list keeps that order (no re-sort);
  dryRunPreemption             nodes in order (offset 0), stopping once
      nonViolating >= 1 and nonViolating + violating >= numCandidates;
  pickOneNodeForPreemption     fewest violations, lowest priority of victims[0],
      lowest sum of (priority + 2^31), fewest victims, latest
      GetEarliestPodStartTime (earliest start among the victims of the true
      maximum priority), then the first.

The filters are oracle/objref.py's, through tests/preemptobjref.py's
recomputing trial state (imported unmodified), so preemptors with host ports or
required pod (anti-)affinity work as they do there.  Labels are strings and
selectors ksim.model.LabelSelector objects; no code is shared with the engine
or with ksim.preemption.pdb_matches.

numCandidates == 0 tries no node: the reading ObjScheduler.preempt, the C
oracle and the engine already have.

``fault`` switches on one wrong reading an implementation could have (FAULTS),
for the test that the scenes of tests/preemptpdbcases.py tell each from the
reference."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

from ksim import profile
from ksim.model import Node, Pod, PodDisruptionBudget
from oracle.objref import IPA_ANTI, IPA_EXIST

import preemptobjref

FAULTS = ("no_violation_level",         # the pick starts at victims[0]'s priority
          "violating_not_first",        # one reprieve loop in importance order
          "shared_budgets",             # one copy of the budgets for every node
          "higher_priority_consume",    # pods that outrank the preemptor decrement too
          "nominated_consume",          # the node's nominated pods decrement too
          "two_pdbs_once",              # a pod stops at the first budget that matches it
          "high_is_max",                # level 2 on the highest victim priority
          "early_sorted_shortcut",      # level 5 among the victims of victims[0]'s priority
          "violations_before_reprieve",  # every violating pod counted, reprieved or not
          "old_cut",                    # the first numCandidates candidates
          "namespace_ignored",
          "empty_selector_matches",
          "unlabelled_matches",
          "disrupted_not_excluded")


def matching(pod: Pod, pdbs: Sequence[PodDisruptionBudget], fault: Optional[str] = None) -> List[int]:
    """The budgets filterPodsWithPDBViolation decrements for ``pod``."""
    if not pod.labels and fault != "unlabelled_matches":
        return []
    out = []
    for i, pdb in enumerate(pdbs):
        if pdb.namespace != pod.namespace and fault != "namespace_ignored":
            continue
        sel = pdb.selector
        if sel is None:                                    # LabelSelectorAsSelector(nil) = Nothing
            continue
        if sel.empty() and fault != "empty_selector_matches":
            continue
        if not sel.matches(dict(pod.labels)):
            continue
        if pod.name in pdb.disrupted_pods and fault != "disrupted_not_excluded":
            continue
        out.append(i)
        if fault == "two_pdbs_once":
            break
    return out


def dry_run(nodes: List[Node], bound: List[Pod], start: Dict[str, int], order: Dict[str, int], pod: Pod,
            priority: int, args=(10, 100), nominated: Optional[Dict[str, List[Pod]]] = None,
            pdbs: Sequence[PodDisruptionBudget] = (), fault: Optional[str] = None,
            filter_order=None) -> Tuple[Optional[str], List[str], int, int, int]:
    """(nominated node name or None, victim names in list order, potential
    nodes, candidates kept, PDB violations on the nominated node)."""
    assert fault is None or fault in FAULTS
    run = preemptobjref._Run(nodes, bound, pod, nominated, None, filter_order)
    s = run.s
    potential = []
    for ni in s.nodes:
        pl, msg = s.filter_with_nominated(pod, ni, run.pts0, run.ipa0, run.nominated)
        if pl in ("NodeResourcesFit", "NodePorts") or (pl == "InterPodAffinity" and msg in (IPA_ANTI, IPA_EXIST)):
            potential.append(ni)
    pa = profile.PreemptionArgs(*args)
    want = min(max(len(potential) * pa.min_candidate_nodes_percentage // 100, pa.min_candidate_nodes_absolute),
               len(potential))
    shared = [b.disruptions_allowed for b in pdbs]

    def more_important(q: Pod):
        return (-q.priority, start[q.name], order[q.name])

    def filter_pods_with_pdb_violation(ni, lower: List[Pod]) -> Tuple[List[Pod], List[Pod]]:
        allowed = shared if fault == "shared_budgets" else [b.disruptions_allowed for b in pdbs]
        walk = list(lower)
        if fault == "higher_priority_consume":
            walk = sorted((pi.pod for pi in ni.pods), key=more_important)
        if fault == "nominated_consume":
            walk = run.staying(ni) + walk
        violating, non_violating = [], []
        for q in walk:
            violated = False
            for i in matching(q, pdbs, fault):
                allowed[i] -= 1
                if allowed[i] < 0:
                    violated = True
            if q in lower:
                (violating if violated else non_violating).append(q)
        return violating, non_violating

    def select_victims_on_node(ni) -> Optional[Tuple[List[Pod], int]]:
        here = [pi.pod for pi in ni.pods]
        lower = sorted((q for q in here if q.priority < priority), key=more_important)
        on = [q for q in here if q.priority >= priority]
        if not run.passes_recomputed(ni, on):
            return None
        violating, non_violating = filter_pods_with_pdb_violation(ni, lower)
        victims, num_violating = [], 0

        def reprieve(q: Pod) -> bool:
            if run.passes_recomputed(ni, on + [q]):
                on.append(q)
                return True
            victims.append(q)
            return False

        if fault == "violating_not_first":
            for q in lower:
                if not reprieve(q) and q in violating:
                    num_violating += 1
        else:
            for q in violating:
                if not reprieve(q):
                    num_violating += 1
            for q in non_violating:
                reprieve(q)
        if fault == "violations_before_reprieve":
            num_violating = len(violating)
        return victims, num_violating

    cands: List[Tuple[object, List[Pod], int]] = []
    clean = 0
    if want > 0:
        for ni in potential:
            if fault == "old_cut" and len(cands) >= want:
                break
            got = select_victims_on_node(ni)
            if got is None:
                continue
            cands.append((ni, got[0], got[1]))
            clean += got[1] == 0
            if fault != "old_cut" and clean >= 1 and len(cands) >= want:
                break
    if not cands:
        return None, [], len(potential), 0, 0

    def criteria(c):                                       # pickOneNodeForPreemption
        _, v, nviol = c
        top = max((q.priority for q in v), default=-(2 ** 31))
        high = (top if fault == "high_is_max" else v[0].priority) if v else -(2 ** 31)
        total = sum(q.priority + 2 ** 31 for q in v)
        among = v[0].priority if (fault == "early_sorted_shortcut" and v) else top
        early = min((start[q.name] for q in v if q.priority == among), default=2 ** 63)
        return (0 if fault == "no_violation_level" else nviol, high, total, len(v), -early)
    best = min(range(len(cands)), key=lambda i: (criteria(cands[i]), i))
    ni, v, nviol = cands[best]
    return ni.node.name, [q.name for q in v], len(potential), len(cands), nviol


def as_indices(result, node_names: Sequence[str], order: Dict[str, int]) -> tuple:
    """The engine's 5-tuple: node position (-1: none), bound-pod table rows, the counts."""
    name, victims, n_pot, n_cand, nviol = result
    return ((list(node_names).index(name) if name is not None else -1), [order[v] for v in victims], n_pot, n_cand,
            nviol)
