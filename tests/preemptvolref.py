"""DefaultPreemption's dry run at the object level for preemptors with counted
volumes (EBSLimits, GCEPDLimits, NodeVolumeLimits, AzureDiskLimits): the
reference of tests/test_gpu_preempt_volumes.py, pinned by
tests/test_preempt_vol_ref.py to tests/preemptobjref.py on every use-free scene.

It is tests/preemptobjref.py's recomputing dry run (``_Run.passes_recomputed``,
imported unmodified) in which every filter pass additionally asks
tests/vollimitref.py ``VolLimitRef.failing(pod, node)`` (unmodified), recomputed
from the pods that stay on the node plus the node's nominated pods, and places
a failing limit plugin at its position in ``filter_order``.  The object
scheduler knows no PVs, so it sees every pod without its claims (VolumeBinding
and VolumeZone pass: the scenes' PVs carry no node affinity and no zone label);
the limit reference sees the real pods.  No code is shared with ksim.volumes or
the engine.

Potential nodes: the first failing filter is NodeResourcesFit, NodePorts or one
of the four limit plugins (all return plain Unschedulable; upstream counts such
a node among nodesWherePreemptionMightHelp).

With ``pdbs`` (budgets) the lower-priority pods are split as
filterPodsWithPDBViolation does and the violating ones are reprieved first, the
way tests/preemptpdbref.py has it (its ``matching`` decides which budgets a pod
decrements); the result then carries the nominated node's violations as a
fifth element.

``flaw`` switches on one wrong reading an implementation of the incremental
rule could have (FLAWS), for the test that the scenes of
tests/preemptvolcases.py tell each from the reference.  ``sums_32bit`` needs
counts no object scene can hold; tests/test_preempt_vol_ref.py shows it on the
array scene, through its numpy restatement of the device rule."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Set, Tuple

from ksim import profile
from ksim.model import Node, Pod
from preemptobjref import _Run, as_indices  # noqa: F401  (as_indices: re-exported)
from preemptpdbref import matching
from vollimitref import PLUGINS, VolLimitRef, owner

FLAWS = ("removed_stay_attached",      # a removed pod's volumes stay attached
         "shared_leaves_early",        # a shared volume leaves with the first holder taken out
         "stale_new",                  # the preemptor's new volumes as the status pass counted them
         "csi_rule_intree",            # in-tree families by the CSI rule
         "intree_rule_csi",            # CSI families fail with new == 0 as well
         "other_family_moves",         # a removed pod's volumes of any family lower the family's count
         "no_limits_in_reprieve",      # the limit plugins skipped while pods are put back
         "limit_not_potential",        # a node failing a limit plugin is no potential node
         "group_volumes_ignored",      # the nominated group's volumes are not on the node
         "absent_plugin_enforced")     # a limit plugin the profile lacks still fails the pod
POTENTIAL = ("NodeResourcesFit", "NodePorts") + PLUGINS


def _strip(q: Pod) -> Pod:
    return dataclasses.replace(q, pvc_claims=[])


class _VolRun(_Run):
    """preemptobjref._Run whose scheduler's filter pass also runs the limit plugins."""

    def __init__(self, nodes, pvs, pvcs, bound, pod, nominated, flaw, filter_order):
        nominated = nominated or {}
        everyone = list(bound) + [pod] + [q for qs in nominated.values() for q in qs]
        self.real = {q.name: q for q in everyone}
        self.guests = {q.name for qs in nominated.values() for q in qs}
        super().__init__(nodes, [_strip(q) for q in bound], _strip(pod),
                         {n: [_strip(q) for q in qs] for n, qs in nominated.items()}, None, filter_order)
        self.vflaw = flaw
        self.vpod = pod
        self.ref = VolLimitRef(nodes, pvs, pvcs, fault=flaw if flaw in ("csi_rule_intree", "intree_rule_csi") else None)
        self.reprieving = False
        self.status: Dict[str, List[Pod]] = {}         # node -> the pods the status pass saw there
        inner = self.s.filter_node

        def filter_node(p, ni, pts, ipa):
            pl, msg = inner(p, ni, pts, ipa)
            bad = self.limit_failures(ni)
            order = self.s.filter_order
            at = {name: (order.index(name) if name in order else len(order)) for name in bad}
            if bad and (pl is None or min(at.values()) < order.index(pl.rstrip("!"))):
                return min(at, key=at.get), "node(s) exceed max volume count"
            return pl, msg
        self.s.filter_node = filter_node

    # ---- the limit plugins on one NodeInfo -------------------------------------------------------
    def limit_failures(self, ni) -> Set[str]:
        flaw, name = self.vflaw, ni.node.name
        on = [self.real[pi.pod.name] for pi in ni.pods]
        if flaw == "group_volumes_ignored":
            on = [q for q in on if q.name not in self.guests]
        if flaw == "no_limits_in_reprieve" and self.reprieving:
            return set()
        was = self.status.setdefault(name, on)           # the first pass over a node is the status pass
        if flaw in ("removed_stay_attached", "shared_leaves_early", "stale_new", "other_family_moves"):
            bad = self._miscounted(on, was, name)
        else:
            self.ref.on[name] = on
            bad = self.ref.failing(self.vpod, name)
        if flaw != "absent_plugin_enforced":
            bad = {pl for pl in bad if pl in self.s.filter_order}
        return bad

    def _miscounted(self, on: List[Pod], was: List[Pod], name: str) -> Set[str]:
        """VolLimitRef.failing's rule over a count moved the wrong way; ``was``:
        the status pass's pods, of which those not in ``on`` are out."""
        vols = self.ref.volumes
        here = {v for q in on for v in vols(q)}
        before = {v for q in was for v in vols(q)}
        gone = {v for q in was if q not in on for v in vols(q)}
        mine = vols(self.vpod)
        bad = set()
        for family in sorted({v[0] for v in mine}):
            of = lambda s: {v for v in s if v[0] == family}   # noqa: E731
            have = of(here)
            new = len(of(mine) - have)
            count = len(have)
            if self.vflaw == "removed_stay_attached":
                have = of(before) | have
                count, new = len(have), len(of(mine) - have)
            elif self.vflaw == "shared_leaves_early":
                have = of(here) - gone
                count, new = len(have), len(of(mine) - have)
            elif self.vflaw == "stale_new":
                new = len(of(mine) - of(before))
            elif self.vflaw == "other_family_moves":
                count = len(of(before)) - len(before - here)
            lim = self.ref.limit(family, name)
            if lim is None:
                continue
            in_tree = owner(family) != "NodeVolumeLimits"
            if (in_tree or new > 0) and count + new > lim:
                bad.add(owner(family))
        return bad


def dry_run(nodes: List[Node], pvs, pvcs, bound: List[Pod], start: Dict[str, int], order: Dict[str, int], pod: Pod,
            priority: int, args=(10, 100), nominated: Optional[Dict[str, List[Pod]]] = None,
            flaw: Optional[str] = None, filter_order=None, pdbs: Optional[Sequence] = None) -> tuple:
    """(nominated node name or None, victim names in reprieve order, potential
    nodes, candidates kept), as preemptobjref.dry_run.  ``nominated``: {node
    name: pods nominated there}; ``flaw``: None for the reference or one of FLAWS.
    ``pdbs``: the PodDisruptionBudgets (None: no budget table, the 4-tuple);
    the 5-tuple of preemptpdbref.dry_run then, cut and pick as there."""
    assert flaw is None or flaw in FLAWS
    run = _VolRun(nodes, pvs, pvcs, bound, pod, nominated, flaw, filter_order)
    s = run.s
    potential = []
    for ni in s.nodes:
        pl, _ = s.filter_with_nominated(run.pod, ni, run.pts0, run.ipa0, run.nominated)
        if pl in POTENTIAL and not (flaw == "limit_not_potential" and pl in PLUGINS):
            potential.append(ni)
    pa = profile.PreemptionArgs(*args)
    want = min(max(len(potential) * pa.min_candidate_nodes_percentage // 100, pa.min_candidate_nodes_absolute),
               len(potential))

    def select_victims(ni):
        here = [pi.pod for pi in ni.pods]
        run.status[ni.node.name] = [run.real[q.name] for q in here + run.staying(ni)]
        lower = [q for q in here if q.priority < priority]
        lower.sort(key=lambda q: (-q.priority, start[q.name], order[q.name]))       # MoreImportantPod
        on = [q for q in here if q.priority >= priority]
        run.reprieving = False
        if not run.passes_recomputed(ni, on):
            return None
        run.reprieving = True
        return reprieve_all(lower, on, lambda pods: run.passes_recomputed(ni, pods), run.real, pdbs)

    cands, clean = [], 0
    for ni in potential if want > 0 else []:
        if len(cands) >= want and clean >= 1:              # without budgets every candidate is clean
            break
        got = select_victims(ni)
        if got is not None:
            cands.append((ni,) + got)
            clean += got[1] == 0
    tail = () if pdbs is None else (0,)
    if not cands:
        return (None, [], len(potential), 0) + tail

    def criteria(c):                                       # pickOneNodeForPreemption
        _, v, nviol = c
        top = max((q.priority for q in v), default=-(2 ** 31))     # v[0]'s without budgets: the list is sorted
        high = v[0].priority if v else -(2 ** 31)
        total = sum(q.priority + 2 ** 31 for q in v)
        early = min((start[q.name] for q in v if q.priority == top), default=2 ** 63)
        return (nviol, high, total, len(v), -early)
    best = min(range(len(cands)), key=lambda i: (criteria(cands[i]), i))
    ni, v, nviol = cands[best]
    return (ni.node.name, [q.name for q in v], len(potential), len(cands)) + (() if pdbs is None else (nviol,))


def reprieve_all(lower: List[Pod], on: List[Pod], passes, real: Dict[str, Pod], pdbs) -> Tuple[List[Pod], int]:
    """The reprieve loops over ``lower`` (MoreImportantPod order) onto ``on``:
    (victims in list order, how many of them violate a budget).
    filterPodsWithPDBViolation walks ``lower`` with a fresh copy of every
    budget; the violating pods are tried first, then the others."""
    allowed = [b.disruptions_allowed for b in pdbs or ()]
    violating = []
    for q in lower:
        hit = False
        for i in matching(real[q.name], pdbs or ()):
            allowed[i] -= 1
            hit = hit or allowed[i] < 0
        if hit:
            violating.append(q)
    victims, num_violating = [], 0
    for group in (violating, [q for q in lower if q not in violating]):
        for q in group:                                    # reprievePod
            if passes(on + [q]):
                on.append(q)
            else:
                victims.append(q)
                num_violating += group is violating
    return victims, num_violating
