"""DefaultPreemption's dry run at the object level for every preemptor the
per-pod cycle accepts (ksim_preempt_full): counted volumes beside host ports,
required pod (anti-)affinity and DoNotSchedule spread, and claims whose PVs
VolumeBinding or VolumeZone reject on some nodes.  The reference of
tests/test_gpu_preempt_full.py, pinned by tests/test_preempt_full_ref.py to
tests/preemptvolref.py, tests/preemptspreadref.py and tests/preemptobjref.py on
their own scenes.  No code is shared with ksim or the engine.

It is tests/preemptobjref.py's recomputing dry run: every trial state of a node
rebuilds the node's NodeInfo from the pods that stay plus its nominated pods
and runs ``pts_prefilter``, ``ipa_prefilter`` and ``filter_node`` from scratch.
Two things differ from the older references:

* the ObjScheduler *knows* the scene's PVs, PVCs and StorageClasses and the
  pods keep their claims, so ``filter_node`` runs VolumeBinding and VolumeZone
  itself, in every pass, as upstream's SelectVictimsOnNode does;
* every pass also asks tests/vollimitref.py ``VolLimitRef.failing`` over the
  pods on the NodeInfo and places a failing limit plugin at its position in
  the filter list, the way tests/preemptvolref.py composes it.

Potential nodes: the first failing filter is NodeResourcesFit, NodePorts, a
limit plugin, InterPodAffinity with one of its two anti-affinity messages, or
PodTopologySpread with the skew message.

With ``pdbs`` (budgets) the lower-priority pods are split and reprieved as
tests/preemptvolref.py ``reprieve_all`` has it (filterPodsWithPDBViolation, the
violating pods first) and the result carries the nominated node's violations
as a fifth element.

``flaw`` switches on one wrong reading (FLAWS) for the test that the scenes of
tests/preemptfullcases.py tell each from the reference.  EQUAL lists readings
that cannot differ: ``static_skipped_in_reprieve`` skips VolumeBinding and
VolumeZone while pods are put back only; both verdicts depend on the node and
the preemptor alone, so a node that fails one fails already with every victim
out and is no candidate either way."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Set, Tuple

import preemptobjref
from ksim import profile
from ksim.model import Container, Node, Pod
from oracle.objref import IPA_ANTI, IPA_EXIST, PTS_SKEW, NodeInfo, ObjScheduler
from preemptvolref import reprieve_all
from vollimitref import PLUGINS, VolLimitRef, owner

FLAWS = ("volumes_stale",                  # volume counts do not move in a trial that moves domain counts
         "domains_stale",                  # domain counts do not move in a trial that moves volume counts
         "shared_leaves_early",            # a shared volume leaves with its first holder
         "limit_not_potential_with_spread",   # a node failing a limit plugin is no potential node (pod with spread)
         "skew_not_potential_with_volumes",   # a node failing the spread skew is none (pod with volumes)
         "static_skipped",                 # VolumeBinding / VolumeZone are not re-run in the dry run
         "vetoed_count_toward_cut",        # nodes the static check vetoes count toward numCandidates
         "vetoed_not_potential",           # ... or are not counted among the potential nodes
         "group_volumes_ignored",          # the nominated group's volumes are ignored, its class adds counted
         "group_adds_ignored",             # the reverse
         "absent_plugin_enforced")         # a limit plugin, VolumeBinding or VolumeZone the profile lacks still fails
EQUAL = ("static_skipped_in_reprieve",)
STATIC = ("VolumeBinding", "VolumeZone")


def _bare(q: Pod) -> Pod:
    """``q`` as a pod that counts into no selector class, holds no port and carries no term."""
    return dataclasses.replace(q, labels={}, pod_affinity_required=[], pod_anti_affinity_required=[],
                               containers=[Container(dict(c.requests)) for c in q.containers])


class _Run(preemptobjref._Run):
    def __init__(self, nodes, pvs, pvcs, classes, bound, pod, nominated, flaw, filter_order):
        super().__init__(nodes, bound, pod, nominated, flaw, filter_order)
        self.s = ObjScheduler(nodes, self.bound, pct=100, seed=0, pvs=pvs, pvcs=pvcs, storage_classes=classes)
        if filter_order is not None:
            self.s.filter_order = list(filter_order)
        self.pts0, self.ipa0 = self.s.pts_prefilter(pod), self.s.ipa_prefilter(pod)
        everyone = self.bound + [pod] + [q for qs in self.nominated.values() for q in qs]
        self.real = {q.name: q for q in everyone}
        self.guests = {q.name for qs in self.nominated.values() for q in qs}
        self.ref = VolLimitRef(nodes, pvs, pvcs)
        self.dry = self.reprieving = self.no_static = False
        self.status: Dict[str, List[Pod]] = {}             # node -> the pods the status pass saw there
        self.state0: Dict[str, tuple] = {}                 # node -> the status pass's (pts, ipa)
        inner = self.s.filter_node

        def filter_node(p, ni, pts, ipa):
            s, order = self.s, self.s.filter_order
            skip = self.no_static or (self.dry and flaw == "static_skipped") or \
                (self.reprieving and flaw == "static_skipped_in_reprieve")
            if skip:
                s.filter_order = [x for x in order if x not in STATIC]
            try:
                pl, msg = inner(p, ni, pts, ipa)
            finally:
                s.filter_order = order
            bad = self.limit_failures(ni)
            at = {name: (order.index(name) if name in order else len(order)) for name in bad}
            if bad and (pl is None or min(at.values()) < order.index(pl.rstrip("!"))):
                return min(at, key=at.get), "node(s) exceed max volume count"
            if pl is None and flaw == "absent_plugin_enforced" and p.pvc_claims:
                if "VolumeBinding" not in order and not s.volume_binding_ok(p, ni.node):
                    return "VolumeBinding", "node(s) had volume node affinity conflict"
                if "VolumeZone" not in order and not s.volume_zone_ok(p, ni.node):
                    return "VolumeZone", "node(s) had no available volume zone"
            return pl, msg
        self.s.filter_node = filter_node

    # ---- the limit plugins on one NodeInfo -------------------------------------------------------
    def limit_failures(self, ni) -> Set[str]:
        flaw, name = self.flaw, ni.node.name
        on = [self.real[pi.pod.name] for pi in ni.pods]
        if flaw == "group_volumes_ignored":
            on = [q for q in on if q.name not in self.guests]
        was = self.status.setdefault(name, on)             # the first pass over a node is the status pass
        if flaw == "volumes_stale":
            on = was
        if flaw == "shared_leaves_early":
            bad = self._leaves_early(on, was, name)
        else:
            self.ref.on[name] = on
            bad = self.ref.failing(self.pod, name)
        if flaw != "absent_plugin_enforced":
            bad = {pl for pl in bad if pl in self.s.filter_order}
        return bad

    def _leaves_early(self, on: List[Pod], was: List[Pod], name: str) -> Set[str]:
        """VolLimitRef.failing's rule with every volume of a pod that is out taken as detached."""
        vols = self.ref.volumes
        here = {v for q in on for v in vols(q)}
        gone = {v for q in was if q not in on for v in vols(q)}
        mine = vols(self.pod)
        bad = set()
        for family in sorted({v[0] for v in mine}):
            have = {v for v in here - gone if v[0] == family}
            new = len({v for v in mine if v[0] == family} - have)
            lim = self.ref.limit(family, name)
            if lim is None:
                continue
            if (owner(family) != "NodeVolumeLimits" or new > 0) and len(have) + new > lim:
                bad.add(owner(family))
        return bad

    # ---- one trial state ----------------------------------------------------------------------------
    def _with(self, ni: NodeInfo, pods_on: List[Pod], fn):
        staying = self.staying(ni)
        if self.flaw == "group_adds_ignored":
            staying = [_bare(q) for q in staying]
        fresh = NodeInfo(ni.node)
        for q in pods_on + staying:
            fresh.add_pod(q)
        s, at = self.s, self.s.nodes.index(ni)
        s.nodes[at] = s.by_name[ni.node.name] = fresh
        try:
            return fn(fresh)
        finally:
            s.nodes[at] = s.by_name[ni.node.name] = ni

    def begin(self, ni: NodeInfo, here: List[Pod]) -> None:
        """What the status pass saw on the node (pass 1: the group on it)."""
        self.status[ni.node.name] = [self.real[q.name] for q in here + self.staying(ni)]
        self.state0[ni.node.name] = self._with(ni, here, lambda _: (self.s.pts_prefilter(self.pod),
                                                                    self.s.ipa_prefilter(self.pod)))

    def passes(self, ni: NodeInfo, pods_on: List[Pod]) -> bool:
        def trial(fresh):
            s = self.s
            pts, ipa = self.state0[ni.node.name] if self.flaw == "domains_stale" else \
                (s.pts_prefilter(self.pod), s.ipa_prefilter(self.pod))
            return s.filter_node(self.pod, fresh, pts, ipa)[0] is None
        return self._with(ni, pods_on, trial)

    def static_ok(self, ni: NodeInfo) -> bool:
        s, p, order = self.s, self.pod, self.s.filter_order
        if not p.pvc_claims:
            return True
        if "VolumeBinding" in order and not (s.volume_binding_ok(p, ni.node) and
                                              s.find_pod_volumes(p, ni.node) is not None):
            return False
        return "VolumeZone" not in order or s.volume_zone_ok(p, ni.node)


def dry_run(nodes: List[Node], pvs, pvcs, bound: List[Pod], start: Dict[str, int], order: Dict[str, int], pod: Pod,
            priority: int, args=(10, 100), nominated: Optional[Dict[str, List[Pod]]] = None,
            flaw: Optional[str] = None, filter_order=None, classes=(), pdbs: Optional[Sequence] = None) -> tuple:
    """(nominated node name or None, victim names in reprieve order, potential
    nodes, candidates kept), as preemptobjref.dry_run.  ``nominated``: {node
    name: pods nominated there}; ``flaw``: None for the reference, one of FLAWS
    or one of EQUAL.  ``pdbs``: the PodDisruptionBudgets (None: no budget table,
    the 4-tuple); the 5-tuple of preemptpdbref.dry_run then, cut and pick as there."""
    assert flaw is None or flaw in FLAWS or flaw in EQUAL
    run = _Run(nodes, pvs, pvcs, classes, bound, pod, nominated, flaw, filter_order)
    s = run.s
    spread = any(c.when_unsatisfiable == "DoNotSchedule" for c in pod.topology_spread)
    counted = bool(run.ref.volumes(pod))
    potential = []
    for ni in s.nodes:
        pl, msg = s.filter_with_nominated(pod, ni, run.pts0, run.ipa0, run.nominated)
        ok = pl in ("NodeResourcesFit", "NodePorts") or \
            (pl in PLUGINS and not (flaw == "limit_not_potential_with_spread" and spread)) or \
            (pl == "InterPodAffinity" and msg in (IPA_ANTI, IPA_EXIST)) or \
            (pl == "PodTopologySpread" and msg == PTS_SKEW and
             not (flaw == "skew_not_potential_with_volumes" and counted))
        if ok and flaw == "vetoed_not_potential" and not run.static_ok(ni):
            ok = False
        if ok:
            potential.append(ni)
    pa = profile.PreemptionArgs(*args)
    want = min(max(len(potential) * pa.min_candidate_nodes_percentage // 100, pa.min_candidate_nodes_absolute),
               len(potential))

    def select_victims(ni, no_static=False):
        here = [pi.pod for pi in ni.pods]
        run.begin(ni, here)
        lower = [q for q in here if q.priority < priority]
        lower.sort(key=lambda q: (-q.priority, start[q.name], order[q.name]))       # MoreImportantPod
        on = [q for q in here if q.priority >= priority]
        run.dry, run.reprieving, run.no_static = True, False, no_static
        try:
            if not run.passes(ni, on):
                return None
            run.reprieving = True
            return reprieve_all(lower, on, lambda pods: run.passes(ni, pods), run.real, pdbs)
        finally:
            run.dry = run.reprieving = run.no_static = False

    cands, found, clean = [], 0, 0
    for ni in potential if want > 0 else []:
        if found >= want and clean >= 1:                   # without budgets every candidate is clean
            break
        got = select_victims(ni)
        if got is not None:
            cands.append((ni,) + got)
            found += 1
            clean += got[1] == 0
        elif flaw == "vetoed_count_toward_cut" and select_victims(ni, no_static=True) is not None:
            found += 1
            clean += 1
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


as_indices = preemptobjref.as_indices
