"""Hand-made clusters for the full DefaultPreemption dry run (ksim_preempt_full;
csrc/ksim_preempt.hip, k_preempt_nodes<FullForm> and k_preempt_static_veto), as model
objects: tests/test_preempt_full_ref.py checks on the CPU that they tell the
reference (tests/preemptfullref.py) from its wrong readings, and
tests/test_gpu_preempt_full.py runs the engine on them.

As in tests/preemptvolcases.py nodes have 16 CPUs unless a scene says otherwise,
bound pods are added with ``bpod`` in table order, the preemptor (``pods[0]``)
has priority 1000 and every potential node is tried (args (100, 0)) unless the
scene sets ``args``.  ``expect_result`` is the hand-derived result with the
scene's nominated group, ``expect_plain`` the one without; scenes without an
``expect_result`` (the wide ones) are checked against the reference alone.
``tells``: the wrong readings (preemptfullref.FLAWS) the scene is there to tell
from the reference.  Sizes: 1 to 8 nodes, 257 (one node past the first
256-thread block) and 300.

The default filter order is NodeUnschedulable, NodeName, TaintToleration,
NodeAffinity, NodePorts, NodeResourcesFit, VolumeRestrictions, the four limit
plugins, VolumeBinding, VolumeZone, PodTopologySpread, InterPodAffinity."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from ksim.model import (ContainerPort, LabelSelector, NodeSelectorTerm, Pod, Requirement,
                        PodAffinityTerm, TopologySpreadConstraint)
from preemptvolcases import AZ_KEY, DEFAULT_ORDER, EBS_KEY, GCE_KEY, PRIO, VolScene

ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"
X, Y, DB = {"app": "x"}, {"app": "y"}, {"app": "db"}
HOG = "15950m"                                   # fills a 16-CPU node against the preemptor's 100m


def csi_key(driver: str) -> str:
    return "attachable-volumes-csi-" + driver


def anti(key: str = HOST, **labels) -> PodAffinityTerm:
    return PodAffinityTerm(key, LabelSelector(dict(labels or X)))


def hard(key: str = ZONE, skew: int = 1, labels=X) -> TopologySpreadConstraint:
    return TopologySpreadConstraint(skew, key, "DoNotSchedule", LabelSelector(dict(labels)))


@dataclass
class FullScene(VolScene):
    classes: List = field(default_factory=list)

    def znode(self, name: str, zone: Optional[str], alloc=None, cpu: str = "16") -> str:
        return self.node(name, alloc, {ZONE: zone} if zone else None, cpu)

    def bpod(self, name, on, prio, vols=(), cpu="100m", start=100, port=0, labels=None, terms=()) -> Pod:
        p = super().bpod(name, on, prio, vols, cpu, start, port)
        p.labels = dict(labels or {})
        p.pod_anti_affinity_required = list(terms)
        return p

    def preemptor(self, vols=(), cpu="100m", ports=(), labels=None, terms=(), aff=(), spread=()) -> Pod:
        p = super().preemptor(vols, cpu)
        p.containers[0].ports = [ContainerPort(q) for q in ports]
        p.labels = dict(labels or {})
        p.pod_anti_affinity_required = list(terms)
        p.pod_affinity_required = list(aff)
        p.topology_spread = list(spread)
        return p

    def nominee(self, name, on, vols=(), cpu="100m", labels=None) -> Pod:
        p = super().nominee(name, on, vols, cpu)
        p.labels = dict(labels or {})
        return p

    def pv_of(self, kind: str, vid: str):
        name = self.pvcs[[c.name for c in self.pvcs].index(self.claim(kind, vid))].volume_name
        return self.pvs[[v.name for v in self.pvs].index(name)]

    def pin(self, kind: str, vid: str, hosts: List[str]) -> None:
        """The volume's PV reaches only ``hosts`` (spec.nodeAffinity on the hostname label)."""
        self.pv_of(kind, vid).node_affinity = [NodeSelectorTerm([Requirement(HOST, "In", list(hosts))])]

    def in_zone(self, kind: str, vid: str, zone: str) -> None:
        self.pv_of(kind, vid).labels[ZONE] = zone


def without(*plugins: str) -> List[str]:
    return [p for p in DEFAULT_ORDER if p not in plugins]


# ---- 1. the StatefulSet replica ---------------------------------------------------------------------
def statefulset_replica(order=None, name="statefulset_replica") -> FullScene:
    """n0 (za) holds one EBS volume at limit 1 (b0, app=x); n1 (zb) is full of a
    priority-2000 pod without labels.  The preemptor is an app=x pod with
    hostname anti-affinity against app=x, maxSkew 1 over the zone, and a new EBS
    volume.  n0 fails EBSLimits first (1 + 1 > 1): potential; n1 fails Fit and
    has nobody to evict.  n0 with b0 out: 0 + 1 volumes, za = 0 and zb = 0
    (0 + 1 - 0 <= 1), no x pod on the host.  b0 back: the limit, the skew (1 + 1
    - 0 > 1) and the anti-affinity all fail: the victim."""
    s = FullScene(name)
    if order is not None:
        s.filter_order = list(order)
    s.znode("n0", "za", {EBS_KEY: "1"})
    s.znode("n1", "zb", {EBS_KEY: "1"})
    s.bpod("b0", "n0", 10, [("ebs", "a")], labels=X)
    s.bpod("h1", "n1", 2000, cpu=HOG)
    s.preemptor([("ebs", "x")], labels=X, terms=[anti()], spread=[hard()])
    s.expect_result = ("n0", ["b0"], 2, 1)
    s.tells = ("volumes_stale", "limit_not_potential_with_spread")
    return s


# ---- 2. one node: the only domain, anti-affinity decides ----------------------------------------------
def one_node_anti(order=None, name="one_node_anti") -> FullScene:
    """One node (za), EBS limit 2.  b0 (10, app=x) holds nothing, b1 (5) holds
    volume a.  The preemptor: hostname anti-affinity against app=x, maxSkew 1
    over the zone for app=x (za is the only domain: match + 1 - match = 1
    always passes), one new EBS volume.  Status: 1 + 1 <= 2 passes, the spread
    passes, InterPodAffinity fails for the anti-affinity: potential.  All out
    passes.  b0 back: the anti-affinity fails, the victim.  b1 back: 1 + 1 = 2
    volumes, it stays."""
    s = FullScene(name)
    if order is not None:
        s.filter_order = list(order)
    s.znode("n0", "za", {EBS_KEY: "2"})
    s.bpod("b0", "n0", 10, labels=X)
    s.bpod("b1", "n0", 5, [("ebs", "a")])
    s.preemptor([("ebs", "x")], labels=X, terms=[anti()], spread=[hard()])
    s.expect_result = ("n0", ["b0"], 1, 1)
    s.tells = ("domains_stale",)
    return s


def one_node_without_ipa() -> FullScene:
    """The scene above under a profile without InterPodAffinity: the node passes
    every filter, nothing is potential."""
    s = one_node_anti(without("InterPodAffinity"), "one_node_without_ipa")
    s.expect_result = (None, [], 0, 0)
    s.tells = ()
    return s


# ---- 3. three victims: a shared volume's last holder while the zone count moves --------------------------
def shared_volume_and_zone(order=None, name="shared_volume_and_zone") -> FullScene:
    """n0 (za), EBS limit 2: b0 (10, app=x) and b1 (8, app=x) both mount s, b2
    (5) mounts t.  n1 (zb): one app=x pod of priority 2000 and a hog, so zb = 1
    and n1 fails Fit with nobody to evict.  The preemptor: app=x, maxSkew 1
    over the zone, one new EBS volume.  n0 fails EBSLimits ({s, t} + 1 > 2):
    potential.  All out: 0 + 1; za = 0: 0 + 1 - min(0, 1) = 1.  b0 back: {s},
    1 + 1 = 2; za = 1: 1 + 1 - 1 = 1: it stays.  b1 back: s is attached
    already, 1 + 1 = 2, but za = 2: 2 + 1 - 1 > 1, a victim.  b2 back: {s, t}
    + 1 > 2, a victim; s is still held by b0 although b1 is out."""
    s = FullScene(name)
    if order is not None:
        s.filter_order = list(order)
    s.znode("n0", "za", {EBS_KEY: "2"})
    s.znode("n1", "zb", {EBS_KEY: "2"})
    s.bpod("b0", "n0", 10, [("ebs", "s")], labels=X)
    s.bpod("b1", "n0", 8, [("ebs", "s")], labels=X)
    s.bpod("b2", "n0", 5, [("ebs", "t")])
    s.bpod("h0", "n1", 2000, labels=X)
    s.bpod("h1", "n1", 2000, cpu="15850m")
    s.preemptor([("ebs", "x")], labels=X, spread=[hard()])
    s.expect_result = ("n0", ["b1", "b2"], 2, 1)
    s.tells = ("shared_leaves_early", "volumes_stale", "domains_stale")
    return s


def shared_volume_without_ebs() -> FullScene:
    """The scene above under a profile without EBSLimits: n0 fails the skew
    first (za = 2, zb = 1: 2 + 1 - 1 > 1), b1 is the only victim and b2 stays."""
    s = shared_volume_and_zone(without("EBSLimits"), "shared_volume_without_ebs")
    s.expect_result = ("n0", ["b1"], 2, 1)
    s.tells = ("absent_plugin_enforced",)
    return s


# ---- 4. the skew fails first ------------------------------------------------------------------------------
def skew_first() -> FullScene:
    """n0 (za): b0 (10) and b1 (5), both app=x, b0 holding an EBS volume at
    limit 5; n1 (zb) is full of an unlabelled priority-2000 pod.  The preemptor:
    app=x, maxSkew 1 over the zone, one new volume.  n0: 1 + 1 <= 5 passes, the
    skew fails (2 + 1 - 0 > 1): potential.  All out: 0 + 1 - 0 = 1.  Either pod
    back: 1 + 1 - 0 > 1: both victims."""
    s = FullScene("skew_first")
    s.znode("n0", "za", {EBS_KEY: "5"})
    s.znode("n1", "zb", {EBS_KEY: "5"})
    s.bpod("b0", "n0", 10, [("ebs", "a")], labels=X)
    s.bpod("b1", "n0", 5, labels=X)
    s.bpod("h1", "n1", 2000, cpu=HOG)
    s.preemptor([("ebs", "x")], labels=X, spread=[hard()])
    s.expect_result = ("n0", ["b0", "b1"], 2, 1)
    s.tells = ("skew_not_potential_with_volumes",)
    return s


# ---- 5. a PV that does not reach the best candidate -----------------------------------------------------
def pv_excludes_best(args=(100, 0), order=None, name="pv_excludes_best") -> FullScene:
    """Three 4-CPU nodes, each with one 3-CPU app=x pod (priorities 1, 5, 7);
    the 2-CPU preemptor has hostname anti-affinity against app=x and mounts an
    EBS volume whose PV reaches n1 and n2 only.  All three fail Fit: potential.
    n0 would be the best candidate (its victim has the lowest priority), but
    VolumeBinding fails there whoever is evicted; of n1 and n2, n1's victim
    ranks lower."""
    s = FullScene(name, args=args)
    if order is not None:
        s.filter_order = list(order)
    for i, prio in enumerate((1, 5, 7)):
        s.node(f"n{i}", {EBS_KEY: "2"}, cpu="4")
        s.bpod(f"b{i}", f"n{i}", prio, cpu="3", labels=X)
    s.preemptor([("ebs", "x")], cpu="2", terms=[anti()])
    s.pin("ebs", "x", ["n1", "n2"])
    s.expect_result = ("n1", ["b1"], 3, 2)
    s.tells = ("static_skipped", "vetoed_not_potential")
    return s


def pv_excludes_best_one_candidate() -> FullScene:
    """The scene above with minCandidateNodesPercentage 0 and
    minCandidateNodesAbsolute 1: the scan stops after one candidate; n0 is
    none, so n1 is found."""
    s = pv_excludes_best((0, 1), name="pv_excludes_best_one_candidate")
    s.expect_result = ("n1", ["b1"], 3, 1)
    s.tells = ("vetoed_count_toward_cut", "static_skipped")
    return s


def pv_without_volume_binding() -> FullScene:
    """... and under a profile without VolumeBinding: n0 wins."""
    s = pv_excludes_best(order=without("VolumeBinding"), name="pv_without_volume_binding")
    s.expect_result = ("n0", ["b0"], 3, 3)
    s.tells = ("absent_plugin_enforced",)
    return s


# ---- 6. a PV zone label ------------------------------------------------------------------------------------
def pv_zone_rejects(order=None, name="pv_zone_rejects") -> FullScene:
    """n0 (za) and n1 (zb), each full of one pod (priorities 1 and 5).  The
    preemptor (app=x, maxSkew 5 over the zone) mounts an EBS volume whose PV is
    labelled zone zb.  Both fail Fit: potential.  VolumeZone rejects n0."""
    s = FullScene(name)
    if order is not None:
        s.filter_order = list(order)
    s.znode("n0", "za", {EBS_KEY: "2"})
    s.znode("n1", "zb", {EBS_KEY: "2"})
    s.bpod("b0", "n0", 1, cpu=HOG)
    s.bpod("b1", "n1", 5, cpu=HOG)
    s.preemptor([("ebs", "x")], labels=X, spread=[hard(skew=5)])
    s.in_zone("ebs", "x", "zb")
    s.expect_result = ("n1", ["b1"], 2, 1)
    s.tells = ("static_skipped", "vetoed_not_potential")
    return s


def pv_zone_without_volume_zone() -> FullScene:
    s = pv_zone_rejects(without("VolumeZone"), "pv_zone_without_volume_zone")
    s.expect_result = ("n0", ["b0"], 2, 2)
    s.tells = ("absent_plugin_enforced",)
    return s


# ---- 7. nominated groups ---------------------------------------------------------------------------------
def group_holds_and_counts() -> FullScene:
    """n0 (za), EBS limit 3: b0 (10, app=x) mounts s, b1 (5) mounts t; g0,
    nominated on n0, is an app=x pod mounting s and q.  n1 (zb): an app=x pod
    of priority 2000 and a hog (zb = 1).  The preemptor: app=x, maxSkew 1 over
    the zone, one new volume.
    With the group: {s, t, q} + 1 > 3 fails EBSLimits: potential.  All out:
    {s, q} + 1 = 3; za = 1 (g0): 1 + 1 - 1 = 1.  b0 back: s is held by g0,
    still 3, but za = 2: 2 + 1 - 1 > 1: a victim.  b1 back: 4 > 3: a victim.
    Without it: {s, t} + 1 = 3 and za = 1 pass: n0 is no potential node."""
    s = FullScene("group_holds_and_counts")
    s.znode("n0", "za", {EBS_KEY: "3"})
    s.znode("n1", "zb", {EBS_KEY: "3"})
    s.bpod("b0", "n0", 10, [("ebs", "s")], labels=X)
    s.bpod("b1", "n0", 5, [("ebs", "t")])
    s.bpod("h0", "n1", 2000, labels=X)
    s.bpod("h1", "n1", 2000, cpu="15850m")
    s.preemptor([("ebs", "x")], labels=X, spread=[hard()])
    s.nominee("g0", "n0", [("ebs", "s"), ("ebs", "q")], labels=X)
    s.expect_result = ("n0", ["b0", "b1"], 2, 1)
    s.expect_plain = (None, [], 1, 0)
    s.tells = ("group_volumes_ignored", "group_adds_ignored")
    return s


def group_holds_and_repels() -> FullScene:
    """One node, EBS limit 1; b0 (5) mounts t.  The preemptor mounts s and has
    hostname anti-affinity against app=y; g0, nominated on the node, is an
    app=y pod that mounts s.  Without the group: {t} + 1 > 1, potential; b0 out
    frees the slot, b0 back fills it: the victim.  With it: {t, s} + 0 > 1
    (in-tree rule), potential; with b0 out {s} + 0 = 1 passes the limit but g0
    stays and matches the anti-affinity: no candidate."""
    s = FullScene("group_holds_and_repels")
    s.node("n0", {EBS_KEY: "1"})
    s.bpod("b0", "n0", 5, [("ebs", "t")])
    s.preemptor([("ebs", "s")], terms=[anti(**Y)])
    s.nominee("g0", "n0", [("ebs", "s")], labels=Y)
    s.expect_result = (None, [], 1, 0)
    s.expect_plain = ("n0", ["b0"], 1, 1)
    s.tells = ("group_adds_ignored",)
    return s


# ---- 8. every use slot -------------------------------------------------------------------------------------
PORTS = tuple(range(8000, 8007))


def every_slot(order=None, name="every_slot") -> FullScene:
    """A preemptor with KSIM_MAX_USES uses: seven host ports, two volume
    families (a shared EBS volume, a new EBS volume, a shared and a new GCE
    disk), hostname anti-affinity, required zone affinity to app=db and two
    DoNotSchedule constraints (hostname and zone).  Four nodes in two zones;
    checked against the reference."""
    s = FullScene(name)
    if order is not None:
        s.filter_order = list(order)
    lim = {EBS_KEY: "2", GCE_KEY: "2"}
    for i, z in enumerate(("za", "za", "zb", "zb")):
        s.znode(f"n{i}", z, lim)
    s.bpod("db0", "n0", 2000, labels=DB)
    s.bpod("b0", "n0", 10, [("ebs", "s")], labels=X, port=8000)
    s.bpod("b1", "n0", 8, [("gce", "g")], port=8003)
    s.bpod("b2", "n0", 5, [("ebs", "s"), ("ebs", "t")], labels=X)
    s.bpod("b3", "n0", 3, [("gce", "g")])
    s.bpod("db1", "n1", 2000, labels=DB, cpu=HOG)
    s.bpod("c0", "n2", 20, [("ebs", "u"), ("ebs", "v")], port=8006)
    s.bpod("c1", "n2", 4, [("gce", "g")], labels=X)
    s.bpod("d0", "n3", 2000, cpu=HOG)
    s.preemptor([("ebs", "s"), ("ebs", "x"), ("gce", "g"), ("gce", "y")], ports=PORTS, labels=X,
                terms=[anti()], aff=[anti(ZONE, **DB)], spread=[hard(HOST, 1), hard(ZONE, 2)])
    return s


def every_slot_without_ports() -> FullScene:
    return every_slot(without("NodePorts"), "every_slot_without_ports")


# ---- 9. eight volume families ------------------------------------------------------------------------------
FAMILIES = ("ebs", "gce", "azure", "csi:a", "csi:b", "csi:c", "csi:d", "csi:e")


def eight_families() -> FullScene:
    """Two nodes at limit 1 in each of eight families (three in-tree, five CSI
    drivers); on n0 eight victims hold one volume each, b3 and b6 app=x as
    well; n1 is full.  The preemptor brings one new volume per family and has
    hostname anti-affinity against app=x: every holder is a victim."""
    s = FullScene("eight_families")
    lim = {EBS_KEY: "1", GCE_KEY: "1", AZ_KEY: "1"}
    lim.update({csi_key(f[4:]): "1" for f in FAMILIES if f.startswith("csi:")})
    s.node("n0", lim)
    s.node("n1", lim)
    for k, fam in enumerate(FAMILIES):
        s.bpod(f"b{k}", "n0", 20 - k, [(fam, f"v{k}")], labels=X if k in (3, 6) else None)
    s.bpod("free", "n0", 1)
    s.bpod("h1", "n1", 2000, cpu=HOG)
    s.preemptor([(fam, f"x{k}") for k, fam in enumerate(FAMILIES)], terms=[anti()])
    s.expect_result = ("n0", [f"b{k}" for k in range(8)], 2, 1)
    return s


# ---- 10. one node past the first block, and 300 -----------------------------------------------------------
def block_edge(n: int = 257) -> FullScene:
    """n nodes at EBS limit 1, each with one app=x victim mounting its own
    volume; the preemptor has hostname anti-affinity against app=x and one new
    volume.  The victim of the last node has the lowest priority."""
    s = FullScene(f"block_edge_{n}")
    for i in range(n):
        s.node(f"n{i:04d}", {EBS_KEY: "1"})
        s.bpod(f"b{i}", f"n{i:04d}", 3 if i == n - 1 else 10 + i % 7, [("ebs", f"v{i}")], labels=X)
    s.preemptor([("ebs", "x")], terms=[anti()])
    s.expect_result = (f"n{n - 1:04d}", [f"b{n - 1}"], n, n)
    return s


def three_hundred_zoned() -> FullScene:
    """300 nodes in three zones at EBS limit 1.  On each, a (10, app=x) and c
    (5, app=x) share one volume and d (3) holds nothing; the last node lacks c.
    The preemptor: app=x, hostname anti-affinity against app=x, maxSkew 400
    over the zone (it moves and never fails), one new volume.  a and c are
    victims everywhere, d stays; the last node has one victim fewer."""
    n = 300
    s = FullScene("three_hundred_zoned")
    for i in range(n):
        s.znode(f"n{i:04d}", "z%d" % (i % 3), {EBS_KEY: "1"})
        s.bpod(f"a{i}", f"n{i:04d}", 10, [("ebs", f"v{i}")], labels=X)
        if i != n - 1:
            s.bpod(f"c{i}", f"n{i:04d}", 5, [("ebs", f"v{i}")], labels=X)
        s.bpod(f"d{i}", f"n{i:04d}", 3)
    s.preemptor([("ebs", "x")], labels=X, terms=[anti()], spread=[hard(skew=400)])
    s.expect_result = (f"n{n - 1:04d}", [f"a{n - 1}"], n, n)
    return s


_ALL = (statefulset_replica, one_node_anti, one_node_without_ipa, shared_volume_and_zone, shared_volume_without_ebs,
        skew_first, pv_excludes_best, pv_excludes_best_one_candidate, pv_without_volume_binding, pv_zone_rejects,
        pv_zone_without_volume_zone, group_holds_and_counts, group_holds_and_repels, every_slot,
        every_slot_without_ports, eight_families, block_edge, three_hundred_zoned)
WIDE = ("block_edge_257", "three_hundred_zoned")        # too wide to run every wrong reading on


# ---- a budget between the rows (not in scenes(): it carries PodDisruptionBudgets) ----------------
def mixed_budget() -> FullScene:
    """tests/preemptvolcases.py mixed_budget for a preemptor that also carries
    hostname anti-affinity against app=q, which no pod matches: the full form
    on the same volumes.  n0, EBS limit 3: b1 (40) and b3 (20) mount a, b2 (30)
    and b4 (10) mount b; the preemptor brings two new volumes.  One budget,
    disruptionsAllowed 1, over b1, b2, b3: b2 and b3 violate.  b2 back, {b}: it
    stays; b3 back, {a, b}: 4 > 3, a violating victim; b1: a attaches again, a
    victim; b4: b is attached (b2), it stays after b3 stayed out.  Without
    budgets: b2 and b4."""
    from ksim.model import PodDisruptionBudget
    s = FullScene("mixed_budget")
    s.znode("n0", "za", {EBS_KEY: "3"})
    for name, prio, vol in (("b1", 40, "a"), ("b2", 30, "b"), ("b3", 20, "a"), ("b4", 10, "b")):
        s.bpod(name, "n0", prio, [("ebs", vol)], labels={"tier": "db"} if name != "b4" else None)
    s.preemptor([("ebs", "x"), ("ebs", "y")], terms=[anti(app="q")])
    s.budgets = [PodDisruptionBudget("db", selector=LabelSelector({"tier": "db"}), disruptions_allowed=1)]
    s.expect_result = ("n0", ["b2", "b4"], 1, 1)
    s.expect_budgets = ("n0", ["b3", "b1"], 1, 1, 1)
    return s


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, FullScene]:
    out = {}
    for make in _ALL:
        s = make()
        out[s.name] = s
    return out


def scene_ids() -> List[str]:
    return list(scenes())


# ---- the scenes compiled for the engine ----------------------------------------------------------------
@dataclass
class Built:
    sc: object
    cluster: object
    enc: object
    table: object
    sp: object
    prof: object
    groups: Optional[List[Tuple[int, List[int]]]]
    nodes: list                                   # the scene's nodes in the cluster's order


def sched_profile(order, args=(100, 0)):
    from ksim import profile
    plugins = profile.convert_for_simulator({"filter": profile.PluginSet([profile.Plugin(n) for n in order],
                                                                         [profile.Plugin("*")])})
    return profile.SchedulerProfile(plugins=plugins, percentage_of_nodes_to_score=100,
                                    preemption=profile.PreemptionArgs(*args))


def build(sc, extra_pods=(), adds: bool = True, holdings: bool = True) -> Built:
    """The scene compiled: the limits compile over the bound pods and every
    pending pod, the pods' uses and volume groups, and the bound-pod table with
    every class of its rows (``adds``) and their volume holdings (``holdings``)."""
    from ksim import profile
    from ksim.encode import encode_cluster, encode_pods
    from ksim.preemption import bound_table
    from ksim.volumes import VolumeIndex
    pending = list(sc.pending) + list(extra_pods)
    index = VolumeIndex.from_nodes(sc.nodes, sc.pvs, sc.pvcs)
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    cluster.set_volume_limits(index.volume_limits(sc.nodes, sc.bound, pending))
    enc = encode_pods(cluster, pending, volumes=index)
    table = bound_table(cluster, sc.bound, sc.start, cluster.topo, full_adds=True, vol_limits=cluster.vol_limits)
    if not adds:                                  # Engine.set_bound_pods then sets no class adds
        table.adds_off = table.adds = None
    if not holdings:                              # ... and no holdings
        table.vol_off = table.vol_uses = None
    sp = sched_profile(sc.filter_order, sc.args)
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    groups = [(pos[n], list(idx)) for n, idx in sc.nominated.items()] or None
    by_name = {n.name: n for n in sc.nodes}
    return Built(sc, cluster, enc, table, sp, profile.compile_profile(sp), groups,
                 [by_name[n] for n in cluster.node_names])
