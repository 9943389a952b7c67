"""Hand-made clusters for DefaultPreemption's dry run of a preemptor with
counted volumes (csrc/ksim_preempt.hip, the volume form), as model objects:
tests/test_preempt_vol_ref.py checks on the CPU that they tell the reference
(tests/preemptvolref.py) from its faulty readings, and
tests/test_gpu_preempt_volumes.py runs the engine on them.

Nodes have 16 CPUs unless a scene says otherwise, bound pods are added with
``bpod`` in table order, the preemptor (``pods[0]``) has priority 1000 and every
potential node is tried (args (100, 0)).  ``expect`` is the hand-derived result
with the scene's nominated group, ``expect_plain`` the one without;
``tells``: the faulty readings (preemptvolref.FLAWS) the scene is there to tell
from the reference.  Sizes: 1 to 8 nodes, plus 257 (one node past the first
256-thread block of k_preempt_nodes<VolumeForm>) and 300."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from ksim import profile
from ksim.model import Container, ContainerPort, Pod
from vollimitcases import AZ_KEY, EBS_KEY, GCE_KEY, Scene
from vollimitref import PLUGINS

PRIO = 1000
CSI_X = "attachable-volumes-csi-x"
DEFAULT_ORDER = profile.SchedulerProfile().filter_order()
LIMITS_FIRST = list(PLUGINS) + [p for p in DEFAULT_ORDER if p not in PLUGINS]


@dataclass
class VolScene(Scene):
    start: Dict[str, int] = field(default_factory=dict)
    order: Dict[str, int] = field(default_factory=dict)      # bound pod name -> table row
    nominated: Dict[str, List[int]] = field(default_factory=dict)   # node -> indices into ``pending``
    args: Tuple[int, int] = (100, 0)
    filter_order: List[str] = field(default_factory=lambda: list(DEFAULT_ORDER))
    expect_result: Optional[tuple] = None
    expect_plain: Optional[tuple] = None
    tells: Tuple[str, ...] = ()
    budgets: List = field(default_factory=list)              # PodDisruptionBudgets (mixed_budget only)
    expect_budgets: Optional[tuple] = None                   # the hand-derived 5-tuple under them

    def bpod(self, name: str, on: str, prio: int, vols=(), cpu: str = "100m", start: int = 100, port: int = 0) -> Pod:
        p = self.pod(name, vols, on=on, cpu=cpu)
        p.priority = prio
        if port:
            p.containers[0].ports = [ContainerPort(port)]
        self.start[name] = start
        self.order[name] = len(self.order)
        return p

    def preemptor(self, vols=(), cpu: str = "100m", port: int = 0) -> Pod:
        p = self.pod("preemptor", vols, cpu=cpu)
        p.priority = PRIO
        if port:
            p.containers[0].ports = [ContainerPort(port)]
        return p

    def nominee(self, name: str, on: str, vols=(), cpu: str = "100m") -> Pod:
        p = self.pod(name, vols, cpu=cpu)
        p.priority = PRIO + 500
        self.nominated.setdefault(on, []).append(len(self.pending) - 1)
        return p

    @property
    def pods(self) -> List[Pod]:
        return self.pending

    def nominated_pods(self) -> Dict[str, List[Pod]]:
        return {n: [self.pending[i] for i in idx] for n, idx in self.nominated.items()}


# ---- 1. the textbook case ---------------------------------------------------------------------
def ebs_slot() -> VolScene:
    """n0 holds 2 EBS volumes at limit 2: the preemptor's third fails EBSLimits
    (potential).  Both out: 0 + 1.  b0 back: 1 + 1 = 2 fits the limit, stays;
    b1 back: 2 + 1 > 2, the victim.  n1 (limit 0, empty) fails too and has
    nothing to evict."""
    s = VolScene("ebs_slot")
    s.node("n0", {EBS_KEY: "2"})
    s.node("n1", {EBS_KEY: "0"})
    s.bpod("b0", "n0", 10, [("ebs", "a")])
    s.bpod("b1", "n0", 5, [("ebs", "b")])
    s.preemptor([("ebs", "x")])
    s.expect_result = ("n0", ["b1"], 2, 1)
    s.tells = ("removed_stay_attached", "limit_not_potential", "no_limits_in_reprieve")
    return s


# ---- 2. two victims share a volume ------------------------------------------------------------------
def two_victims_share() -> VolScene:
    """Limit 2, attached {s, t}: b0 (10) and b1 (5) both mount s, b2 (8) mounts
    t.  All out: 0 + 1.  b0 back: {s}, 1 + 1 = 2 stays.  b2 back: {s, t}, 3 > 2,
    a victim.  b1 back: s is attached already (b0), 1 + 1 = 2: it stays."""
    s = VolScene("two_victims_share")
    s.node("n0", {EBS_KEY: "2"})
    s.bpod("b0", "n0", 10, [("ebs", "s")])
    s.bpod("b1", "n0", 5, [("ebs", "s")])
    s.bpod("b2", "n0", 8, [("ebs", "t")])
    s.preemptor([("ebs", "x")])
    s.expect_result = ("n0", ["b2"], 1, 1)
    s.tells = ("shared_leaves_early", "removed_stay_attached")
    return s


# ---- 3. a volume shared by a victim and a higher-priority pod ------------------------------------
def shared_with_higher() -> VolScene:
    """Limit 1; h0 (2000) and b0 (5) mount s.  With b0 out the volume is still
    attached (h0): 1 + 1 > 1, no candidate."""
    s = VolScene("shared_with_higher")
    s.node("n0", {EBS_KEY: "1"})
    s.bpod("h0", "n0", 2000, [("ebs", "s")])
    s.bpod("b0", "n0", 5, [("ebs", "s")])
    s.preemptor([("ebs", "x")])
    s.expect_result = (None, [], 1, 0)
    s.tells = ("shared_leaves_early",)
    return s


# ---- 4. the preemptor mounts a victim's volume -------------------------------------------------------
def preemptor_mounts_victims_volume() -> VolScene:
    """4 CPUs, limit 1.  b0 (3 CPUs) mounts s; the preemptor (2 CPUs) mounts s
    and x.  Fit fails first (potential).  With b0 out nobody holds s: attached
    0, new 2 > 1: no candidate.  The status pass's new (1: s was attached) would
    let it in."""
    s = VolScene("preemptor_mounts_victims_volume")
    s.node("n0", {EBS_KEY: "1"}, cpu="4")
    s.bpod("b0", "n0", 5, [("ebs", "s")], cpu="3")
    s.preemptor([("ebs", "s"), ("ebs", "x")], cpu="2")
    s.expect_result = (None, [], 1, 0)
    s.tells = ("stale_new",)
    return s


def last_holder_leaves() -> VolScene:
    """Limit 1, attached {s, t} (over the limit): the preemptor mounts s, new 0,
    and the in-tree rule still fails it.  All out: 0 + 1.  b0 (mounts s) back:
    1 + 0 stays.  b1 (t) back: 2 + 0 > 1, the victim."""
    s = VolScene("last_holder_leaves")
    s.node("n0", {EBS_KEY: "1"})
    s.bpod("b0", "n0", 10, [("ebs", "s")])
    s.bpod("b1", "n0", 5, [("ebs", "t")])
    s.preemptor([("ebs", "s")])
    s.expect_result = ("n0", ["b1"], 1, 1)
    s.tells = ("csi_rule_intree",)
    return s


# ---- 5. CSI over its limit with nothing new --------------------------------------------------------
def csi_over_limit_nothing_new() -> VolScene:
    """n0: driver x limit 1, attached {h0, h1}; the preemptor mounts h0: new 0,
    NodeVolumeLimits passes, n0 is no potential node.  n1 (limit 0, empty) fails
    for the new volume and has nothing to evict."""
    s = VolScene("csi_over_limit_nothing_new")
    s.node("n0", {CSI_X: "1"})
    s.node("n1", {CSI_X: "0"})
    s.bpod("b0", "n0", 10, [("csi:x", "h0")])
    s.bpod("b1", "n0", 5, [("csi:x", "h1")])
    s.preemptor([("csi:x", "h0")])
    s.expect_result = (None, [], 1, 0)
    s.tells = ("intree_rule_csi",)
    return s


# ---- 6. a CSI node without the key -------------------------------------------------------------------
def csi_node_without_key() -> VolScene:
    """n0 publishes no key for driver x (no limit) and is short of CPU; n1 has
    limit 1 and one volume.  Both are candidates with one victim of priority 5;
    n0's started later (100 against 90), so n0 wins."""
    s = VolScene("csi_node_without_key")
    s.node("n0", cpu="4")
    s.node("n1", {CSI_X: "1"})
    s.bpod("b0", "n0", 5, [("csi:x", "h0")], cpu="3", start=100)
    s.bpod("b1", "n1", 5, [("csi:x", "h1")], start=90)
    s.preemptor([("csi:x", "h9")], cpu="2")
    s.expect_result = ("n0", ["b0"], 2, 2)
    return s


# ---- 7. two families, and a victim holding a third ------------------------------------------------------
def two_families_and_a_third() -> VolScene:
    """EBS and GCE limit 1, one volume each (b1, b2); b0 holds an Azure disk
    only.  The preemptor brings one EBS and one GCE volume.  b0 back changes
    neither family: it stays; b1 and b2 each fill their family: victims."""
    s = VolScene("two_families_and_a_third")
    s.node("n0", {EBS_KEY: "1", GCE_KEY: "1", AZ_KEY: "1"})
    s.bpod("b0", "n0", 10, [("azure", "z")])
    s.bpod("b1", "n0", 8, [("ebs", "a")])
    s.bpod("b2", "n0", 5, [("gce", "g")])
    s.preemptor([("ebs", "x"), ("gce", "y")])
    s.expect_result = ("n0", ["b1", "b2"], 1, 1)
    s.tells = ("other_family_moves",)
    return s


# ---- 8. Fit fails first, the limit decides the reprieve ----------------------------------------------
def fit_first_limit_decides(limits_first: bool = False) -> VolScene:
    """4 CPUs, EBS limit 1.  b0 (0.1 CPU) mounts a, b1 takes 3 CPUs; the
    preemptor needs 2 CPUs and one EBS volume.  Fit is the first failing filter
    (EBSLimits with ``limits_first``); b0 back fits but fills the limit: a
    victim; b1 back does not fit: a victim."""
    s = VolScene("limits_before_fit" if limits_first else "fit_first_limit_decides")
    if limits_first:
        s.filter_order = list(LIMITS_FIRST)
    s.node("n0", {EBS_KEY: "1"}, cpu="4")
    s.bpod("b0", "n0", 10, [("ebs", "a")])
    s.bpod("b1", "n0", 5, cpu="3")
    s.preemptor([("ebs", "x")], cpu="2")
    s.expect_result = ("n0", ["b0", "b1"], 1, 1)
    s.tells = ("limit_not_potential",) if limits_first else ("no_limits_in_reprieve",)
    return s


# ---- 9. a profile without EBSLimits -------------------------------------------------------------------
def profile_without_ebs() -> VolScene:
    """The scene above under a profile that leaves EBSLimits out: b0 stays."""
    s = fit_first_limit_decides()
    s.name = "profile_without_ebs"
    s.filter_order = [p for p in DEFAULT_ORDER if p != "EBSLimits"]
    s.expect_result = ("n0", ["b1"], 1, 1)
    s.tells = ("absent_plugin_enforced",)
    return s


# ---- 10. a nominated group holding volumes -----------------------------------------------------------
def group_holds_volumes() -> VolScene:
    """Limit 3.  b0 (10) mounts s, b1 (5) mounts t; the pod nominated on n0
    mounts s as well and one volume of its own.  With it: {s, t, q} + 1 > 3
    fails pass 1.  All out: {q, s} + 1 = 3.  b0 back: s is held by the nominated
    pod, still 3: it stays.  b1 back: 4 > 3, the victim.  Without the group the
    node passes and nothing is potential."""
    s = VolScene("group_holds_volumes")
    s.node("n0", {EBS_KEY: "3"})
    s.bpod("b0", "n0", 10, [("ebs", "s")])
    s.bpod("b1", "n0", 5, [("ebs", "t")])
    s.preemptor([("ebs", "x")])
    s.nominee("g0", "n0", [("ebs", "s"), ("ebs", "q")])
    s.expect_result = ("n0", ["b1"], 1, 1)
    s.expect_plain = (None, [], 0, 0)
    s.tells = ("group_volumes_ignored",)
    return s


def group_shares_with_victim() -> VolScene:
    """Limit 1.  b0 (5) and the nominated pod both mount s.  With the group:
    {s} + 1 > 1 and with b0 out s is still attached: no candidate.  Without it:
    b0 out frees the slot, b0 is the victim."""
    s = VolScene("group_shares_with_victim")
    s.node("n0", {EBS_KEY: "1"})
    s.bpod("b0", "n0", 5, [("ebs", "s")])
    s.preemptor([("ebs", "x")])
    s.nominee("g0", "n0", [("ebs", "s")])
    s.expect_result = (None, [], 1, 0)
    s.expect_plain = ("n0", ["b0"], 1, 1)
    s.tells = ("group_volumes_ignored", "shared_leaves_early")
    return s


# ---- 11. a host port and a volume -------------------------------------------------------------------
def port_and_volume() -> VolScene:
    """The preemptor wants host port 8080 and one EBS volume; b0 holds the port,
    b1 the node's only EBS slot.  NodePorts fails first; both are victims."""
    s = VolScene("port_and_volume")
    s.node("n0", {EBS_KEY: "1"})
    s.bpod("b0", "n0", 10, port=8080)
    s.bpod("b1", "n0", 5, [("ebs", "a")])
    s.preemptor([("ebs", "x")], port=8080)
    s.expect_result = ("n0", ["b0", "b1"], 1, 1)
    return s


# ---- 12. one node past the first block, and 300 ---------------------------------------------------------
def block_edge(n: int = 257) -> VolScene:
    """n nodes at EBS limit 1, each with one victim mounting its own volume; the
    victim of the last node has the lowest priority, so that node wins."""
    s = VolScene(f"block_edge_{n}")
    for i in range(n):
        s.node(f"n{i:04d}", {EBS_KEY: "1"})
        s.bpod(f"b{i}", f"n{i:04d}", 3 if i == n - 1 else 10 + i % 7, [("ebs", f"v{i}")])
    s.preemptor([("ebs", "x")])
    s.expect_result = (f"n{n - 1:04d}", [f"b{n - 1}"], n, n)
    return s


def three_hundred_shared() -> VolScene:
    """300 nodes at limit 1; on each, two pods (10 and 5) share one volume, so
    both are victims; on the last a single pod (10) holds it: fewer victims."""
    n = 300
    s = VolScene("three_hundred_shared")
    for i in range(n):
        s.node(f"n{i:04d}", {EBS_KEY: "1"})
        s.bpod(f"a{i}", f"n{i:04d}", 10, [("ebs", f"v{i}")])
        if i != n - 1:
            s.bpod(f"c{i}", f"n{i:04d}", 5, [("ebs", f"v{i}")])
    s.preemptor([("ebs", "x")])
    s.expect_result = (f"n{n - 1:04d}", [f"a{n - 1}"], n, n)
    s.tells = ("shared_leaves_early",)
    return s


# ---- 13. sums past 2^31 (tables patched by the tests: no object scene holds 2^31 volumes) ------------
PAST_ATTACHED, PAST_HELD, PAST_ARG, PAST_LIMIT = 2147483000, 2147482000, 1000, 2 ** 31 - 2


def past_2_31() -> VolScene:
    """One node, one victim, one new volume for the preemptor, all EBS.  The
    tests patch the compiled tables: limit INT32_MAX - 1, attached 2147483000
    of which the victim holds 2147482000, and the preemptor brings 1000.
    attached + arg = 2147484000 > limit only in 64 bits (potential); with the
    victim out 1000 + 1000 passes; put back it fails: the victim."""
    s = VolScene("past_2_31")
    s.node("n0", {EBS_KEY: "39"})
    s.bpod("b0", "n0", 5, [("ebs", "a")])
    s.preemptor([("ebs", "x")])
    s.expect_result = ("n0", ["b0"], 1, 1)
    return s


_ALL = (ebs_slot, two_victims_share, shared_with_higher, preemptor_mounts_victims_volume, last_holder_leaves,
        csi_over_limit_nothing_new, csi_node_without_key, two_families_and_a_third, fit_first_limit_decides,
        functools.partial(fit_first_limit_decides, True), profile_without_ebs, group_holds_volumes,
        group_shares_with_victim, port_and_volume, block_edge, three_hundred_shared)


# ---- a budget between the rows (not in scenes(): it carries PodDisruptionBudgets) ----------------
def mixed_budget() -> VolScene:
    """n0: EBS limit 3, four lower-priority pods holding two shared volumes
    two-and-two: b1 (40) and b3 (20) mount a, b2 (30) and b4 (10) mount b.  The
    preemptor brings two new volumes: 2 + 2 > 3 (potential); all out: 0 + 2.
    ``budgets``: one budget, disruptionsAllowed 1, over b1, b2, b3 (tier=db):
    b1 takes the one disruption, b2 and b3 violate.  The violating pods first:
    b2 back, {b}: 1 + 2 stays; b3 back, {a, b}: 4 > 3, a victim that violates.
    Then b1: a left with b3, so it attaches again, 4 > 3, a victim; b4: b is
    attached (b2 was reprieved), 1 + 2, it stays after b3 stayed out.
    Without budgets (``expect_result``): b1 stays, b2 out, b3 stays (a is
    attached), b4 out."""
    from ksim.model import LabelSelector, PodDisruptionBudget
    s = VolScene("mixed_budget")
    s.node("n0", {EBS_KEY: "3"})
    for name, prio, vol in (("b1", 40, "a"), ("b2", 30, "b"), ("b3", 20, "a"), ("b4", 10, "b")):
        s.bpod(name, "n0", prio, [("ebs", vol)]).labels = {"tier": "db"} if name != "b4" else {}
    s.preemptor([("ebs", "x"), ("ebs", "y")])
    s.budgets = [PodDisruptionBudget("db", selector=LabelSelector({"tier": "db"}), disruptions_allowed=1)]
    s.expect_result = ("n0", ["b2", "b4"], 1, 1)
    s.expect_budgets = ("n0", ["b3", "b1"], 1, 1, 1)
    return s


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, VolScene]:
    out = {}
    for make in _ALL:
        s = make()
        out[s.name] = s
    return out


def scene_ids() -> List[str]:
    return list(scenes())
