"""Hand-made clusters for DefaultPreemption's dry run of a preemptor with
required pod (anti-)affinity (csrc/ksim_preempt.hip, the domain form), as model
objects: tests/test_preempt_affinity_ref.py checks on the CPU that they tell
the reference (tests/preemptobjref.py) from its faulty variants, and
tests/test_gpu_preempt_affinity.py runs the engine on them.

Every node has 10 CPUs.  Bound pods are written as
(node, priority, start, cpu milli, labels[, extras]) rows in table order; the
preemptor has priority 1000 unless said otherwise."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from ksim.model import (Container, ContainerPort, LabelSelector, Node, Pod, PodAffinityTerm,
                        TopologySpreadConstraint, WeightedPodAffinityTerm)

ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"
IMAGE = "registry.example/app:v1"
PRIO = 1000


@dataclass
class AffScene:
    name: str
    nodes: List[Node]
    bound: List[Pod]
    start: Dict[str, int]
    pods: List[Pod]                                 # pods[0]: the preemptor; the rest: nominated pods
    nominated: Dict[str, List[int]] = field(default_factory=dict)   # node name -> indices into pods
    args: Tuple[int, int] = (100, 0)                # every potential node is tried
    kinds: Tuple[str, ...] = ()                     # use kinds the compiled preemptor must carry (abi.USE_<kind>)
    expect: Optional[tuple] = None                  # (node name or None, victim names, potential, candidates)
    note: str = ""

    @property
    def order(self) -> Dict[str, int]:
        return {p.name: i for i, p in enumerate(self.bound)}

    def nominated_pods(self) -> Dict[str, List[Pod]]:
        return {n: [self.pods[i] for i in idx] for n, idx in self.nominated.items()}


def node(i: int, zone: Optional[str]) -> Node:
    labels = {HOST: f"n{i:04d}"}
    if zone is not None:
        labels[ZONE] = zone
    return Node(name=f"n{i:04d}", labels=labels, allocatable={"cpu": "10000m", "memory": "64Gi", "pods": "110"})


def term(key: str, **labels) -> PodAffinityTerm:
    return PodAffinityTerm(key, LabelSelector(dict(labels)))


def bound_pods(nodes: List[Node], rows) -> Tuple[List[Pod], Dict[str, int]]:
    """rows: (node, priority, start, cpu milli, labels[, {"anti": [terms], "ports": [...]}])."""
    bound, start = [], {}
    for i, row in enumerate(rows):
        at, prio, st, cpu, labels = row[:5]
        extra = row[5] if len(row) > 5 else {}
        bound.append(Pod(f"b{i}", node_name=nodes[at].name, priority=int(prio), labels=dict(labels),
                         containers=[Container({"cpu": f"{cpu}m"}, [ContainerPort(*p) for p in extra.get("ports", ())])],
                         pod_anti_affinity_required=list(extra.get("anti", ()))))
        start[f"b{i}"] = int(st)
    return bound, start


def preemptor(cpu: int = 1000, anti=(), aff=(), labels=None, name="preemptor", prio=PRIO, **more) -> Pod:
    return Pod(name, priority=prio, labels=dict(labels or {}), containers=[Container({"cpu": f"{cpu}m"})],
               pod_anti_affinity_required=list(anti), pod_affinity_required=list(aff), **more)


X, Y, DB, NONE = {"app": "x"}, {"app": "y"}, {"app": "db"}, {}


def _zones(counts: Dict[str, int]) -> List[Node]:
    out = []
    for z, k in counts.items():
        out += [node(len(out) + j, z) for j in range(k)]
    return out


# ---- 1. the headline case -----------------------------------------------------------------
def headline(holder_prio=10) -> AffScene:
    """No resource pressure; zone anti-affinity against app=x.  Zone za's only
    x pod (node 1) ranks below the preemptor unless ``holder_prio`` says
    otherwise; zone zb's (node 4) outranks it."""
    nodes = _zones({"za": 3, "zb": 3})
    rows = [(1, holder_prio, 100, 1000, X), (1, 5, 90, 1000, NONE), (0, 5, 100, 1000, NONE), (2, 7, 100, 1000, Y),
            (4, 2000, 100, 1000, X), (3, 5, 100, 1000, NONE), (5, 5, 100, 1000, NONE)]
    bound, start = bound_pods(nodes, rows)
    low = holder_prio < PRIO
    return AffScene("headline" if low else "headline_outranked", nodes, bound, start,
                    [preemptor(anti=[term(ZONE, app="x")])], kinds=("IPA_ANTI",),
                    expect=("n0001", ["b0"], 6, 1) if low else (None, [], 6, 0))


# ---- 2. existing anti-affinity --------------------------------------------------------------
def existing_anti(twice=False, holder_prio=10) -> AffScene:
    """A bound pod carries a required zone anti-affinity term that matches the
    preemptor (role=p); ``twice``: it carries the term two times, so its node's
    zone counts 2 and its removal must take 2 away."""
    nodes = _zones({"za": 3, "zb": 3})
    t = term(ZONE, role="p")
    rows = [(1, holder_prio, 100, 1000, NONE, {"anti": [t, t] if twice else [t]}), (1, 5, 90, 1000, NONE),
            (0, 5, 100, 1000, NONE), (4, 2000, 100, 1000, NONE, {"anti": [t]}), (3, 5, 100, 1000, NONE)]
    bound, start = bound_pods(nodes, rows)
    low = holder_prio < PRIO
    name = "existing_anti" + ("_twice" if twice else "") + ("" if low else "_outranked")
    return AffScene(name, nodes, bound, start, [preemptor(labels={"role": "p"})], kinds=("IPA_EXISTING_ANTI",),
                    expect=("n0001", ["b0"], 6, 1) if low else (None, [], 6, 0))


# ---- 3. a hostname key and a zone key in one preemptor ---------------------------------------
def host_and_zone() -> AffScene:
    """Anti-affinity on the hostname against app=x (the node's own count) and on
    the zone against app=y (a domain sum); node 5 has no zone label, so its y
    pod counts nowhere; a ScheduleAnyway constraint with an empty selector is a
    use without a class (cls -1)."""
    nodes = _zones({"za": 3, "zb": 2}) + [node(5, None)]
    rows = [(0, 10, 100, 1000, X), (1, 20, 100, 1000, Y), (1, 5, 100, 1000, NONE), (2, 5, 100, 1000, NONE),
            (3, 2000, 100, 1000, Y), (4, 5, 100, 1000, NONE), (5, 30, 100, 1000, X), (5, 40, 100, 1000, Y)]
    bound, start = bound_pods(nodes, rows)
    p = preemptor(anti=[term(HOST, app="x"), term(ZONE, app="y")],
                  topology_spread=[TopologySpreadConstraint(1, ZONE, "ScheduleAnyway", LabelSelector())])
    # node 0: its x pod goes, but za still holds y (node 1); node 1: y goes, the zone is clear, the
    # other pod stays; node 2: nothing to remove; zb: y outranks; node 5: x goes, y (no zone) stays
    return AffScene("host_and_zone", nodes, bound, start, [p], kinds=("IPA_ANTI", "PTS_SOFT"),
                    expect=("n0001", ["b1"], 6, 2))


# ---- 4. Fit and anti-affinity together ----------------------------------------------------------
def fit_and_anti() -> AffScene:
    """Every node of za is short of CPU for the 4-CPU preemptor (Fit fails
    first).  Node 1 holds two x pods of priority 30 and 10: both must go although
    the CPU would fit beside them; the unrelated pod of priority 20 between them
    is reprieved; the 5.5-CPU pod of priority 5 goes for CPU."""
    nodes = _zones({"za": 3, "zb": 2})
    rows = [(1, 30, 100, 1000, X), (1, 20, 100, 2000, NONE), (1, 10, 100, 1000, X), (1, 5, 100, 5500, NONE),
            (0, 50, 100, 9000, NONE), (2, 50, 100, 4000, NONE), (2, 60, 100, 4000, NONE),
            (3, 2000, 100, 9500, NONE), (4, 40, 100, 9500, X)]
    bound, start = bound_pods(nodes, rows)
    return AffScene("fit_and_anti", nodes, bound, start, [preemptor(4000, anti=[term(ZONE, app="x")])],
                    kinds=("IPA_ANTI",), expect=("n0001", ["b0", "b2", "b3"], 5, 2))


# ---- 5. required affinity ---------------------------------------------------------------------------
def affinity() -> AffScene:
    """Zone affinity to app=db, 4 CPUs.
    za: node 0 is short of CPU (potential) but za holds no db pod: no
        candidate; node 1 has room and fails the affinity rule itself
        (UnschedulableAndUnresolvable): not potential.
    zb: node 2 is short of CPU and the zone's only db pod is its own
        lower-priority pod.  SelectVictimsOnNode first removes every
        lower-priority pod, then runs the filters: with the db pod out the
        affinity fails, so upstream gives up on the node before any reprieve.
    zc: node 3 is short of CPU; its db pod (priority 40) goes out with the
        rest, the zone keeps node 4's db pod (priority 2000), so the node is a
        candidate and its own db pod is reprieved first; the 6-CPU filler goes."""
    nodes = _zones({"za": 2, "zb": 1, "zc": 2})
    rows = [(0, 10, 100, 9000, NONE), (1, 10, 100, 1000, NONE),
            (2, 10, 100, 1000, DB), (2, 5, 100, 8500, NONE),
            (3, 40, 100, 1000, DB), (3, 20, 100, 6000, NONE), (3, 10, 100, 2500, NONE),
            (4, 2000, 100, 9500, DB)]
    bound, start = bound_pods(nodes, rows)
    return AffScene("affinity", nodes, bound, start, [preemptor(4000, aff=[term(ZONE, app="db")])],
                    kinds=("IPA_AFFINITY",), expect=("n0003", ["b5"], 4, 1))


def first_pod() -> AffScene:
    """The preemptor matches its own affinity term (app=db); the only db pods of
    the cluster are two lower-priority pods of node 1, which is short of CPU.
    With both out no pod matches anywhere, so the first-pod rule lets the
    preemptor in; put back, the first db pod fits beside it, the second does
    not (CPU).  Node 0 (za, short of CPU) is a candidate as well, beside node
    1's db pods, at a higher victim priority; node 2 (zb) is none: with its
    filler out the affinity still fails there, and za's db pods keep the
    first-pod rule off."""
    nodes = _zones({"za": 2, "zb": 1})
    rows = [(1, 30, 100, 3000, DB), (1, 20, 100, 6500, DB), (0, 25, 100, 9000, NONE), (2, 10, 100, 9000, NONE)]
    bound, start = bound_pods(nodes, rows)
    return AffScene("first_pod", nodes, bound, start, [preemptor(4000, aff=[term(ZONE, app="db")], labels=DB)],
                    kinds=("IPA_AFFINITY",), expect=("n0001", ["b1"], 3, 2))


# ---- 6. sixteen uses ------------------------------------------------------------------------------
def sixteen_uses() -> AffScene:
    """Two host ports, two ScheduleAnyway constraints, an image, required
    affinity (self-matching), three required anti-affinity terms, two carried
    anti-affinity terms of bound pods, and preferred terms up to 16 uses."""
    nodes = _zones({"za": 4, "zb": 4, "zc": 2})
    for i, n in enumerate(nodes):
        if i % 2 == 0:
            n.images = [([IMAGE], 500 * 2 ** 20)]
    tz, th = term(ZONE, role="p"), term(HOST, role="p")
    rows = [(0, 10, 100, 1000, X), (1, 20, 100, 1000, Y), (1, 15, 100, 1000, DB), (2, 30, 100, 1000, NONE, {"anti": [th]}),
            (3, 5, 100, 1000, NONE, {"ports": [(80, "TCP", "")]}),
            (4, 2000, 100, 1000, X), (5, 10, 100, 1000, DB), (6, 10, 100, 1000, NONE, {"ports": [(81, "UDP", "10.0.0.1")]}),
            (7, 10, 100, 1000, NONE), (8, 10, 100, 1000, DB, {"anti": [tz]}), (9, 10, 100, 1000, NONE)]
    bound, start = bound_pods(nodes, rows)
    p = preemptor(anti=[term(ZONE, app="x"), term(HOST, app="y"), term(HOST, app="x")], aff=[term(ZONE, app="db")],
                  labels={"role": "p", "app": "db"},
                  topology_spread=[TopologySpreadConstraint(1, ZONE, "ScheduleAnyway", LabelSelector(dict(X))),
                                   TopologySpreadConstraint(1, HOST, "ScheduleAnyway", LabelSelector(dict(Y)))],
                  pod_affinity_preferred=[WeightedPodAffinityTerm(10 + k, term(ZONE, tier=f"t{k}")) for k in range(4)])
    p.containers[0].image = IMAGE
    p.containers[0].ports = [ContainerPort(80, "TCP", ""), ContainerPort(81, "UDP", "")]
    return AffScene("sixteen_uses", nodes, bound, start, [p],
                    kinds=("IPA_ANTI", "IPA_AFFINITY", "IPA_EXISTING_ANTI", "NODE_PORT", "PTS_SOFT", "IPA_SCORE", "IMAGE"))


# ---- 7. 300 nodes, one zone across the block boundary ----------------------------------------------
def two_blocks() -> AffScene:
    """One zone of 300 nodes (two blocks of k_preempt_nodes): zone affinity to
    app=db, whose only pod sits on node 290 and outranks the preemptor, and zone
    anti-affinity against app=x, whose only pod is node 10's: every node fails
    the anti-affinity rule, node 10 alone is a candidate, and its thread reads a
    domain sum that node 290's block contributed."""
    nodes = _zones({"z0": 300})
    rows = [(v, 5, 100, 1000, NONE) for v in range(0, 300, 7)]
    rows += [(10, 10, 100, 1000, X), (290, 2000, 100, 1000, DB)]
    bound, start = bound_pods(nodes, rows)
    holder = f"b{len(rows) - 2}"
    return AffScene("two_blocks", nodes, bound, start,
                    [preemptor(anti=[term(ZONE, app="x")], aff=[term(ZONE, app="db")])],
                    kinds=("IPA_ANTI", "IPA_AFFINITY"), expect=("n0010", [holder], 300, 1))


# ---- 8. nominated groups ---------------------------------------------------------------------------
def nominated_holder() -> AffScene:
    """Node 1's x pod is a nominated pod of higher priority: only node 1 sees it
    (pass 1), it cannot be evicted, so the node is potential and no candidate.
    Zone zb's x pod (node 3) is bound and of lower priority."""
    nodes = _zones({"za": 2, "zb": 2})
    rows = [(0, 5, 100, 1000, NONE), (1, 5, 100, 1000, NONE), (3, 10, 100, 1000, X), (2, 5, 100, 1000, NONE)]
    bound, start = bound_pods(nodes, rows)
    nom = Pod("nominated", priority=1500, labels=dict(X), containers=[Container({"cpu": "500m"})])
    return AffScene("nominated_holder", nodes, bound, start, [preemptor(anti=[term(ZONE, app="x")]), nom],
                    nominated={"n0001": [1]}, kinds=("IPA_ANTI",), expect=("n0003", ["b2"], 3, 1))


def nominated_match() -> AffScene:
    """Zone affinity to app=db; the only db pod anywhere is nominated to node 1,
    which is short of CPU with it on.  Pass 1 of node 1 fails Fit (potential);
    its dry run keeps the group on the node, so the affinity holds and the
    filler goes.  Node 2 is short of CPU too (potential), but no db pod is in
    its zone: no candidate.  The other nodes fail the affinity rule itself:
    not potential."""
    nodes = _zones({"za": 2, "zb": 2})
    rows = [(1, 10, 100, 6000, NONE), (1, 20, 100, 1000, NONE), (0, 5, 100, 1000, NONE), (2, 5, 100, 9500, NONE)]
    bound, start = bound_pods(nodes, rows)
    nom = Pod("nominated", priority=1500, labels=dict(DB), containers=[Container({"cpu": "1000m"})])
    return AffScene("nominated_match", nodes, bound, start, [preemptor(4000, aff=[term(ZONE, app="db")]), nom],
                    nominated={"n0001": [1]}, kinds=("IPA_AFFINITY",), expect=("n0001", ["b0"], 2, 1))


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, AffScene]:
    out = [headline(), headline(2000), existing_anti(), existing_anti(holder_prio=2000), existing_anti(twice=True),
           host_and_zone(), fit_and_anti(), affinity(), first_pod(), sixteen_uses(), two_blocks(),
           nominated_holder(), nominated_match()]
    table = {s.name: s for s in out}
    assert len(table) == len(out)
    return table


def scene_ids() -> List[str]:
    return list(scenes())
