"""Hand-made clusters for DefaultPreemption's dry run of a preemptor with
DoNotSchedule topology spread (csrc/ksim_preempt.hip, the spread form), as
model objects: tests/test_preempt_spread_ref.py checks on the CPU that they
tell the reference (tests/preemptspreadref.py) from its faulty readings, and
tests/test_gpu_preempt_spread.py runs the engine on them.

As in tests/preemptaffcases.py every node has 10 CPUs, bound pods are
(node, priority, start, cpu milli, labels[, extras]) rows in table order
(extras: "anti", "ports", and here "ns"), the preemptor has priority 1000 and
every potential node is tried (args (100, 0)).  ``expect`` is the hand-derived
result with the scene's nominated groups, ``expect_plain`` the one without."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

from ksim.model import Container, ContainerPort, LabelSelector, Pod, Taint, TopologySpreadConstraint
from preemptaffcases import DB, HOST, NONE, PRIO, X, Y, ZONE, AffScene, _zones, bound_pods, node, preemptor, term

__all__ = ["SpreadScene", "scenes", "scene_ids", "hard", "PRIO", "ZONE", "HOST", "X", "Y", "DB", "NONE"]


@dataclass
class SpreadScene(AffScene):
    expect_plain: Optional[tuple] = None            # the result without the nominated groups (scenes that have some)
    drop: Tuple[str, ...] = ()                      # filter plugins the scene's profile leaves out


def hard(key: str = ZONE, skew: int = 1, labels=X, **policies) -> TopologySpreadConstraint:
    return TopologySpreadConstraint(skew, key, "DoNotSchedule", LabelSelector(dict(labels)), **policies)


def rows_to_pods(nodes, rows) -> Tuple[List[Pod], Dict[str, int]]:
    """bound_pods plus the "ns" extra: the row's namespace."""
    bound, start = bound_pods(nodes, rows)
    for p, row in zip(bound, rows):
        if len(row) > 5 and "ns" in row[5]:
            p.namespace = row[5]["ns"]
    return bound, start


def _nominee(i: int, labels, cpu: int = 100) -> Pod:
    return Pod(f"nominated{i}", priority=1500, labels=dict(labels), containers=[Container({"cpu": f"{cpu}m"})])


# ---- A. the headline case -------------------------------------------------------------------
def headline() -> SpreadScene:
    """za x3, zb x2; maxSkew 1 on the zone over app=x; the preemptor is an x pod.
    za counts 3 (node 0: priorities 20 and 10; node 1: 15), zb 1, and zb is full
    of priority-2000 pods.  Every za node fails for skew (3 + 1 - 1 > 1): all
    three are potential.  Node 0 with both x pods out: za = 1, 1 + 1 - 1 = 1
    passes; each one put back makes za 2: 2 + 1 - 1 > 1, a victim.  Node 1 with
    its x pod out: za = 2, still too many.  Node 2 has nothing to remove."""
    nodes = _zones({"za": 3, "zb": 2})
    rows = [(0, 20, 100, 1000, X), (0, 10, 100, 1000, X), (1, 15, 100, 1000, X),
            (3, 2000, 100, 9500, X), (4, 2000, 100, 9500, NONE)]
    bound, start = rows_to_pods(nodes, rows)
    return SpreadScene("headline", nodes, bound, start, [preemptor(labels=X, topology_spread=[hard()])],
                       kinds=("PTS_HARD",), expect=("n0000", ["b0", "b1"], 5, 1))


# ---- B. a nominated group lifts the own domain above the second minimum ------------------------
def group_lifts_own_domain() -> SpreadScene:
    """za x2, zb x2; za counts 1 (node 0's x pod, priority 10), zb 2 (priority
    2000); nodes 1 to 3 are full.  Node 0 is short of CPU for the 4-CPU
    preemptor beside the 5.5-CPU hog (priority 5).
    Without a group: all out za = 0; the x pod back: 1 + 1 - min(1, 2) = 1
    passes and fits (reprieved); the hog does not fit: the victim.
    With two x pods nominated on node 0 (0.1 CPU each): all out za = 2,
    2 + 1 - min(2, 2) = 1 passes; the x pod back: 3 + 1 - min(3, 2) = 2 > 1, a
    victim; the hog back: 5.5 + 0.2 + 4 CPUs fit, reprieved.  A minimum kept
    from the status pass (1) would fail the node with all out: 2 + 1 - 1."""
    nodes = _zones({"za": 2, "zb": 2})
    rows = [(0, 10, 100, 1000, X), (0, 5, 100, 5500, NONE), (1, 2000, 100, 9500, NONE),
            (2, 2000, 100, 9500, X), (3, 2000, 100, 9500, X)]
    bound, start = rows_to_pods(nodes, rows)
    return SpreadScene("group_lifts_own_domain", nodes, bound, start,
                       [preemptor(4000, labels=X, topology_spread=[hard()]), _nominee(0, X), _nominee(1, X)],
                       nominated={"n0000": [1, 2]}, kinds=("PTS_HARD",),
                       expect=("n0000", ["b0"], 4, 1), expect_plain=("n0000", ["b1"], 4, 1))


# ---- C. a node the inclusion policy excludes ---------------------------------------------------
def tainted_node_moves_nothing() -> SpreadScene:
    """A profile without TaintToleration; the constraint says nodeTaintsPolicy:
    Honor and node 0 carries a taint the preemptor does not tolerate, so its two
    x pods count nowhere: za = 3 (nodes 1 and 2, priority 2000), zb = 1.  Node 0
    fails for skew (potential); with its pods out za still stands at 3: no
    candidate.  Nodes 1 and 2 fail for skew too, nodes 3 and 4 are full."""
    nodes = _zones({"za": 3, "zb": 2})
    nodes[0].taints = [Taint("dedicated", "batch", "NoSchedule")]
    rows = [(0, 10, 100, 1000, X), (0, 20, 100, 1000, X), (1, 2000, 100, 1000, X), (1, 2000, 90, 1000, X),
            (2, 2000, 100, 1000, X), (3, 2000, 100, 9500, X), (4, 2000, 100, 9500, NONE)]
    bound, start = rows_to_pods(nodes, rows)
    p = preemptor(labels=X, topology_spread=[hard(node_taints_policy="Honor")])
    return SpreadScene("tainted_node_moves_nothing", nodes, bound, start, [p], kinds=("PTS_HARD",),
                       expect=(None, [], 5, 0), drop=("TaintToleration",))


def unselected_node_moves_nothing() -> SpreadScene:
    """The same under nodeAffinityPolicy (Honor by default) in a profile without
    NodeAffinity: the preemptor selects pool=a, node 0 alone lacks that label,
    so its two x pods count nowhere and its dry run moves nothing."""
    sc = tainted_node_moves_nothing()
    sc.nodes[0].taints = []
    for n in sc.nodes[1:]:
        n.labels["pool"] = "a"
    p = preemptor(labels=X, topology_spread=[hard()], node_selector={"pool": "a"})
    return SpreadScene("unselected_node_moves_nothing", sc.nodes, sc.bound, sc.start, [p], kinds=("PTS_HARD",),
                       expect=(None, [], 5, 0), drop=("NodeAffinity",))


# ---- D. two hard constraints, a node without the zone label --------------------------------------
def zone_and_hostname() -> SpreadScene:
    """maxSkew 1 on the zone and on the hostname over app=x.  Node 4 has no zone
    label: it fails for the missing label (not potential), and lacking a key it
    is eligible for neither constraint, so its x pods count nowhere.
    za = 2 (node 0: priorities 20 and 10), zb = 1; hosts: node 0 counts 2, the
    minimum over hosts is 0.  Node 0 fails for skew; all out: zone 0 + 1 - 0 and
    host 0 + 1 - 0 pass; either x pod back: host 1 + 1 - 0 > 1, a victim."""
    nodes = _zones({"za": 2, "zb": 2}) + [node(4, None)]
    rows = [(0, 20, 100, 1000, X), (0, 10, 100, 1000, X), (1, 2000, 100, 9500, NONE), (2, 2000, 100, 9500, X),
            (3, 2000, 100, 9500, NONE), (4, 10, 100, 1000, X), (4, 12, 100, 1000, X)]
    bound, start = rows_to_pods(nodes, rows)
    p = preemptor(labels=X, topology_spread=[hard(ZONE), hard(HOST)])
    return SpreadScene("zone_and_hostname", nodes, bound, start, [p], kinds=("PTS_HARD",),
                       expect=("n0000", ["b0", "b1"], 4, 1))


# ---- E. the own domain is the only one; a tie between the minima ------------------------------------
def only_domain() -> SpreadScene:
    """One zone: no other domain, the critical path is the own count whatever
    moves (3 + 1 - 3 with the group's two x pods and all of node 0 out).  A kept
    minimum (2) would fail that state.  The hog goes for CPU."""
    nodes = _zones({"za": 2})
    rows = [(0, 10, 100, 1000, X), (0, 5, 100, 8000, NONE), (1, 2000, 100, 9500, X)]
    bound, start = rows_to_pods(nodes, rows)
    return SpreadScene("only_domain", nodes, bound, start,
                       [preemptor(4000, labels=X, topology_spread=[hard()]), _nominee(0, X), _nominee(1, X)],
                       nominated={"n0000": [1, 2]}, kinds=("PTS_HARD",),
                       expect=("n0000", ["b1"], 2, 1), expect_plain=("n0000", ["b1"], 2, 1))


def tied_minima() -> SpreadScene:
    """za = 2, zb = 1, zc = 1: the two minima tie.  Node 0 (za) fails for skew
    and is a candidate without its x pod (1 + 1 - 1); node 2 (zb) is short of
    CPU: its x pod is reprieved (1 + 1 - min(1, 1)), the hog goes.  Node 0's
    victim ranks lower: it wins."""
    nodes = _zones({"za": 2, "zb": 2, "zc": 1})
    rows = [(0, 10, 100, 1000, X), (1, 2000, 100, 9500, X), (2, 30, 100, 1000, X), (2, 20, 100, 8000, NONE),
            (3, 2000, 100, 9500, NONE), (4, 2000, 100, 9500, X)]
    bound, start = rows_to_pods(nodes, rows)
    return SpreadScene("tied_minima", nodes, bound, start, [preemptor(4000, labels=X, topology_spread=[hard()])],
                       kinds=("PTS_HARD",), expect=("n0000", ["b0"], 5, 2))


# ---- F. hard spread beside zone anti-affinity and a host port ------------------------------------------
def spread_anti_and_port() -> SpreadScene:
    """The preemptor spreads over app=x by zone, is anti-affine to app=y by zone
    and wants port 80.  Node 0 holds 9.5 CPUs of lower-priority pods: two x pods,
    a y pod, the port's holder and a hog.  All out everything passes; back in
    importance order: x (20): za = 2, a victim; y (15): anti-affinity; the holder
    (12): the port; x (10): za = 2 again; the hog (5) fits: reprieved.  Node 1
    keeps za at 1 with a pod that outranks the preemptor; node 2 fails for skew
    with nothing to remove; zb is full."""
    nodes = _zones({"za": 3, "zb": 2})
    rows = [(0, 10, 100, 1000, X), (0, 20, 100, 1000, X), (0, 15, 100, 1000, Y),
            (0, 12, 100, 1000, NONE, {"ports": [(80, "TCP", "")]}), (0, 5, 100, 5500, NONE),
            (1, 2000, 100, 9500, X), (3, 2000, 100, 9500, X), (4, 2000, 100, 9500, NONE)]
    bound, start = rows_to_pods(nodes, rows)
    p = preemptor(4000, labels=X, anti=[term(ZONE, app="y")], topology_spread=[hard()])
    p.containers[0].ports = [ContainerPort(80, "TCP", "")]
    return SpreadScene("spread_anti_and_port", nodes, bound, start, [p],
                       kinds=("PTS_HARD", "IPA_ANTI", "NODE_PORT"), expect=("n0000", ["b1", "b2", "b3", "b0"], 5, 1))


# ---- G. 300 hostname domains ---------------------------------------------------------------------
def three_hundred_hosts() -> SpreadScene:
    """maxSkew 1 on the hostname over app=x on 300 nodes: a domain table of 300
    values, past the 256 threads of k_preempt_spread_mins and of one block of
    k_preempt_nodes.  Every node holds one x pod that outranks the preemptor
    (the minimum is 1) except: node 255 holds two more (20 and 10): skew, both
    go; node 256 holds a lower-priority x pod and a 8-CPU hog (50): short of
    CPU, the x pod is reprieved (1 + 1 - 1), the hog goes; node 299 holds two
    that outrank and one that does not: 2 + 1 - 1 > 1 without it, no candidate.
    Node 255's first victim ranks lower than node 256's: it wins."""
    nodes = _zones({"z0": 300})
    rows = [(v, 2000, 100, 1000, X) for v in range(300) if v != 256]
    k = len(rows)
    rows += [(255, 20, 100, 1000, X), (255, 10, 100, 1000, X), (256, 30, 100, 1000, X), (256, 50, 100, 8000, NONE),
             (299, 2000, 90, 1000, X), (299, 10, 100, 1000, X)]
    bound, start = rows_to_pods(nodes, rows)
    return SpreadScene("three_hundred_hosts", nodes, bound, start,
                       [preemptor(2000, labels=X, topology_spread=[hard(HOST)])], kinds=("PTS_HARD",),
                       expect=("n0255", [f"b{k}", f"b{k + 1}"], 3, 2))


# ---- H. no self match; a matching pod in another namespace -----------------------------------------------
def other_namespace() -> SpreadScene:
    """The preemptor carries no label, so it does not match its own selector
    (selfMatch 0).  za = 3 in its namespace (node 0: priority 10; node 1: two
    that outrank), zb = 1; node 0 also holds an x pod of namespace "other"
    (priority 5), which counts nowhere.  Node 0 fails for skew (3 - 1 > 1); all
    out za = 2: passes; the x pod back: 3 - 1, a victim; the other namespace's
    pod back moves nothing: reprieved."""
    nodes = _zones({"za": 2, "zb": 2})
    rows = [(0, 10, 100, 1000, X), (0, 5, 100, 1000, X, {"ns": "other"}), (1, 2000, 100, 4500, X),
            (1, 2000, 90, 5000, X), (2, 2000, 100, 9500, X), (3, 2000, 100, 9500, NONE)]
    bound, start = rows_to_pods(nodes, rows)
    return SpreadScene("other_namespace", nodes, bound, start, [preemptor(topology_spread=[hard()])],
                       kinds=("PTS_HARD",), expect=("n0000", ["b0"], 4, 1))


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, SpreadScene]:
    out = [headline(), group_lifts_own_domain(), tainted_node_moves_nothing(), unselected_node_moves_nothing(),
           zone_and_hostname(), only_domain(),
           tied_minima(), spread_anti_and_port(), three_hundred_hosts(), other_namespace()]
    table = {s.name: s for s in out}
    assert len(table) == len(out)
    return table


def scene_ids() -> List[str]:
    return list(scenes())


def filter_order(sc: SpreadScene) -> List[str]:
    """The reference's filter list for the scene: the default one without ``sc.drop``."""
    from oracle.objref import ObjScheduler
    return [pl for pl in ObjScheduler(sc.nodes, []).filter_order if pl not in sc.drop]
