"""Hand-made clusters for DefaultPreemption's dry run with PodDisruptionBudgets
(csrc/ksim_preempt.hip, the PDB form; ksim_set_bound_pod_pdbs), as model
objects: tests/test_preempt_pdb_ref.py checks on the CPU that each scene has
the property its name claims and that the scenes tell the reference
(tests/preemptpdbref.py) from its faulty variants, and
tests/test_gpu_preempt_pdb.py runs the engine on them.

Every node has 10 CPUs and, unless said otherwise, the preemptor asks for 8
(priority 1000): a pod of more than 2 CPUs cannot stay beside it.  Bound pods
are rows (node, priority, start, cpu milli, labels[, extras]) in table order,
named b0, b1, ... (tests/preemptaffcases.py bound_pods).  ``A`` pods are the
ones the budget ``guard`` (app=a, disruptionsAllowed 0 unless said otherwise)
selects."""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import preemptaffcases as ac
import preemptpdbref
from ksim.model import Container, ContainerPort, LabelSelector, Pod, PodDisruptionBudget, Requirement

PRIO = ac.PRIO
A, T, AT, NONE = {"app": "a"}, {"tier": "t"}, {"app": "a", "tier": "t"}, {}
PICK_THREADS = 1024                                  # k_preempt_pick's block
WAVE = 64


def pdb(name: str, allowed: int = 0, namespace: str = "default", disrupted=(), **labels) -> PodDisruptionBudget:
    return PodDisruptionBudget(name, namespace, LabelSelector(dict(labels)), allowed, tuple(disrupted))


@dataclass
class PdbScene(ac.AffScene):
    pdbs: List[PodDisruptionBudget] = field(default_factory=list)
    aims: Tuple[str, ...] = ()                       # the faults of preemptpdbref.FAULTS the scene is aimed at
    claim: Optional[Callable[["PdbScene", tuple], bool]] = None   # the property the name claims, of the reference result
    want: Optional[int] = None                       # numCandidates (the cut scenes)

    def grouped(self) -> "PdbScene":
        """The scene with a nominated pod of higher priority (an A pod of 0.7
        CPU) on its second node, through ksim_preempt_nominated; a scene that
        has a group of its own stays as it is."""
        if self.nominated:
            return self
        nom = Pod("nominated", priority=PRIO + 500, labels=dict(A), containers=[Container({"cpu": "700m"})])
        return dataclasses.replace(self, pods=list(self.pods) + [nom],
                                   nominated={self.nodes[min(1, len(self.nodes) - 1)].name: [len(self.pods)]})


def _scene(name, n_nodes, rows, pdbs, aims=(), claim=None, pods=None, zones=None, args=(100, 0), **more) -> PdbScene:
    nodes = ac._zones(zones or {"z0": n_nodes})
    bound, start = ac.bound_pods(nodes, rows)
    return PdbScene(name, nodes, bound, start, pods or [ac.preemptor(8000)], args=args, pdbs=pdbs, aims=tuple(aims),
                    claim=claim, **more)


def _prio(sc: PdbScene, name: str) -> int:
    return next(p.priority for p in sc.bound if p.name == name)


OUTRANKS = (2, 2000, 100, 9000, NONE)                # node 2: potential, never a candidate


# ---- the pick -------------------------------------------------------------------------------
def violations_level() -> PdbScene:
    """Five candidates that tie on every level below the first; the first
    three evict an A pod.  Level 1 alone sends the pick to node 3."""
    rows = [(v, 50, 100, 2500, A if v < 3 else NONE) for v in range(5)]

    def claim(sc, r):
        return r[:2] == ("n0003", ["b3"]) and r[3] == 5 and r[4] == 0
    return _scene("violations_level", 5, rows, [pdb("guard", app="a")], ["no_violation_level"], claim)


def high_is_first() -> PdbScene:
    """Node 0's list is [b1 (20, violating), b0 (60)]: level 2 reads 20, not 60,
    and beats node 1's single violating victim of priority 30."""
    rows = [(0, 60, 100, 2500, NONE), (0, 20, 100, 2500, A), (1, 30, 100, 2500, A), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0000", ["b1", "b0"]) and r[4] == 1 and _prio(sc, r[1][0]) < max(_prio(sc, v) for v in r[1])
    return _scene("high_is_first", 3, rows, [pdb("guard", app="a")], ["high_is_max"], claim)


def early_true_max() -> PdbScene:
    """Two nodes tie down to level 4 with lists [(20, violating), (60)].  Level
    5 reads the start of the priority-60 victims (50 against 200: node 1 is
    later and wins); the starts of the priority-20 ones (300 against 10) say
    the opposite."""
    rows = [(0, 60, 50, 2500, NONE), (0, 20, 300, 2500, A), (1, 60, 200, 2500, NONE), (1, 20, 10, 2500, A), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0001", ["b3", "b2"]) and r[4] == 1
    return _scene("early_true_max", 3, rows, [pdb("guard", app="a")], ["early_sorted_shortcut"], claim)


# ---- SelectVictimsOnNode ----------------------------------------------------------------------
def violating_first() -> PdbScene:
    """Node 0 has room for one 2-CPU pod beside the preemptor.  The violating
    pod of priority 40 is reprieved before the ordinary one of priority 50,
    which becomes the victim, without a violation."""
    rows = [(0, 50, 100, 2000, NONE), (0, 40, 100, 2000, A), (1, 2000, 100, 9000, NONE), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0000", ["b0"]) and r[4] == 0 and _prio(sc, "b1") < _prio(sc, "b0")
    return _scene("violating_first", 3, rows, [pdb("guard", app="a")], ["violating_not_first"], claim)


def count_after_reprieve() -> PdbScene:
    """Node 0's violating pod (1 CPU) is reprieved, so the node counts no
    violation and wins at level 2 (50 below node 1's 70)."""
    rows = [(0, 50, 100, 2500, NONE), (0, 40, 100, 1000, A), (1, 70, 100, 2500, NONE), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0000", ["b0"]) and r[4] == 0
    return _scene("count_after_reprieve", 3, rows, [pdb("guard", app="a")], ["violations_before_reprieve"], claim)


def budget_per_node() -> PdbScene:
    """One budget with disruptionsAllowed 1 and an A pod on each of two nodes:
    each node's dry run starts from 1, so neither violates and node 1's lower
    victim priority wins."""
    rows = [(0, 50, 100, 2500, A), (1, 10, 100, 2500, A), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0001", ["b1"]) and r[4] == 0 and sc.pdbs[0].disruptions_allowed == 1
    return _scene("budget_per_node", 3, rows, [pdb("guard", 1, app="a")], ["shared_budgets"], claim)


def allowed_one_two_pods() -> PdbScene:
    """disruptionsAllowed 1 and two A pods on one node: the more important one
    takes the budget, the other violates and leads the list."""
    rows = [(0, 60, 100, 2500, A), (0, 50, 100, 2500, A), (1, 2000, 100, 9000, NONE), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0000", ["b1", "b0"]) and r[4] == 1
    return _scene("allowed_one_two_pods", 3, rows, [pdb("guard", 1, app="a")], [], claim)


def outranking_consume_nothing() -> PdbScene:
    """Node 0 holds an A pod that outranks the preemptor and one below it;
    disruptionsAllowed 1 goes to the lower one alone.  Everything ties with
    node 1, so the first node wins."""
    rows = [(0, 2000, 100, 1000, A), (0, 50, 100, 2500, A), (1, 50, 100, 2500, NONE), OUTRANKS]

    def claim(sc, r):
        return r[:2] == ("n0000", ["b1"]) and r[4] == 0 and _prio(sc, "b0") >= PRIO
    return _scene("outranking_consume_nothing", 3, rows, [pdb("guard", 1, app="a")], ["higher_priority_consume"], claim)


def nominated_consume_nothing() -> PdbScene:
    """The same with the outranking A pod nominated on node 0 instead of bound."""
    rows = [(0, 50, 100, 2500, A), (1, 50, 100, 2500, NONE), OUTRANKS]
    nom = Pod("nominated", priority=1500, labels=dict(A), containers=[Container({"cpu": "1000m"})])

    def claim(sc, r):
        return r[:2] == ("n0000", ["b0"]) and r[4] == 0
    return _scene("nominated_consume_nothing", 3, rows, [pdb("guard", 1, app="a")], ["nominated_consume"], claim,
                  pods=[ac.preemptor(8000), nom], nominated={"n0000": [1]})


def two_budgets() -> PdbScene:
    """b0 matches both budgets and decrements both: ``tier`` (allowed 1) is used
    up when b1 comes, which violates.  ``app`` allows more than the node holds.
    Node 1's clean victim of priority 70 wins at level 1."""
    rows = [(0, 60, 100, 2500, AT), (0, 50, 100, 2500, T), (1, 70, 100, 2500, NONE), OUTRANKS]

    def claim(sc, r):
        both = preemptpdbref.matching(sc.bound[0], sc.pdbs)
        return r[:2] == ("n0001", ["b2"]) and r[4] == 0 and both == [0, 1] and sc.pdbs[0].disruptions_allowed > 2
    return _scene("two_budgets", 3, rows, [pdb("app", 5, app="a"), pdb("tier", 1, tier="t")], ["two_pdbs_once"], claim)


# ---- the match rule ---------------------------------------------------------------------------
def _first_node_is_clean(sc, r):
    return r[:2] == ("n0000", ["b0"]) and r[4] == 0


def other_namespace() -> PdbScene:
    """b0 lives in another namespace than the budget: no match, node 0 ties with
    node 1 and comes first."""
    sc = _scene("other_namespace", 3, [(0, 50, 100, 2500, A), (1, 50, 100, 2500, NONE), OUTRANKS],
                [pdb("guard", app="a")], ["namespace_ignored"], _first_node_is_clean)
    sc.bound[0].namespace = "other"
    return sc


def empty_selector() -> PdbScene:
    """An empty selector and a nil one select nothing here."""
    pdbs = [PodDisruptionBudget("empty", "default", LabelSelector(), 0), PodDisruptionBudget("nil", "default", None, 0)]
    return _scene("empty_selector", 3, [(0, 50, 100, 2500, A), (1, 50, 100, 2500, NONE), OUTRANKS], pdbs,
                  ["empty_selector_matches"], _first_node_is_clean)


def unlabelled_pod() -> PdbScene:
    """The selector `x DoesNotExist` matches an empty label set, but a pod
    without labels is skipped before any selector is tried.  Node 1's pod
    carries x, so it matches under no reading."""
    sel = LabelSelector({}, [Requirement("x", "DoesNotExist", [])])
    return _scene("unlabelled_pod", 3, [(0, 50, 100, 2500, NONE), (1, 50, 100, 2500, {"x": "1"}), OUTRANKS],
                  [PodDisruptionBudget("nox", "default", sel, 0)], ["unlabelled_matches"], _first_node_is_clean)


def disrupted_pod() -> PdbScene:
    """b0 is a key of status.disruptedPods: the budget already counted it."""
    return _scene("disrupted_pod", 3, [(0, 50, 100, 2500, A), (1, 50, 100, 2500, NONE), OUTRANKS],
                  [pdb("guard", disrupted=["b0"], app="a")], ["disrupted_not_excluded"], _first_node_is_clean)


# ---- the three kernel forms ---------------------------------------------------------------------
def ports_form() -> PdbScene:
    """A host-port preemptor (1 CPU; the ports form of k_preempt_nodes): the
    holders of port 80 must go.  Node 0's holder is an A pod, node 1's is not
    and has the higher priority: level 1 picks node 1.  Node 3 holds the port
    with two pods, the violating one leads its list."""
    port = {"ports": [(80, "TCP", "")]}
    rows = [(0, 10, 100, 1000, A, port), (0, 5, 100, 1000, NONE), (1, 50, 100, 1000, NONE, port),
            (2, 2000, 100, 1000, NONE, port), (3, 60, 100, 1000, NONE, port), (3, 20, 100, 1000, A, port)]
    p = ac.preemptor(1000)
    p.containers[0].ports = [ContainerPort(80, "TCP", "")]

    def claim(sc, r):
        return r == ("n0001", ["b2"], 4, 3, 0)
    return _scene("ports_form", 5, rows, [pdb("guard", app="a")], ["no_violation_level"], claim, pods=[p],
                  kinds=("NODE_PORT",))


def anti_affinity_form() -> PdbScene:
    """A zone anti-affinity preemptor (the domain form): za's only x pod is
    guarded by the budget, zb's is not and has the higher priority.  Level 1
    picks zb's holder."""
    rows = [(1, 10, 100, 1000, {"app": "x", "guard": "y"}), (1, 5, 90, 1000, NONE), (0, 5, 100, 1000, NONE),
            (4, 20, 100, 1000, {"app": "x"}), (3, 5, 100, 1000, NONE), (5, 5, 100, 1000, {"guard": "y"})]

    def claim(sc, r):
        return r == ("n0004", ["b3"], 6, 2, 0)
    return _scene("anti_affinity_form", 6, rows, [pdb("guard", guard="y")], ["no_violation_level"], claim,
                  pods=[ac.preemptor(anti=[ac.term(ac.ZONE, app="x")])], zones={"za": 3, "zb": 3}, kinds=("IPA_ANTI",))


# ---- many budgets -----------------------------------------------------------------------------------
def three_hundred_budgets() -> PdbScene:
    """70 nodes, four pods each, 300 budgets (no mask could hold them): pod i
    carries id=i%300 and, every third one, group=i%7; budget k < 293 selects
    id=k, the last seven select group=0..6, so a third of the pods sit in two
    budgets.  disruptionsAllowed runs over 0, 1 and 9 (more than a node
    holds)."""
    rows = []
    for v in range(70):
        for j in range(4):
            i = len(rows)
            labels = {"id": str(i % 300)}
            if i % 3 == 0:
                labels["group"] = str(i % 7)
            rows.append((v, 10 + (i * 7) % 50, 100 + (i * 13) % 40, 2500 if j < 3 else 1500, labels))
    pdbs = [pdb(f"id{k}", (0, 1, 9)[k % 3], id=str(k)) for k in range(293)]
    pdbs += [pdb(f"group{g}", g % 2, group=str(g)) for g in range(7)]

    def claim(sc, r):
        twice = sum(1 for p in sc.bound if len(preemptpdbref.matching(p, sc.pdbs)) == 2)
        return len(sc.pdbs) == 300 and twice > 50 and r[0] is not None and r[2] == 70
    return _scene("three_hundred_budgets", 70, rows, pdbs, [], claim)


# ---- the cut ------------------------------------------------------------------------------------------
def small_cut() -> PdbScene:
    """numCandidates 2; the first three candidates violate, the fourth is the
    first clean one and ends the scan; the fifth (the best below level 1) is
    never tried."""
    rows = [(v, 50, 100, 2500, A if v < 3 else NONE) for v in range(4)] + [(4, 10, 100, 2500, NONE), (5, 50, 100, 2500, NONE)]

    def claim(sc, r):
        return r == ("n0003", ["b3"], 6, 4, 0) and r[3] > sc.want
    return _scene("small_cut", 6, rows, [pdb("guard", app="a")], ["old_cut"], claim, args=(0, 2), want=2)


CUT_WANT = 25                                        # above 1 % of 2,049 potential nodes


def cut_positions(n: int) -> List[int]:
    """Where the first clean candidate sits: the last node of a k_preempt_pick
    thread's chunk and the first of the next, and the same either side of a
    64-thread wave's range of nodes; all past numCandidates."""
    chunk = (n + PICK_THREADS - 1) // PICK_THREADS
    at_chunk = (CUT_WANT // chunk + 2) * chunk       # first node of a chunk beyond the cut
    at_wave = WAVE * chunk                           # first node of the second wave
    return sorted({at_chunk - 1, at_chunk, at_wave - 1, at_wave})


def cut_scene(n: int, c: int) -> PdbScene:
    """``n`` nodes, every one a candidate with one victim.  Nodes [0, c) evict an
    A pod (violating), node c is the first clean one: the scan keeps c + 1
    candidates, far past numCandidates = 25, and picks node c.  Node c - 1
    (violating, victim priority 5) is the best by levels 2 to 6 and lies past
    the old cut; node c + 1 (clean, priority 1) would beat node c and is cut."""
    assert CUT_WANT <= c - 1 and c + 1 < n
    rows = [(v, 5 if v == c - 1 else 1 if v == c + 1 else 50, 100, 2500, A if v < c else NONE) for v in range(n)]

    def claim(sc, r):
        return r == (f"n{c:04d}", [f"b{c}"], n, c + 1, 0) and r[3] > sc.want
    return _scene(f"cut_n{n}_at{c}", n, rows, [pdb("guard", app="a")], ["old_cut", "no_violation_level"], claim,
                  args=(1, CUT_WANT), want=CUT_WANT)


CUT_N = (1023, 1024, 1025, 2049)


def _small() -> List[PdbScene]:
    return [violations_level(), high_is_first(), early_true_max(), violating_first(), count_after_reprieve(),
            budget_per_node(), allowed_one_two_pods(), outranking_consume_nothing(), nominated_consume_nothing(),
            two_budgets(), other_namespace(), empty_selector(), unlabelled_pod(), disrupted_pod(), ports_form(),
            anti_affinity_form(), three_hundred_budgets(), small_cut()]


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, PdbScene]:
    out = _small() + [cut_scene(n, c) for n in CUT_N for c in cut_positions(n)]
    table = {s.name: s for s in out}
    assert len(table) == len(out)
    return table


def scene_ids() -> List[str]:
    return list(scenes())


def small_ids() -> List[str]:
    return [s.name for s in _small()]


@functools.lru_cache(maxsize=None)
def reference(name: str, grouped: bool = False, fault: Optional[str] = None) -> tuple:
    """preemptpdbref.dry_run on a scene (names, not positions); computed once
    and shared by the CPU and the GPU tests."""
    sc = scenes()[name]
    if grouped:
        sc = sc.grouped()
    return preemptpdbref.dry_run(sc.nodes, sc.bound, sc.start, sc.order, sc.pods[0], PRIO, sc.args,
                                 sc.nominated_pods(), sc.pdbs, fault)
