"""Designed scenes for the per-pod cycle (csrc/ksim_kernels.hip: k_window,
k_extrema, k_select / bind_cycle, k_fw_normalize and the sharded k_wcount_sh,
k_window_sh, k_wfinal_sh, k_best_pack, k_bind_sh; normalize_value in
csrc/ksim_device.h).  The random generators reach a given window geometry, a
given extremum holder or a given tie only by luck; these scenes put them there.

Scenes are ksim.model objects, so every feasibility bit and raw score is known
by construction: a node is full (allocatable pods 0) or roomy, carries the
labels that preferred node-affinity terms of chosen weights match, a count of
PreferNoSchedule taints nobody tolerates, bound pods that preferred pod
(anti-)affinity terms or ScheduleAnyway constraints count, and the key labels
of those constraints or not.  No node carries a zone label unless the scene
says so, so nodeTree order is input order and positions are the node numbers.

Every scene sets nextStartNodeIndex and the pod sequence itself, names the
launch form its schedule_loaded run must take (``cycle_form`` restates the
host's choice: launch_cycle, run_range, shard_cycle) and carries its claimed
property as a predicate over tests/cycleref.py's results.

How a scene reaches the per-pod path (``route``):
  port   every queue pod holds a host port nobody else holds (pod_batchable
         returns 0 for a use that is no image use); works on any handle
  ab     the "ab" flavor sends ADAPT pods whose normalized scores vary there
         without a use: the windowed cycle without topology kernels
  shard  node shards take normalized-score pods there anyway (the sharded
         runs use the port scenes as they are)

tests/test_cycle_cases.py proves on the CPU that the model equals the C oracle
on every scene, that every scene has its property and that the scenes tell
cycleref.FAULTS apart; tests/test_gpu_cycle_edges.py runs them on the GPU."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.model import (Container, ContainerPort, Controller, LabelSelector, Node, NodeSelectorTerm, Pod,
                        PodAffinityTerm, PreferredTerm, Requirement, Taint, TopologySpreadConstraint,
                        WeightedPodAffinityTerm)
from ksim.topology import SpreadDefaults
from oracle.oracle import Oracle

import cycleref
from cycleref import DEFAULT, MINMAX, NONE, PTS, REVERSE, Inputs, SoftUse

HOST = "kubernetes.io/hostname"
ZONE = "topology.kubernetes.io/zone"
RACK = "example.com/rack"
SEED = 0x4B53494D
SEED2 = 0x5EED5EED

KIND_OF = {"TaintToleration": REVERSE, "NodeAffinity": DEFAULT, "PodTopologySpread": PTS, "InterPodAffinity": MINMAX}
SCORE_NAMES = [p.name for p in profile.SchedulerProfile().score_plugins()]
SLOT = {name: i for i, name in enumerate(SCORE_NAMES)}
KINDS = [KIND_OF.get(name, NONE) for name in SCORE_NAMES]
NA, TT, IPA, SPREAD = SLOT["NodeAffinity"], SLOT["TaintToleration"], SLOT["InterPodAffinity"], SLOT["PodTopologySpread"]

GRAPH_CYCLES = 128                                 # csrc/ksim_engine.cpp kGraphCycles
WINDOW_THREADS = 1024                              # csrc/ksim_kernels.hip kFinalThreads: k_window's chunks


def cycle_form(n_nodes: int, pct: int, soft_uses: Sequence[int], sharded: bool = False, compat: bool = False) -> str:
    """The host's choice of launch form for a per-pod run whose pods carry
    ``soft_uses`` ScheduleAnyway constraints each (csrc/ksim_kernels.hip
    launch_cycle / launch_cycle_t, csrc/ksim_engine.cpp run_range; the profile
    has no NetworkBandwidth): K from the cluster's node count, the fused form
    only when every pod of the run has at most one soft use, never in COMPAT."""
    if sharded:
        return "sharded"
    nowin = cycleref.num_feasible_nodes_to_find(n_nodes, pct) >= n_nodes
    if not nowin:
        return "windowed"
    if compat or any(u > 1 for u in soft_uses):
        return "nowin_unfused"
    return "nowin_fused"


# kernels of a per-pod run by form (Engine.time_kernels)
FORM_KERNELS = {"windowed": (True, True), "nowin_unfused": (False, True), "nowin_fused": (False, False)}


@dataclass
class Scene:
    name: str
    nodes: List[Node]
    queue: List[Pod]
    form: str                                      # the form schedule_loaded must take
    claim: Callable[["Scene", List[dict]], bool]   # over cycleref.finish of every pod
    bound: List[Pod] = field(default_factory=list)
    pct: int = 0
    weights: Optional[Dict[str, int]] = None
    seed: int = SEED
    s0: int = 0
    seq0: int = 0
    route: str = "port"
    worlds: Tuple[int, ...] = ()                   # node-shard groups it also runs on
    ext: Optional[Callable[[int], Tuple[Optional[np.ndarray], Optional[np.ndarray]]]] = None
    defaults: bool = False                         # system-defaulted spread constraints (a ReplicaSet owns the pods)
    schedule: bool = True                          # runs through schedule_loaded (not the extender scenes)

    @property
    def n(self) -> int:
        return len(self.nodes)

    @property
    def k(self) -> int:
        return cycleref.num_feasible_nodes_to_find(self.n, self.pct)

    @functools.cached_property
    def sp(self) -> profile.SchedulerProfile:
        sp = profile.SchedulerProfile(percentage_of_nodes_to_score=self.pct, tiebreak_seed=self.seed)
        return sp.with_weights({**{n: 1 for n in SCORE_NAMES}, **self.weights}) if self.weights else sp

    @functools.cached_property
    def prof(self):
        return profile.compile_profile(self.sp)

    @functools.cached_property
    def encoded(self):
        """(cluster, pods); tests take copy_state() of the cluster."""
        cluster, order = encode_cluster(self.nodes, self.bound)
        if not any(ZONE in n.labels for n in self.nodes):
            assert order == list(range(self.n)), self.name
        spread = SpreadDefaults(self.sp.spread, [], [Controller("ReplicaSet", "rs", "default",
                                                                  LabelSelector({"app": "rs"}))]) \
            if self.defaults else None
        pods = encode_pods(cluster, self.queue, spread=spread)
        return cluster, pods

    @functools.cached_property
    def soft_uses(self) -> List[int]:
        _, pods = self.encoded
        out = []
        for p in pods.pods:
            u = pods.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
            out.append(int((u["kind"] == abi.USE_PTS_SOFT).sum()))
        return out

    def restated_form(self, sharded: bool = False, compat: bool = False) -> str:
        return cycle_form(self.n, self.pct, self.soft_uses, sharded, compat)

    def extender(self):
        return self.ext(self.n) if self.ext else (None, None)


# ---- the scenes' inputs, read off the oracle's Filter / Score of every node -----------------
class Feed:
    """Per-pod inputs of the model under the binds so far: the C oracle's
    Filter of every node of the scan and Score of every feasible node (both
    leave the scheduler state alone), its count classes, and the pod's uses."""

    def __init__(self, scene: Scene):
        self.scene = scene
        cluster, self.pods = scene.encoded
        self.cluster = cluster.copy_state()
        self.ora = Oracle(self.cluster, scene.prof)
        self.weights = [int(scene.prof.score_weight[s]) for s in range(scene.prof.n_score)]

    def inputs(self, j: int) -> Inputs:
        c, pods = self.cluster, self.pods
        p = pods.pods[j]
        f = self.ora.fw_prefilter(pods, j)
        feasible = f["fail_plugin"] == abi.PASSED
        raw = np.zeros((len(KINDS), c.n_nodes), np.int64)
        if feasible.any():
            raw = self.ora.fw_score(np.nonzero(feasible)[0])["raw"]
        cc = self.ora.class_count()
        uses = pods.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
        soft, nonempty = [], False
        for u in uses:
            col = int(u["col"])
            value = c.labels[col].astype(np.int64) if col != abi.COL_NONE else np.zeros(c.n_nodes, np.int64)
            if u["kind"] == abi.USE_PTS_SOFT:
                # the inclusion policies: no queue pod of a spread scene has a node selector or required terms
                assert int(p["sel_count"]) == 0 and int(p["req_term_count"]) == 0 and \
                    not (int(u["flags"]) & abi.USEF_HONOR_TAINTS)
                soft.append(SoftUse(value, cc[int(u["cls"])].astype(np.int64), int(u["arg"]),
                                    bool(int(u["flags"]) & abi.USEF_HOSTNAME)))
            elif u["kind"] in (abi.USE_IPA_SCORE, abi.USE_IPA_SCORE_HARD):
                nonempty = nonempty or bool(((value != 0) & (cc[int(u["cls"])] != 0)).any())
        flags = int(p["flags"])
        scan = None
        if flags & abi.POD_NODE_NAMES:
            scan = [int(x) for x in pods.nn[int(p["nn_first"]):int(p["nn_first"]) + int(p["nn_count"])]]
        ef, es = self.scene.extender()
        return Inputs(c.n_nodes, feasible, raw, KINDS, self.weights, scan, bool(flags & abi.POD_NODE_NAMES_UNKNOWN),
                      soft, bool(int(p["topo_flags"]) & abi.POD_PTS_SYSTEM_DEFAULT), nonempty, ef, es,
                      f["fail_plugin"])

    def bound(self, j: int, node: int) -> None:
        self.ora.assume(self.pods, j, node)


def reference(scene: Scene, fault: Optional[str] = None, keep_inputs: bool = False):
    """cycleref.schedule over the scene's queue.  Returns the Run (and the
    inputs of every pod when asked)."""
    feed = Feed(scene)
    seen: List[Inputs] = []

    def inputs_of(j):
        inp = feed.inputs(j)
        if keep_inputs:
            seen.append(inp)
        return inp

    cluster, pods = scene.encoded
    run = cycleref.schedule(cluster, pods, inputs_of, feed.bound, scene.pct, scene.seed, scene.s0, scene.seq0, fault)
    return (run, seen) if keep_inputs else run


@functools.lru_cache(maxsize=None)
def truth(name: str):
    """(Run, inputs per pod) of the right reading, computed once."""
    return reference(scene(name), None, True)


# ---- building blocks ---------------------------------------------------------------------------
def node(i: int, labels: Optional[dict] = None, taints: int = 0, full: bool = False, pods: int = 110,
         host: bool = True) -> Node:
    name = f"n{i:05d}"
    lb = {HOST: name} if host else {}
    lb.update(labels or {})
    return Node(name, lb, [Taint(f"soft{t}", "", "PreferNoSchedule") for t in range(taints)],
                {"cpu": "64", "memory": "256Gi", "pods": "0" if full else str(pods)})


def ring(n: int, full=(), labels: Optional[Dict[int, dict]] = None, taints: Optional[Dict[int, int]] = None,
         pods: int = 110, nohost=()) -> List[Node]:
    full, labels, taints, nohost = set(full), labels or {}, taints or {}, set(nohost)
    return [node(i, labels.get(i), taints.get(i, 0), i in full, pods, i not in nohost) for i in range(n)]


def qpod(j: int, prefer: Sequence[Tuple[int, str, str]] = (), affinity: Sequence[Tuple[int, str, str]] = (),
         anti: Sequence[Tuple[int, str, str]] = (), spread: Sequence[Tuple[int, str, str]] = (), names=None,
         port: bool = True, labels: Optional[dict] = None, owner=None, cpu: str = "100m") -> Pod:
    """Queue pod j.  prefer: (weight, label key, value) preferred node-affinity
    terms; affinity / anti: (weight, topology key, app) preferred pod terms;
    spread: (maxSkew, topology key, app) ScheduleAnyway constraints; names: a
    PreFilterResult list (metadata.name In ...)."""
    sel = lambda app: LabelSelector({"app": app})                                      # noqa: E731
    p = Pod(f"q{j:04d}", labels=dict(labels or {}), owner=owner,
            containers=[Container({"cpu": cpu, "memory": "128Mi"},
                                  [ContainerPort(20000 + j)] if port else [])])
    p.preferred_terms = [PreferredTerm(w, NodeSelectorTerm([Requirement(k, "In", [v])])) for w, k, v in prefer]
    p.pod_affinity_preferred = [WeightedPodAffinityTerm(w, PodAffinityTerm(k, sel(a))) for w, k, a in affinity]
    p.pod_anti_affinity_preferred = [WeightedPodAffinityTerm(w, PodAffinityTerm(k, sel(a))) for w, k, a in anti]
    p.topology_spread = [TopologySpreadConstraint(m, k, "ScheduleAnyway", sel(a)) for m, k, a in spread]
    if names is not None:
        # a field selector takes one value: one term per name (their union is the list, in name order)
        p.required_terms = [NodeSelectorTerm(match_fields=[Requirement("metadata.name", "In", [x])]) for x in names]
    return p


def bpods(app: str, counts: Dict[int, int]) -> List[Pod]:
    """counts[node] bound pods labelled app on each node (they request nothing)."""
    return [Pod(f"b-{app}-{i}-{c}", labels={"app": app}, containers=[Container({})], node_name=f"n{i:05d}")
            for i, cnt in counts.items() for c in range(cnt)]


def name_of(i: int) -> str:
    return f"n{i:05d}"


SCENES: Dict[str, Callable[[], Scene]] = {}


def scene_fn(f):
    SCENES[f.__name__] = f
    return f


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    s = SCENES[name]() if name in SCENES else PARAM[name]()
    assert s.name == name, (s.name, name)
    return s


PARAM: Dict[str, Callable[[], Scene]] = {}
PREFER_A = [(3, "tier", "gold")]


def _every(rs, pred) -> bool:
    return all(pred(r) for r in rs)


# ---- window scenes ---------------------------------------------------------------------------------
@scene_fn
def exactly_k():
    """101 nodes, exactly 100 feasible: no cut, the whole ring processed."""
    return Scene("exactly_k", ring(101, full=[50], labels={3: {"tier": "gold"}}), [qpod(0, PREFER_A), qpod(1, PREFER_A)],
                 "windowed", s0=7, worlds=(2, 3, 8),
                 claim=lambda s, rs: _every(rs, lambda r: r["cut"] < 0 and r["n_processed"] == 101 and
                                            r["n_feasible"] == 100 == s.k and r["next_start"] == 7))


def _k_plus_1(s0):
    def build():
        last = (s0 + 100) % 101
        return Scene(f"exactly_k_plus_1_s{s0}", ring(101, labels={last: {"tier": "gold"}}), [qpod(0, PREFER_A)],
                     "windowed", s0=s0, worlds=(2, 3, 8) if s0 == 50 else (),
                     claim=lambda s, rs: rs[0]["cut"] == last and rs[0]["n_evaluated"] == 101 and
                     rs[0]["n_processed"] == 100 and rs[0]["next_start"] == (s0 + 100) % 101 and
                     rs[0]["chosen"] != last)
    return build


for _s0 in (0, 1, 50, 100):
    PARAM[f"exactly_k_plus_1_s{_s0}"] = _k_plus_1(_s0)


def _best(n, s0, holder, name, worlds=()):
    """Node ``holder`` carries the highest raw score of every normalized slot
    (both preferred labels, three taints, the bound pods an affinity term
    counts); kept nodes hold smaller ones."""
    labels = {holder: {"tier": "gold", "disk": "ssd"}, (s0 + 3) % n: {"tier": "gold"}, (s0 + 40) % n: {"disk": "ssd"}}
    taints = {holder: 3, (s0 + 5) % n: 1, (s0 + 41) % n: 2}
    bound = bpods("db", {holder: 4, (s0 + 7) % n: 1, (s0 + 42) % n: 2})
    q = [qpod(0, [(3, "tier", "gold"), (2, "disk", "ssd")], affinity=[(5, HOST, "db")])]

    def claim(s, rs):
        r, inp = rs[0], truth(name)[1][0]
        outside = holder not in r["kept"]
        tops = all(int(inp.raw[x][holder]) > max(int(inp.raw[x][m]) for m in r["kept"]) for x in (NA, TT, IPA))
        return outside and tops and r["chosen"] != holder and r["cut"] == (s0 + s.k) % n
    return Scene(name, ring(n, labels=labels, taints=taints), q, "windowed", claim, bound=bound, s0=s0, worlds=worlds)


@scene_fn
def cut_holds_best():
    return _best(120, 10, 110, "cut_holds_best")


@scene_fn
def max_past_cut():
    return _best(120, 10, 115, "max_past_cut")


@scene_fn
def sparse_feasibility():
    """Every third node full: scan position and feasible rank differ."""
    full = [i for i in range(200) if i % 3 == 1]
    return Scene("sparse_feasibility", ring(200, full=full, labels={8: {"tier": "gold"}}),
                 [qpod(j, PREFER_A) for j in range(3)], "windowed", s0=5,
                 claim=lambda s, rs: _every(rs, lambda r: r["cut"] >= 0 and r["n_evaluated"] > s.k + 1 and
                                            r["n_processed"] == r["n_evaluated"] - 1))


@scene_fn
def wrapped_cut():
    return Scene("wrapped_cut", ring(150, labels={120: {"tier": "gold"}, 60: {"tier": "gold"}}), [qpod(0, PREFER_A)],
                 "windowed", s0=100,
                 claim=lambda s, rs: rs[0]["cut"] == 50 and rs[0]["chosen"] == 120 and rs[0]["next_start"] == 50)


@scene_fn
def start_on_last_node():
    return Scene("start_on_last_node", ring(150, labels={149: {"tier": "gold"}}), [qpod(0, PREFER_A), qpod(1, PREFER_A)],
                 "windowed", s0=149,
                 claim=lambda s, rs: rs[0]["kept"][0] == 149 and rs[0]["cut"] == 99 and rs[0]["chosen"] == 149 and
                 rs[1]["kept"][0] == 99)


@scene_fn
def start_on_infeasible():
    return Scene("start_on_infeasible", ring(150, full=[140, 141, 20]), [qpod(0, PREFER_A)], "windowed", s0=140,
                 claim=lambda s, rs: rs[0]["kept"][0] == 142 and rs[0]["cut"] == (140 + 103) % 150 and
                 rs[0]["n_evaluated"] == 104)


@scene_fn
def none_feasible():
    return Scene("none_feasible", ring(120, full=range(120)), [qpod(0), qpod(1)], "windowed", s0=17, worlds=(2,),
                 claim=lambda s, rs: _every(rs, lambda r: r["status"] == cycleref.STATUS_UNSCHEDULABLE and
                                            r["n_evaluated"] == 120 and r["next_start"] == 17))


@scene_fn
def one_feasible():
    """One feasible node: scheduled unscored (totals and ``scored`` 0)."""
    return Scene("one_feasible", ring(101, full=[i for i in range(101) if i != 33], labels={33: {"tier": "gold"}}),
                 [qpod(0, PREFER_A)], "windowed", s0=40, worlds=(3,),
                 claim=lambda s, rs: rs[0]["chosen"] == 33 and not rs[0]["scored"].any() and not rs[0]["total"].any())


@scene_fn
def two_equal():
    return Scene("two_equal", ring(101, full=[i for i in range(101) if i not in (12, 77)]),
                 [qpod(j) for j in range(2)], "windowed", s0=30, seq0=5,
                 claim=lambda s, rs: rs[0]["total"][12] == rs[0]["total"][77] > 0 and rs[0]["n_feasible"] == 2)


def _threshold(n, pct):
    def build():
        k = cycleref.num_feasible_nodes_to_find(n, pct)
        form = "windowed" if k < n else "nowin_fused"
        return Scene(f"threshold_{n}_pct{pct}", ring(n, labels={n - 1: {"tier": "gold"}, 2: {"tier": "gold"}}),
                     [qpod(0, PREFER_A), qpod(1, PREFER_A)], form, pct=pct, s0=n - 2,
                     claim=lambda s, rs: rs[0]["k_to_find"] == k and (rs[0]["cut"] >= 0) == (k < n))
    return build


THRESHOLDS = [(99, 0), (100, 0), (101, 0), (101, 100), (200, 50), (200, 99)]
for _n, _p in THRESHOLDS:
    PARAM[f"threshold_{_n}_pct{_p}"] = _threshold(_n, _p)


def _chunk(n, pos, s0):
    """The (K + 1)-th feasible node at scan position ``pos``: the first K scan
    positions and ``pos`` feasible, the positions between them full."""
    def build():
        k = cycleref.num_feasible_nodes_to_find(n, 0)
        full = [(s0 + i) % n for i in range(k, pos)]
        cut = (s0 + pos) % n
        return Scene(f"chunk_{n}_at{pos}_s{s0}", ring(n, full=full, labels={(s0 + k - 1) % n: {"tier": "gold"}}),
                     [qpod(0, PREFER_A), qpod(1, PREFER_A)], "windowed", s0=s0,
                     claim=lambda s, rs: rs[0]["cut"] == cut and rs[0]["n_evaluated"] == pos + 1 and
                     rs[0]["n_processed"] == pos and rs[0]["chosen"] == (s0 + k - 1) % n and
                     rs[1]["kept"][0] == cut)
    return build


CHUNKS = [(1024, 1022, 0), (1024, 1023, 0), (1024, 1023, 5), (1025, 1022, 0), (1025, 1023, 0), (1025, 1024, 0),
          (1025, 1024, 1000), (2049, 2046, 0), (2049, 2048, 0), (2049, 2046, 700)]
for _n, _pos, _s in CHUNKS:
    PARAM[f"chunk_{_n}_at{_pos}_s{_s}"] = _chunk(_n, _pos, _s)


# ---- PreFilterResult lists ------------------------------------------------------------------------
@scene_fn
def list_3_of_300():
    """3 of 300 nodes with an incoming start past the list's length."""
    names = [name_of(i) for i in (250, 20, 130)]
    return Scene("list_3_of_300", ring(300, labels={130: {"tier": "gold"}}),
                 [qpod(0, PREFER_A, names=names), qpod(1, names=names)], "windowed", s0=7,
                 claim=lambda s, rs: rs[0]["k_to_find"] == 3 and rs[0]["n_evaluated"] == 3 and
                 rs[0]["next_start"] == 1 and rs[0]["chosen"] == 130 and rs[0]["kept"][0] == 130)


@scene_fn
def list_150_of_300():
    """150 scattered nodes: K = 100 of the 150, a cut inside the list."""
    picks = [i for i in range(300) if i % 2 == 1]
    return Scene("list_150_of_300", ring(300, labels={picks[40]: {"tier": "gold"}, picks[145]: {"tier": "gold"}}),
                 [qpod(0, PREFER_A, names=[name_of(i) for i in picks]), qpod(1, PREFER_A)], "windowed", s0=200,
                 claim=lambda s, rs: rs[0]["k_to_find"] == 100 and rs[0]["kept"][0] == picks[50] and
                 rs[0]["cut"] == picks[0] and rs[0]["next_start"] == 0 and rs[0]["chosen"] == picks[145])


@scene_fn
def list_unknown_node():
    return Scene("list_unknown_node", ring(300), [qpod(0, names=[name_of(5), "nowhere"]), qpod(1)], "windowed", s0=211,
                 claim=lambda s, rs: rs[0]["chosen"] == cycleref.CHOSEN_ERROR and rs[0]["n_evaluated"] == 0 and
                 rs[0]["next_start"] == 211 and rs[1]["kept"][0] == 211)


@scene_fn
def list_all_fail():
    return Scene("list_all_fail", ring(300, full=[10, 11, 12, 13]),
                 [qpod(0, names=[name_of(i) for i in (10, 11, 12, 13)]), qpod(1)], "windowed", s0=209,
                 claim=lambda s, rs: rs[0]["status"] == cycleref.STATUS_UNSCHEDULABLE and rs[0]["n_evaluated"] == 4 and
                 rs[0]["next_start"] == (209 + 4) % 4 and rs[1]["kept"][0] == 1)


@scene_fn
def list_alternating():
    """Listed and plain pods in turn: the start carries across both moduli."""
    names = [name_of(i) for i in range(30, 37)]
    q = [qpod(j, PREFER_A, names=names if j % 2 else None) for j in range(8)]
    return Scene("list_alternating", ring(300, labels={33: {"tier": "gold"}, 199: {"tier": "gold"}}), q, "windowed",
                 s0=296,
                 claim=lambda s, rs: [r["next_start"] for r in rs[:4]] == [140, (140 + 7) % 7, 144, (144 + 7) % 7])


@scene_fn
def captured_run():
    """129 pods on 101 nodes that fill up as it goes (the eleven preferred
    nodes hold twelve pods each): one graph of 128 cycles and a single cycle,
    the window moving by 100 nodes a pod until the first node is full, then
    no cut any more."""
    nodes = [node(i, {"tier": "gold"} if i % 10 == 0 else None, pods=12 if i % 10 == 0 else 110) for i in range(101)]
    return Scene("captured_run", nodes, [qpod(j, PREFER_A) for j in range(129)], "windowed", s0=95,
                 claim=lambda s, rs: len(rs) > GRAPH_CYCLES and {r["n_processed"] for r in rs} == {100, 101} and
                 any(r["cut"] < 0 for r in rs) and any(r["cut"] >= 0 for r in rs))


# ---- NormalizeScore scenes ---------------------------------------------------------------------------
def _norm_of(r, slot, node_):
    return int(r["norm"][slot][node_])


def _default_scene(name, n, pct, form, full=(), worlds=()):
    """NodeAffinity raw 1, 2, 3 (33 / 66 / 100) and 1, 2, 3 untolerated taints (67 / 34 / 0)."""
    labels = {4: {"a": "1"}, 5: {"b": "1"}, 6: {"a": "1", "b": "1"}}
    taints = {7: 1, 8: 2, 9: 3}
    q = [qpod(0, [(1, "a", "1"), (2, "b", "1")])]
    return Scene(name, ring(n, full=full, labels=labels, taints=taints), q, form, pct=pct, s0=2, worlds=worlds,
                 claim=lambda s, rs: [_norm_of(rs[0], NA, i) for i in (4, 5, 6, 10)] == [33, 66, 100, 0] and
                 [_norm_of(rs[0], TT, i) for i in (7, 8, 9, 10)] == [67, 34, 0, 100])


@scene_fn
def default_thirds_nowin():
    return _default_scene("default_thirds_nowin", 60, 100, "nowin_fused")


@scene_fn
def default_thirds_windowed():
    return _default_scene("default_thirds_windowed", 130, 0, "windowed", worlds=(2,))


@scene_fn
def default_zero_max():
    """Terms that match no feasible node (the one node they match is full)
    and no untolerated taint: the raw scores pass, reverse gives 100."""
    return Scene("default_zero_max", ring(60, full=[9], labels={9: {"tier": "gold"}}, taints={9: 2}), [qpod(0, PREFER_A)],
                 "nowin_fused", pct=100, worlds=(2,),
                 claim=lambda s, rs: not rs[0]["norm"][NA].any() and
                 all(_norm_of(rs[0], TT, i) == 100 for i in rs[0]["kept"]))


@scene_fn
def default_weights():
    s = _default_scene("default_weights", 60, 100, "nowin_fused")
    s.weights = {"NodeAffinity": 3, "TaintToleration": 2, "NodeResourcesFit": 0}
    return s


def _ipa_scene(name, bound, q, claim, n=60, pct=100, form="nowin_fused", labels=None, worlds=(), **kw):
    return Scene(name, ring(n, labels=labels), q, form, claim, bound=bound, pct=pct, worlds=worlds, **kw)


@scene_fn
def ipa_anti_only():
    """Maximum 0, negative minimum."""
    return _ipa_scene("ipa_anti_only", bpods("db", {3: 1, 4: 2}), [qpod(0, anti=[(4, HOST, "db")])],
                      lambda s, rs: [_norm_of(rs[0], IPA, i) for i in (3, 4, 5)] == [50, 0, 100] and
                      int(rs[0]["raw"][IPA][4]) == -8)


@scene_fn
def ipa_mixed_signs():
    return _ipa_scene("ipa_mixed_signs", bpods("db", {3: 1, 4: 2}) + bpods("web", {4: 1, 6: 3}),
                      [qpod(0, affinity=[(2, HOST, "web")], anti=[(3, HOST, "db")])],
                      lambda s, rs: [int(rs[0]["raw"][IPA][i]) for i in (3, 4, 6, 7)] == [-3, -4, 6, 0] and
                      [_norm_of(rs[0], IPA, i) for i in (3, 4, 6, 7)] == [10, 0, 100, 40], worlds=(3,))


@scene_fn
def ipa_all_equal():
    """Every kept node equal and non-zero (one rack holds them all): difference 0."""
    return _ipa_scene("ipa_all_equal", bpods("db", {3: 2}), [qpod(0, affinity=[(7, RACK, "db")])],
                      lambda s, rs: set(rs[0]["raw"][IPA][rs[0]["kept"]]) == {14} and not rs[0]["norm"][IPA].any(),
                      labels={i: {RACK: "r0"} for i in range(60)})


@scene_fn
def ipa_empty_topology_score():
    """No matching pod anywhere: the scores pass as they are."""
    return _ipa_scene("ipa_empty_topology_score", bpods("web", {3: 2}), [qpod(0, anti=[(7, HOST, "db")])],
                      lambda s, rs: not truth("ipa_empty_topology_score")[1][0].topology_score_nonempty and
                      not rs[0]["norm"][IPA].any())


@scene_fn
def ipa_float64():
    """(v - min, max - min) = (29, 100), (57, 100), (58, 100) and (29, 50):
    Go's 100 * (x / d) truncates to 28, 56, 57 and 57, integer division gives
    29, 57, 58 and 58."""
    nodes = [node(i, pods=200) for i in range(60)]
    bound = bpods("a", {1: 29, 2: 57, 3: 58, 4: 100}) + bpods("b", {5: 29, 6: 50})
    return Scene("ipa_float64", nodes, [qpod(0, affinity=[(1, HOST, "a")]), qpod(1, affinity=[(1, HOST, "b")])],
                 "nowin_fused", bound=bound, pct=100,
                 claim=lambda s, rs: [_norm_of(rs[0], IPA, i) for i in (1, 2, 3, 4)] == [28, 56, 57, 100] and
                 [_norm_of(rs[1], IPA, i) for i in (5, 6)] == [57, 100])


# PodTopologySpread ScheduleAnyway
def _rack_labels(n, racks, missing=()):
    return {i: {RACK: f"r{i % racks}"} for i in range(n) if i not in set(missing)}


@scene_fn
def pts_hostname_fused():
    """One hostname constraint at K = N (the fused form), maxSkew 3, nodes
    without the hostname label ignored, an ignored node with the fewest pods."""
    bound = bpods("web", {i: 1 + i % 4 for i in range(60) if i != 7})
    return Scene("pts_hostname_fused", ring(60, nohost=[7, 20]), [qpod(j, spread=[(3, HOST, "web")]) for j in range(2)],
                 "nowin_fused", bound=bound, pct=100, worlds=(3,),
                 claim=lambda s, rs: rs[0]["ignored"] == {7, 20} and _norm_of(rs[0], SPREAD, 7) == 0 and
                 rs[0]["sizes"] == [58] and rs[0]["extrema"][SPREAD][0] > 0)


@scene_fn
def pts_rack_small():
    """A rack-keyed constraint on a column of at most 64 values; nodes missing
    the key on several shards; a rack on two shards is one registered pair."""
    missing = [0, 40, 70, 59]
    bound = bpods("web", {i: (i * 7) % 5 for i in range(101)})
    return Scene("pts_rack_small", ring(101, labels=_rack_labels(101, 9, missing)),
                 [qpod(j, spread=[(1, RACK, "web")]) for j in range(2)], "windowed", bound=bound, s0=60,
                 worlds=(2, 3, 8),
                 claim=lambda s, rs: rs[0]["sizes"] == [9] and rs[0]["ignored"] == {0, 40, 70} and
                 rs[0]["cut"] == 59)


@scene_fn
def pts_rack_wide():
    """A column of more than 64 values (the atomic registration path), windowed:
    the nodes past the cut carry racks no kept node has."""
    labels = {i: {RACK: f"r{i}" if i >= 100 else f"r{i % 70}"} for i in range(130)}
    bound = bpods("web", {i: 1 + (i * 3) % 4 for i in range(130)})
    return Scene("pts_rack_wide", ring(130, labels=labels), [qpod(0, spread=[(2, RACK, "web")])], "windowed",
                 bound=bound, s0=0, worlds=(2,),
                 claim=lambda s, rs: rs[0]["sizes"] == [70] and rs[0]["cut"] == 100 and
                 rs[0]["extrema"][SPREAD][0] > 0)


@scene_fn
def pts_two_constraints():
    """Two constraints (the unfused no-window form)."""
    bound = bpods("web", {i: i % 3 for i in range(60)})
    return Scene("pts_two_constraints", ring(60, labels=_rack_labels(60, 5, [11]), nohost=[12]),
                 [qpod(j, spread=[(1, RACK, "web"), (2, HOST, "web")]) for j in range(2)], "nowin_unfused", bound=bound,
                 pct=100, worlds=(2,),
                 claim=lambda s, rs: rs[0]["ignored"] == {11, 12} and rs[0]["sizes"] == [5, 58])


@scene_fn
def pts_all_ignored():
    """Every kept node ignored: all normalize to 0, the maximum stays 0."""
    return Scene("pts_all_ignored", ring(60), [qpod(0, PREFER_A, spread=[(1, RACK, "web")])], "nowin_fused", pct=100,
                 claim=lambda s, rs: len(rs[0]["ignored"]) == 60 and not rs[0]["norm"][SPREAD].any())


@scene_fn
def pts_one_not_ignored():
    bound = bpods("web", {30: 2})
    return Scene("pts_one_not_ignored", ring(60, labels={30: {RACK: "r0"}}), [qpod(0, spread=[(1, RACK, "web")])],
                 "nowin_fused", bound=bound, pct=100,
                 claim=lambda s, rs: len(rs[0]["ignored"]) == 59 and _norm_of(rs[0], SPREAD, 30) == 100 and
                 rs[0]["sizes"] == [1])


@scene_fn
def pts_system_default():
    """A system-defaulted pair (hostname maxSkew 3, zone maxSkew 5) on a cluster
    where some nodes lack the zone label: nothing is ignored, the unlabelled
    nodes' empty value is a pair of its own."""
    nodes = [node(i, {ZONE: f"z{i % 3}"} if i % 5 else None) for i in range(60)]
    bound = [Pod(f"b{i}-{c}", labels={"app": "rs"}, containers=[Container({})], node_name=name_of(i))
             for i in range(60) for c in range(i % 4)]
    q = [qpod(j, labels={"app": "rs"}, owner=("apps/v1", "ReplicaSet", "rs")) for j in range(2)]
    return Scene("pts_system_default", nodes, q, "nowin_unfused", bound=bound, pct=100, defaults=True,
                 claim=lambda s, rs: not rs[0]["ignored"] and sorted(rs[0]["sizes"]) == [4, 60] and
                 s.soft_uses == [2, 2])


@scene_fn
def combined():
    """All four normalized plugins, non-unit weights and an extender score."""
    labels = {i: {RACK: f"r{i % 6}", **({"tier": "gold"} if i % 9 == 0 else {})} for i in range(120) if i != 15}
    taints = {i: i % 3 for i in range(120)}
    bound = bpods("web", {i: (i * 5) % 4 for i in range(120)}) + bpods("db", {i: i % 2 for i in range(0, 120, 7)})
    q = [qpod(j, PREFER_A, affinity=[(3, HOST, "web")], anti=[(2, RACK, "db")], spread=[(2, RACK, "web")])
         for j in range(2)]

    def ext(n):
        return None, (np.arange(n, dtype=np.int64) * 37 % 11) * 10

    return Scene("combined", ring(120, labels=labels, taints=taints), q, "windowed", bound=bound, s0=33, ext=ext,
                 weights={"NodeAffinity": 2, "TaintToleration": 3, "InterPodAffinity": 2, "PodTopologySpread": 5},
                 schedule=False,
                 claim=lambda s, rs: all(len(set(rs[0]["norm"][x][rs[0]["kept"]])) > 1 for x in (NA, TT, IPA, SPREAD)))


# ---- selectHost scenes ---------------------------------------------------------------------------
def _ties(n, seed, seq0):
    def build():
        return Scene(f"ties_{n}_seed{seed & 0xF}_seq{seq0}", ring(n), [qpod(0), qpod(1)], "nowin_fused", pct=100,
                     seed=seed, seq0=seq0,
                     claim=lambda s, rs: len(set(rs[0]["total"])) == 1 and rs[0]["chosen"] != 0)
    return build


TIES = [(257, SEED, 0), (257, SEED2, 0), (257, SEED, 9), (513, SEED, 0), (513, SEED2, 9)]
for _n, _sd, _sq in TIES:
    PARAM[f"ties_{_n}_seed{_sd & 0xF}_seq{_sq}"] = _ties(_n, _sd, _sq)


@scene_fn
def ties_on_grid_edges():
    """Equal best totals exactly on nodes 0, 63, 64, 255, 256 and 512."""
    at = (0, 63, 64, 255, 256, 512)
    return Scene("ties_on_grid_edges", ring(513, labels={i: {"tier": "gold"} for i in at}),
                 [qpod(j, PREFER_A) for j in range(3)], "nowin_fused", pct=100, seq0=3,
                 claim=lambda s, rs: set(np.nonzero(rs[0]["total"] == rs[0]["total"].max())[0]) == set(at) and
                 _every(rs, lambda r: r["chosen"] in at))


def _blocks65(pct):
    """16,640 nodes (65 blocks of 256: a second lap of reduce_block_best's
    stride of 64 blocks).  The unique best on node 16,639, then on node 16,384,
    then ties between nodes 0 and 16,384 and between nodes 1 and 16,385 (the two
    records of a lane).  Few feasible nodes, so the windowed form keeps them all."""
    def build():
        n = 16640
        roomy = set(range(0, n, 32)) | {1, 16385, 16639}
        labels = {16639: {"a": "1"}, 16384: {"b": "1", "c": "1"}, 0: {"c": "1"}, 1: {"d": "1"}, 16385: {"d": "1"}}
        nodes = [node(i, labels.get(i), full=i not in roomy) for i in range(n)]
        q = [qpod(0, [(5, "c", "1")]), qpod(1, [(5, "a", "1")]), qpod(2, [(5, "d", "1")]), qpod(3, [(5, "b", "1")])]
        name = f"blocks65_pct{pct}"

        def claim(s, rs):
            t0, t2 = rs[0]["total"], rs[2]["total"]
            return t0[0] == t0[16384] == t0.max() and t2[1] == t2[16385] == t2.max() and \
                rs[1]["chosen"] == 16639 and rs[3]["chosen"] == 16384 and rs[0]["chosen"] in (0, 16384) and \
                _every(rs, lambda r: r["cut"] < 0 and r["n_feasible"] == len(roomy))
        return Scene(name, nodes, q, "windowed" if pct == 0 else "nowin_fused", claim, pct=pct, s0=16000)
    return build


for _p in (0, 100):
    PARAM[f"blocks65_pct{_p}"] = _blocks65(_p)


# ---- sharded geometry (257 nodes, K = 123; partition(257, 2) = 192 + 65, (257, 3) = 128 + 128 + 1) ------
def _shard_scene(tag, s0, full=(), note=""):
    def build():
        n = 257
        k = cycleref.num_feasible_nodes_to_find(n, 0)
        order = [(s0 + i) % n for i in range(n) if (s0 + i) % n not in set(full)]
        cut, winner, holder = order[k], order[k - 1], order[k + 1]
        labels = {winner: {"tier": "gold"}, order[5]: {"tier": "gold"}, holder: {"tier": "gold", "disk": "ssd"}}
        q = [qpod(j, [(3, "tier", "gold"), (4, "disk", "ssd")]) for j in range(2)]
        return Scene(f"shard_{tag}", ring(n, full=full, labels=labels), q, "windowed", s0=s0, worlds=(2, 3),
                     claim=lambda s, rs: rs[0]["cut"] == cut and rs[0]["chosen"] in (winner, order[5]) and
                     _norm_of(rs[0], NA, winner) == 100)
    return build


SHARD_GEOMETRY = {
    "cut_in_own_hi_run": (10, ()),                 # start inside shard 0, the cut (133) after it on the same shard
    "cut_in_own_lo_run": (150, ()),                # world 2: the cut (16) wraps into the start's own shard
    "cut_on_later_shard": (100, ()),               # cut 223
    "cut_on_earlier_shard": (200, ()),             # cut 66
    "cut_on_shard_first_node": (69, ()),           # cut 192: the first node of world 2's second shard
    "cut_on_shard_last_node": (68, ()),            # cut 191
    "cut_on_one_node_shard": (133, ()),            # cut 256: world 3's one-node shard
    "empty_shard": (20, tuple(range(192, 257))),   # world 2's second shard has no feasible node
}
for _t, (_s, _f) in SHARD_GEOMETRY.items():
    PARAM[f"shard_{_t}"] = _shard_scene(_t, _s, _f)


@scene_fn
def shard_ties_across():
    """Equal best totals on different shards of every world."""
    at = (3, 60, 100)
    return Scene("shard_ties_across", ring(101, labels={i: {"tier": "gold"} for i in at}),
                 [qpod(j, PREFER_A) for j in range(3)], "windowed", s0=90, seq0=2, worlds=(2, 3, 8),
                 claim=lambda s, rs: set(np.nonzero(rs[0]["total"] == rs[0]["total"].max())[0]) <= set(at) and
                 rs[0]["total"][3] == rs[0]["total"][60])


@scene_fn
def shard_start_in_empty_shard():
    """101 nodes on 8 shards (13 or 12 nodes each): the fourth shard (nodes 39
    to 51) has no feasible node and holds the start; 88 feasible nodes, no cut."""
    return Scene("shard_start_in_empty_shard",
                 ring(101, full=range(39, 52), labels={38: {"tier": "gold"}, 52: {"tier": "gold"}}),
                 [qpod(j, PREFER_A) for j in range(2)], "windowed", s0=45, seq0=1, worlds=(2, 8),
                 claim=lambda s, rs: rs[0]["kept"][0] == 52 and rs[0]["kept"][-1] == 38 and rs[0]["cut"] < 0 and
                 rs[0]["n_feasible"] == 88 and rs[0]["total"][38] == rs[0]["total"][52])


# ---- extender scenes (Engine.eval_pod_extenders) ------------------------------------------------------
def _ext_scene(name, drop, claim, score=False):
    """Nodes 20 (both labels, three taints, four db pods) holds every maximum."""
    def build():
        n, s0 = 120, 10
        labels = {20: {"tier": "gold", "disk": "ssd"}, 30: {"tier": "gold"}}
        bound = bpods("db", {20: 4, 31: 1})
        q = [qpod(0, [(3, "tier", "gold"), (2, "disk", "ssd")], affinity=[(5, HOST, "db")]), qpod(1, PREFER_A)]

        def ext(n_):
            fail = np.zeros(n_, np.uint8)
            kept = [(s0 + i) % n_ for i in range(100)]
            fail[[x for x in kept if drop(x)]] = 1
            es = (np.arange(n_, dtype=np.int64) % 7) * 50
            es[40] = 2000
            return fail, es if score else None
        return Scene(name, ring(n, labels=labels, taints={20: 3, 32: 1}), q, "windowed", claim, bound=bound, s0=s0,
                     ext=ext, schedule=False)
    return build


PARAM["ext_drops_max_holder"] = _ext_scene(
    "ext_drops_max_holder", lambda x: x == 20,
    lambda s, rs: 20 not in rs[0]["kept"] and rs[0]["n_feasible"] == 99 and _norm_of(rs[0], NA, 30) == 100 and
    rs[0]["fail_plugin"][20] == cycleref.FAIL_EXTENDER)
PARAM["ext_drops_all_but_one"] = _ext_scene(
    "ext_drops_all_but_one", lambda x: x != 31,
    lambda s, rs: rs[0]["kept"] == [31] and rs[0]["chosen"] == 31 and not rs[0]["scored"].any())
PARAM["ext_drops_all"] = _ext_scene(
    "ext_drops_all", lambda x: True,
    lambda s, rs: rs[0]["status"] == cycleref.STATUS_UNSCHEDULABLE and rs[0]["n_processed"] == 100 and
    rs[0]["next_start"] == 110)
PARAM["ext_scores_added"] = _ext_scene(
    "ext_scores_added", lambda x: False,
    lambda s, rs: rs[0]["chosen"] == 40 and int(rs[0]["total"][27]) - int(rs[0]["total"][28]) == 300, score=True)


ALL = list(SCENES) + list(PARAM)


def sharded() -> List[Tuple[str, int]]:
    return [(n, w) for n in ALL for w in scene(n).worlds]


EXTENDER = [n for n in ALL if n.startswith("ext_")] + ["combined"]
# the "ab" flavor takes these without a use (plain pods whose normalized scores vary, ADAPT)
AB = ["cut_holds_best", "max_past_cut", "exactly_k_plus_1_s50", "default_thirds_windowed", "chunk_1025_at1024_s0"]


def without_ports(s: Scene) -> Scene:
    """The scene with plain queue pods (the "ab" route)."""
    import copy
    t = copy.copy(s)
    for attr in ("encoded", "soft_uses", "prof", "sp"):
        t.__dict__.pop(attr, None)
    t.queue = []
    for p in s.queue:
        p2 = copy.deepcopy(p)
        for c in p2.containers:
            c.ports = []
        t.queue.append(p2)
    t.route = "ab"
    return t
