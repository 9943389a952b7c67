"""Hand-built edge scenes for the topology batch path (csrc/ksim_tbatch.hip
k_tb_filter, k_tb_select, k_tb_merge, k_tb_chain_pairs, k_tb_commit; its host
side tbatch_admit, tbatch_vuse, tbatch_runs in csrc/ksim_engine.cpp).
gen.config3_objects, which every other GPU test of that path draws from,
gives hundreds of feasible nodes, every label on every node, no taints and
three zones; these scenes sit where it never goes: 0, 1, kTopT and kTopT + 1
feasible nodes, ignored and unkeyed nodes, variant keys of 1 to 4 domains and
past them, slots without a feasible node, partial and full node blocks, runs
of exactly kTbPods pods and one more, the hard_small admission boundary, lone
holders of an extremum, one-node clusters and one-wave feasible sets.

The scenes are objects (ksim.model) so oracle/objref.py runs them too; each
holds its nodes, bound pods and queue, a profile kind, what the engine must
report about the path it took, and ``reaches``: the edges it claims, each with
a predicate over the oracle's cycle outputs (a Trace).
tests/test_tbatch_cases.py proves the claims on the CPU;
tests/test_gpu_tbatch_edges.py runs the scenes through the engine.

Scenes reshaped to be admitted (tbatch_admit takes a pod only when every
domain sum it reads comes from a persistent table, build_ptab):
  * a DoNotSchedule key must be on every node (col_total), so a node without
    the zone label sends the whole queue to the per-pod path.
    ignored_and_unkeyed keeps that cluster as its "zoneless" form (every pod a
    per-pod cycle) and
    puts the unkeyed node under a table-read use that is admitted: a preferred
    anti-affinity term on a rack key one node lacks (value id 0 in the table).
    The variant use itself is always a DoNotSchedule key, so no admitted pod
    meets value id 0 there.
  * nodeTaintsPolicy Honor on a DoNotSchedule constraint is refused once the
    cluster has a NoSchedule taint; tiny_tainted carries Honor on the
    ScheduleAnyway hostname constraint, which reads the node's own count.
  * maxSkew is at least 1 and the self match at most 1, so the least loaded
    marked domain always passes: tb_var_setup's mask is never empty.  What a
    queue can reach is a slot whose passing domains hold no feasible node
    (nf == 0 for that slot): variant_slots fills those domains' nodes.
  * a key of one domain gives every landing the same mask, so every reader
    stays on slot 0 and tb_variant_pods stays 0 there."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

from ksim import profile
from ksim.encode import encode_cluster, encode_pods
from ksim.model import (Container, LabelSelector, Node, Pod, PodAffinityTerm, Taint, TopologySpreadConstraint,
                        WeightedPodAffinityTerm)
from oracle.oracle import Oracle

# csrc/ksim_internal.h and csrc/ksim_device.h (tests/test_tbatch_cases.py reads them back)
K_TB_PODS = 32
K_TOP_T = 8
K_VAR_DOM = 4
K_TB_MAX_BLOCKS = 64
K_FUSE_MIN_VALUES = 256
CONSTANTS = {"kTbPods": K_TB_PODS, "kTopT": K_TOP_T, "kVarDom": K_VAR_DOM, "kTbMaxBlocks": K_TB_MAX_BLOCKS,
             "kFuseMinValues": K_FUSE_MIN_VALUES}
BLOCK = 256                                        # nodes per block of k_tb_filter / k_tb_select
MAX_NODES = K_TB_MAX_BLOCKS * BLOCK

HOST = "kubernetes.io/hostname"
ZONE = "topology.kubernetes.io/zone"
RACK = "example.com/rack"

SCORE_NAMES = [p.name for p in profile.SchedulerProfile().score_plugins()]
PTS = SCORE_NAMES.index("PodTopologySpread")
IPA = SCORE_NAMES.index("InterPodAffinity")


# ---- the oracle's view of a scene ------------------------------------------------------
@dataclass
class Trace:
    """Oracle.cycle over the scene's queue, pod by pod (pct 100)."""
    scene: "Scene"
    cluster: object
    chosen: List[int]                              # node position or -1
    nf: List[int]                                  # n_feasible
    scored: List[np.ndarray]                       # [N] bool
    total: List[np.ndarray]                        # [N] int64
    pts: List[np.ndarray]                          # raw PodTopologySpread
    ipa: List[np.ndarray]                          # raw InterPodAffinity
    npts: List[np.ndarray] = field(default_factory=list)   # normalized PodTopologySpread
    nipa: List[np.ndarray] = field(default_factory=list)   # normalized InterPodAffinity

    def names(self) -> List[Optional[str]]:
        return [self.cluster.node_names[c] if c >= 0 else None for c in self.chosen]


Claim = Callable[[Trace], bool]


@dataclass
class Scene:
    name: str
    nodes: List[Node]
    bound: List[Pod]
    queue: List[Pod]
    kind: str = "default"                          # scheduler_profile's kind
    reaches: Dict[str, Claim] = field(default_factory=dict)
    route: str = "tbatch"                          # "tbatch": no per-pod cycle; "perpod": every pod takes one
    multi: bool = True                             # some batch holds several pods
    multi_plain: bool = True                       # ... and without zone variants too (ab64, replicas)
    variants: Optional[bool] = None                # diag()["tb_variant_pods"] > 0 / == 0 / not pinned
    objref: bool = True                            # small enough for oracle/objref.py
    positional: bool = False                       # the claims speak of node positions: input order is nodeTree order
    twin: Optional[str] = None                     # the scene without the edge: its placements must differ

    def __post_init__(self):
        assert len(self.queue) <= 100, self.name

    @functools.cached_property
    def encoded(self):
        """(cluster, pods); tests take copy_state() of the cluster."""
        cluster, order = encode_cluster(self.nodes, self.bound)
        if self.positional:
            assert order == list(range(len(self.nodes))), self.name
        pods = encode_pods(cluster, self.queue)
        return cluster, pods


def scheduler_profile(kind: str = "default", pct: int = 100) -> profile.SchedulerProfile:
    assert kind == "default"
    return profile.SchedulerProfile(percentage_of_nodes_to_score=pct)


def compiled(kind: str = "default", pct: int = 100):
    return profile.compile_profile(scheduler_profile(kind, pct))


@functools.lru_cache(maxsize=None)
def trace(name: str) -> Trace:
    s = scene(name)
    cluster, pods = s.encoded
    ora = Oracle(cluster.copy_state(), compiled(s.kind))
    t = Trace(s, cluster, [], [], [], [], [], [])
    for j in range(pods.n_pods):
        o = ora.cycle(pods, j)
        t.chosen.append(int(o["chosen"]))
        t.nf.append(int(o["n_feasible"]))
        t.scored.append(np.asarray(o["scored"]).astype(bool))
        t.total.append(np.asarray(o["total"]).copy())
        t.pts.append(np.asarray(o["raw"][PTS]).copy())
        t.ipa.append(np.asarray(o["raw"][IPA]).copy())
        t.npts.append(np.asarray(o["norm"][PTS]).copy())
        t.nipa.append(np.asarray(o["norm"][IPA]).copy())
    ora.close()
    return t


def slot_feasible(name: str, adder: int, reader: int) -> Dict[Optional[str], int]:
    """The reader's n_feasible per landing of the adder: the queue before the
    adder scheduled as the oracle does, then the adder assumed on one node of
    each zone in turn (None: nowhere), then the reader's cycle.  These are the
    per-slot feasible counts tb_var_setup's masks give."""
    s = scene(name)
    cluster, pods = s.encoded
    out: Dict[Optional[str], int] = {}
    zones: Dict[Optional[str], int] = {None: -1}
    for pos, lb in enumerate(cluster.node_labels):
        zones.setdefault(lb[ZONE], pos)
    for z, pos in zones.items():
        ora = Oracle(cluster.copy_state(), compiled(s.kind))
        if adder:
            ora.schedule(pods, 0, adder)
        if pos >= 0:
            ora.assume(pods, adder, pos)
        out[z] = int(ora.cycle(pods, reader)["n_feasible"])
        ora.close()
    return out


# ---- claims over a trace ----------------------------------------------------------------
def nf_is(*seq) -> Claim:
    return lambda t: t.nf[:len(seq)] == list(seq)


def nf_all(v: int) -> Claim:
    return lambda t: all(x == v for x in t.nf)


def some_nf(v: int) -> Claim:
    return lambda t: v in t.nf


def window(j: int) -> range:
    """The pods ahead of pod j in its kTbPods-pod window (runs start at the
    queue's first pod and hold at most kTbPods pods)."""
    return range(j - j % K_TB_PODS, j)


def unschedulable_inside_a_window(t: Trace) -> bool:
    return any(t.chosen[j] < 0 and any(t.chosen[k] >= 0 for k in window(j)) for j in range(len(t.chosen)))


def top_ties(m: int) -> Claim:
    """Some pod has at least m scored nodes sharing the top total."""
    def claim(t):
        return any(sc.any() and int((tot[sc] == tot[sc].max()).sum()) >= m for sc, tot in zip(t.scored, t.total))
    return claim


def chosen_in(lo: int, hi: int) -> Claim:
    return lambda t: any(lo <= c < hi for c in t.chosen)


def node_chosen(node: str) -> Claim:
    return lambda t: node in t.names()


def queue_len(n: int) -> Claim:
    return lambda t: len(t.chosen) == n


def static(ok: bool) -> Claim:
    return lambda t: bool(ok)


def _lone(values: np.ndarray, scored: np.ndarray, top: bool) -> int:
    """The one scored node holding the extremum alone, or -1."""
    if int(scored.sum()) < 2:
        return -1
    v = np.where(scored, values, values[scored].min() if top else values[scored].max())
    x = v.max() if top else v.min()
    at = np.nonzero(scored & (values == x))[0]
    return int(at[0]) if at.size == 1 else -1


def first_pod_takes_the_lone_holder(t: Trace) -> bool:
    """Pod 0 lands on the one node that holds its app's PodTopologySpread
    minimum and InterPodAffinity maximum alone, and pod 1 is of the same app:
    for pod 1 (j == 1) an extremum with one holder (hmin == 1 <= j) moves."""
    q = t.scene.queue
    h = _lone(t.pts[0], t.scored[0], False)
    return h >= 0 and h == _lone(t.ipa[0], t.scored[0], True) == t.chosen[0] and \
        q[0].labels["app"] == q[1].labels["app"]


def _norm_pts(s: int, mx: int, mn: int) -> int:
    return 100 if mx <= 0 else 100 * (mx + mn - s) // mx            # ksim_device.h normalize_value kNormPTS


def _norm_ipa(s: int, mx: int, mn: int) -> int:
    return int(100.0 * ((s - mn) / (mx - mn))) if mx > mn else 0     # ... kNormIPA, the score map not empty


def stale_extrema_move_the_choice(t: Trace) -> bool:
    """Pod 1's totals with its two topology scores normalized against the
    extrema of the snapshot before pod 0 (what a batch that did not notice the
    lone holder moving would use): the node the oracle chooses for pod 1 is not
    a best node under them.  The normalization is checked against the
    oracle's own normalized scores first."""
    w = {p.name: p.weight for p in scheduler_profile(t.scene.kind).score_plugins()}
    sc = t.scored[1]
    if not (sc == t.scored[0]).all():
        return False
    idx = np.nonzero(sc)[0]
    h = t.chosen[0]
    true_p, true_i = t.pts[1], t.ipa[1]
    for raw, nrm, f in ((true_p, t.npts[1], _norm_pts), (true_i, t.nipa[1], _norm_ipa)):
        mx, mn = int(raw[idx].max()), int(raw[idx].min())
        if any(f(int(raw[i]), mx, mn) != int(nrm[i]) for i in idx):
            return False
    stale_p, stale_i = true_p.copy(), true_i.copy()
    stale_p[h], stale_i[h] = t.pts[0][h], t.ipa[0][h]
    ext = [(int(x[idx].max()), int(x[idx].min())) for x in (stale_p, stale_i)]
    if ext == [(int(x[idx].max()), int(x[idx].min())) for x in (true_p, true_i)]:
        return False
    wrong = {int(i): int(t.total[1][i])
             + w["PodTopologySpread"] * (_norm_pts(int(true_p[i]), *ext[0]) - int(t.npts[1][i]))
             + w["InterPodAffinity"] * (_norm_ipa(int(true_i[i]), *ext[1]) - int(t.nipa[1][i])) for i in idx}
    return wrong[t.chosen[1]] < max(wrong.values())


def ipa_map_fills_mid_window(t: Trace) -> bool:
    """The first pod scores no InterPodAffinity pair anywhere; a later pod of
    its window does (kTopoScoreNonEmpty flips inside the batch)."""
    if t.ipa[0][t.scored[0]].any():
        return False
    return any(t.ipa[j][t.scored[j]].any() for j in range(1, min(K_TB_PODS, len(t.chosen))))


# ---- objects ----------------------------------------------------------------------------
def node(name: str, zone: Optional[str], cpu: str = "8", mem: str = "32Gi", host: bool = True, taints=(),
         extra: Optional[dict] = None) -> Node:
    labels = {}
    if host:
        labels[HOST] = name
    if zone is not None:
        labels[ZONE] = zone
    labels.update(extra or {})
    return Node(name, labels, list(taints), {"cpu": cpu, "memory": mem, "pods": "110"})


def spread_pod(name: str, app: str, cpu: str = "100m", mem: str = "128Mi", zone_skew: int = 1, host_skew: int = 2,
               anti: int = 50, zone_sel: Optional[str] = None, hard_key: str = ZONE, soft_sel: Optional[str] = None,
               soft_taints: Optional[str] = None, rack_anti: int = 0) -> Pod:
    """Config 3's incoming pod: hard_key DoNotSchedule at zone_skew (0: none),
    hostname ScheduleAnyway at host_skew (0: none) and preferred anti-affinity
    on the hostname at weight anti (0: none), all on the pod's own app unless
    zone_sel / soft_sel name another; rack_anti: a preferred anti-affinity term
    on the rack key as well."""
    sel = LabelSelector({"app": app})
    ts = []
    if zone_skew:
        ts.append(TopologySpreadConstraint(zone_skew, hard_key, "DoNotSchedule",
                                           LabelSelector({"app": zone_sel or app})))
    if host_skew:
        ts.append(TopologySpreadConstraint(host_skew, HOST, "ScheduleAnyway", LabelSelector({"app": soft_sel or app}),
                                           node_taints_policy=soft_taints))
    terms = []
    if anti:
        terms.append(WeightedPodAffinityTerm(anti, PodAffinityTerm(HOST, sel)))
    if rack_anti:
        terms.append(WeightedPodAffinityTerm(rack_anti, PodAffinityTerm(RACK, sel)))
    return Pod(name, labels={"app": app}, containers=[Container({"cpu": cpu, "memory": mem})], topology_spread=ts,
               pod_anti_affinity_preferred=terms)


def bound_pod(name: str, app: str, on: str, cpu: str = "100m", mem: str = "128Mi") -> Pod:
    return Pod(name, labels={"app": app}, containers=[Container({"cpu": cpu, "memory": mem})], node_name=on)


def zoned(n: int, zones: int = 3, **kw) -> List[Node]:
    """n nodes round-robin over the zones: nodeTree order is input order."""
    return [node(f"n{i:05d}", f"z{i % zones}", **kw) for i in range(n)]


def many_apps(n: int, **kw) -> List[Pod]:
    """n pods of n apps: no pod reads a class another adds, so runs are full."""
    return [spread_pod(f"p{k:03d}", f"a{k}", **kw) for k in range(n)]


# ---- nf_ladder ---------------------------------------------------------------------------
def nf_ladder() -> Scene:
    """Three nodes, one per zone, one app at maxSkew 1: each pod closes the
    zone it lands in until the three are level again."""
    return Scene("nf_ladder", zoned(3), [], [spread_pod(f"p{k:02d}", "a") for k in range(12)], variants=True,
                 multi_plain=False,                # one app: without variants every pod reads what the last one adds
                 reaches={"n_feasible runs 3, 2, 1, 3, 2, 1": nf_is(3, 2, 1, 3, 2, 1, 3, 2, 1),
                          "kStatOne: a pod with one feasible node": some_nf(1),
                          "has_soft off and on inside a run (nf 1 next to nf 2)": nf_is(3, 2, 1)})


def nf_ladder_full_one_app() -> Scene:
    """1-CPU nodes under 400m pods of one app at maxSkew 2: two pods fill a
    node, the seventh pod finds none."""
    return Scene("nf_ladder_full_one_app", zoned(3, cpu="1"), [],
                 [spread_pod(f"p{k:02d}", "a", cpu="400m", zone_skew=2) for k in range(10)], multi_plain=False,
                 reaches={"n_feasible runs 3, 3, 3, 3, 2, 1, 0, 0": nf_is(3, 3, 3, 3, 2, 1, 0, 0, 0, 0),
                          "nf == 0": some_nf(0), "kStatOne": some_nf(1)})


def nf_ladder_full_apps() -> Scene:
    """The same nodes under ten apps: one run holds the whole ladder, the
    unschedulable pods behind placed ones."""
    return Scene("nf_ladder_full_apps", zoned(3, cpu="1"), [], many_apps(10, cpu="400m"), variants=False,
                 reaches={"n_feasible runs 3, 3, 3, 3, 2, 1, 0, 0": nf_is(3, 3, 3, 3, 2, 1, 0, 0, 0, 0),
                          "unschedulable pods inside a run": unschedulable_inside_a_window})


# ---- many_apps_few_nodes -----------------------------------------------------------------
FEW_NODES = (1, 2, 3, 8, 9)


def many_apps_few_nodes(n: int) -> Scene:
    """40 pods of 40 apps (a 32-pod run and an 8-pod tail) on n large nodes;
    nine nodes sit in one zone (nd == 1)."""
    nodes = zoned(n, zones=1 if n == 9 else 3, cpu="64", mem="256Gi")
    reaches = {f"every pod has {n} feasible nodes": nf_all(n), "a full run and a tail": queue_len(K_TB_PODS + 8)}
    if n <= K_TOP_T:
        reaches["topk_complete: a complete list shorter than the run"] = static(n <= K_TOP_T < K_TB_PODS)
    if n == K_TOP_T:
        reaches["nf == kTopT"] = some_nf(K_TOP_T)
    if n == K_TOP_T + 1:
        reaches["nf == kTopT + 1: the smallest incomplete list"] = some_nf(K_TOP_T + 1)
        reaches["a variant key of one domain"] = lambda t: len({lb[ZONE] for lb in t.cluster.node_labels}) == 1
    if n == 1:
        reaches["kStatOne for a whole run"] = nf_all(1)
    # from eight nodes on a pod takes a sixteenth of a node: a node an earlier pod of the batch guessed
    # scores six points lower than an untouched one, so the one node past a pod's top-T list is its
    # best once the list's nodes are taken, and a list wrongly read as complete places the pod wrong
    big = n >= K_TOP_T
    if big:
        reaches["a placed pod lowers its node's total"] = lambda t: all(
            t.total[j + 1][t.chosen[j]] < t.total[j][t.chosen[j]] for j in range(len(t.chosen) - 1))
    return Scene(f"many_apps_few_nodes_{n}", nodes, [],
                 many_apps(K_TB_PODS + 8, cpu="4" if big else "1", mem="16Gi" if big else "4Gi"),
                 reaches=reaches, variants=False)


def exhausted_list() -> Scene:
    """Nine nodes of 50 cores / 50 Gi in one zone, node k loaded to 2 k percent
    by an unrelated pod, under twelve apps' pods of a quarter node each: every
    pod's snapshot totals fall by two points from node to node, so every list
    is nodes 0 .. 7 and the ninth node is on none (nf == kTopT + 1).  Pods
    0 .. 7 take the list's nodes; the ninth pod finds its list exhausted and
    incomplete.  A placed pod costs its node 25 points, more than the 16
    between the first node and the last, so the ninth pod belongs on the ninth
    node: read as complete, its list would leave it to the pair keys, which
    know only the eight guessed nodes."""
    nodes = [node(f"n{k}", "z0", cpu="50", mem="50Gi") for k in range(9)]
    bound = [Pod(f"load{k}", containers=[Container({"cpu": str(k), "memory": f"{k}Gi"})], node_name=f"n{k}")
             for k in range(1, 9)]

    def ladder(t):
        order = np.argsort(-t.total[0], kind="stable")
        strict = all(t.total[0][order[k]] > t.total[0][order[k + 1]] for k in range(8))
        spread = int(t.total[0][order[0]] - t.total[0][order[8]])
        cost = int(t.total[0][t.chosen[0]] - t.total[1][t.chosen[0]])
        return strict and spread < cost and t.chosen[:9] == [int(x) for x in order]
    return Scene("exhausted_list", nodes, bound, many_apps(12, cpu="12500m", mem="12800Mi"), variants=False,
                 reaches={"the ninth pod's list (the first eight nodes) is taken; it lands on the ninth node": ladder,
                          "nf == kTopT + 1": nf_all(K_TOP_T + 1)})


# ---- run_lengths -------------------------------------------------------------------------
RUN_LENGTHS = (K_TB_PODS - 1, K_TB_PODS, K_TB_PODS + 1, 2 * K_TB_PODS + 1)


def run_lengths(n_pods: int) -> Scene:
    """The same queue cut at 31, 32, 33 and 65 pods on twelve nodes."""
    return Scene(f"run_lengths_{n_pods}", zoned(12, cpu="16"), [], many_apps(n_pods, cpu="200m"), variants=False,
                 reaches={f"a queue of {n_pods} pods (tb_count)": queue_len(n_pods),
                          "no pod reads a class another adds": lambda t: len({p.labels["app"] for p in t.scene.queue})
                          == len(t.scene.queue)})


# ---- block_edges -------------------------------------------------------------------------
BLOCK_EDGES = (BLOCK - 1, BLOCK, BLOCK + 1, MAX_NODES, MAX_NODES + 1)


def _top_positions(n: int) -> range:
    """Eleven to sixteen positions around the start of the last node block
    (the cluster's last eleven where there is one block)."""
    b = (n - 1) // BLOCK * BLOCK
    return range(n - 11, n) if b == 0 else range(b - 10, min(n, b + 6))


def block_edges(n: int, twin: bool = False) -> Scene:
    """n small nodes, of which those at _top_positions are eight times as
    large: 40 pods of 40 apps find them all at the same total, more than kTopT
    of them, so the tie-break decides and the top-T lists of two blocks (or of
    one partial block) merge.  The twin makes the large nodes of the last
    block small again."""
    b = (n - 1) // BLOCK * BLOCK
    top = _top_positions(n)
    nodes = zoned(n)
    for p in top:
        if not (twin and p >= b):
            nodes[p].allocatable = {"cpu": "64", "memory": "256Gi", "pods": "110"}
    reaches = {"more than kTopT scored nodes share the top total": top_ties(K_TOP_T + 1),
               "a node of the last block is chosen": chosen_in(b, n)}
    if b:
        reaches["a node of the block before is chosen (the tie crosses a block boundary)"] = chosen_in(b - BLOCK, b)
    if n % BLOCK:
        reaches["the last block is partial"] = static(n % BLOCK != 0)
    if n == MAX_NODES:
        reaches["N == kTbMaxBlocks * 256: every lane of k_tb_merge holds a block"] = static(True)
        reaches["a guess at a node id past kTbHoldSlots / 2"] = chosen_in(MAX_NODES // 2, MAX_NODES)
    if n > MAX_NODES:
        reaches["N past kTbMaxBlocks * 256"] = static(True)
    if twin:
        reaches = {"no large node in the last block": lambda t: not chosen_in(b, n)(t)}
    return Scene(f"block_edges_{n}" + ("_twin" if twin else ""), nodes, [], many_apps(40, cpu="1", mem="4Gi"),
                 reaches=reaches, route="perpod" if n > MAX_NODES else "tbatch", variants=False,
                 objref=n <= BLOCK + 1, positional=True,
                 twin=f"block_edges_{n}_twin" if n == BLOCK + 1 and not twin else None)


# ---- ignored_and_unkeyed ---------------------------------------------------------------------
def ignored_and_unkeyed(form: str = "scene") -> Scene:
    """Nine 1-CPU nodes over three zones and three racks, a large node without
    the hostname label (IgnoredNodes under the ScheduleAnyway hostname
    constraint: q.ign, nign, topo_log[nf - nign]) and a node without the rack
    label under a preferred anti-affinity term keyed by rack (value id 0 of a
    table-read use).  36 pods of four apps at 300m: the small nodes fill and
    the ignored node takes pods.
      "labelled": the twin, the large node carries its hostname label;
      "zoneless": the rackless node lacks the zone label instead:
                  DoNotSchedule on a key some node lacks reads no persistent
                  table, so every pod takes a per-pod cycle."""
    nodes = [node(f"n{i}", f"z{i % 3}", cpu="1", extra={RACK: f"r{i // 3}"}) for i in range(9)]
    nodes.append(node("hostless", "z0", cpu="16", host=form == "labelled", extra={RACK: "r0"}))
    if form == "zoneless":
        nodes.append(node("unkeyed", None, cpu="1", extra={RACK: "r1"}))
    else:
        nodes.append(node("unkeyed", "z1", cpu="1"))
    queue = [spread_pod(f"p{k:02d}", f"a{k % 4}", cpu="300m", zone_skew=2, rack_anti=0 if form == "zoneless" else 10)
             for k in range(36)]
    reaches = {"the hostless node is chosen": node_chosen("hostless"),
               "the unkeyed node is chosen": node_chosen("unkeyed"),
               "the hostless node is scored next to others (nign == 1 < nf)":
                   lambda t: any(sc[t.cluster.node_names.index("hostless")] and sc.sum() > 2 for sc in t.scored)}
    if form == "zoneless":
        del reaches["the unkeyed node is chosen"]
        reaches["a node without the DoNotSchedule key (it fails the filter)"] = lambda t: (
            ZONE not in t.cluster.node_labels[t.cluster.node_names.index("unkeyed")] and max(t.nf) == 10)
    if form == "labelled":
        reaches = {"every node carries the hostname label": lambda t: all(HOST in lb for lb in t.cluster.node_labels)}
    return Scene("ignored_and_unkeyed" + ("" if form == "scene" else "_" + form), nodes, [], queue, reaches=reaches,
                 route="perpod" if form == "zoneless" else "tbatch",
                 twin="ignored_and_unkeyed_labelled" if form == "scene" else None)


def mostly_ignored() -> Scene:
    """One labelled 1-CPU node and two large nodes without the hostname label
    under eight apps at 300m: nf - nign is 1 for three pods, then the labelled
    node is full and it is 0 (every feasible node ignored)."""
    nodes = [node("n0", "z0", cpu="1"), node("h1", "z1", cpu="16", host=False), node("h2", "z2", cpu="16", host=False)]
    return Scene("mostly_ignored", nodes, [], many_apps(8, cpu="300m"), variants=False,
                 reaches={"nf - nign == 1, then 0": nf_is(3, 3, 3, 2, 2),
                          "the labelled node fills": lambda t: t.names().count("n0") == 3})


def unignored_weight_placements(name: str, nign: int) -> List[int]:
    """The oracle's placements of the scene with topologyNormalizingWeight
    read at nf where it belongs at nf - nign: the cluster's weight table
    (topo_log) shifted by nign entries, nign being constant over the queue."""
    s = scene(name)
    cluster, pods = s.encoded
    c = cluster.copy_state()
    c.topo_log = np.concatenate([cluster.topo_log[nign:], np.repeat(cluster.topo_log[-1], nign)])
    ora = Oracle(c, compiled(s.kind))
    chosen, _ = ora.schedule(pods)
    ora.close()
    return [int(x) for x in chosen]


def ignored_weight() -> Scene:
    """Three labelled nodes holding 4, 0 and 1 pods of the app and six large
    nodes without the hostname label, under 30 pods of the app with only the
    node-local uses: nf == 9 and nign == 6 for every pod, and the labelled
    nodes' counts differ, so the weight log(nf - nign + 2) reaches the
    placements (with log(nf + 2) they move)."""
    nodes = [node(f"l{i}", f"z{i}") for i in range(3)] + \
            [node(f"h{i}", f"z{i % 3}", cpu="32", mem="64Gi", host=False) for i in range(6)]
    bound = [bound_pod(f"b{i}-{r}", "a", f"l{i}", cpu="10m") for i, c in enumerate((4, 0, 1)) for r in range(c)]
    queue = [spread_pod(f"p{k:02d}", "a", cpu="500m", zone_skew=0) for k in range(30)]
    return Scene("ignored_weight", nodes, bound, queue, variants=False,
                 reaches={"nf == 9 with nign == 6 for every pod": lambda t: all(
                     x == 9 and int(sc.sum()) == 9 for x, sc in zip(t.nf, t.scored)),
                     "the weight at nf instead of nf - nign moves placements":
                         lambda t: unignored_weight_placements("ignored_weight", 6) != t.chosen})


# ---- variant_slots -----------------------------------------------------------------------
R, F ="8", "100m"                                 # a roomy node and one no 200m pod fits
ZONE_LAYOUT = {1: [[R, R]], 2: [[R, R], [R, F]], 3: [[R, R], [R, F], [F, F]], 4: [[R, R], [R, F], [F, F], [F, F]]}


def _zone_nodes(layout) -> List[Node]:
    return [node(f"z{d}n{k}", f"z{d}", cpu=cpu) for d, zone in enumerate(layout) for k, cpu in enumerate(zone)]


def variant_slots(nd: int) -> Scene:
    """A zone key of nd domains (nd <= kVarDom) of two nodes each; the last
    zone with a roomy node has one, and from three zones on the zones behind
    it have none.  The queue, one run:
      x, x     the reader's slots by where its adder lands: one slot has one
               feasible node (the half-full zone), another has more         (b)
      y, y     app y is bound in every roomy zone but the half-full one: the
               adder has that one node (kStatOne), and once it is there the
               reader's passing domains hold no feasible node (nf == 0)     (a)
      f, f     app f is bound in every roomy zone: only the full zone passes,
               the adder is unschedulable (slot 0) and so is the reader     (c)
      v, w     w's zone constraint selects app v (self match 0)             (d)
      four pods of other apps.
    App x is bound once in every zone (10m pods, on the full nodes where the
    zone has one): the zones stay level, so the verdicts are those of an
    unbound app, but the InterPodAffinity score map of x's anti-affinity term
    is not empty.  Without that the first placement of an app flips
    kTopoScoreNonEmpty and cuts the batch before its reader
    (k_tb_chain_pairs' hit_score), and no reader would commit on a variant
    slot."""
    layout = ZONE_LAYOUT[nd]
    nodes = _zone_nodes(layout)
    roomy = [d for d, z in enumerate(layout) if R in z]
    bound = [bound_pod(f"by{d}", "y", f"z{d}n0", cpu="10m") for d in roomy[:-1]] + \
            [bound_pod(f"bf{d}", "f", f"z{d}n0", cpu="10m") for d in roomy] + \
            [bound_pod(f"bx{d}", "x", f"z{d}n1", cpu="10m") for d in range(nd)]
    P = functools.partial(spread_pod, cpu="200m")
    queue = [P("x0", "x"), P("x1", "x"), P("y0", "y"), P("y1", "y"), P("f0", "f"), P("f1", "f"), P("v0", "v"),
             P("w0", "w", zone_sel="v")] + [P(f"t{k}", f"t{k}") for k in range(4)]
    name = f"variant_slots_{nd}"
    reaches: Dict[str, Claim] = {f"a variant key of {nd} domains": lambda t: len(
        {lb[ZONE] for lb in t.cluster.node_labels}) == nd,
        "a reader whose selector is foreign (self match 0)": static(True)}
    if nd >= 2:
        def slots_differ(t):
            per = slot_feasible(name, 0, 1)
            return 1 in per.values() and max(per.values()) > 1
        reaches["one slot has one feasible node, another several"] = slots_differ
        reaches["kStatOne for an adder"] = lambda t: t.nf[2] == 1
    if nd >= 3:
        def empty_slot(t):
            per = slot_feasible(name, 2, 3)
            return t.nf[3] == 0 and 0 in per.values() and max(per.values()) > 0
        reaches["a slot whose passing domains hold no feasible node (nf == 0), another with one"] = empty_slot
        reaches["an unschedulable adder (slot 0) and its reader"] = lambda t: t.nf[4] == 0 and t.nf[5] == 0
    return Scene(name, nodes, bound, queue, reaches=reaches, variants=nd >= 2)


def variant_two_adders() -> Scene:
    """Three zones; per app two pods that carry only a hostname constraint on
    another app (they add to the app's classes, read none of them) and then a
    pod with the zone constraint: two earlier pods of its run add the class it
    reads, so there is no adder, the run ends before it, and no pod takes a
    variant."""
    queue = []
    for k in range(4):
        app = f"e{k}"
        queue += [spread_pod(f"{app}p0", app, cpu="200m", zone_skew=0, anti=0, soft_sel="other"),
                  spread_pod(f"{app}p1", app, cpu="200m", zone_skew=0, anti=0, soft_sel="other"),
                  spread_pod(f"{app}p2", app, cpu="200m")]

    def two_adders(t):
        q = t.scene.queue
        return all(sum(q[j - d].labels["app"] == q[j].labels["app"] for d in (1, 2)) == 2
                   and q[j].topology_spread[0].when_unsatisfiable == "DoNotSchedule" for j in range(2, len(q), 3))
    return Scene("variant_two_adders", _zone_nodes(ZONE_LAYOUT[3]), [], queue, variants=False,
                 reaches={"two pods of the run add the class the third reads": two_adders})


def variant_wide(nd: int) -> Scene:
    """A zone key of nd > kVarDom domains (5; 17, past the 4-bit clamp
    min(vdom, 15u)): pairs of pods per app, no variants, runs end at the
    second pod of an app."""
    nodes = [node(f"z{d}n{k}", f"z{d}") for k in range(2) for d in range(nd)]
    queue = [spread_pod(f"p{k:02d}", f"a{k // 2}", cpu="200m") for k in range(16)]
    return Scene(f"variant_wide_{nd}", nodes, [bound_pod("b0", "a0", "z0n0"), bound_pod("b1", "a1", f"z{nd - 1}n1")],
                 queue, variants=False,
                 reaches={f"a DoNotSchedule key of {nd} values": lambda t: len(
                     {lb[ZONE] for lb in t.cluster.node_labels}) == nd,
                     "the second pod of an app loses the first's zone": lambda t: t.nf[1] < t.nf[0]})


# ---- hard_hostname -----------------------------------------------------------------------
def hard_hostname(n: int) -> Scene:
    """DoNotSchedule on the hostname key at maxSkew 1 over n nodes: the key's
    column has n + 1 values (col_nvals counts value id 0), admitted up to
    kFuseMinValues.  40 pods of 20 apps; apps a0 and a1 are bound on some
    nodes, which their pods lose."""
    nodes = zoned(n)
    bound = [bound_pod(f"b{k}", f"a{k % 2}", f"n{7 * k:05d}") for k in range(12)]
    queue = [spread_pod(f"p{k:02d}", f"a{k % 20}", cpu="200m", hard_key=HOST, host_skew=0) for k in range(40)]

    def nvals(t):
        c = t.cluster
        return len(c.label_values[c.label_keys.index(HOST)]) == n + 1
    edge = "at" if n + 1 == K_FUSE_MIN_VALUES else "one past"
    return Scene(f"hard_hostname_{n}", nodes, bound, queue, variants=False,
                 route="tbatch" if n + 1 <= K_FUSE_MIN_VALUES else "perpod",
                 reaches={f"the DoNotSchedule key has {n + 1} values, {edge} kFuseMinValues": nvals,
                          "bound pods close nodes": lambda t: t.nf[0] == n - 6})


HARD_HOSTNAME = (K_FUSE_MIN_VALUES - 1, K_FUSE_MIN_VALUES)


# ---- lone_holder -------------------------------------------------------------------------
def lone_holder(form: str = "scene") -> Scene:
    """Twelve nodes, node-local uses only (hostname ScheduleAnyway and
    preferred anti-affinity; no zone constraint), so runs cross every class
    conflict.  App a0 is bound nowhere on n00000, twice on n00001, three times
    on n00002 and once on each other node: n00000 holds a0's PodTopologySpread
    minimum and InterPodAffinity maximum alone.  The queue opens with two pods
    of a0: the first lands on n00000, so for the second (j == 1) a lone
    holder (hmin == 1 <= j) has moved and both extrema with it
    (tb_keeps_extrema).  The sizes make that matter: n00001 is large and
    empty, the others are 4-core nodes loaded to 86 % of their cpu, 85 points
    of Fit + BalancedAllocation behind it.  Against the moved extrema a node
    bound once is 96 points ahead of n00001 in the two topology scores and
    wins; against the extrema of before the first pod it is 77 ahead and
    loses.  Four more pods of a0 and thirty of two other apps follow.
      "even":  the twin, n00000 bound once as well (no lone holder);
      "empty": no pod of the apps bound, the InterPodAffinity score map starts
               empty and the first placement of an app fills it mid-batch."""
    nodes = zoned(12, cpu="4", mem="16Gi")
    nodes[1].allocatable = {"cpu": "32", "memory": "128Gi", "pods": "110"}
    bound = [Pod(f"load{i}", containers=[Container({"cpu": "3340m", "memory": "64Mi"})], node_name=f"n{i:05d}")
             for i in range(12) if i != 1]
    if form != "empty":
        counts = [1 if form == "even" else 0, 2, 3] + [1] * 9
        bound += [bound_pod(f"b{i}-{r}", "a0", f"n{i:05d}", cpu="1m", mem="1Mi") for i, c in enumerate(counts)
                  for r in range(c)]
    queue = [spread_pod(f"p{k:02d}", "a0" if k < 6 else f"a{1 + k % 2}", zone_skew=0) for k in range(36)]
    if form == "scene":
        reaches = {"the first pod takes the lone holder of its app's extrema, the next pod is of the app":
                   first_pod_takes_the_lone_holder,
                   "against the extrema of before the first pod the second is placed elsewhere":
                   stale_extrema_move_the_choice}
    elif form == "empty":
        reaches = {"kTopoScoreNonEmpty flips inside a batch": ipa_map_fills_mid_window}
    else:
        reaches = {"no lone holder before the first pod": lambda t: _lone(t.pts[0], t.scored[0], False) < 0}
    return Scene("lone_holder" + ("" if form == "scene" else "_" + form), nodes, bound, queue, reaches=reaches,
                 variants=False, twin="lone_holder_even" if form == "scene" else None)


# ---- tiny_tainted ------------------------------------------------------------------------
def tiny_one_node() -> Scene:
    """One node, two apps at maxSkew 1 over its one zone."""
    return Scene("tiny_one_node", zoned(1), [], [spread_pod(f"p{k}", f"a{k % 2}") for k in range(8)],
                 reaches={"every pod has one feasible node": nf_all(1), "N == 1": lambda t: t.cluster.n_nodes == 1})


def tiny_tainted() -> Scene:
    """Two nodes in two zones, one tainted NoSchedule; the pods tolerate
    nothing and their hostname constraint carries nodeTaintsPolicy Honor.  The
    tainted node's zone still counts as a domain of the zone constraint
    (nodeTaintsPolicy Ignore there), so an app's second pod finds no node."""
    nodes = [node("n0", "z0"), node("n1", "z1", taints=[Taint("dedicated", "infra", "NoSchedule")])]
    queue = [spread_pod(f"p{k}", f"a{k % 3}", soft_taints="Honor") for k in range(9)]
    return Scene("tiny_tainted", nodes, [], queue,
                 reaches={"the first pod of an app has one feasible node, the next none": nf_is(1, 1, 1, 0, 0, 0),
                          "unschedulable pods inside a run": unschedulable_inside_a_window})


WAVE = range(64, 128)


def tiny_one_wave() -> Scene:
    """300 nodes of which only positions 64 .. 127 fit a 200m pod: the
    feasible set is one 64-lane wave of block 0, the block's other three waves
    and the whole of block 1 list nothing."""
    nodes = zoned(300, cpu=F)
    for p in WAVE:
        nodes[p].allocatable = {"cpu": "4", "memory": "32Gi", "pods": "110"}
    return Scene("tiny_one_wave", nodes, [], many_apps(24, cpu="200m"), positional=True, variants=False,
                 reaches={"every scored node lies in one wave of block 0":
                          lambda t: all(sc.any() and not sc[:WAVE.start].any() and not sc[WAVE.stop:].any()
                                        for sc in t.scored),
                          "64 feasible nodes": nf_all(len(WAVE))})


# ---- the registry ------------------------------------------------------------------------
def _registry() -> Dict[str, Callable[[], Scene]]:
    out: Dict[str, Callable[[], Scene]] = {}

    def add(name, make):
        out[name] = make
    for f in (nf_ladder, nf_ladder_full_one_app, nf_ladder_full_apps, exhausted_list, mostly_ignored, ignored_weight,
              variant_two_adders, tiny_one_node,
              tiny_tainted, tiny_one_wave):
        add(f.__name__, f)
    for n in FEW_NODES:
        add(f"many_apps_few_nodes_{n}", functools.partial(many_apps_few_nodes, n))
    for n in RUN_LENGTHS:
        add(f"run_lengths_{n}", functools.partial(run_lengths, n))
    for n in BLOCK_EDGES:
        add(f"block_edges_{n}", functools.partial(block_edges, n))
    add(f"block_edges_{BLOCK + 1}_twin", functools.partial(block_edges, BLOCK + 1, True))
    for form in ("scene", "labelled", "zoneless"):
        add("ignored_and_unkeyed" + ("" if form == "scene" else "_" + form),
            functools.partial(ignored_and_unkeyed, form))
    for nd in sorted(ZONE_LAYOUT):
        add(f"variant_slots_{nd}", functools.partial(variant_slots, nd))
    for nd in (K_VAR_DOM + 1, 17):
        add(f"variant_wide_{nd}", functools.partial(variant_wide, nd))
    for n in HARD_HOSTNAME:
        add(f"hard_hostname_{n}", functools.partial(hard_hostname, n))
    for form in ("scene", "even", "empty"):
        add("lone_holder" + ("" if form == "scene" else "_" + form), functools.partial(lone_holder, form))
    return out


SCENES = _registry()


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    """The scene, built once."""
    s = SCENES[name]()
    assert s.name == name, (s.name, name)
    return s


# the edges the topology batch path had no test for, each named by some scene's reaches
EDGES = {
    "nf == 0": ("nf_ladder_full_one_app", "nf == 0"),
    "nf == 1 (kStatOne)": ("nf_ladder", "kStatOne: a pod with one feasible node"),
    "has_soft = nf > 1": ("nf_ladder", "has_soft off and on inside a run (nf 1 next to nf 2)"),
    "nf <= kTopT (topk_complete)": ("many_apps_few_nodes_8", "nf == kTopT"),
    "nf == kTopT + 1": ("many_apps_few_nodes_9", "nf == kTopT + 1: the smallest incomplete list"),
    "an exhausted incomplete list cuts the chain": (
        "exhausted_list", "the ninth pod's list (the first eight nodes) is taken; it lands on the ninth node"),
    "unschedulable pods inside a run": ("nf_ladder_full_apps", "unschedulable pods inside a run"),
    "IgnoredNodes": ("ignored_and_unkeyed", "the hostless node is chosen"),
    "nf - nign == 1 and 0": ("mostly_ignored", "nf - nign == 1, then 0"),
    "topo_log[nf - nign]": ("ignored_weight", "the weight at nf instead of nf - nign moves placements"),
    "a node without a table-read key": ("ignored_and_unkeyed", "the unkeyed node is chosen"),
    "nd == 1": ("many_apps_few_nodes_9", "a variant key of one domain"),
    "a key past the 4-bit clamp": ("variant_wide_17", "a DoNotSchedule key of 17 values"),
    "a slot with nf == 0": ("variant_slots_3",
                            "a slot whose passing domains hold no feasible node (nf == 0), another with one"),
    "a slot with nf == 1 next to a larger one": ("variant_slots_3", "one slot has one feasible node, another several"),
    "an unschedulable adder": ("variant_slots_3", "an unschedulable adder (slot 0) and its reader"),
    "a foreign selector": ("variant_slots_2", "a reader whose selector is foreign (self match 0)"),
    "two adders end the run": ("variant_two_adders", "two pods of the run add the class the third reads"),
    "a partial last block": ("block_edges_257", "the last block is partial"),
    "N == kTbMaxBlocks * 256": ("block_edges_16384", "N == kTbMaxBlocks * 256: every lane of k_tb_merge holds a block"),
    "N past kTbMaxBlocks * 256": ("block_edges_16385", "N past kTbMaxBlocks * 256"),
    "a tie across a block boundary": ("block_edges_257",
                                      "a node of the block before is chosen (the tie crosses a block boundary)"),
    "runs of kTbPods and kTbPods + 1 pods": ("run_lengths_33", "a queue of 33 pods (tb_count)"),
    "hard_small at kFuseMinValues": ("hard_hostname_255", "the DoNotSchedule key has 256 values, at kFuseMinValues"),
    "hard_small past kFuseMinValues": ("hard_hostname_256",
                                       "the DoNotSchedule key has 257 values, one past kFuseMinValues"),
    "a lone extremum holder guessed earlier": (
        "lone_holder", "the first pod takes the lone holder of its app's extrema, the next pod is of the app"),
    "kTopoScoreNonEmpty flips": ("lone_holder_empty", "kTopoScoreNonEmpty flips inside a batch"),
    "one-wave feasible set": ("tiny_one_wave", "every scored node lies in one wave of block 0"),
}
