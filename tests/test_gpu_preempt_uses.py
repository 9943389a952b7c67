"""ksim_preempt / ksim_preempt_nominated for preemptors that carry uses
(csrc/ksim_preempt.hip, ksim_set_bound_pod_adds).

Score-only uses (ScheduleAnyway spread, a preferred pod-affinity term, an
image some nodes hold): the engine's 4-tuple must equal the C oracle's for the
same pod with the uses stripped, on every case of tests/preemptcases.py,
without and with a nominated group.

Host ports: the oracle refuses these pods, so the reference is the numpy
restatement tests/preemptref.py (pinned to the oracle on use-free pods by
tests/test_preempt_uses.py) over the oracle's own per-node filter statuses.
Shapes run from 3 nodes to 300, across the 64-lane wave and the 256-thread
block of k_preempt_nodes."""
import dataclasses
import functools
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import pytest

import preemptcases as pc
import preemptref
from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.model import (Container, ContainerPort, Controller, LabelSelector, Node, Pod, PodAffinityTerm,
                        TopologySpreadConstraint, WeightedPodAffinityTerm)
from ksim.preemption import bound_table
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"
IMAGE = "registry.example/app:v1"


# ---- objects ---------------------------------------------------------------------------
def _nodes(n: int) -> List[Node]:
    """preemptcases' nodes (10 CPUs) in one zone (nodeTree order == list order),
    every other one holding the image."""
    return [Node(name=f"n{i:04d}", labels={HOST: f"n{i:04d}", ZONE: "z0"},
                 allocatable={"cpu": f"{pc.ALLOC_CPU}m", "memory": "64Gi", "pods": "110"},
                 images=[([IMAGE], 500 * 2 ** 20)] if i % 2 == 0 else []) for i in range(n)]


def _bound(nodes, rows):
    """rows: (node, priority, start, cpu milli[, host ports]) -> bound pods, start times.
    A third of them carry app=y (the preferred affinity term counts them), a
    third app=x (the spread constraint does)."""
    bound, start = [], {}
    for i, row in enumerate(rows):
        node, prio, st, cpu = row[:4]
        ports = row[4] if len(row) > 4 else ()
        labels = {"app": "y"} if i % 3 == 0 else {"app": "x"} if i % 3 == 1 else {}
        bound.append(Pod(f"b{i}", node_name=nodes[node].name, priority=int(prio), labels=labels,
                         containers=[Container({"cpu": f"{cpu}m"}, [ContainerPort(*p) for p in ports])]))
        start[f"b{i}"] = int(st)
    return bound, start


def _preemptor(prio: int, cpu: int, ports=(), score_uses=True, name="preemptor") -> Pod:
    p = Pod(name, priority=prio, containers=[Container({"cpu": f"{cpu}m"}, [ContainerPort(*x) for x in ports])])
    if score_uses:
        p.labels = {"app": "x"}
        p.containers[0].image = IMAGE
        p.topology_spread = [TopologySpreadConstraint(1, ZONE, "ScheduleAnyway", LabelSelector({"app": "x"}))]
        p.pod_affinity_preferred = [WeightedPodAffinityTerm(10, PodAffinityTerm(ZONE, LabelSelector({"app": "y"})))]
    return p


def _kinds(enc, index=0) -> List[int]:
    p = enc.pods[index]
    return [int(k) for k in enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]]


def _profile(args=(10, 100), ports="default", pct=100):
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=pct, preemption=profile.PreemptionArgs(*args))
    en = sp.plugins["filter"].enabled
    at = {profile.original_name(p.name): i for i, p in enumerate(en)}
    if ports == "after_fit":
        pl = en.pop(at["NodePorts"])
        en.insert(at["NodeResourcesFit"], pl)              # Fit moved up by the pop: this lands behind it
        assert sp.filter_order().index("NodePorts") == sp.filter_order().index("NodeResourcesFit") + 1
    elif ports == "absent":
        en.pop(at["NodePorts"])
    return sp, profile.compile_profile(sp)


@pytest.fixture(scope="module")
def engines():
    """One handle per cluster, created once every pod of its test is encoded
    (a later compile could add count classes the device table lacks)."""
    from ksim.engine import Engine
    held = {}

    def get(cluster, prof):
        key = id(cluster)
        if key not in held:
            if len(held) >= 4:                           # keep few handles open
                held.pop(next(iter(held)))[0].close()
            e = Engine(0)
            e.set_profile(prof)
            e.set_cluster(cluster)
            held[key] = (e, cluster)
        else:
            held[key][0].set_profile(prof)
        return held[key][0]

    yield get
    for e, _ in held.values():
        e.close()


# ---- score-only uses against the oracle -------------------------------------------------
@functools.lru_cache(maxsize=4)
def _uses_cluster(n_nodes: int, load: tuple):
    """The cluster of ``n_nodes`` nodes holding pods of these (node, cpu), with
    the classes of the use-carrying preemptor and the nominated pod registered."""
    nodes = _nodes(n_nodes)
    bound, _ = _bound(nodes, [(n, 0, 0, c) for n, c in load])
    cluster, _ = encode_cluster(nodes, bound)
    assert list(cluster.node_names) == [n.name for n in nodes]
    encode_pods(cluster, [_preemptor(0, 100), _preemptor(0, 100, score_uses=False), _nominated(0)])
    return cluster


def _nominated(prio: int) -> Pod:
    return Pod("nominated", priority=prio, containers=[Container({"cpu": "700m"})])


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_score_only_uses_equal_the_oracle_without_them(engines, name, grouped):
    case = pc.all_cases()[name]
    cluster = _uses_cluster(case.n_nodes, tuple((r[0], r[3]) for r in case.rows))
    classes = cluster.class_count.shape[0]
    prio, cpu = case.preemptor
    rich = encode_pods(cluster, [_preemptor(prio, cpu), _nominated(prio + 1)])
    bare = encode_pods(cluster, [_preemptor(prio, cpu, score_uses=False), _nominated(prio + 1)])
    assert cluster.class_count.shape[0] == classes               # the device table stays valid
    assert {abi.USE_PTS_SOFT, abi.USE_IMAGE, abi.USE_IPA_SCORE} <= set(_kinds(rich)) and _kinds(bare) == []
    rows = np.array(case.rows, np.int64).reshape(-1, 4)
    req = np.zeros((len(case.rows), abi.PREEMPT_REQ), np.int64)
    req[:, 0] = rows[:, 3]
    table = abi.BoundPods(rows[:, 0], rows[:, 1], rows[:, 2], req)
    _, prof = _profile(case.args)
    groups = [(min(1, case.n_nodes - 1), [1])] if grouped else None
    eng = engines(cluster, prof)
    eng.set_bound_pods(table)                                    # no adds: a pod without port uses needs none
    got = eng.preempt(rich, 0, prio, groups=groups)
    want = Oracle(cluster, prof).preempt(bare, 0, prio, table, groups)
    assert got == want
    if not grouped:
        assert got[0] == case.winner


# ---- host ports against preemptref --------------------------------------------------------
@dataclass
class Scene:
    cluster: object
    enc: object                                   # pod 0: the preemptor; then further preemptors / nominated pods
    table: object
    prof: object
    priority: int
    groups: Optional[List[Tuple[int, List[int]]]] = None
    bound: list = field(default_factory=list)
    start: dict = field(default_factory=dict)


def _scene(n_nodes, rows, pods, priority, prof=None, groups=None) -> Scene:
    nodes = _nodes(n_nodes)
    bound, start = _bound(nodes, rows)
    cluster, _ = encode_cluster(nodes, bound)
    assert list(cluster.node_names) == [n.name for n in nodes]
    enc = encode_pods(cluster, pods)
    table = bound_table(cluster, bound, start, cluster.topo)     # after the compile: its port classes exist
    return Scene(cluster, enc, table, prof or _profile()[1], priority, groups, bound, start)


def _statuses(sc: Scene, index=0) -> np.ndarray:
    """Per node the first failing filter of the oracle's cycle for the pod; a
    grouped node's is RunFilterPluginsWithNominatedPods' (pass 1 with the
    group assumed unless that passes)."""
    fail = Oracle(sc.cluster, sc.prof).cycle(sc.enc, index)["fail_plugin"].copy()
    for node, idx in sc.groups or []:
        o = Oracle(sc.cluster, sc.prof)
        for j in idx:
            o.assume(sc.enc, j, node)
        f1 = int(o.cycle(sc.enc, index)["fail_plugin"][node])
        if f1 != abi.PASSED:
            fail[node] = f1
    return fail


def _reference(sc: Scene, index=0, priority=None) -> tuple:
    req, ports = preemptref.pod_inputs(sc.enc, index)
    fit, port = preemptref.filter_positions(sc.prof)
    groups = [preemptref.group_inputs(sc.enc, idx, node) for node, idx in sc.groups or []]
    return preemptref.dry_run(_statuses(sc, index), preemptref.columns(sc.cluster), sc.table,
                              sc.priority if priority is None else priority, req, ports, fit, port,
                              sc.prof.preempt_min_pct, sc.prof.preempt_min_abs, groups)


def _engine(engines, sc: Scene, index=0, priority=None, set_table=True) -> tuple:
    eng = engines(sc.cluster, sc.prof)
    if set_table:
        eng.set_bound_pods(sc.table)
    return eng.preempt(sc.enc, index, sc.priority if priority is None else priority, groups=sc.groups)


W80 = (80, "TCP", "")                             # 0.0.0.0:80


def _ports_only_scene():
    """70 nodes; each holds the port (priority 10) beside two portless pods of
    lower priority still; the preemptor (2 CPUs of the 7 free) fails NodePorts
    alone.  Node 37's holder has the lowest priority of all holders."""
    rows = []
    for v in range(70):
        rows += [(v, 5 if v == 37 else 10, 100, 1000, [W80]), (v, 3, 50, 1000), (v, 1, 60, 1000)]
    return _scene(70, rows, [_preemptor(1000, 2000, [W80])], 1000)


def test_port_holder_is_the_single_victim(engines):
    sc = _ports_only_scene()
    fit, port = preemptref.filter_positions(sc.prof)
    assert (_statuses(sc) == port).all() and port < fit
    want = _reference(sc)
    assert want == (37, [37 * 3], 70, 70)         # the two less important pods are reprieved
    assert _engine(engines, sc) == want


def test_holder_at_or_above_the_preemptors_priority_is_no_candidate(engines):
    rows = []
    for v in range(5):
        rows += [(v, 1000 if v == 2 else 2000, 100, 1000, [W80]), (v, 3, 50, 1000)]
    sc = _scene(5, rows, [_preemptor(1000, 2000, [W80])], 1000)
    want = _reference(sc)
    assert want == (-1, [], 5, 0)
    assert _engine(engines, sc) == want


def _ports_and_cpu_rows(n):
    """Every node: the holder (priority 30, 3 CPUs) and two portless pods (20 and
    10, 3 CPUs each): 9 of 10 CPUs used.  Node n - 20's pods rank lowest.  For
    a 5-CPU preemptor Fit alone evicts the pods of priority 20 and 10 (rows 0
    and 2 of the node) and keeps the holder."""
    rows = []
    for v in range(n):
        d = 5 if v == n - 20 else 0
        rows += [(v, 20 - d, 100, 3000), (v, 30 - d, 100, 3000, [W80]), (v, 10 - d, 100, 3000)]
    return rows


def test_port_and_cpu_victims(engines):
    """300 nodes (two blocks): the holder, first in the reprieve order, stays out
    for its port; the preemptor (5 CPUs) then fits beside the next pod, and the
    least important one goes for CPU.  Fit alone would have kept the holder."""
    sc = _scene(300, _ports_and_cpu_rows(300), [_preemptor(1000, 5000, [W80])], 1000,
                prof=_profile((100, 0))[1])
    want = _reference(sc)
    assert want == (280, [280 * 3 + 1, 280 * 3 + 2], 300, 300)
    assert _engine(engines, sc) == want


def test_two_holders_of_one_wildcard_class(engines):
    """10.0.0.1:80 and 10.0.0.2:80 on a node both conflict with 0.0.0.0:80."""
    rows = []
    for v in range(65):
        rows += [(v, 10, 100, 1000, [(80, "TCP", "10.0.0.1")]), (v, 20, 100, 1000, [(80, "TCP", "10.0.0.2")]),
                 (v, 5, 100, 1000)]
    rows[64 * 3] = (64, 8, 100, 1000, [(80, "TCP", "10.0.0.1")])          # the last lane of the second wave
    sc = _scene(65, rows, [_preemptor(1000, 2000, [W80])], 1000)
    want = _reference(sc)
    assert want == (64, [64 * 3 + 1, 64 * 3], 65, 65)
    assert _engine(engines, sc) == want


@pytest.mark.parametrize("wants, holds", [((80, "TCP", "10.0.0.5"), W80), (W80, (80, "TCP", "10.0.0.5"))],
                         ids=["specific_vs_wildcard", "wildcard_vs_specific"])
def test_specific_ip_against_wildcard(engines, wants, holds):
    """A specific ip conflicts with 0.0.0.0 and the reverse; another specific ip
    (node 1, full of CPU) does not, so there only Fit picks the victims."""
    rows = [(0, 10, 100, 1000, [holds]), (0, 5, 100, 1000),
            (1, 10, 100, 4000, [(80, "TCP", "10.0.0.6")]), (1, 5, 100, 5000),
            (2, 2000, 100, 1000, [holds])]
    sc = _scene(3, rows, [_preemptor(1000, 2000, [wants])], 1000)
    fit, port = preemptref.filter_positions(sc.prof)
    st = _statuses(sc)
    # 10.0.0.6 conflicts with 0.0.0.0 too: node 1 fails NodePorts only for the wildcard preemptor
    assert st[0] == port and st[2] == port and st[1] == (port if wants == W80 else fit)
    want = _reference(sc)
    assert want[0] in (0, 1) and want[2] == 3 and want[3] == 2
    assert _engine(engines, sc) == want


def test_sixteen_uses_ports_interleaved_with_score_uses(engines):
    """KSIM_MAX_USES uses, NodePorts ones at 0, 3, 5, 8, 11 and 15 between
    score-only ones; each node holds one of the five ports, so every port use
    decides somewhere."""
    wanted = [(80, "TCP", ""), (81, "TCP", ""), (82, "TCP", "10.0.0.5"), (83, "UDP", ""), (84, "TCP", "")]
    held = [(80, "TCP", "10.1.1.1"), (81, "TCP", ""), (82, "TCP", "10.0.0.5"), (83, "UDP", "10.2.2.2"),
            (84, "TCP", ""), (82, "TCP", "")]
    rows = []
    for v in range(130):
        rows += [(v, 10 + v % 7, 100 + v, 1000, [held[v % 6]]), (v, 5, 100, 1000)]
    sc = _scene(130, rows, [_preemptor(1000, 2000, wanted)], 1000, prof=_profile((100, 0))[1])
    p = sc.enc.pods[0]
    u = sc.enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
    port = [x for x in u if int(x["kind"]) == abi.USE_NODE_PORT]
    score = [x for x in u if int(x["kind"]) != abi.USE_NODE_PORT]
    assert len(port) == 6 and len(score) >= 3
    order = "PSSPSPSSPSSPSSSP"
    uses = np.zeros(abi.MAX_USES, abi.TOPO_USE_DTYPE)
    pi = si = 0
    for k, c in enumerate(order):
        if c == "P":
            uses[k] = port[pi]
            pi += 1
        else:
            uses[k] = score[si % len(score)]
            si += 1
    pods = sc.enc.pods.copy()
    pods[0]["use_first"], pods[0]["use_count"] = 0, abi.MAX_USES
    sc = dataclasses.replace(sc, enc=dataclasses.replace(sc.enc, pods=pods, uses=uses))
    assert [int(k) == abi.USE_NODE_PORT for k in _kinds(sc.enc)] == [c == "P" for c in order]
    want = _reference(sc)
    assert want[2:] == (130, 130) and len(want[1]) == 1
    assert _engine(engines, sc) == want


def test_node_ports_after_fit_in_the_profile(engines):
    """Fit first: nodes short of CPU fail Fit although they also hold the port;
    nodes with CPU to spare fail NodePorts.  Both kinds are potential nodes."""
    rows = _ports_and_cpu_rows(40)
    for v in range(40, 70):
        rows += [(v, 12, 100, 1000, [W80]), (v, 3, 50, 1000)]
    sc = _scene(70, rows, [_preemptor(1000, 5000, [W80])], 1000, prof=_profile((100, 0), ports="after_fit")[1])
    fit, port = preemptref.filter_positions(sc.prof)
    st = _statuses(sc)
    assert port == fit + 1 and (st[:40] == fit).all() and (st[40:] == port).all()
    want = _reference(sc)
    assert want[2:] == (70, 70)
    assert _engine(engines, sc) == want


def test_node_ports_absent_from_the_profile(engines):
    """No NodePorts filter: the port uses are ignored, the result is the
    oracle's for the pod without them, and no adds are needed."""
    sp, prof = _profile((100, 0), ports="absent")
    assert "NodePorts" not in sp.filter_order()
    sc = _scene(70, _ports_and_cpu_rows(70), [_preemptor(1000, 5000, [W80]),
                                              _preemptor(1000, 5000, score_uses=False, name="bare")], 1000, prof=prof)
    assert abi.USE_NODE_PORT in _kinds(sc.enc, 0) and _kinds(sc.enc, 1) == []
    want = Oracle(sc.cluster, prof).preempt(sc.enc, 1, 1000, sc.table)
    assert want == _reference(sc) == (50, [150, 152], 70, 70)    # Fit alone: the holder (row 151) stays
    eng = engines(sc.cluster, prof)
    eng.set_bound_pods(bound_table(sc.cluster, sc.bound, sc.start))
    assert eng.preempt(sc.enc, 0, 1000) == want


def test_nominated_group_holding_the_port(engines):
    """Node 0's port is held by a nominated pod of higher priority: it is no
    bound pod, cannot be evicted, and the node is a potential node but no
    candidate.  Node 1's holder is bound and of lower priority."""
    rows = [(0, 5, 100, 1000), (0, 6, 100, 1000),
            (1, 10, 100, 1000, [W80]), (1, 5, 100, 1000),
            (2, 2000, 100, 9000)]
    nom = Pod("nominated", priority=1500, containers=[Container({"cpu": "500m"}, [ContainerPort(*W80)])])
    sc = _scene(3, rows, [_preemptor(1000, 2000, [W80]), nom], 1000, groups=[(0, [1])])
    fit, port = preemptref.filter_positions(sc.prof)
    assert _statuses(sc).tolist() == [port, port, fit]
    want = _reference(sc)
    assert want == (1, [2], 3, 1)
    assert _engine(engines, sc) == want


def test_two_preemptors_in_sequence_on_one_handle(engines):
    """A port preemptor, then a portless one of lower priority on the same table
    and handle: the second result carries no victim flags and no holdings of
    the first."""
    sc = _scene(70, _ports_and_cpu_rows(70), [_preemptor(1000, 5000, [W80]),
                                              _preemptor(25, 2000, score_uses=False, name="second")], 1000,
                prof=_profile((100, 0))[1])
    first = _engine(engines, sc)
    assert first == _reference(sc) and len(first[1]) == 2
    second = _engine(engines, sc, index=1, priority=25, set_table=False)
    assert second == Oracle(sc.cluster, sc.prof).preempt(sc.enc, 1, 25, sc.table)
    assert second == _reference(sc, index=1, priority=25)
    assert second == (50, [152], 70, 70)                         # only the least important pod of node 50 goes


# ---- interface ---------------------------------------------------------------------------
def test_hard_spread_preemptor_is_still_refused(engines):
    from ksim.engine import KsimError
    hard = _preemptor(1000, 2000, score_uses=False)
    hard.labels = {"app": "x"}
    hard.topology_spread = [TopologySpreadConstraint(1, ZONE, "DoNotSchedule", LabelSelector({"app": "x"}))]
    sc = _scene(3, [(0, 5, 100, 9000), (1, 5, 100, 9000), (2, 5, 100, 9000)], [hard], 1000)
    assert _kinds(sc.enc) == [abi.USE_PTS_HARD]
    with pytest.raises(KsimError) as e:
        _engine(engines, sc)
    assert e.value.code == abi.E_UNSUPPORTED and "PTS_HARD" in str(e.value)


def test_adds_call_contract(engines):
    """Without the adds a port preemptor is E_INVALID (the message names the
    call); a class out of range is E_INVALID; a new table drops the adds."""
    from ksim.engine import KsimError
    sc = _ports_only_scene()
    plain = bound_table(sc.cluster, sc.bound, sc.start)
    eng = engines(sc.cluster, sc.prof)
    eng.set_bound_pods(plain)
    with pytest.raises(KsimError) as e:
        eng.preempt(sc.enc, 0, 1000)
    assert e.value.code == abi.E_INVALID and "ksim_set_bound_pod_adds" in str(e.value)
    off = np.zeros(plain.n + 1, np.int32)
    off[1:] = 1
    for cls in (sc.cluster.class_count.shape[0], -1):
        with pytest.raises(KsimError) as e:
            eng.set_bound_pod_adds(off, [[cls, 1]])
        assert e.value.code == abi.E_INVALID
    with pytest.raises(KsimError) as e:
        eng.set_bound_pod_adds(off[::-1].copy(), [[0, 1]])       # offsets not monotone
    assert e.value.code == abi.E_INVALID
    eng.set_bound_pod_adds(sc.table.adds_off, sc.table.adds)     # the adds alone, after the table
    want = _reference(sc)
    assert eng.preempt(sc.enc, 0, 1000) == want
    eng.set_bound_pods(plain)                                    # a new table: the adds are gone
    with pytest.raises(KsimError) as e:
        eng.preempt(sc.enc, 0, 1000)
    assert e.value.code == abi.E_INVALID
    eng.set_bound_pods(sc.table)                                 # table and adds together
    assert eng.preempt(sc.enc, 0, 1000) == want


# ---- the framework mirror ------------------------------------------------------------------
def test_framework_post_filter_nominates_for_a_replicaset_pod(engines):
    """A ReplicaSet-selected pod (System default spreading: two ScheduleAnyway
    uses) of high priority on a full cluster: the framework-driven cycle ends
    in DefaultPreemption's nomination, the one the oracle gives the same pod
    compiled without the defaults."""
    from fwmirror import EngineBackend, Framework
    from ksim.fwplugins import EnginePlugins
    from ksim.resultstore import Store
    from ksim.topology import SpreadDefaults
    nodes = _nodes(12)
    rows = []
    for v in range(12):
        rows += [(v, 10 + v % 3, 100 + v, 4500), (v, 50, 100, 4500)]
    bound, start = _bound(nodes, rows)
    cluster, _ = encode_cluster(nodes, bound)
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=0)
    prof = profile.compile_profile(sp)
    pod = Pod("web-1", priority=1000, labels={"app": "web"}, owner=("apps/v1", "ReplicaSet", "web"),
              containers=[Container({"cpu": "3000m"})])
    spread = SpreadDefaults(sp.spread, [], [Controller("ReplicaSet", "web", "default", LabelSelector({"app": "web"}))])
    enc = encode_pods(cluster, [pod], spread=spread)
    bare = encode_pods(cluster, [pod])
    assert (enc.pods["topo_flags"] & abi.POD_PTS_SYSTEM_DEFAULT).all()
    assert _kinds(enc).count(abi.USE_PTS_SOFT) == 2 and _kinds(bare) == []
    table = bound_table(cluster, bound, start, cluster.topo)
    eng = engines(cluster, prof)
    fw = Framework(EnginePlugins(EngineBackend(eng), cluster, sp), sp, Store(profile.default_score_weights()), seed=1)
    rec = fw.schedule_one(enc, 0, 1000, table)
    want = Oracle(cluster, prof).preempt(bare, 0, 1000, table)
    assert rec["status"] == abi.STATUS_UNSCHEDULABLE and rec["chosen"] == -1
    assert rec["nominated"] == want[0] >= 0 and rec["victims"] == want[1] and len(want[1]) == 1
