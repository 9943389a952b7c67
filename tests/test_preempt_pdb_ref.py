"""The reference of the dry run with PodDisruptionBudgets
(tests/preemptpdbref.py) and the host side of the budgets, on the CPU.

1. Agreement on what already exists: with no budget, and with a budget that
   matches no lower-priority pod, the reference equals oracle/objref.py
   ObjScheduler.preempt (node and victims) and the C oracle (the 4-tuple, no
   violation) on every case of tests/preemptcases.py, without and with a
   nominated group.
2. Every scene of tests/preemptpdbcases.py has the property its name claims,
   every faulty variant (preemptpdbref.FAULTS) differs from the reference on
   the scenes aimed at it, and the cut scenes sit where they say.
3. ksim.preemption.pdb_matches / bound_table(pdbs=...) and
   ksim.k8sjson.pdb_from_dict on the corners of the match rule.
4. The export exists."""
import numpy as np
import pytest

import preemptcases as pc
import preemptpdbcases as pp
import preemptpdbref
from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.k8sjson import pdb_from_dict
from ksim.model import Container, LabelSelector, Pod, PodDisruptionBudget, Requirement
from ksim.preemption import bound_table, pdb_matches
from oracle.objref import ObjScheduler
from oracle.oracle import Oracle


# ---- 1. what already exists ------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_reference_equals_objref_and_oracle_without_effective_budgets(name, grouped):
    case = pc.all_cases()[name]
    prio = case.preemptor[0]
    nodes, bound, start, order, pod = pc.objects(case)
    names = [n.name for n in nodes]
    nom = Pod("nominated", priority=prio + 1, labels=dict(pp.A), containers=[Container({"cpu": "700m"})])
    at = min(1, case.n_nodes - 1)
    nominated = {names[at]: [nom]} if grouped else None
    ref = ObjScheduler(nodes, bound, pct=100, seed=0, preemption=profile.PreemptionArgs(*case.args))
    want_obj = ref.preempt(pod, prio, start, order, nominated=nominated)
    cluster, table, _, prof = pc.encoded(case)
    assert list(cluster.node_names) == names
    enc = encode_pods(cluster, [pod, nom])
    want = Oracle(cluster, prof).preempt(enc, 0, prio, table, [(at, [1])] if grouped else None)
    # a budget over app=a with nothing allowed: only pods that outrank the preemptor (and the
    # nominated pod) carry the label
    for q in bound:
        if q.priority >= prio:
            q.labels = dict(pp.A)
    for pdbs in ([], [pp.pdb("guard", app="a")]):
        got = preemptpdbref.dry_run(nodes, bound, start, order, pod, prio, case.args, nominated, pdbs)
        assert got[:2] == want_obj
        assert preemptpdbref.as_indices(got, names, order) == want + (0,)
    if not grouped:
        assert want[0] == case.winner


# ---- 2. the scenes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pp.scene_ids())
def test_scene_has_the_property_its_name_claims(name):
    sc = pp.scenes()[name]
    got = pp.reference(name)
    assert sc.claim is not None and sc.claim(sc, got), got
    # no scene is vacuous: a budget matches a lower-priority pod of a potential node
    assert any(preemptpdbref.matching(q, sc.pdbs) for q in sc.bound if q.priority < pp.PRIO) or \
        name in ("other_namespace", "empty_selector", "unlabelled_pod", "disrupted_pod")
    for fault in sc.aims:
        assert pp.reference(name, False, fault) != got, fault


@pytest.mark.parametrize("fault", preemptpdbref.FAULTS)
def test_scenes_discriminate(fault):
    aimed = [name for name, sc in pp.scenes().items() if fault in sc.aims]
    assert aimed, f"no scene is aimed at {fault}"
    assert any(pp.reference(name, False, fault) != pp.reference(name) for name in aimed)


def test_scene_properties_in_detail():
    sc = pp.scenes()
    # level 1 decides among five candidates that tie on every level below it
    got = pp.reference("violations_level")
    assert got[3] >= 3 and got[4] == 0
    assert pp.reference("violations_level", False, "no_violation_level")[0] == "n0000"
    rows = {(q.priority, sc["violations_level"].start[q.name]) for q in sc["violations_level"].bound}
    assert len(rows) == 1
    # victims[0] is not the highest-priority victim
    s, got = sc["high_is_first"], pp.reference("high_is_first")
    prio = {q.name: q.priority for q in s.bound}
    assert prio[got[1][0]] < max(prio[v] for v in got[1])
    # more candidates kept than numCandidates
    for name, s in sc.items():
        if s.want is not None:
            got = pp.reference(name)
            assert got[3] > s.want and pp.reference(name, False, "old_cut")[3] == s.want, name
    # a group's pod matches the budget and consumes nothing
    s = sc["nominated_consume_nothing"]
    assert preemptpdbref.matching(s.pods[1], s.pdbs) == [0] and s.pods[1].priority >= pp.PRIO


def test_cut_scenes_sit_at_the_chunk_and_wave_boundaries():
    for n in pp.CUT_N:
        chunk = (n + pp.PICK_THREADS - 1) // pp.PICK_THREADS
        at = pp.cut_positions(n)
        assert len(at) == 4 and all(c - 1 >= pp.CUT_WANT for c in at)
        # a pair either side of a thread's chunk, a pair either side of a wave
        assert any(a + 1 == b and a // chunk != b // chunk and a // (chunk * 64) == b // (chunk * 64)
                   for a, b in zip(at, at[1:]))
        assert any(a + 1 == b and a // (chunk * 64) != b // (chunk * 64) for a, b in zip(at, at[1:]))
        for c in at:
            s = pp.scenes()[f"cut_n{n}_at{c}"]
            assert s.want == min(max(n * s.args[0] // 100, s.args[1]), n) == pp.CUT_WANT
    assert {(n + 1023) // 1024 for n in pp.CUT_N} == {1, 2, 3}


# ---- 3. the host side ---------------------------------------------------------------------------
def _pod(name, labels, namespace="default"):
    return Pod(name, namespace=namespace, labels=dict(labels), containers=[Container({"cpu": "100m"})])


def test_pdb_matches_on_the_corners_of_the_rule():
    pdbs = [pp.pdb("a", app="a"),                                            # 0 plain
            pp.pdb("other", namespace="other", app="a"),                     # 1 another namespace
            PodDisruptionBudget("empty", "default", LabelSelector(), 0),     # 2 empty selector
            PodDisruptionBudget("nil", "default", None, 0),                  # 3 nil selector
            pp.pdb("gone", disrupted=["p0"], app="a"),                       # 4 p0 already disrupted
            PodDisruptionBudget("nox", "default", LabelSelector({}, [Requirement("x", "DoesNotExist", [])]), 0),  # 5
            PodDisruptionBudget("in", "default", LabelSelector({}, [Requirement("app", "In", ["a", "b"])]), 3)]   # 6
    rows = [_pod("p0", {"app": "a"}), _pod("p1", {"app": "a"}), _pod("p2", {}), _pod("p3", {"app": "b", "x": "1"}),
            _pod("p4", {"app": "a"}, "other"), _pod("p5", {"y": "1"})]
    assert pdb_matches(rows, pdbs) == [[0, 5, 6], [0, 4, 5, 6], [], [6], [1], [5]]
    assert pdb_matches(rows, pdbs) == [preemptpdbref.matching(p, pdbs) for p in rows]
    assert pdb_matches(rows, []) == [[]] * len(rows)


def test_pdb_matches_equals_the_reference_on_every_scene():
    for sc in pp.scenes().values():
        assert pdb_matches(sc.bound, sc.pdbs) == [preemptpdbref.matching(p, sc.pdbs) for p in sc.bound], sc.name


def test_pdb_from_dict():
    doc = {"apiVersion": "policy/v1", "kind": "PodDisruptionBudget",
           "metadata": {"name": "guard", "namespace": "prod"},
           "spec": {"minAvailable": 2, "selector": {"matchLabels": {"app": "a"},
                                                     "matchExpressions": [{"key": "tier", "operator": "In",
                                                                           "values": ["t", "u"]}]}},
           "status": {"disruptionsAllowed": 2, "disruptedPods": {"p7": "2024-01-01T00:00:00Z"}, "currentHealthy": 4}}
    b = pdb_from_dict(doc)
    assert (b.name, b.namespace, b.disruptions_allowed, b.disrupted_pods) == ("guard", "prod", 2, ("p7",))
    assert b.selector.matches({"app": "a", "tier": "u"}) and not b.selector.matches({"app": "a"})
    # no status (no disruption controller ran): nothing allowed; no namespace: default
    bare = pdb_from_dict({"metadata": {"name": "bare"}, "spec": {"selector": {}}})
    assert (bare.namespace, bare.disruptions_allowed, bare.disrupted_pods) == ("default", 0, ())
    assert bare.selector is not None and bare.selector.empty()
    assert pdb_from_dict({"metadata": {"name": "nil"}, "spec": {}}).selector is None
    assert pdb_from_dict({"metadata": {"name": "null"}, "spec": {"selector": None}, "status": None}).selector is None
    assert pdb_matches([_pod("p", {"app": "a", "tier": "t"}, "prod")], [b, bare]) == [[0]]


def test_bound_table_carries_the_budgets():
    sc = pp.scenes()["two_budgets"]
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    plain = bound_table(cluster, sc.bound, sc.start)
    assert plain.pdb_off is None and plain.pdb_ids is None and plain.pdb_allowed is None
    assert bound_table(cluster, sc.bound, sc.start, pdbs=[]).pdb_off is None
    t = bound_table(cluster, sc.bound, sc.start, pdbs=sc.pdbs)
    assert t.pdb_allowed.tolist() == [5, 1] and t.pdb_allowed.dtype == np.int32
    assert t.pdb_off.tolist() == [0, 2, 3, 3, 3] and t.pdb_ids.tolist() == [0, 1, 1]
    for k in ("node", "priority", "start_time", "req"):
        np.testing.assert_array_equal(getattr(plain, k), getattr(t, k))
    with pytest.raises(ValueError):
        abi.BoundPods(plain.node, plain.priority, plain.start_time, plain.req, pdb_allowed=[0])
    with pytest.raises(ValueError):
        abi.BoundPods(plain.node, plain.priority, plain.start_time, plain.req, pdb_allowed=[0], pdb_off=[0], pdb_ids=[])


# ---- 4. the export ----------------------------------------------------------------------------------
def test_the_export_exists():
    from ksim import engine
    assert "ksim_set_bound_pod_pdbs" in engine.EXPORTS
    L = engine.lib()
    assert hasattr(L, "ksim_set_bound_pod_pdbs")
    assert L.ksim_abi_version() == 12
    assert ctypes_sizeof_preempt_out() == 32


def ctypes_sizeof_preempt_out() -> int:
    import ctypes
    out = abi.PreemptOut(1)
    assert [f[0] for f in type(out.c)._fields_][-1] == "n_pdb_violations"
    return ctypes.sizeof(out.c)
