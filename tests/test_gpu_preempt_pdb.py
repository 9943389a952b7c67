"""ksim_preempt / ksim_preempt_nominated with PodDisruptionBudgets
(csrc/ksim_preempt.hip, the PDB form of k_preempt_nodes; ksim_set_bound_pod_pdbs).

The C oracle knows no budgets, so the reference is the object-level dry run
tests/preemptpdbref.py over oracle/objref.py (pinned to ObjScheduler.preempt and
the C oracle where no budget takes effect, and shown to tell fourteen wrong
readings apart on these very scenes, by tests/test_preempt_pdb_ref.py).  The
engine's (nominated, victims, n_potential, n_candidates, n_pdb_violations) must
equal it exactly on every scene of tests/preemptpdbcases.py, as it stands and
with a nominated group: 3 to 70 nodes for the rules, 1,023 to 2,049 for the cut
at k_preempt_pick's chunk and wave boundaries.  The preemptors cover the three
forms of k_preempt_nodes (use-free, host ports, the domain form)."""
import json

import numpy as np
import pytest

import preemptcases as pc
import preemptpdbcases as pp
import preemptpdbref
from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.engine import KsimError
from ksim.preemption import bound_table
from oracle.oracle import Oracle
from test_gpu_preempt_uses import Scene, _kinds, _profile, engines  # noqa: F401  (engines: the fixture)

pytestmark = pytest.mark.gpu


def _build(sc: pp.PdbScene, extra_pods=(), pdbs="scene") -> Scene:
    """The scene compiled: cluster, pods (the scene's, then ``extra_pods``), the
    bound-pod table with every class of every row and the budgets, the
    nominated groups by node position."""
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    enc = encode_pods(cluster, list(sc.pods) + list(extra_pods))
    table = bound_table(cluster, sc.bound, sc.start, cluster.topo, full_adds=True,
                        pdbs=sc.pdbs if pdbs == "scene" else pdbs)
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    groups = [(pos[n], list(idx)) for n, idx in sc.nominated.items()] or None
    return Scene(cluster, enc, table, _profile(sc.args)[1], pp.PRIO, groups, sc.bound, sc.start)


def _reference(name: str, cluster, grouped=False) -> tuple:
    sc = pp.scenes()[name]
    return preemptpdbref.as_indices(pp.reference(name, grouped), cluster.node_names, sc.order)


def _engine(engines, s: Scene, index=0, priority=pp.PRIO, set_table=True, groups="scene") -> tuple:
    eng = engines(s.cluster, s.prof)
    if set_table:
        eng.set_bound_pods(s.table)
    return eng.preempt(s.enc, index, priority, groups=s.groups if groups == "scene" else groups, with_pdb=True)


# ---- the engine against the reference ---------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pp.scene_ids())
def test_engine_equals_the_reference(engines, name, grouped):
    sc = pp.scenes()[name]
    s = _build(sc.grouped() if grouped else sc)
    assert (s.groups is not None) == (grouped or bool(sc.nominated))
    assert {getattr(abi, "USE_" + k) for k in sc.kinds} <= set(_kinds(s.enc)), name
    if not sc.kinds:
        assert _kinds(s.enc) == []                          # the use-free form
    assert s.table.pdb_allowed.size == len(sc.pdbs)
    got = _engine(engines, s)
    assert got == _reference(name, s.cluster, grouped)
    # the 4-tuple is the 5-tuple's head
    assert engines(s.cluster, s.prof).preempt(s.enc, 0, pp.PRIO, groups=s.groups) == got[:4]


def test_the_three_kernel_forms_and_the_budget_shapes_are_covered():
    """What the scenes above ran, read off the scenes themselves."""
    sc = pp.scenes()
    assert sc["ports_form"].kinds == ("NODE_PORT",) and sc["anti_affinity_form"].kinds == ("IPA_ANTI",)
    assert sum(1 for s in sc.values() if not s.kinds) >= 30
    allowed = {b.disruptions_allowed for s in sc.values() for b in s.pdbs}
    assert {0, 1} <= allowed and max(allowed) > 4            # more than any node holds
    assert len(sc["three_hundred_budgets"].pdbs) == 300
    assert preemptpdbref.matching(sc["two_budgets"].bound[0], sc["two_budgets"].pdbs) == [0, 1]


# ---- a handle keeps nothing of a dry run with budgets ------------------------------------------
def test_two_preemptors_in_sequence_the_second_without_budgets(engines):
    """A dry run with budgets leaves violating marks on the rows; a second
    preemptor on the same handle and table, after the budgets were cleared,
    equals the oracle (victims in importance order, no violation), and the
    first repeats once the budgets are back."""
    sc = pp.scenes()["allowed_one_two_pods"]
    s = _build(sc, extra_pods=[pp.ac.preemptor(7000, name="second", prio=55)])
    want = _reference(sc.name, s.cluster)
    first = _engine(engines, s)
    assert first == want and first[1] == [1, 0] and first[4] == 1
    eng = engines(s.cluster, s.prof)
    eng.set_bound_pod_pdbs([], [], [])
    second = eng.preempt(s.enc, 1, 55, with_pdb=True)
    assert second == Oracle(s.cluster, s.prof).preempt(s.enc, 1, 55, s.table) + (0,)
    assert second[0] == 0 and second[1] == [1]
    # the first preemptor without budgets: importance order again
    plain = eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True)
    assert plain == Oracle(s.cluster, s.prof).preempt(s.enc, 0, pp.PRIO, s.table) + (0,) and plain[1] == [0, 1]
    eng.set_bound_pod_pdbs(s.table.pdb_allowed, s.table.pdb_off, s.table.pdb_ids)
    assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == want


# ---- the interface ----------------------------------------------------------------------------------
def _invalid(eng, allowed, off, ids):
    with pytest.raises(KsimError) as e:
        eng.set_bound_pod_pdbs(allowed, off, ids)
    assert e.value.code == abi.E_INVALID and "ksim_set_bound_pod_pdbs" in str(e.value)
    return str(e.value)


def test_invalid_budget_tables_are_refused_and_change_nothing():
    from ksim.engine import Engine
    sc = pp.scenes()["two_budgets"]
    s = _build(sc)
    n = s.table.n
    assert n == 4
    eng = Engine(0)
    try:
        eng.set_profile(s.prof)
        eng.set_cluster(s.cluster)
        assert "ksim_set_bound_pods first" in _invalid(eng, [0], [0] * (n + 1), [])          # no table
        eng.set_bound_pods(s.table)
        want = _reference(sc.name, s.cluster)
        assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == want
        assert "monotone" in _invalid(eng, [0, 0], [0, 2, 1, 2, 2], [0, 1])
        assert "start at 0" in _invalid(eng, [0, 0], [1, 1, 1, 1, 1], [0])
        assert "out of range" in _invalid(eng, [0, 0], [0, 1, 1, 1, 1], [2])
        assert "out of range" in _invalid(eng, [0, 0], [0, 1, 1, 1, 1], [-1])
        assert "twice" in _invalid(eng, [0, 0], [0, 3, 3, 3, 3], [1, 0, 1])
        with pytest.raises(KsimError) as e:
            eng._chk(eng.L.ksim_set_bound_pod_pdbs(eng.h, -1, None, None, None))
        assert e.value.code == abi.E_INVALID
        # the same id in two different rows is fine, and a refused call left the budgets as they were
        assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == want
        eng.set_bound_pod_pdbs([1, 5], [0, 1, 2, 2, 2], [0, 0])
    finally:
        eng.close()


def test_a_new_table_drops_the_budgets_and_zero_budgets_equal_never_set(engines):
    sc = pp.scenes()["violations_level"]
    s = _build(sc)
    plain_table = bound_table(s.cluster, sc.bound, sc.start, s.cluster.topo, full_adds=True)
    assert plain_table.pdb_off is None
    oracle = Oracle(s.cluster, s.prof).preempt(s.enc, 0, pp.PRIO, s.table) + (0,)
    want = _reference(sc.name, s.cluster)
    assert want != oracle and oracle[0] == 0
    eng = engines(s.cluster, s.prof)
    eng.set_bound_pods(plain_table)
    never_set = eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True)
    assert never_set == oracle
    eng.set_bound_pod_pdbs(s.table.pdb_allowed, s.table.pdb_off, s.table.pdb_ids)
    assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == want
    eng.set_bound_pod_pdbs([], [], [])                       # n_pdbs = 0
    assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == never_set
    eng.set_bound_pods(s.table)                              # the table brings its budgets
    assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == want
    eng.set_bound_pods(plain_table)                          # a new table drops them
    assert eng.preempt(s.enc, 0, pp.PRIO, with_pdb=True) == never_set


# ---- end to end --------------------------------------------------------------------------------------
def test_compat_cycle_with_budgets_records_the_nominated_node(engines):
    """ksim.wrapped.compat_cycle with ``pdbs``: the pod is unschedulable,
    DefaultPreemption nominates the first node without a violation (node 3; node
    0 without the budgets), and the store records it."""
    from ksim.resultstore import POSTFILTER_RESULT, POST_FILTER_NOMINATED_MESSAGE, Store
    from ksim.wrapped import compat_cycle
    sc = pp.scenes()["violations_level"]
    sp, prof = _profile(sc.args)
    s = _build(sc)
    eng = engines(s.cluster, prof)
    eng.set_bound_pods(bound_table(s.cluster, sc.bound, sc.start))
    store = Store(profile.default_score_weights())
    assert compat_cycle(eng, store, s.cluster, sp, s.enc, 0, pp.PRIO)["nominated"] == 0
    store = Store(profile.default_score_weights())
    res = compat_cycle(eng, store, s.cluster, sp, s.enc, 0, pp.PRIO,
                       pdbs=(s.table.pdb_allowed, s.table.pdb_off, s.table.pdb_ids))
    assert res["status"] == abi.STATUS_UNSCHEDULABLE
    assert res["nominated"] == _reference(sc.name, s.cluster)[0] == 3
    ann = {}
    store.add_stored_result_to_pod(*s.enc.names[0], ann)
    post = json.loads(ann[POSTFILTER_RESULT])
    assert [n for n, v in post.items() if v.get("DefaultPreemption") == POST_FILTER_NOMINATED_MESSAGE] == ["n0003"]


# ---- budgets that select nothing -----------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_a_budget_table_without_matches_equals_the_oracle(engines, name):
    """Every case of tests/preemptcases.py through the PDB form of the kernels
    (one budget, no row in it): the oracle's result, no violation."""
    case = pc.all_cases()[name]
    cluster, table, enc, prof = pc.encoded(case)
    want = Oracle(cluster, prof).preempt(enc, 0, case.preemptor[0], table) + (0,)
    eng = engines(cluster, prof)
    eng.set_bound_pods(table)
    eng.set_bound_pod_pdbs([0], np.zeros(table.n + 1, np.int32), [])
    assert eng.preempt(enc, 0, case.preemptor[0], with_pdb=True) == want
    assert want[0] == case.winner
