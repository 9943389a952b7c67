"""ksim_preempt_spread: DefaultPreemption's dry run for preemptors with
DoNotSchedule topology spread (csrc/ksim_preempt.hip, k_preempt_spread_mins and
the spread form of k_preempt_nodes).

The C oracle refuses these pods, so the reference is the object-level dry run
tests/preemptspreadref.py (pinned to tests/preemptobjref.py on scenes without
such constraints, and shown to tell the faulty readings apart on these very
scenes, by tests/test_preempt_spread_ref.py).  The engine's (nominated,
victims, n_potential, n_candidates) must equal it exactly on every scene of
tests/preemptspreadcases.py, with and without the scene's nominated groups: 2
to 300 nodes, the last with a 300-value domain table across the 256 threads of
both kernels."""
import numpy as np
import pytest

import preemptaffcases as ac
import preemptcases as pc
import preemptspreadcases as sc_mod
import preemptspreadref as ref
from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.preemption import bound_table
from oracle.oracle import Oracle
from test_gpu_preempt_uses import Scene, _kinds, engines  # noqa: F401  (engines: the fixture)

pytestmark = pytest.mark.gpu


def _profile(args=(100, 0), drop=()):
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100, preemption=profile.PreemptionArgs(*args))
    en = sp.plugins["filter"].enabled
    for name in drop:
        en.pop([profile.original_name(p.name) for p in en].index(name))
        assert name not in sp.filter_order()
    return sp, profile.compile_profile(sp)


def _build(sc, extra_pods=(), drop=None, full_adds=True) -> Scene:
    """The scene compiled: cluster, pods (the scene's, then ``extra_pods``), the
    bound-pod table with every class of every row, the nominated groups by
    node position, the scene's profile (``drop``: filters left out)."""
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    enc = encode_pods(cluster, list(sc.pods) + list(extra_pods))
    table = bound_table(cluster, sc.bound, sc.start, cluster.topo, full_adds=True) if full_adds else \
        bound_table(cluster, sc.bound, sc.start)
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    groups = [(pos[n], list(idx)) for n, idx in sc.nominated.items()] or None
    prof = _profile(sc.args, getattr(sc, "drop", ()) if drop is None else drop)[1]
    return Scene(cluster, enc, table, prof, sc_mod.PRIO, groups, sc.bound, sc.start)


def _reference(sc, cluster, grouped=True) -> tuple:
    got = ref.dry_run(sc.nodes, sc.bound, sc.start, sc.order, sc.pods[0], sc_mod.PRIO, sc.args,
                      sc.nominated_pods() if grouped else None, filter_order=sc_mod.filter_order(sc))
    return ref.as_indices(got, cluster.node_names, sc.order)


def _engine(engines, s: Scene, index=0, priority=sc_mod.PRIO, set_table=True, grouped=True, **kw) -> tuple:
    eng = engines(s.cluster, s.prof)
    if set_table:
        eng.set_bound_pods(s.table)
    kw.setdefault("hard_spread", True)
    return eng.preempt(s.enc, index, priority, groups=s.groups if grouped else None, **kw)


def _indices(sc, cluster, expect) -> tuple:
    pos = list(cluster.node_names)
    return (pos.index(expect[0]) if expect[0] else -1, [sc.order[v] for v in expect[1]], expect[2], expect[3])


# ---- the scenes: the engine against the reference -----------------------------------------------
@pytest.mark.parametrize("name", sc_mod.scene_ids())
def test_engine_equals_the_reference(engines, name):
    sc = sc_mod.scenes()[name]
    s = _build(sc)
    assert {getattr(abi, "USE_" + k) for k in sc.kinds} <= set(_kinds(s.enc)), name
    if name == "three_hundred_hosts":
        p = s.enc.pods[0]
        u = s.enc.uses[int(p["use_first"])]
        assert int(s.cluster.n_nodes) == 300 and int(u["kind"]) == abi.USE_PTS_HARD
    want = _reference(sc, s.cluster)
    assert want == _indices(sc, s.cluster, sc.expect)
    assert _engine(engines, s) == want
    if sc.nominated:
        plain = _reference(sc, s.cluster, grouped=False)
        assert plain == _indices(sc, s.cluster, sc.expect_plain)
        assert _engine(engines, s, set_table=False, grouped=False) == plain
        assert _engine(engines, s, set_table=False) == want          # and the group again: nothing is left behind


# ---- pods without hard uses: the new call is the old one ---------------------------------------------
@pytest.mark.parametrize("name", ["headline", "fit_and_anti", "first_pod", "nominated_holder", "nominated_match"])
def test_new_call_equals_the_old_one_without_hard_uses(engines, name):
    sc = ac.scenes()[name]
    s = _build(sc, drop=())
    assert abi.USE_PTS_HARD not in _kinds(s.enc)
    old = _engine(engines, s, hard_spread=False)
    assert old == _indices(sc, s.cluster, sc.expect)
    assert _engine(engines, s, set_table=False) == old


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
def test_new_call_equals_the_oracle_on_a_use_free_case(engines, grouped):
    from ksim.model import Container, Pod
    case = pc.all_cases()[pc.cascade_ids()[0]]
    prio = case.preemptor[0]
    cluster, table, _, prof = pc.encoded(case)
    enc = encode_pods(cluster, [pc.preemptor_pod(case.preemptor),
                                Pod("nominated", priority=prio + 1, containers=[Container({"cpu": "700m"})])])
    groups = [(min(1, case.n_nodes - 1), [1])] if grouped else None
    eng = engines(cluster, prof)
    eng.set_bound_pods(table)
    want = Oracle(cluster, prof).preempt(enc, 0, prio, table, groups)
    assert eng.preempt(enc, 0, prio, groups=groups, hard_spread=True) == want
    assert eng.preempt(enc, 0, prio, groups=groups) == want
    if not grouped:
        assert want[0] == case.winner


# ---- the interface -----------------------------------------------------------------------------------
def test_without_the_adds_the_new_call_is_invalid(engines):
    from ksim.engine import KsimError
    sc = sc_mod.scenes()["headline"]
    s = _build(sc)
    eng = engines(s.cluster, s.prof)
    eng.set_bound_pods(bound_table(s.cluster, sc.bound, sc.start))          # the table alone
    with pytest.raises(KsimError) as e:
        eng.preempt(s.enc, 0, sc_mod.PRIO, hard_spread=True)
    assert e.value.code == abi.E_INVALID and "ksim_set_bound_pod_adds" in str(e.value)
    eng.set_bound_pod_adds(s.table.adds_off, s.table.adds)
    assert eng.preempt(s.enc, 0, sc_mod.PRIO, hard_spread=True) == _reference(sc, s.cluster)


def test_old_entry_points_still_refuse_on_the_same_handle(engines):
    from ksim.engine import KsimError
    sc = sc_mod.scenes()["group_lifts_own_domain"]
    s = _build(sc)
    want = _reference(sc, s.cluster)
    assert _engine(engines, s) == want
    for grouped in (False, True):                       # ksim_preempt, ksim_preempt_nominated
        with pytest.raises(KsimError) as e:
            _engine(engines, s, set_table=False, grouped=grouped, hard_spread=False)
        assert e.value.code == abi.E_UNSUPPORTED and "PTS_HARD" in str(e.value)
    assert _engine(engines, s, set_table=False) == want


def test_profile_without_pod_topology_spread_ignores_the_use(engines):
    """No PodTopologySpread filter: the hard use is ignored, the result is the
    oracle's for the pod without its constraint, and no adds are needed."""
    sc = sc_mod.scenes()["group_lifts_own_domain"]
    bare = ac.preemptor(4000, labels=ac.X, name="bare")
    s = _build(sc, extra_pods=[bare], drop=("PodTopologySpread",), full_adds=False)
    assert abi.USE_PTS_HARD in _kinds(s.enc) and _kinds(s.enc, 3) == [] and s.table.adds is None
    want = Oracle(s.cluster, s.prof).preempt(s.enc, 3, sc_mod.PRIO, s.table, s.groups)
    assert want[0] >= 0 and want != _reference(sc, s.cluster)               # Fit alone: the x pod is reprieved
    assert _engine(engines, s) == want


# ---- a handle keeps nothing of a spread dry run -------------------------------------------------------------
def test_spread_then_use_free_then_a_cycle_on_one_handle(engines):
    """A spread dry run, a use-free one, the spread one again, then a compat
    cycle of a pod that spreads over the same selector and key: each equals its
    oracle / reference, so no domain table, minimum, topology flag or victim
    flag of one call reaches the next."""
    sc = sc_mod.scenes()["spread_anti_and_port"]
    probe = ac.preemptor(100, name="probe", prio=0, labels=ac.X, topology_spread=[sc_mod.hard(skew=2)])
    s = _build(sc, extra_pods=[ac.preemptor(4000, name="second", prio=25), probe])
    assert _kinds(s.enc, 1) == [] and _kinds(s.enc, 2) == [abi.USE_PTS_HARD]
    want = _reference(sc, s.cluster)
    first = _engine(engines, s)
    assert first == want and len(first[1]) == 4
    second = _engine(engines, s, index=1, priority=25, set_table=False)
    assert second == Oracle(s.cluster, s.prof).preempt(s.enc, 1, 25, s.table)
    assert second[0] >= 0 and second[1]
    assert _engine(engines, s, set_table=False) == want
    eng = engines(s.cluster, s.prof)
    e, o = eng.eval_pod(s.enc, 2), Oracle(s.cluster, s.prof).cycle(s.enc, 2)
    assert e["chosen"] == o["chosen"]
    for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
        assert np.array_equal(e[k], o[k]), k
    pts = _profile()[0].filter_order().index("PodTopologySpread")
    assert (np.asarray(o["fail_plugin"]) == pts).any() and (np.asarray(o["fail_plugin"]) == abi.PASSED).any()


# ---- the spread x PDB instantiation, from two derived facts ------------------------------------------------
@pytest.mark.parametrize("name", ["headline", "spread_anti_and_port", "group_lifts_own_domain"])
def test_budgets_that_allow_every_victim_change_nothing(engines, name):
    sc = sc_mod.scenes()[name]
    s = _build(sc)
    want = _reference(sc, s.cluster)
    eng = engines(s.cluster, s.prof)
    eng.set_bound_pods(s.table)
    n = s.table.n
    eng.set_bound_pod_pdbs([n + 1], np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32))
    assert eng.preempt(s.enc, 0, sc_mod.PRIO, groups=s.groups, with_pdb=True, hard_spread=True) == want + (0,)
    eng.set_bound_pod_pdbs([], [0], [])
    assert eng.preempt(s.enc, 0, sc_mod.PRIO, groups=s.groups, with_pdb=True, hard_spread=True) == want + (0,)


@pytest.mark.parametrize("name", ["headline", "spread_anti_and_port", "group_lifts_own_domain"])
def test_a_budget_that_allows_nothing_marks_every_victim(engines, name):
    """One budget with allowed = 0 over every lower-priority pod: every such pod
    violates, so all are reprieved in the first pass, in the order they had: the
    same victims in the same order, each one a violation.  (One candidate per
    scene, so the pick's first criterion changes nothing.)"""
    sc = sc_mod.scenes()[name]
    s = _build(sc)
    want = _reference(sc, s.cluster)
    assert want[3] == 1 and want[1]
    eng = engines(s.cluster, s.prof)
    eng.set_bound_pods(s.table)
    low = np.asarray(s.table.priority) < sc_mod.PRIO
    off = np.concatenate([[0], np.cumsum(low)]).astype(np.int32)
    eng.set_bound_pod_pdbs([0], off, np.zeros(int(low.sum()), np.int32))
    got = eng.preempt(s.enc, 0, sc_mod.PRIO, groups=s.groups, with_pdb=True, hard_spread=True)
    assert got == want + (len(want[1]),)


# ---- end to end ---------------------------------------------------------------------------------------
def test_compat_cycle_records_the_nominated_node(engines):
    """ksim.wrapped.compat_cycle(..., hard_spread=True) over the engine: the
    spreading pod is unschedulable, DefaultPreemption nominates node 0, and the
    store records it; without the keyword the cycle raises as before."""
    import json
    from ksim.engine import KsimError
    from ksim.resultstore import POSTFILTER_RESULT, POST_FILTER_NOMINATED_MESSAGE, Store
    from ksim.wrapped import compat_cycle
    sc = sc_mod.scenes()["headline"]
    sp, prof = _profile(sc.args)
    s = _build(sc)
    eng = engines(s.cluster, prof)
    eng.set_bound_pods(s.table)
    with pytest.raises(KsimError) as e:
        compat_cycle(eng, Store(profile.default_score_weights()), s.cluster, sp, s.enc, 0, sc_mod.PRIO)
    assert e.value.code == abi.E_UNSUPPORTED
    store = Store(profile.default_score_weights())
    res = compat_cycle(eng, store, s.cluster, sp, s.enc, 0, sc_mod.PRIO, hard_spread=True)
    want = _reference(sc, s.cluster)
    assert res["status"] == abi.STATUS_UNSCHEDULABLE
    assert res["nominated"] == want[0] == s.cluster.node_names.index("n0000")
    ann = {}
    store.add_stored_result_to_pod(*s.enc.names[0], ann)
    post = json.loads(ann[POSTFILTER_RESULT])
    assert [n for n, v in post.items() if v.get("DefaultPreemption") == POST_FILTER_NOMINATED_MESSAGE] == ["n0000"]
