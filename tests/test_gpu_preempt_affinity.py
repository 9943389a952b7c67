"""ksim_preempt / ksim_preempt_nominated for preemptors with required pod
(anti-)affinity (csrc/ksim_preempt.hip, the domain form of k_preempt_nodes).

The C oracle refuses these pods, so the reference is the object-level dry run
tests/preemptobjref.py over oracle/objref.py (pinned to ObjScheduler.preempt and
the C oracle on use-free pods, and shown to tell the faulty variants apart on
these very scenes, by tests/test_preempt_affinity_ref.py).  The engine's
(nominated, victims, n_potential, n_candidates) must equal it exactly on every
scene of tests/preemptaffcases.py: 5 to 300 nodes, the last across the
256-thread block of k_preempt_nodes."""
import numpy as np
import pytest

import preemptaffcases as ac
import preemptobjref
from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.model import LabelSelector, TopologySpreadConstraint
from ksim.preemption import bound_table
from oracle.oracle import Oracle
from test_gpu_preempt_uses import Scene, _kinds, _profile, engines  # noqa: F401  (engines: the fixture)

pytestmark = pytest.mark.gpu


def _build(sc: ac.AffScene, prof=None, extra_pods=(), full_adds=True) -> Scene:
    """The scene compiled: cluster, pods (the scene's, then ``extra_pods``), the
    bound-pod table with every class of every row, the nominated groups by
    node position."""
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    enc = encode_pods(cluster, list(sc.pods) + list(extra_pods))
    table = bound_table(cluster, sc.bound, sc.start, cluster.topo, full_adds=True) if full_adds else \
        bound_table(cluster, sc.bound, sc.start)
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    groups = [(pos[n], list(idx)) for n, idx in sc.nominated.items()] or None
    return Scene(cluster, enc, table, prof or _profile(sc.args)[1], ac.PRIO, groups, sc.bound, sc.start)


def _reference(sc: ac.AffScene, cluster) -> tuple:
    got = preemptobjref.dry_run(sc.nodes, sc.bound, sc.start, sc.order, sc.pods[0], ac.PRIO, sc.args,
                                sc.nominated_pods())
    return preemptobjref.as_indices(got, cluster.node_names, sc.order)


def _engine(engines, s: Scene, index=0, priority=ac.PRIO, set_table=True, groups="scene") -> tuple:
    eng = engines(s.cluster, s.prof)
    if set_table:
        eng.set_bound_pods(s.table)
    return eng.preempt(s.enc, index, priority, groups=s.groups if groups == "scene" else groups)


def _assert_kinds(sc: ac.AffScene, enc):
    assert {getattr(abi, "USE_" + k) for k in sc.kinds} <= set(_kinds(enc)), sc.name


# ---- scenes 1 to 8: the engine against the reference --------------------------------------
@pytest.mark.parametrize("name", ac.scene_ids())
def test_engine_equals_the_reference(engines, name):
    sc = ac.scenes()[name]
    s = _build(sc)
    _assert_kinds(sc, s.enc)
    if name == "sixteen_uses":
        assert len(_kinds(s.enc)) == abi.MAX_USES
    if name == "host_and_zone":
        p = s.enc.pods[0]
        u = s.enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
        assert (np.asarray(u["cls"]) == -1).any()
        assert ac.ZONE not in sc.nodes[5].labels
    want = _reference(sc, s.cluster)
    if sc.expect is not None:
        pos = list(s.cluster.node_names)
        assert want == (pos.index(sc.expect[0]) if sc.expect[0] else -1, [sc.order[v] for v in sc.expect[1]],
                        sc.expect[2], sc.expect[3])
    assert _engine(engines, s) == want


# ---- scene 9: a handle keeps nothing of an affinity dry run -----------------------------------
def test_two_preemptors_in_sequence_and_a_cycle_afterwards(engines):
    """An affinity preemptor, then a use-free one on the same handle and table:
    the second equals the oracle (no stale domain tables, topology flags or
    victim flags), and the affinity dry run repeats.  Then a compat cycle of a
    pod whose preferred affinity term scores by the zone's count of app=x (its
    use 0, the slot of the preemptor's anti-affinity use) equals the oracle's:
    the domain tables were re-zeroed, or the counts would come out doubled."""
    from ksim.model import WeightedPodAffinityTerm
    sc = ac.scenes()["fit_and_anti"]
    probe = ac.preemptor(100, name="probe", prio=0,
                         pod_affinity_preferred=[WeightedPodAffinityTerm(7, ac.term(ac.ZONE, app="x"))])
    s = _build(sc, extra_pods=[ac.preemptor(4000, name="second", prio=25), probe])
    _assert_kinds(sc, s.enc)
    assert _kinds(s.enc, 1) == [] and _kinds(s.enc, 2) == [abi.USE_IPA_SCORE]
    want = _reference(sc, s.cluster)
    first = _engine(engines, s)
    assert first == want and len(first[1]) == 3
    second = _engine(engines, s, index=1, priority=25, set_table=False)
    assert second == Oracle(s.cluster, s.prof).preempt(s.enc, 1, 25, s.table)
    assert second[0] >= 0 and second[1]
    assert _engine(engines, s, set_table=False) == want
    eng = engines(s.cluster, s.prof)
    e, o = eng.eval_pod(s.enc, 2), Oracle(s.cluster, s.prof).cycle(s.enc, 2)
    assert e["chosen"] == o["chosen"] >= 0
    for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
        assert np.array_equal(e[k], o[k]), k
    slot = [p.name for p in _profile(sc.args)[0].score_plugins()].index("InterPodAffinity")
    assert np.asarray(o["raw"]).reshape(-1, s.cluster.n_nodes)[slot].max() > 0


# ---- scene 10: the interface ---------------------------------------------------------------------
def test_affinity_preemptor_without_the_adds_is_invalid(engines):
    from ksim.engine import KsimError
    sc = ac.scenes()["headline"]
    s = _build(sc)
    _assert_kinds(sc, s.enc)
    eng = engines(s.cluster, s.prof)
    eng.set_bound_pods(bound_table(s.cluster, sc.bound, sc.start))          # the table alone
    with pytest.raises(KsimError) as e:
        eng.preempt(s.enc, 0, ac.PRIO)
    assert e.value.code == abi.E_INVALID and "ksim_set_bound_pod_adds" in str(e.value)
    eng.set_bound_pod_adds(s.table.adds_off, s.table.adds)
    assert eng.preempt(s.enc, 0, ac.PRIO) == _reference(sc, s.cluster)


def test_hard_spread_beside_anti_affinity_is_still_refused(engines):
    from ksim.engine import KsimError
    sc = ac.scenes()["headline"]
    hard = ac.preemptor(anti=[ac.term(ac.ZONE, app="x")], labels=ac.X, name="hard",
                        topology_spread=[TopologySpreadConstraint(1, ac.ZONE, "DoNotSchedule",
                                                                  LabelSelector(dict(ac.X)))])
    s = _build(sc, extra_pods=[hard])
    assert {abi.USE_PTS_HARD, abi.USE_IPA_ANTI} <= set(_kinds(s.enc, 1))
    with pytest.raises(KsimError) as e:
        _engine(engines, s, index=1)
    assert e.value.code == abi.E_UNSUPPORTED and "PTS_HARD" in str(e.value)


def test_profile_without_inter_pod_affinity_ignores_the_uses(engines):
    """No InterPodAffinity filter: the uses are ignored, the result is the
    oracle's for the pod without its terms, and no adds are needed."""
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100, preemption=profile.PreemptionArgs(100, 0))
    en = sp.plugins["filter"].enabled
    en.pop([profile.original_name(p.name) for p in en].index("InterPodAffinity"))
    assert "InterPodAffinity" not in sp.filter_order()
    prof = profile.compile_profile(sp)
    sc = ac.scenes()["fit_and_anti"]
    s = _build(sc, prof=prof, extra_pods=[ac.preemptor(4000, name="bare")], full_adds=False)
    _assert_kinds(sc, s.enc)
    assert _kinds(s.enc, 1) == [] and s.table.adds is None
    want = Oracle(s.cluster, prof).preempt(s.enc, 1, ac.PRIO, s.table)
    assert want[0] >= 0 and want != _reference(sc, s.cluster)               # Fit alone: the x pods stay
    assert _engine(engines, s) == want


# ---- scene 11: end to end ------------------------------------------------------------------------
def test_compat_cycle_records_the_nominated_node(engines):
    """ksim.wrapped.compat_cycle over the engine with the full-adds table: the
    anti-affine pod is unschedulable, DefaultPreemption nominates the holder's
    node, and the store records it."""
    import json
    from ksim.resultstore import POSTFILTER_RESULT, POST_FILTER_NOMINATED_MESSAGE, Store
    from ksim.wrapped import compat_cycle
    sc = ac.scenes()["headline"]
    sp, prof = _profile(sc.args)
    s = _build(sc, prof=prof)
    _assert_kinds(sc, s.enc)
    eng = engines(s.cluster, prof)
    eng.set_bound_pods(s.table)
    store = Store(profile.default_score_weights())
    res = compat_cycle(eng, store, s.cluster, sp, s.enc, 0, ac.PRIO)
    want = _reference(sc, s.cluster)
    assert res["status"] == abi.STATUS_UNSCHEDULABLE
    assert res["nominated"] == want[0] == s.cluster.node_names.index("n0001")
    ann = {}
    store.add_stored_result_to_pod(*s.enc.names[0], ann)
    post = json.loads(ann[POSTFILTER_RESULT])
    assert [n for n, v in post.items() if v.get("DefaultPreemption") == POST_FILTER_NOMINATED_MESSAGE] == ["n0001"]
