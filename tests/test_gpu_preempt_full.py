"""ksim_preempt_full: DefaultPreemption's dry run for every preemptor the
per-pod cycle accepts (csrc/ksim_preempt.hip: k_preempt_nodes<FullForm>, the row
side and the volume side in one thread, and k_preempt_static_veto, VolumeBinding
and VolumeZone on the candidates).

No older entry point takes a pod with counted volumes beside required pod
(anti-)affinity or DoNotSchedule spread, and none re-runs VolumeBinding or
VolumeZone, so the reference is the object-level dry run
tests/preemptfullref.py (pinned to the three older references on their own
scenes and shown to tell the wrong readings apart on these very scenes, by
tests/test_preempt_full_ref.py).  The engine's (nominated, victims,
n_potential, n_candidates) must equal it exactly on every scene of
tests/preemptfullcases.py, with and without the scene's nominated group: 1 to 8
nodes, 257 (one thread in a second block) and 300."""
import functools

import numpy as np
import pytest

import preemptaffcases as ac
import preemptcases as pc
import preemptfullcases as cases
import preemptfullref as ref
import preemptspreadcases as sc_mod
import preemptvolcases as vc
import preemptvolmodel
from ksim import abi, profile
from ksim.encode import encode_pods
from ksim.engine import Engine, KsimError
from ksim.model import Container, Pod
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """One handle per compiled scene, created once every pod of its test is encoded."""
    held = {}

    def get(b):
        key = id(b.cluster)
        if key not in held:
            if len(held) >= 4:                           # keep few handles open
                held.pop(next(iter(held)))[0].close()
            e = Engine(0)
            e.set_profile(b.prof)
            e.set_cluster(b.cluster)
            e.set_bound_pods(b.table)
            held[key] = (e, b)
        return held[key][0]

    yield get
    for e, _ in held.values():
        e.close()


@functools.lru_cache(maxsize=None)
def _built(name):
    return cases.build(cases.scenes()[name])


@functools.lru_cache(maxsize=None)
def _reference(name, grouped=True) -> tuple:
    s = cases.scenes()[name]
    b = _built(name)
    got = ref.dry_run(b.nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], cases.PRIO, s.args,
                      s.nominated_pods() if grouped else None, filter_order=s.filter_order, classes=s.classes)
    return ref.as_indices(got, b.cluster.node_names, s.order)


def _state(eng):
    return eng.volume_attached().copy(), eng.class_count().copy()


def _run(eng, b, grouped=True, index=0, priority=cases.PRIO, **kw):
    """One dry run through the new call, and that it left no trace."""
    before = _state(eng)
    kw.setdefault("full", True)
    got = eng.preempt(b.enc, index, priority, groups=b.groups if grouped else None, **kw)
    after = _state(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    return got


# ---- the scenes: the engine against the reference -----------------------------------------------
@pytest.mark.parametrize("name", cases.scene_ids())
def test_engine_equals_the_reference(engines, name):
    b = _built(name)
    eng = engines(b)
    want = _reference(name)
    plain = _reference(name, False)
    assert _run(eng, b) == want
    assert _run(eng, b, grouped=False) == plain
    if b.groups:
        assert plain != want
    assert _run(eng, b) == want                          # and again: nothing is left behind
    assert _run(eng, b, grouped=False) == plain


def test_the_scenes_cover_the_victim_counts():
    """0, 1 and at least 3 victims on a node, the last with a shared volume."""
    assert _reference("one_node_without_ipa")[1] == [] and len(_reference("statefulset_replica")[1]) == 1
    assert len(_reference("every_slot")[1]) >= 3 and len(_reference("eight_families")[1]) == 8
    assert len(cases.scenes()["shared_volume_and_zone"].bound) >= 3 and _built("every_slot").cluster.n_nodes == 4
    assert _built("block_edge_257").cluster.n_nodes == 257 and _built("three_hundred_zoned").cluster.n_nodes == 300


# ---- the PDB instantiation, from two derived facts ------------------------------------------------------
PDB_SCENES = ["statefulset_replica", "shared_volume_and_zone", "group_holds_and_counts", "every_slot",
              "pv_zone_rejects"]


@pytest.mark.parametrize("name", PDB_SCENES)
def test_budgets_that_allow_every_victim_change_nothing(engines, name):
    b = _built(name)
    want = _reference(name)
    eng = engines(b)
    n = b.table.n
    try:
        eng.set_bound_pod_pdbs([n + 1], np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32))
        assert _run(eng, b, with_pdb=True) == want + (0,)
    finally:
        eng.set_bound_pod_pdbs([], [0], [])
    assert _run(eng, b, with_pdb=True) == want + (0,)


@pytest.mark.parametrize("name", PDB_SCENES)
def test_a_budget_that_allows_nothing_marks_every_victim(engines, name):
    """One budget with allowed = 0 over every lower-priority pod: every such pod
    violates, so all are reprieved in the first pass, in the order they had: the
    same victims in the same order, each one a violation.  (One candidate per
    scene, so the pick's first criterion changes nothing.)"""
    b = _built(name)
    want = _reference(name)
    assert want[3] == 1 and want[1]
    eng = engines(b)
    low = np.asarray(b.table.priority) < cases.PRIO
    off = np.concatenate([[0], np.cumsum(low)]).astype(np.int32)
    try:
        eng.set_bound_pod_pdbs([0], off, np.zeros(int(low.sum()), np.int32))
        assert _run(eng, b, with_pdb=True) == want + (len(want[1]),)
    finally:
        eng.set_bound_pod_pdbs([], [0], [])


def test_a_budget_between_the_rows(engines):
    """preemptfullcases.mixed_budget, the full form on shared volumes: b2 and b3
    violate the budget (disruptionsAllowed 1 over b1, b2, b3); b2 is reprieved,
    b3 stays out violating, then b1 is a victim because b3 is out (the shared
    volume would attach again) and b4 is reprieved because b2 is back.  Against
    the reference with its budget table (tests/test_preempt_budget_refs.py),
    and without budgets on the same handle."""
    import preemptpdbref
    sc = cases.mixed_budget()
    b = cases.build(sc)
    p = b.enc.pods[0]
    kinds = {int(k) for k in b.enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]}
    assert {abi.USE_VOLUME, abi.USE_IPA_ANTI} <= kinds
    names = b.cluster.node_names

    def want(pdbs):
        got = ref.dry_run(b.nodes, sc.pvs, sc.pvcs, sc.bound, sc.start, sc.order, sc.pods[0], cases.PRIO, sc.args,
                          None, filter_order=sc.filter_order, classes=sc.classes, pdbs=pdbs)
        return preemptpdbref.as_indices(got, names, sc.order)
    assert [sc.order[n] for n in ("b1", "b2", "b3", "b4")] == [0, 1, 2, 3]
    eng = engines(b)
    try:
        eng.set_bound_pod_pdbs([1], [0, 1, 2, 3, 3], [0, 0, 0])      # b1, b2, b3 in budget 0
        got = _run(eng, b, with_pdb=True)
        assert got == want(sc.budgets) and got[1] == [2, 0] and got[4] == 1
    finally:
        eng.set_bound_pod_pdbs([], [0], [])
    plain = _run(eng, b, with_pdb=True)
    assert plain == want([]) and plain[1] == [1, 3]


# ---- without the combination the new call is the older one ---------------------------------------------
@pytest.mark.parametrize("name", ["two_victims_share", "group_holds_volumes", "port_and_volume"])
def test_equals_the_volume_call_on_a_volume_only_scene(name):
    b = preemptvolmodel.build(vc.scenes()[name])
    eng = Engine(0)
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(b.table)
        for groups in (b.groups, None):
            old = eng.preempt(b.enc, 0, vc.PRIO, groups=groups, volumes=True)
            assert eng.preempt(b.enc, 0, vc.PRIO, groups=groups, full=True) == old
        assert old[0] >= 0 or name == "group_holds_volumes"
    finally:
        eng.close()


def _spread_scene(sc):
    from test_gpu_preempt_spread import _build
    return _build(sc)


@pytest.mark.parametrize("name", ["headline", "group_lifts_own_domain"])
def test_equals_the_spread_call_on_a_spread_only_scene(name):
    sc = sc_mod.scenes()[name]
    s = _spread_scene(sc)
    eng = Engine(0)
    try:
        eng.set_profile(s.prof)
        eng.set_cluster(s.cluster)
        eng.set_bound_pods(s.table)
        for groups in (s.groups, None):
            old = eng.preempt(s.enc, 0, sc_mod.PRIO, groups=groups, hard_spread=True)
            assert old[0] >= 0
            assert eng.preempt(s.enc, 0, sc_mod.PRIO, groups=groups, full=True) == old
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["headline", "fit_and_anti", "nominated_holder"])
def test_equals_the_plain_call_on_an_affinity_only_scene(name):
    sc = ac.scenes()[name]
    s = _spread_scene(sc)
    eng = Engine(0)
    try:
        eng.set_profile(s.prof)
        eng.set_cluster(s.cluster)
        eng.set_bound_pods(s.table)
        old = eng.preempt(s.enc, 0, ac.PRIO, groups=s.groups)
        assert eng.preempt(s.enc, 0, ac.PRIO, groups=s.groups, full=True) == old
    finally:
        eng.close()


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
def test_equals_the_plain_call_and_the_oracle_on_a_use_free_case(grouped):
    case = pc.all_cases()[pc.cascade_ids()[0]]
    prio = case.preemptor[0]
    cluster, tab, _, prof = pc.encoded(case)
    enc = encode_pods(cluster, [pc.preemptor_pod(case.preemptor),
                                Pod("nominated", priority=prio + 1, containers=[Container({"cpu": "700m"})])])
    groups = [(min(1, case.n_nodes - 1), [1])] if grouped else None
    eng = Engine(0)
    try:
        eng.set_profile(prof)
        eng.set_cluster(cluster)
        eng.set_bound_pods(tab)
        want = Oracle(cluster, prof).preempt(enc, 0, prio, tab, groups)
        assert eng.preempt(enc, 0, prio, groups=groups, full=True) == want
        assert eng.preempt(enc, 0, prio, groups=groups) == want
    finally:
        eng.close()


# ---- the older calls keep their refusals; the gap the new call closes -----------------------------------
def test_the_volume_call_still_refuses_the_combined_preemptor(engines):
    b = _built("statefulset_replica")
    eng = engines(b)
    want = _reference("statefulset_replica")
    assert _run(eng, b) == want
    with pytest.raises(KsimError) as e:
        eng.preempt(b.enc, 0, cases.PRIO, volumes=True)
    assert e.value.code == abi.E_UNSUPPORTED
    assert "KSIM_USE_VOLUME" in str(e.value) and "the volume form moves no domain counts" in str(e.value)
    assert "KSIM_USE_PTS_HARD" in str(e.value) or "KSIM_USE_IPA" in str(e.value)
    with pytest.raises(KsimError) as e:                  # the host's refusal of the two flags together
        eng.preempt(b.enc, 0, cases.PRIO, volumes=True, hard_spread=True)
    assert e.value.code == abi.E_UNSUPPORTED and "KSIM_USE_PTS_HARD" in str(e.value)
    for kw in ({}, {"hard_spread": True}):               # ksim_preempt, ksim_preempt_spread
        with pytest.raises(KsimError) as e:
            eng.preempt(b.enc, 0, cases.PRIO, **kw)
        assert e.value.code == abi.E_UNSUPPORTED and "KSIM_USE_VOLUME" in str(e.value)
    assert _run(eng, b) == want


def test_the_volume_call_nominates_a_node_the_pv_does_not_reach():
    """pv_excludes_best with a second preemptor that has the volume and no
    anti-affinity, which ksim_preempt_volumes accepts: it re-runs neither
    VolumeBinding nor VolumeZone and names n0 and its victim; the new call
    equals the reference, on both preemptors."""
    sc = cases.scenes()["pv_excludes_best"]
    first = sc.pods[0]
    bare = Pod("volume_only", containers=first.containers, pvc_claims=list(first.pvc_claims), priority=cases.PRIO)
    b = cases.build(sc, extra_pods=[bare])
    at = len(sc.pods)
    kinds = {int(k) for k in b.enc.uses["kind"][int(b.enc.pods[at]["use_first"]):][:int(b.enc.pods[at]["use_count"])]}
    assert kinds == {abi.USE_VOLUME} and int(b.enc.pods[at]["vb_count"]) > 0
    got = ref.dry_run(b.nodes, sc.pvs, sc.pvcs, sc.bound, sc.start, sc.order, bare, cases.PRIO, sc.args,
                      filter_order=sc.filter_order)
    want = ref.as_indices(got, b.cluster.node_names, sc.order)
    names = list(b.cluster.node_names)
    assert want == (names.index("n1"), [sc.order["b1"]], 3, 2)
    eng = Engine(0)
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(b.table)
        old = eng.preempt(b.enc, at, cases.PRIO, volumes=True)
        assert old == (names.index("n0"), [sc.order["b0"]], 3, 3)
        assert _run(eng, b, index=at) == want != old
        assert _run(eng, b) == _reference("pv_excludes_best") == want
    finally:
        eng.close()


# ---- missing tables ------------------------------------------------------------------------------------
def test_without_the_adds_or_the_holdings_the_call_is_invalid():
    sc = cases.scenes()["shared_volume_and_zone"]
    bare = Pod("bare", priority=25, containers=[Container({"cpu": "15900m"})])
    b = cases.build(sc, extra_pods=[bare])
    at = len(sc.pods)
    eng = Engine(0)
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        plain = Oracle(b.cluster, b.prof).preempt(b.enc, at, 25, b.table)
        assert plain[1]
        for adds, holdings, call in ((False, True, "ksim_set_bound_pod_adds"), (True, False, "ksim_set_bound_pod_volumes")):
            eng.set_bound_pods(cases.build(sc, extra_pods=[bare], adds=adds, holdings=holdings).table)
            with pytest.raises(KsimError) as e:
                eng.preempt(b.enc, 0, cases.PRIO, full=True)
            assert e.value.code == abi.E_INVALID and call in str(e.value)
            assert eng.preempt(b.enc, at, 25, full=True) == plain    # the handle still runs a plain dry run
            assert eng.preempt(b.enc, at, 25) == plain
        eng.set_bound_pods(b.table)
        assert _run(eng, b) == _reference("shared_volume_and_zone")
    finally:
        eng.close()


# ---- a handle keeps nothing of a full dry run --------------------------------------------------------------
def test_full_then_use_free_then_a_cycle_on_one_handle():
    """A full dry run, a use-free one, the full one again, then a compat cycle
    of the preemptor: the dry runs equal their references, and the cycle's
    per-node codes equal those of a fresh handle that ran nothing."""
    sc = cases.scenes()["shared_volume_and_zone"]
    bare = Pod("bare", priority=25, containers=[Container({"cpu": "15900m"})])
    b = cases.build(sc, extra_pods=[bare])
    want = _reference("shared_volume_and_zone")
    eng, fresh = Engine(0), Engine(0)
    try:
        for e in (eng, fresh):
            e.set_profile(b.prof)
            e.set_cluster(b.cluster)
        eng.set_bound_pods(b.table)
        assert _run(eng, b) == want
        second = _run(eng, b, index=len(sc.pods), priority=25)
        assert second == Oracle(b.cluster, b.prof).preempt(b.enc, len(sc.pods), 25, b.table) and second[1]
        assert second == eng.preempt(b.enc, len(sc.pods), 25)
        assert _run(eng, b) == want
        got, clean = eng.eval_pod(b.enc, 0), fresh.eval_pod(b.enc, 0)
        assert got["status"] == clean["status"] == abi.STATUS_UNSCHEDULABLE
        for k in ("fail_plugin", "fail_detail"):
            assert np.array_equal(got[k], clean[k]), k
    finally:
        eng.close()
        fresh.close()


# ---- end to end -------------------------------------------------------------------------------------------
def test_compat_cycle_and_post_filter_record_the_nominated_node(engines):
    import json
    from ksim.fwplugins import EnginePlugins
    from ksim.resultstore import POSTFILTER_RESULT, POST_FILTER_NOMINATED_MESSAGE, Store
    from ksim.wrapped import compat_cycle
    b = _built("statefulset_replica")
    eng = engines(b)
    with pytest.raises(KsimError) as e:                  # without the keyword the cycle raises as before
        compat_cycle(eng, Store(profile.default_score_weights()), b.cluster, b.sp, b.enc, 0, cases.PRIO, volumes=True)
    assert e.value.code == abi.E_UNSUPPORTED
    store = Store(profile.default_score_weights())
    res = compat_cycle(eng, store, b.cluster, b.sp, b.enc, 0, cases.PRIO, full=True)
    want = _reference("statefulset_replica")
    assert res["status"] == abi.STATUS_UNSCHEDULABLE
    assert res["nominated"] == want[0] == b.cluster.node_names.index("n0")
    ann = {}
    store.add_stored_result_to_pod(*b.enc.names[0], ann)
    post = json.loads(ann[POSTFILTER_RESULT])
    assert [n for n, v in post.items() if v.get("DefaultPreemption") == POST_FILTER_NOMINATED_MESSAGE] == ["n0"]
    pl = EnginePlugins(eng, b.cluster, b.sp)
    assert pl.pre_filter(b.enc, 0)[0].is_success()
    with pytest.raises(KsimError) as e:
        pl.post_filter(cases.PRIO, volumes=True)
    assert e.value.code == abi.E_UNSUPPORTED
    status, node, victims, override = pl.post_filter(cases.PRIO, full=True)
    assert status.is_success() and override and (node, victims) == want[:2]
