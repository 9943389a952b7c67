"""ksim_preempt_volumes: DefaultPreemption's dry run for preemptors with
counted volumes (csrc/ksim_preempt.hip, k_preempt_nodes<VolumeForm>: the volume form).

The C oracle knows no volume limits and the three older entry points refuse
these pods, so the reference is the object-level dry run tests/preemptvolref.py
(pinned to tests/preemptobjref.py on the use-free cases, shown to tell the
faulty readings apart on these very scenes, and matched by a numpy restatement
of the device rule over the compiled tables, all by
tests/test_preempt_vol_ref.py).  The engine's (nominated, victims, n_potential,
n_candidates) must equal it exactly on every scene of tests/preemptvolcases.py,
with and without the scene's nominated group: 1 to 8 nodes, 257 (one thread in
a second block) and 300."""
import functools

import numpy as np
import pytest

import preemptcases as pc
import preemptobjref
import preemptvolcases as cases
import preemptvolmodel as model
import preemptvolref as ref
from ksim import abi, profile
from ksim.encode import encode_pods
from ksim.engine import Engine, KsimError
from ksim.model import Container, LabelSelector, Pod, PodAffinityTerm, TopologySpreadConstraint
from ksim.preemption import bound_table
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """One handle per compiled scene, created once every pod of its test is encoded."""
    held = {}

    def get(b, prof=None):
        key = id(b.cluster)
        if key not in held:
            if len(held) >= 4:                           # keep few handles open
                held.pop(next(iter(held)))[0].close()
            e = Engine(0)
            e.set_profile(prof or b.prof)
            e.set_cluster(b.cluster)
            e.set_bound_pods(b.table)
            held[key] = (e, b)
        elif prof is not None:
            held[key][0].set_profile(prof)
        return held[key][0]

    yield get
    for e, _ in held.values():
        e.close()


@functools.lru_cache(maxsize=None)
def _reference(name, grouped=True) -> tuple:
    s = cases.scenes()[name]
    b = _built(name)
    got = ref.dry_run(b.nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], cases.PRIO, s.args,
                      s.nominated_pods() if grouped else None, filter_order=s.filter_order)
    return preemptobjref.as_indices(got, b.cluster.node_names, s.order)


@functools.lru_cache(maxsize=None)
def _built(name):
    return model.build(cases.scenes()[name])


def _state(eng):
    return eng.volume_attached().copy(), eng.class_count().copy()


def _run(eng, b, grouped=True, index=0, priority=cases.PRIO, **kw):
    """One dry run through the new call, and that it left no trace."""
    before = _state(eng)
    kw.setdefault("volumes", True)
    got = eng.preempt(b.enc, index, priority, groups=b.groups if grouped else None, **kw)
    after = _state(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    return got


# ---- the scenes: the engine against the reference -----------------------------------------------
@pytest.mark.parametrize("name", cases.scene_ids())
def test_engine_equals_the_reference(engines, name):
    b = _built(name)
    p = b.enc.pods[0]
    kinds = [int(k) for k in b.enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]]
    assert abi.USE_VOLUME in kinds
    eng = engines(b)
    want = _reference(name)
    assert _run(eng, b) == want
    plain = _reference(name, False)
    assert _run(eng, b, grouped=False) == plain
    if b.groups:
        assert plain != want
        assert _run(eng, b) == want                      # and the group again: nothing is left behind


def test_sums_past_2_31(engines):
    """limit INT32_MAX - 1, attached + arg past 2^31: the patched tables of
    preemptvolcases.past_2_31, against the hand-derived result (which the numpy
    restatement gives in 64 bits and loses in 32)."""
    sc = cases.past_2_31()
    b = model.build(sc)
    model.patch_past_2_31(b)
    want = (0, [0], 1, 1)
    assert model.device_rule(b) == want and model.device_rule(b, wrap32=True) != want
    eng = engines(b)
    assert int(eng.volume_attached()[0, 0]) == cases.PAST_ATTACHED
    assert _run(eng, b) == want


# ---- pods without a volume use: the new call is ksim_preempt_nominated ------------------------------
@pytest.mark.parametrize("table", [False, True], ids=["no_volume_table", "volume_table"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
def test_new_call_equals_the_old_one_and_the_oracle_on_a_use_free_case(grouped, table):
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
        if table:
            n = cluster.n_nodes
            eng.set_volume_limits([abi.PL_EBS_LIMITS], np.full((1, n), 3, np.int32), np.ones((1, n), np.int32))
        eng.set_bound_pods(tab)
        want = Oracle(cluster, prof).preempt(enc, 0, prio, tab, groups)
        assert eng.preempt(enc, 0, prio, groups=groups, volumes=True) == want
        assert eng.preempt(enc, 0, prio, groups=groups) == want
        if not grouped:
            assert want[0] == case.winner
    finally:
        eng.close()


# ---- the interface --------------------------------------------------------------------------------------
def test_without_the_holdings_the_new_call_is_invalid(engines):
    b = _built("two_victims_share")
    sc = b.sc
    eng = engines(b)
    eng.set_bound_pods(bound_table(b.cluster, sc.bound, sc.start, b.cluster.topo))     # no holdings
    with pytest.raises(KsimError) as e:
        eng.preempt(b.enc, 0, cases.PRIO, volumes=True)
    assert e.value.code == abi.E_INVALID and "ksim_set_bound_pod_volumes" in str(e.value)
    eng.set_bound_pod_volumes(b.table.vol_off, b.table.vol_uses)
    assert _run(eng, b) == _reference("two_victims_share")
    eng.set_bound_pods(b.table)


def _bad_csr(b):
    """(what, off, uses) for every malformed holdings CSR the header names."""
    t = b.table
    good_off, good = t.vol_off.copy(), t.vol_uses.copy()
    assert good.size >= 2 and good_off[-1] == good.size

    def use(**kw):
        u = good.copy()
        for k, v in kw.items():
            u[k][0] = v
        return u
    down = good_off.copy()
    down[1] = down[-1] + 1                               # above the next row's offset
    assert down.size > 2
    return [("offsets", down, good), ("kind", good_off, use(kind=abi.USE_NODE_PORT)),
            ("family", good_off, use(col=b.vl.limit.shape[0])),
            ("class_high", good_off, use(cls=b.cluster.class_count.shape[0], arg=1)),
            ("class_low", good_off, use(cls=-2))]


def test_malformed_holdings_are_invalid(engines):
    b = _built("two_victims_share")
    eng = engines(b)
    want = _reference("two_victims_share")
    for what, off, uses in _bad_csr(b):
        with pytest.raises(KsimError) as e:
            eng.set_bound_pod_volumes(off, uses)
        assert e.value.code == abi.E_INVALID, what
        assert "ksim_set_bound_pod_volumes" in str(e.value), what
    assert _run(eng, b) == want                          # a refused call leaves the holdings set before it
    case = pc.all_cases()[pc.cascade_ids()[0]]
    cluster, tab, _, prof = pc.encoded(case)
    fresh = Engine(0)
    try:
        fresh.set_profile(prof)
        fresh.set_cluster(cluster)
        none = np.zeros(0, abi.TOPO_USE_DTYPE)
        with pytest.raises(KsimError) as e:              # no bound-pod table
            fresh.set_bound_pod_volumes([0], none)
        assert e.value.code == abi.E_INVALID and "ksim_set_bound_pods first" in str(e.value)
        fresh.set_bound_pods(tab)
        with pytest.raises(KsimError) as e:              # a table, but no volume table
            fresh.set_bound_pod_volumes(np.zeros(tab.n + 1, np.int32), none)
        assert e.value.code == abi.E_INVALID and "ksim_set_volume_limits" in str(e.value)
    finally:
        fresh.close()


def _with_extra_use(b, extra: Pod):
    """The scene compiled with a second preemptor: the first one's volumes plus ``extra``'s constraint."""
    sc = b.sc
    first = sc.pods[0]
    both = Pod("both", containers=first.containers, pvc_claims=list(first.pvc_claims), priority=cases.PRIO,
               labels={"app": "x"}, topology_spread=extra.topology_spread,
               pod_anti_affinity_required=extra.pod_anti_affinity_required)
    return model.build(sc, extra_pods=[both])


@pytest.mark.parametrize("kind", ["PTS_HARD", "IPA_ANTI"])
def test_volume_with_affinity_or_spread_uses_is_unsupported(kind):
    sc = cases.scenes()["ebs_slot"]
    sel = LabelSelector({"app": "x"})
    extra = Pod("extra", topology_spread=[TopologySpreadConstraint(1, "kubernetes.io/hostname", "DoNotSchedule", sel)]) \
        if kind == "PTS_HARD" else Pod("extra", pod_anti_affinity_required=[PodAffinityTerm("kubernetes.io/hostname", sel)])
    b = _with_extra_use(_built("ebs_slot"), extra)
    at = len(sc.pods)
    p = b.enc.pods[at]
    kinds = {int(k) for k in b.enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]}
    assert {abi.USE_VOLUME, getattr(abi, "USE_" + kind)} <= kinds
    eng = Engine(0)
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(bound_table(b.cluster, sc.bound, sc.start, b.cluster.topo, full_adds=True,
                                       vol_limits=b.cluster.vol_limits))
        with pytest.raises(KsimError) as e:
            eng.preempt(b.enc, at, cases.PRIO, volumes=True)
        assert e.value.code == abi.E_UNSUPPORTED
        assert "KSIM_USE_VOLUME" in str(e.value) and "KSIM_USE_" + kind in str(e.value)
        if kind == "PTS_HARD":                           # the host refuses the two flags together, in the engine's words
            with pytest.raises(KsimError) as e:
                eng.preempt(b.enc, at, cases.PRIO, volumes=True, hard_spread=True)
            assert e.value.code == abi.E_UNSUPPORTED
            assert "KSIM_USE_VOLUME" in str(e.value) and "KSIM_USE_PTS_HARD" in str(e.value)
        # the plain preemptor still runs
        assert eng.preempt(b.enc, 0, cases.PRIO, volumes=True)[0] == b.cluster.node_names.index("n0")
    finally:
        eng.close()


def test_old_entry_points_still_refuse_on_the_same_handle(engines):
    b = _built("group_holds_volumes")
    eng = engines(b)
    want = _reference("group_holds_volumes")
    assert _run(eng, b) == want
    for kw in ({"groups": None}, {"groups": b.groups}, {"groups": b.groups, "hard_spread": True}):
        with pytest.raises(KsimError) as e:              # ksim_preempt, ksim_preempt_nominated, ksim_preempt_spread
            eng.preempt(b.enc, 0, cases.PRIO, **kw)
        assert e.value.code == abi.E_UNSUPPORTED
        assert "KSIM_USE_VOLUME" in str(e.value) and "does not re-run the node volume limit plugins" in str(e.value)
    assert _run(eng, b) == want


# ---- the PDB instantiation, from two derived facts ------------------------------------------------------
PDB_SCENES = ["two_victims_share", "two_families_and_a_third", "group_holds_volumes", "port_and_volume"]


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
    """preemptvolcases.mixed_budget: four lower-priority pods on two shared
    volumes two-and-two, one budget (disruptionsAllowed 1) over three of them.
    b2 and b3 violate; b2 is reprieved, b3 stays out violating, then b1 is a
    victim because b3 is out (the shared volume would attach again) and b4 is
    reprieved because b2 is back: a reprieved row between violating and
    non-violating rows, which neither derived fact above reaches.  Against the
    reference with its budget table (tests/test_preempt_budget_refs.py), and
    without budgets on the same handle."""
    import preemptpdbref
    sc = cases.mixed_budget()
    b = model.build(sc)
    names = b.cluster.node_names

    def want(pdbs):
        got = ref.dry_run(b.nodes, sc.pvs, sc.pvcs, sc.bound, sc.start, sc.order, sc.pods[0], cases.PRIO, sc.args,
                          None, filter_order=sc.filter_order, pdbs=pdbs)
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


# ---- a handle keeps nothing of a volume dry run -----------------------------------------------------------
def test_volume_then_use_free_then_a_cycle_on_one_handle():
    """A volume dry run, a use-free one, the volume one again, then a compat
    cycle of the preemptor: the dry runs equal their references, and the
    cycle's per-node codes equal those of a fresh handle that ran nothing."""
    sc = cases.scenes()["two_victims_share"]
    bare = Pod("bare", priority=25, containers=[Container({"cpu": "15900m"})])
    b = model.build(sc, extra_pods=[bare])
    want = _reference("two_victims_share")
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
        ebs = b.sp.filter_order().index("EBSLimits")
        assert list(np.asarray(got["fail_plugin"])) == [ebs]
    finally:
        eng.close()
        fresh.close()


# ---- end to end -------------------------------------------------------------------------------------------
def test_compat_cycle_and_post_filter_record_the_nominated_node(engines):
    """ksim.wrapped.compat_cycle(..., volumes=True) over the engine: the pod is
    unschedulable, DefaultPreemption nominates n0, and the store records it;
    without the keyword the cycle raises as before."""
    import json
    from ksim.resultstore import POSTFILTER_RESULT, POST_FILTER_NOMINATED_MESSAGE, Store
    from ksim.wrapped import compat_cycle
    b = _built("ebs_slot")
    eng = engines(b)
    with pytest.raises(KsimError) as e:
        compat_cycle(eng, Store(profile.default_score_weights()), b.cluster, b.sp, b.enc, 0, cases.PRIO)
    assert e.value.code == abi.E_UNSUPPORTED
    store = Store(profile.default_score_weights())
    res = compat_cycle(eng, store, b.cluster, b.sp, b.enc, 0, cases.PRIO, volumes=True)
    want = _reference("ebs_slot")
    assert res["status"] == abi.STATUS_UNSCHEDULABLE
    assert res["nominated"] == want[0] == b.cluster.node_names.index("n0")
    ann = {}
    store.add_stored_result_to_pod(*b.enc.names[0], ann)
    post = json.loads(ann[POSTFILTER_RESULT])
    assert [n for n, v in post.items() if v.get("DefaultPreemption") == POST_FILTER_NOMINATED_MESSAGE] == ["n0"]
    # the framework-driven PostFilter (ksim.fwplugins) takes the flag through as well
    from ksim.fwplugins import EnginePlugins
    pl = EnginePlugins(eng, b.cluster, b.sp)
    assert pl.pre_filter(b.enc, 0)[0].is_success()
    with pytest.raises(KsimError) as e:
        pl.post_filter(cases.PRIO)
    assert e.value.code == abi.E_UNSUPPORTED
    status, node, victims, override = pl.post_filter(cases.PRIO, volumes=True)
    assert status.is_success() and override and (node, victims) == want[:2]
