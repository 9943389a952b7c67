"""DefaultPreemption PostFilter: the C oracle's dry run
(ksim_oracle_preempt) against the object-level restatement (oracle/objref.py
ObjScheduler.preempt) on crowded clusters with mixed priorities, and both
against a plain-Python restatement of the header's rules on the hand-made
clusters of tests/preemptcases.py (one per level of the pick cascade, and the
numCandidates cut either side of the best candidate)."""
import numpy as np
import pytest

from ksim import gen
from ksim.encode import encode_cluster, encode_pods
from ksim.model import Container, Pod
from ksim.preemption import bound_table
from ksim import profile
from oracle.objref import ObjScheduler
from oracle.oracle import Oracle


def crowded(n_nodes=40, per_node=6, seed=3):
    """Config-1 nodes, each holding bound pods of mixed priorities and start times."""
    rng = np.random.default_rng(seed)
    nodes, _ = gen.config1_objects(n_nodes=n_nodes, n_pods=1)
    bound, start, order = [], {}, {}
    for ni, n in enumerate(nodes):
        for k in range(per_node):
            name = f"b{ni}-{k}"
            p = Pod(name, node_name=n.name, priority=int(rng.choice([0, 10, 100, 1000])),
                    containers=[Container({"cpu": f"{int(rng.integers(2, 12)) * 100}m",
                                           "memory": f"{int(rng.integers(1, 6))}Gi"})])
            bound.append(p)
            start[name] = int(rng.integers(0, 50))       # ties on purpose
            order[name] = len(order)
    return nodes, bound, start, order


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_preempt_oracle_vs_objref(seed):
    nodes, bound, start, order = crowded(seed=seed)
    cluster, _ = encode_cluster(nodes, bound)
    table = bound_table(cluster, bound, start)
    rng = np.random.default_rng(seed + 100)
    pods = [Pod(f"p{i}", priority=int(rng.choice([0, 5, 50, 500, 5000])),
                containers=[Container({"cpu": f"{int(rng.integers(10, 400)) * 100}m",
                                       "memory": f"{int(rng.integers(4, 40))}Gi"})]) for i in range(30)]
    enc = encode_pods(cluster, pods)
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    ora = Oracle(cluster, profile.compile_profile(sp))
    ref = ObjScheduler(nodes, bound, pct=100, seed=sp.tiebreak_seed)
    nominated = 0
    for i, pod in enumerate(pods):
        node, victims, n_pot, n_cand = ora.preempt(enc, i, pod.priority, table)
        rnode, rvictims = ref.preempt(pod, pod.priority, start, order)
        got = cluster.node_names[node] if node >= 0 else None
        assert got == rnode, f"pod {i}"
        assert [bound[v].name for v in victims] == rvictims, f"pod {i}"
        nominated += node >= 0
    assert 0 < nominated < len(pods)


def test_postfilter_records_nominated_node():
    """wrappedPlugin.PostFilter records the nominated node of DefaultPreemption
    as "preemption victim" and "" otherwise (wrappedplugin.go:529-538,
    store.go:437-452): compat_cycle feeds ksim_preempt's pick into the store."""
    import json
    from ksim.resultstore import POSTFILTER_RESULT, POST_FILTER_NOMINATED_MESSAGE, Store
    from ksim.wrapped import compat_cycle
    nodes, bound, start, order = crowded(seed=4)
    cluster, _ = encode_cluster(nodes, bound)
    table = bound_table(cluster, bound, start)
    rng = np.random.default_rng(104)
    pods = [Pod(f"p{i}", priority=int(rng.choice([0, 5, 50, 500, 5000])),
                containers=[Container({"cpu": f"{int(rng.integers(10, 400)) * 100}m",
                                       "memory": f"{int(rng.integers(4, 40))}Gi"})]) for i in range(30)]
    enc = encode_pods(cluster, pods)
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    ora = Oracle(cluster, profile.compile_profile(sp))
    ref = Oracle(cluster.copy_state(), profile.compile_profile(sp))
    store = Store(profile.default_score_weights())
    seen = 0
    for i, pod in enumerate(pods):
        res = compat_cycle(ora, store, cluster, sp, enc, i, pod.priority, table)
        ann = {}
        store.add_stored_result_to_pod(*enc.names[i], ann)
        if res["status"] != 1:
            ref.cycle(enc, i)
            continue
        want, _, _, _ = ref.preempt(enc, i, pod.priority, table)
        ref.cycle(enc, i)
        assert res["nominated"] == want
        post = json.loads(ann[POSTFILTER_RESULT])
        marked = [n for n, v in post.items() if v.get("DefaultPreemption") == POST_FILTER_NOMINATED_MESSAGE]
        assert marked == ([cluster.node_names[want]] if want >= 0 else [])
        seen += want >= 0
    assert seen > 0


# ---- hand-made cases (tests/preemptcases.py): the cascade and the cut ---------------
import preemptcases as pc


def _oracle_result(case, preemptor=None):
    cluster, table, enc, prof = pc.encoded(case, preemptor)
    return Oracle(cluster, prof).preempt(enc, 0, (preemptor or case.preemptor)[0], table)


def _objref_result(case, preemptor=None):
    """ObjScheduler.preempt's (node, victims) as (node position, table rows)."""
    nodes, bound, start, order, _ = pc.objects(case)
    pod = pc.preemptor_pod(preemptor or case.preemptor)
    ref = ObjScheduler(nodes, bound, pct=100, seed=0, preemption=profile.PreemptionArgs(*case.args))
    rnode, rvictims = ref.preempt(pod, pod.priority, start, order)
    return ([n.name for n in nodes].index(rnode) if rnode is not None else -1), [order[v] for v in rvictims]


@pytest.mark.parametrize("name", pc.cascade_ids())
def test_cascade_case_oracle_and_objref_vs_criteria(name):
    """The C oracle and the object-level restatement both give criteria()'s
    pick, victim list (reprieve order) and counts."""
    case = pc.all_cases()[name]
    v = pc.criteria(case)
    assert v.pick == case.winner
    assert _oracle_result(case) == v.result
    assert case.n_nodes <= 16 and _objref_result(case) == v.result[:2]


@pytest.mark.parametrize("name", pc.cascade_ids())
def test_cascade_case_is_decided_at_its_level(name):
    """From criteria() alone: the first tuple position where the winner and the
    runner-up differ is the level the case is for, and at least three kept
    candidates tie on every level above it."""
    case = pc.all_cases()[name]
    v = pc.criteria(case)
    if case.level is None:
        assert v.pick == -1 and not v.kept
        return
    assert pc.deciding_level(v) == case.level
    assert pc.tie_width(v, case.level) >= 3


def test_cascade_cases_cover_every_level():
    decided = {pc.deciding_level(pc.criteria(c)) for c in pc.cascade_cases()}
    assert decided >= set(pc.LEVELS)
    by_name = {c.name: c for c in pc.cascade_cases()}
    assert [by_name[f"level_{lv}"].level for lv in pc.LEVELS] == list(pc.LEVELS)


def test_cascade_side_cases_are_what_they_say():
    t = pc.all_cases()
    v = pc.criteria(t["fits_somewhere"])
    assert 5 not in v.potential and len(v.potential) == 9 and v.kept[2][0] == 900
    v = pc.criteria(t["int32_min_victim"])
    assert v.kept[3][:3] == (pc.I32_MIN, 0, 1) and 6 not in v.potential
    case = t["reprieve"]
    v = pc.criteria(case)
    assert v.result[1] == [3, 2] and [case.rows[i][1] for i in v.result[1]] == [30, 20]
    assert len([r for r in case.rows if r[0] == 2 and r[1] < case.preemptor[0]]) == 4     # two were reprieved
    v = pc.criteria(t["all_outrank"])
    assert {0, 1} <= set(v.potential) and not {0, 1} & set(v.all_candidates)
    v = pc.criteria(t["empty_node"])
    assert 3 not in v.potential and not any(r[0] == 3 for r in t["empty_node"].rows)
    v = pc.criteria(t["level_nv"])
    assert {k[1] for k in v.kept.values()} == {2 ** 31} and {k[2] for k in v.kept.values()} == {1, 2}
    v = pc.criteria(t["level_early"])                    # the winner's low-priority victim started first of all
    assert min(r[2] for r in t["level_early"].rows) == 5 and v.kept[4][3] == -300


@pytest.mark.parametrize("name", pc.geometry_ids())
def test_cut_case_vs_oracle(name):
    """Every node is a candidate, the best candidate sits at exactly the
    stated rank either side of the cut, and the C oracle agrees with criteria()."""
    case = pc.all_cases()[name]
    v = pc.criteria(case)
    assert v.all_candidates == list(range(case.n_nodes)) and v.want == case.want
    best = min(range(case.n_nodes), key=lambda n: case.rows[n][1])
    assert best == case.best_rank and case.best_rank in (case.want - 1, case.want)
    assert sum(1 for r in case.rows if r[1] == case.rows[best][1]) == 1
    assert (v.pick == best) == (case.best_rank < case.want) and v.pick == case.winner
    assert v.result[2:] == (case.n_nodes, case.want)
    assert _oracle_result(case) == v.result
    if case.n_nodes <= 16:
        assert _objref_result(case) == v.result[:2]


def test_cut_cases_cover_the_geometries():
    cs = pc.geometry_cases()
    assert {c.n_nodes for c in cs} == set(pc.GEOMETRY_N)
    for n in pc.GEOMETRY_N:
        wants = {c.want for c in cs if c.n_nodes == n}
        assert {1, n} <= wants
        inside = sorted(w for w in wants if pc.inside_a_chunk(n, w))
        chunk = (n + pc.PICK_THREADS - 1) // pc.PICK_THREADS
        if n > pc.PICK_THREADS:
            assert chunk >= 2 and len(inside) >= 2
            assert inside[0] < 2 * n // 3 and (inside[-1] - 1) // chunk >= (n - 2) // chunk   # the middle; the last chunk
            for w in inside:                              # both sides of each cut exist
                assert {c.best_rank for c in cs if c.n_nodes == n and c.want == w} == {w - 1, w}
        else:
            assert not inside
    assert {w % 3 for w in (c.want for c in cs if c.n_nodes == 2049) if pc.inside_a_chunk(2049, w)} == {1, 2}
    assert all(c.want % 2 == 1 for c in cs if c.n_nodes == 3000 and pc.inside_a_chunk(3000, c.want))


def test_sequence_high_then_low_priority_preemptor():
    """Two preemptors on one table: the second, lower one has fewer victims on
    the same node (the first call's victims 50 and 40 outrank it)."""
    got = [_oracle_result(pc.SEQUENCE, p) for p in pc.SEQUENCE_PREEMPTORS]
    want = []
    for p in pc.SEQUENCE_PREEMPTORS:
        c = pc.Case("sequence", pc.SEQUENCE.n_nodes, pc.SEQUENCE.rows, p, pc.SEQUENCE.args)
        want.append(pc.criteria(c).result)
    assert got == want
    assert [_objref_result(pc.SEQUENCE, p) for p in pc.SEQUENCE_PREEMPTORS] == [w[:2] for w in want]
    assert got[0][0] == got[1][0] == 2 and len(got[0][1]) == 4 and got[1][1] == [3, 2]
