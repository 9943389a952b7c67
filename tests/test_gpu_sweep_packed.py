"""Packed policy sweep (ksim_sweep_loaded, Engine.sweep_loaded, sweep.run_sweep):
many score-weight vectors over one snapshot and queue in shared launches, one
lane per vector.  Row v must be what set_profile(v) / load_pods / reset_cluster
/ schedule_loaded gives, which is what the CPU oracle gives under profile v.

All runs keep every node (percentageOfNodesToScore=100); the weight vectors
are PAIRS, (NodeResourcesBalancedAllocation, NodeResourcesFit), every other
plugin at 1."""
import ctypes
import functools

import numpy as np
import pytest

from ksim import abi, gen, profile, sweep
from ksim.engine import Engine, KsimError
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (1, 10), (10, 1), (3, 7)]
BIT_DEF, BIT_GENERIC, BIT_FLUSH = 1 << 24, 1 << 25, 1 << 26


def _profiles(base, pairs=PAIRS):
    return [profile.compile_profile(base.with_weights(
        {"NodeResourcesBalancedAllocation": ba, "NodeResourcesFit": fit})) for ba, fit in pairs]


def _engine(cluster, prof):
    eng = Engine(0)
    eng.set_profile(prof)
    eng.set_cluster(cluster)
    return eng


def _oracle_rows(cluster, pods, profs):
    return np.stack([Oracle(cluster, pr).schedule(pods, nthreads=16)[0] for pr in profs])


def _check_stats(rows, stats, n_pods):
    for v, st in enumerate(stats):
        assert st.pods == n_pods
        assert st.scheduled == int((rows[v] >= 0).sum()), v
        assert st.unschedulable == int((rows[v] < 0).sum()), v
        assert st.perpod_cycles == 0
        assert st.batches > 0 and st.device_ms == stats[0].device_ms


@functools.lru_cache(maxsize=None)
def _saturating():
    """100 nodes x 6,000 pods: the cluster fills up, differently per vector."""
    cluster, pods = gen.config2(n_nodes=100, n_pods=6000)
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    profs = _profiles(base)
    rows = _oracle_rows(cluster, pods, profs)
    rows.setflags(write=False)
    return cluster, pods, base, profs, rows


def test_saturating_parity_graphs_and_variants():
    cluster, pods, base, profs, want = _saturating()
    # what makes this input tell the lanes apart (the oracle's rows): distinct
    # rows, distinct saturation points, many unschedulable pods
    unsched = (want < 0).sum(axis=1)
    first_un = [int(np.argmax(r < 0)) for r in want]
    print("unschedulable per vector", unsched.tolist(), "first at", first_un)
    for a in range(len(want)):
        for b in range(a + 1, len(want)):
            assert not np.array_equal(want[a], want[b]), (a, b)
    assert all(920 <= u <= 1156 for u in unsched), unsched
    assert all(4802 <= f <= 5041 for f in first_un), first_un
    assert len(set(zip(first_un, unsched.tolist()))) == len(want)   # no two vectors saturate alike

    eng = _engine(cluster, profs[0])
    eng.load_pods(pods)
    g0 = eng.diag()["graph_captures"]
    rows, stats = eng.sweep_loaded(profs)
    g1 = eng.diag()["graph_captures"]
    np.testing.assert_array_equal(rows, want)
    _check_stats(rows, stats, pods.n_pods)
    assert g1 > g0                                   # 6,000 pods: at least 24 batches, graph replay
    rows2, stats2 = eng.sweep_loaded(profs)
    assert eng.diag()["graph_captures"] == g1        # the graph is reused
    np.testing.assert_array_equal(rows2, want)
    for a, b in zip(stats, stats2):
        for f in ("scheduled", "unschedulable", "evals", "batches", "truncations"):
            assert getattr(a, f) == getattr(b, f), f
    v = eng.diag()["variants"]
    assert v & BIT_DEF and v & BIT_FLUSH, hex(v)
    # the serial sequence of the contract on the same handle: same rows and counters
    for k in (0, 5):
        eng.set_profile(profs[k])
        eng.load_pods(pods)
        eng.reset_cluster()
        ch, st = eng.schedule_loaded(0, pods.n_pods)
        np.testing.assert_array_equal(ch, want[k])
        for f in ("pods", "scheduled", "unschedulable", "evals", "batches", "truncations"):
            assert getattr(st, f) == getattr(stats[k], f), (k, f)
    eng.close()


@pytest.mark.parametrize("max_lanes", [3, 1])
def test_refill(max_lanes):
    cluster, pods, base, profs, want = _saturating()
    eng = _engine(cluster, profs[0])
    eng.load_pods(pods)
    rows, stats = eng.sweep_loaded(profs, max_lanes=max_lanes)
    np.testing.assert_array_equal(rows, want)
    _check_stats(rows, stats, pods.n_pods)
    eng.close()


def test_handle_untouched():
    cluster, pods, base, profs, want = _saturating()
    ora = Oracle(cluster, profs[0])
    o_head, _ = ora.schedule(pods, 0, 500)
    o_tail, _ = ora.schedule(pods, 500, 5500)
    eng = _engine(cluster, profs[0])
    eng.load_pods(pods)
    head, _ = eng.schedule_loaded(0, 500)
    np.testing.assert_array_equal(head, o_head)
    state, ns = eng.node_state(), eng.next_start
    rows, _ = eng.sweep_loaded(profs)
    np.testing.assert_array_equal(rows, want)
    after = eng.node_state()
    for k in state:
        np.testing.assert_array_equal(after[k], state[k], err_msg=k)
    assert eng.next_start == ns
    tail, _ = eng.schedule_loaded(500, 5500)
    np.testing.assert_array_equal(tail, o_tail)
    eng.close()


def test_sub_range():
    cluster, pods, base, profs, _ = _saturating()
    eng = _engine(cluster, profs[0])
    eng.load_pods(pods)
    rows, stats = eng.sweep_loaded(profs, first=273, count=1000)
    assert rows.shape == (len(profs), 1000)
    other = _engine(cluster, profs[0])
    for v, pr in enumerate(profs):
        other.set_profile(pr)
        other.load_pods(pods)
        other.reset_cluster()
        ch, st = other.schedule_loaded(273, 1000)
        np.testing.assert_array_equal(rows[v], ch, err_msg=str(v))
        for f in ("pods", "scheduled", "unschedulable", "evals", "batches", "truncations"):
            assert getattr(st, f) == getattr(stats[v], f), (v, f)
    eng.close()
    other.close()


def test_keep_boundary_partial_batches():
    # 8,192 nodes: the largest cluster of the KEEP forms; 600 pods: fewer than
    # one graph, single launches with a partial last batch
    cluster, pods = gen.config2(n_nodes=8192, n_pods=600)
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    profs = _profiles(base, [PAIRS[0], PAIRS[1], PAIRS[2], PAIRS[6]])
    want = _oracle_rows(cluster, pods, profs)
    eng = _engine(cluster, profs[0])
    eng.load_pods(pods)
    g0 = eng.diag()["graph_captures"]
    rows, stats = eng.sweep_loaded(profs)
    np.testing.assert_array_equal(rows, want)
    _check_stats(rows, stats, pods.n_pods)
    assert eng.diag()["graph_captures"] == g0
    eng.close()


def test_generic_key_shape():
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100,
                                    fit=profile.FitArgs(resources=[("cpu", 2), ("memory", 1)]))
    cluster, pods = gen.config2(300, 900)
    profs = _profiles(base, PAIRS[4:])
    want = _oracle_rows(cluster, pods, profs)
    eng = _engine(cluster, profs[0])
    eng.load_pods(pods)
    rows, stats = eng.sweep_loaded(profs)
    np.testing.assert_array_equal(rows, want)
    _check_stats(rows, stats, pods.n_pods)
    assert eng.diag()["variants"] & BIT_GENERIC
    eng.close()


def _refused(eng, profs, **kw):
    with pytest.raises(KsimError) as e:
        eng.sweep_loaded(profs, **kw)
    return e.value


def test_refusals():
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    # a profile that differs in NodeResourcesFitArgs
    cluster, pods = gen.config2(300, 300)
    eng = _engine(cluster, profile.compile_profile(base))
    eng.load_pods(pods)
    odd = profile.compile_profile(profile.SchedulerProfile(
        percentage_of_nodes_to_score=100, fit=profile.FitArgs(resources=[("cpu", 2), ("memory", 1)])))
    err = _refused(eng, _profiles(base, PAIRS[:2]) + [odd])
    assert err.code == abi.E_UNSUPPORTED and "profile 2" in str(err)
    # argument errors
    profs = _profiles(base, PAIRS[:2])
    assert _refused(eng, []).code == abi.E_INVALID
    assert _refused(eng, profs, first=200, count=101).code == abi.E_INVALID
    assert _refused(eng, profs, first=-1, count=10).code == abi.E_INVALID
    assert _refused(eng, profs, max_lanes=65).code == abi.E_INVALID
    assert _refused(eng, profs, max_lanes=-1).code == abi.E_INVALID
    arr = (abi.Profile * 2)(*profs)
    assert eng.L.ksim_sweep_loaded(eng.h, 0, 10, arr, 2, 0, None, None) == abi.E_INVALID
    bad = _profiles(base, PAIRS[:2])
    bad[1].score_weight[0] = -1
    assert _refused(eng, bad).code == abi.E_INVALID
    # ... and none of them disturbed the engine: the call still works
    rows, _ = eng.sweep_loaded(profs)
    np.testing.assert_array_equal(rows, _oracle_rows(cluster, pods, profs))
    empty, st = eng.sweep_loaded(profs, first=5, count=0)
    assert empty.shape == (2, 0) and st[0].pods == 0
    eng.close()
    # a handle in ADAPT mode (the default percentage scores a window of 300 nodes)
    adapt = profile.SchedulerProfile(percentage_of_nodes_to_score=0)
    eng = _engine(cluster, profile.compile_profile(adapt))
    eng.load_pods(pods)
    err = _refused(eng, _profiles(adapt, PAIRS[:2]))
    assert err.code == abi.E_UNSUPPORTED and "ADAPT" in str(err)
    eng.close()


@pytest.mark.parametrize("case", ["past_keep", "config1"])
def test_serial_fallback(case):
    """Where the packed path does not apply, sweep.run_sweep runs the vectors
    one after another, returns the same matrix and puts the engine back."""
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    if case == "past_keep":
        cluster, pods = gen.config2(8193, 300)       # one node past the KEEP forms
    else:
        cluster, pods = gen.config1(300, 300)        # static-class / generic keys: no deferred commit
    profs = _profiles(base, PAIRS[:3])
    own = profile.compile_profile(base)
    eng = _engine(cluster, own)
    eng.load_pods(pods)
    assert _refused(eng, profs).code == abi.E_UNSUPPORTED
    rows, stats, packed = sweep.run_sweep(eng, pods, profs)
    assert packed is False and len(stats) == len(profs)
    np.testing.assert_array_equal(rows, _oracle_rows(cluster, pods, profs))
    # the engine's own profile again: a batch under it matches the oracle
    ch, _ = eng.schedule_batch(pods)
    np.testing.assert_array_equal(ch, Oracle(cluster, own).schedule(pods, nthreads=16)[0])
    eng.close()


def test_run_sweep_packed_flag():
    cluster, pods = gen.config2(300, 600)
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    profs = _profiles(base, PAIRS[:3])
    eng = _engine(cluster, profs[0])
    rows, stats, packed = sweep.run_sweep(eng, pods, profs, max_lanes=2)
    assert packed is True
    np.testing.assert_array_equal(rows, _oracle_rows(cluster, pods, profs))
    eng.close()
