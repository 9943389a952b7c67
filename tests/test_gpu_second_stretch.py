"""The second stretch of the deferred-commit batches (csrc/ksim_batch.hip
batch_top_commit_body): a batch goes on committing pods behind its first pair
cut while max(M_j, D_j, F_j) <= G_j, and ends before the first pod where that
fails.  KSIM_ONE_CUT=1 (read at every run) keeps every batch to its first cut.

Every scene runs under both settings.  Each run's placements, evaluation
count, scheduled / unschedulable counts, next_start and every node_state()
column are compared bit for bit with the oracle (computed once per scene), so
the placements are the same under both; the stretch never takes more batches,
and its counters are zero with the switch set.  test_fewer_batches asserts
that it takes strictly fewer on the wide scene."""
import contextlib
import functools
import os

import numpy as np
import pytest

from ksim import abi, gen, profile
from ksim.encode import EncodedPods
from ksim.engine import Engine, group_schedule_loaded
from oracle.oracle import Oracle

import runfeedcases as rf

pytestmark = pytest.mark.gpu

B = rf.B
GI, MI = 1 << 30, 1 << 20


@contextlib.contextmanager
def one_cut(on):
    old = os.environ.get("KSIM_ONE_CUT")
    if on:
        os.environ["KSIM_ONE_CUT"] = "1"
    else:
        os.environ.pop("KSIM_ONE_CUT", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("KSIM_ONE_CUT", None)
        else:
            os.environ["KSIM_ONE_CUT"] = old


# ---- scenes: (cluster, pods, [(first, count, reset before the run)]) ----------------------

def _wide():
    """gen.bare_cluster at 1,024 nodes, 160 classes: nearly every batch ends at a pair cut."""
    return gen.bare_cluster(1024, rf.SEED), rf.queue(8 * B + 1, 10, 16, tag=5), [(0, 8 * B + 1, False)]


def _narrow(n):
    return lambda: (rf.narrow_cluster(n), rf.queue(2 * B + 1 + rf.FOLLOW), [(0, 2 * B + 1, False), (2 * B + 1, rf.FOLLOW, False)])


def _lengths():
    """255, 256, 257 and 513 pods, each from the reset snapshot of one handle
    (two runs on one handle with reset_cluster between them, four times)."""
    return gen.bare_cluster(1024, rf.SEED), rf.queue(2 * B + 1, 2, 2, tag=1), [(0, n, True) for n in (B - 1, B, B + 1, 2 * B + 1)]


def _non_zero_start():
    return rf.narrow_cluster(64), rf.queue(3 * B), [(0, 300, False), (37, 2 * B + 3, False)]


def _no_table():
    """160 classes over 600 pods: fewer than 8 pods per class, so no request-class table."""
    return rf.narrow_cluster(96), rf.queue(600, 10, 16, tag=5), [(0, 600, False)]


def _node_stationary():
    """Past the KEEP range (more than 8,192 nodes): the node-stationary form, direct overlay."""
    return gen.bare_cluster(9000, rf.SEED), rf.queue(2 * B + 1, 2, 2, tag=2), [(0, 2 * B + 1, False)]


def _hash_overlay():
    """More than 32,768 nodes: the hash overlay (node-stationary form), one short run."""
    return gen.bare_cluster(33000, rf.SEED), rf.queue(B + 44, 2, 2, tag=3), [(0, B + 44, False)]


def _unschedulable():
    """test_gpu_reqpatch's fit shapes on 100 nodes: ephemeral storage fits
    twice per node.  Every third pod of the first run (600 pods, 200 of them)
    asks for it and uses all of it up, so in the second run, where every other
    pod asks for it, those pods have no feasible node at all (g1 = 0) and sit
    between pods that bind."""
    n = 100
    cluster = gen.bare_cluster(n, rf.SEED)
    unit = 5 * GI
    cluster.alloc_eph[:] = 100 * GI
    cluster.req_eph[:] = 100 * GI - 2 * unit - 1
    base = gen.bare_pods(900, rf.SEED + 3, 2, 2)
    p = base.pods
    i = np.arange(900)
    p["req_eph"][((i < 600) & (i % 3 == 1)) | ((i >= 600) & (i % 2 == 1))] = unit
    pods = EncodedPods(p, np.zeros(0, abi.LABEL_EXPR_DTYPE), np.zeros(0, abi.TERM_DTYPE), base.names)
    return cluster, pods, [(0, 600, False), (600, 300, False)]


SCENES = {"wide": _wide, "narrow32": _narrow(32), "narrow64": _narrow(64), "narrow96": _narrow(96),
          "lengths": _lengths, "non_zero_start": _non_zero_start, "no_table": _no_table,
          "node_stationary": _node_stationary, "hash_overlay": _hash_overlay, "unschedulable": _unschedulable}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _want(name):
    """The oracle's answer to every run of the scene, computed once and frozen."""
    cluster, pods, runs = _scene(name)
    out, ora = [], None
    for first, count, reset in runs:
        if ora is None or reset:
            ora = Oracle(cluster.copy_state(), rf.prof())
        chosen, st = ora.schedule(pods, first, count, nthreads=16)
        chosen.setflags(write=False)
        state = ora.node_state()
        for v in state.values():
            v.setflags(write=False)
        out.append((chosen, (st.evals, st.scheduled, st.unschedulable), ora.next_start, state))
    return tuple(out)


def _diag(e):
    d = e.diag()
    return {k: d[k] for k in ("batches", "cuts", "truncations", "stretches", "stretch_pods", "reqtab_runs")}


def _run_scene(name, on):
    """Every run of the scene on one handle under the setting, each checked
    against the oracle; the runs' diag() counters."""
    cluster, pods, runs = _scene(name)
    out = []
    with one_cut(on):
        e = rf.engine(cluster, pods, rf.prof())
        for (first, count, reset), (chosen, stats, next_start, state) in zip(runs, _want(name)):
            tag = f"{name} one_cut={on} run {first}+{count}"
            if reset:
                e.reset_cluster()
            r0 = e.diag()["reqtab_runs"]
            c, st = e.schedule_loaded(first, count)
            np.testing.assert_array_equal(c, chosen, err_msg=tag)
            assert (st.evals, st.scheduled, st.unschedulable) == stats, tag
            assert e.next_start == next_start, tag
            es = e.node_state()
            for k in es:
                np.testing.assert_array_equal(es[k], state[k], err_msg=f"{tag} {k}")
            d = _diag(e)
            d["reqtab_runs"] -= r0
            out.append(d)
        e.close()
    return out


@functools.lru_cache(maxsize=None)
def _both(name):
    new, old = _run_scene(name, False), _run_scene(name, True)
    print(name, "stretch:", new)
    print(name, "one cut:", old)
    for a, b in zip(new, old):
        assert a["batches"] <= b["batches"], (name, a, b)
        assert b["stretches"] == 0 and b["stretch_pods"] == 0, (name, b)
        assert a["stretch_pods"] >= a["stretches"], (name, a)
        assert a["reqtab_runs"] == b["reqtab_runs"], (name, a, b)
    return new, old


@pytest.mark.parametrize("name", ["wide", "narrow32", "narrow64", "narrow96", "lengths", "non_zero_start"])
def test_table_scenes(name):
    new, old = _both(name)
    assert all(d["reqtab_runs"] == 1 for d in new), new
    assert sum(d["stretches"] for d in new) > 0, new


def test_fewer_batches():
    """1,024 bare nodes: nearly every one-cut batch ends at a pair cut, and the
    stretch takes strictly fewer batches for the same placements."""
    new, old = _both("wide")
    assert old[0]["cuts"] > old[0]["batches"] // 2, old
    assert new[0]["batches"] < old[0]["batches"], (new, old)
    assert new[0]["stretches"] > 0 and new[0]["stretch_pods"] > 0, new


def test_cuts_and_truncations_mix():
    """The narrow clusters: every scene has batches that end at pair events,
    and over the three some end at exhausted lists too, under both settings."""
    for setting in (0, 1):
        runs = [d for name in ("narrow32", "narrow64", "narrow96") for d in _both(name)[setting]]
        assert all(d["cuts"] > 0 for d in runs), runs
        assert sum(d["truncations"] for d in runs) > 0, runs


@pytest.mark.parametrize("name", ["no_table", "node_stationary", "hash_overlay"])
def test_forms_without_the_table(name):
    new, old = _both(name)
    assert all(d["reqtab_runs"] == 0 for d in new), new
    assert sum(d["stretches"] for d in new) > 0, new


def test_flush_makes_the_second_cut(monkeypatch):
    """KSIM_FEED_FLUSH=1: every stretch of launches ends with a flush, which
    commits the batch before it by the same rule: the same counters as the
    unforced runs', under both settings."""
    want = _both("narrow32")
    monkeypatch.setenv("KSIM_FEED_FLUSH", "1")
    got = _run_scene("narrow32", False), _run_scene("narrow32", True)
    assert got == want, (got, want)
    assert _run_scene("no_table", False) == _both("no_table")[0]


def test_unschedulable_pod_inside_a_stretch():
    """The second run's every other pod has no feasible node (g1 = 0).  Such a
    pod commits as unschedulable (the oracle's placements) and does not end
    the stretch: if it did, no stretch there could hold more than one pod."""
    new, old = _both("unschedulable")
    chosen = _want("unschedulable")[1][0]
    odd = (600 + np.arange(300)) % 2 == 1
    assert (chosen[odd] < 0).all() and (chosen[~odd] >= 0).all()
    assert new[1]["stretches"] > 0, new
    assert new[1]["stretch_pods"] > new[1]["stretches"], new


def test_packed_sweep():
    """Three lanes of the packed sweep (k_sweep_top_commit): every row is the
    oracle's under both settings, and no lane takes more batches with the stretch."""
    cluster, pods = gen.config2(n_nodes=100, n_pods=1500)
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    profs = [profile.compile_profile(base.with_weights(
        {"NodeResourcesBalancedAllocation": ba, "NodeResourcesFit": fit})) for ba, fit in ((1, 1), (1, 3), (10, 1))]
    want = np.stack([Oracle(cluster, pr).schedule(pods, nthreads=16)[0] for pr in profs])
    batches = {}
    for on in (False, True):
        with one_cut(on):
            e = Engine(0)
            e.set_profile(profs[0])
            e.set_cluster(cluster)
            e.load_pods(pods)
            rows, stats = e.sweep_loaded(profs)
            np.testing.assert_array_equal(rows, want, err_msg=f"one_cut={on}")
            batches[on] = [st.batches for st in stats]
            # the serial run of one vector on the same handle: the same batches
            e.set_profile(profs[1])
            e.load_pods(pods)
            e.reset_cluster()
            ch, st = e.schedule_loaded(0, pods.n_pods)
            np.testing.assert_array_equal(ch, want[1])
            assert st.batches == stats[1].batches, (on, st.batches, stats[1].batches)
            e.close()
    print("sweep batches:", batches)
    assert all(a <= b for a, b in zip(batches[False], batches[True])), batches
    assert sum(batches[False]) < sum(batches[True]), batches


def test_replica_pair_uneven_ranges():
    """Two replicas of 1,031 nodes keying 400 and 631 of them: the oracle's
    placements and node state on both, under both settings."""
    cluster, pods = gen.config2(n_nodes=1031, n_pods=1500)
    pr = rf.prof()
    ora = Oracle(cluster, pr)
    want, ost = ora.schedule(pods, nthreads=16)
    state = ora.node_state()
    batches = {}
    for on in (False, True):
        with one_cut(on):
            engines = []
            for lo, hi in ((0, 400), (400, 1031)):
                e = Engine(0)
                e.set_profile(pr)
                e.set_cluster(cluster)
                e.set_eval_range(lo, hi)
                e.load_pods(pods)
                engines.append(e)
            chosen, st = group_schedule_loaded(engines, 0, pods.n_pods)
            np.testing.assert_array_equal(chosen, want, err_msg=f"one_cut={on}")
            assert (st.evals, st.scheduled) == (ost.evals, ost.scheduled), on
            for e in engines:
                es = e.node_state()
                for k in es:
                    np.testing.assert_array_equal(es[k], state[k], err_msg=f"one_cut={on} {k}")
            d = [e.diag() for e in engines]
            assert d[0]["batches"] == d[1]["batches"] and d[0]["stretch_pods"] == d[1]["stretch_pods"], d
            assert (d[0]["stretches"] > 0) == (not on), (on, d[0])
            batches[on] = d[0]["batches"]
            for e in engines:
                e.close()
    print("replica batches:", batches)
    assert batches[False] <= batches[True], batches
