"""The deferred-commit runs' host loop (csrc/ksim_engine.cpp run_lazy).

A run begins with one launch (counters, run header, window state, X[1] = X[0],
st[1] = st[0], the ring emptied), is fed from the progress word the batches
store to host memory (16-batch graphs, 4-batch tail graphs, single launches;
never a batch that could start past the end), commits its last batch with a
flush and ends with one launch when that flush's ring index is odd.  Every
case compares placements, evals, scheduled, unschedulable, next_start and
every node_state() column with the oracle; diag()'s feed_* counters tell what
the loop did.  KSIM_FEED_FLUSH=1 forces the loop's fallback on every stretch
(a flush and a synchronised state read: the loop this one replaced), which
must give the same batches, cuts and truncations."""
import numpy as np
import pytest

from ksim import gen
from oracle.oracle import Oracle

import runfeedcases as rf

pytestmark = pytest.mark.gpu


def _check_edges(runs, table):
    for d in runs:
        assert d["feed_past_end"] == 0, d                     # no batch was enqueued past its run's end
        assert d["feed_syncs"] <= d["feed_fallbacks"], d      # the loop itself never synchronises
        assert d["batches"] >= (d["pods"] + rf.B - 1) // rf.B, d
        assert d["reqtab_runs"] == (1 if table and d["pods"] >= 32 else 0), d
    assert max(d["feed_topups"] - d["feed_fallbacks"] for d in runs) >= 3, runs   # topped up by the word, often
    odd = sum(d["feed_odd_ends"] for d in runs)
    assert 0 < odd < len(runs), runs                          # both end parities


def test_length_edges_table():
    """32 nodes, 4 request classes: every run of 32 pods or more takes the
    request-class table, whose graphs later runs reuse."""
    pods = rf.queue(16 * rf.B + 1 + rf.FOLLOW)
    runs = rf.length_edges(rf.narrow_cluster(32), pods, rf.prof())
    _check_edges(runs, table=True)
    # the 1-pod run has no table: the plain graph and its tail graph, then the table's two, none after
    assert [d["graph_captures"] for d in runs[:2]] == [2, 2], runs[:2]
    assert sum(d["graph_captures"] for d in runs[2:]) == 0, runs


def test_length_edges_no_table():
    """160 request classes: no run below 1,280 pods takes the table, so the
    plain deferred-commit graphs run; the 16 x 256 runs take the table."""
    pods = rf.queue(16 * rf.B + 1 + rf.FOLLOW, 10, 16, tag=1)
    cluster = rf.narrow_cluster(24)
    e = rf.engine(cluster, pods, rf.prof())
    seen = []
    for n in rf.LENGTHS:
        e.reset_cluster()
        ora = Oracle(cluster.copy_state(), rf.prof())
        for first, count in ((0, n), (n, rf.FOLLOW)):
            d0 = rf.feed(e)
            rf.run_and_check(e, ora, pods, first, count, f"{n} pods: run {first}+{count}")
            d = rf.delta(rf.feed(e), d0)
            assert d["feed_past_end"] == 0 and d["feed_syncs"] <= d["feed_fallbacks"], d
            assert d["reqtab_runs"] == (1 if count >= 8 * 160 else 0), (count, d)
            seen.append(d)
    # the plain graphs with the first run, the table's with the first 4,096-pod run, none after
    assert seen[0]["graph_captures"] == 2, seen[0]
    assert sum(d["graph_captures"] for d in seen) == 4, seen
    assert sum(d["graph_captures"] for d in seen[-3:]) == 0, seen[-3:]
    e.close()


@pytest.mark.parametrize("n_nodes", [5, 33])
def test_column_sizes_off_the_16_byte_grid(n_nodes):
    """N = 5 and N = 33: no column of the begin and end launches' copies is a
    whole number of 16-byte words (num_pods: 20 and 132 bytes)."""
    pods = rf.queue(4 * rf.B + 1 + rf.FOLLOW)
    runs = rf.length_edges(rf.narrow_cluster(n_nodes, 150), pods, rf.prof(),
                           lengths=(1, rf.B + 1, 4 * rf.B + 1))
    for d in runs:
        assert d["feed_past_end"] == 0, d
    assert 0 < sum(d["feed_odd_ends"] for d in runs) < len(runs), runs


def test_sub_range():
    """first > 0 and first + count < n_pods: the pods outside stay unplaced
    and the node rows hold the range's pods alone."""
    pods = rf.queue(1200)
    cluster = rf.narrow_cluster(32)
    e = rf.engine(cluster, pods, rf.prof())
    ora = Oracle(cluster.copy_state(), rf.prof())
    st = rf.run_and_check(e, ora, pods, 100, 700, "sub-range")
    assert st.scheduled + st.unschedulable == 700
    assert int(e.node_state()["num_pods"].sum()) == st.scheduled
    assert e.diag()["feed_past_end"] == 0
    e.close()


@pytest.mark.parametrize("seps", [(450,), (0, 450)])
def test_several_runs_in_one_call(seps):
    """A pod that takes the per-pod path (it adds node bandwidth) in the
    middle of the queue: a batch run, a per-pod run, a batch run in one call,
    whose counters cover all three; with pod 0 one too, the call's first run
    is a per-pod run, and the batch run behind it must keep its counts."""
    pods = gen.bare_pods(900, rf.SEED + 2, 2, 2)
    for i in seps:
        pods.pods["nb_add"][i] = 1
    cluster = rf.narrow_cluster(32)
    e = rf.engine(cluster, pods, rf.prof())
    ora = Oracle(cluster.copy_state(), rf.prof())
    st = rf.run_and_check(e, ora, pods, 0, 900, f"separators {seps}")
    assert st.perpod_cycles == len(seps) and st.scheduled + st.unschedulable == 900
    assert st.batches >= 4
    # the same call again: the counters start from zero again
    e.reset_cluster()
    ora = Oracle(cluster.copy_state(), rf.prof())
    st2 = rf.run_and_check(e, ora, pods, 0, 900, "again")
    assert (st2.batches, st2.truncations, st2.evals) == (st.batches, st.truncations, st.evals)
    e.close()


def test_length_edges_adapt():
    """ADAPT (K = 144 of 300 nodes) shares the loop."""
    pods = rf.queue(16 * rf.B + 1 + rf.FOLLOW, tag=3)
    runs = rf.length_edges(rf.narrow_cluster(300, 110), pods, rf.prof(0))
    for d in runs:
        assert d["feed_past_end"] == 0 and d["feed_syncs"] <= d["feed_fallbacks"] and d["reqtab_runs"] == 0, d
    assert sum(d["graph_captures"] for d in runs) == 2, runs


def _stall_scene():
    return rf.narrow_cluster(32), rf.queue(360, tag=4)


def test_forced_fallback_is_the_same_run(monkeypatch):
    """KSIM_FEED_FLUSH=1: every stretch ends with a flush and a state read.
    Same placements, rows and counters as the oracle's and the product's."""
    cluster, pods = _stall_scene()
    e = rf.engine(cluster, pods, rf.prof())
    ora = Oracle(cluster.copy_state(), rf.prof())
    st = rf.run_and_check(e, ora, pods, 0, pods.n_pods, "product")
    d1 = rf.feed(e)
    monkeypatch.setenv("KSIM_FEED_FLUSH", "1")
    e.reset_cluster()
    ora = Oracle(cluster.copy_state(), rf.prof())
    st2 = rf.run_and_check(e, ora, pods, 0, pods.n_pods, "forced")
    d2 = rf.delta(rf.feed(e), d1)
    assert d2["feed_fallbacks"] >= 3 and d2["feed_syncs"] == d2["feed_fallbacks"], d2
    assert d2["feed_past_end"] == 0, d2
    assert (st2.batches, st2.truncations) == (st.batches, st.truncations)
    d2abs = rf.feed(e)
    assert (d2abs["batches"], d2abs["cuts"], d2abs["truncations"]) == (d1["batches"], d1["cuts"], d1["truncations"])
    e.close()


def test_no_stall_per_stretch(monkeypatch):
    """About 50 batches on 32 nodes.  The loop this one replaced launched
    ceil(left / 256) batches, flushed, read the state and synchronised, again
    and again: the forced form counts those stretches (at least 3 here, far
    more in fact).  The product's run may synchronise once more than it took
    fallbacks, and is topped up by the progress word instead."""
    cluster, pods = _stall_scene()
    e = rf.engine(cluster, pods, rf.prof())
    ora = Oracle(cluster.copy_state(), rf.prof())
    d0 = rf.feed(e)
    st = rf.run_and_check(e, ora, pods, 0, pods.n_pods, "product")
    d = rf.delta(rf.feed(e), d0)
    assert 30 <= st.batches <= 80, st.batches
    print("product:", d)
    assert d["feed_syncs"] <= d["feed_fallbacks"] + 1, d
    assert d["feed_topups"] - d["feed_fallbacks"] >= 3, d
    monkeypatch.setenv("KSIM_FEED_FLUSH", "1")
    e.reset_cluster()
    d0 = rf.feed(e)
    e.schedule_loaded(0, pods.n_pods)
    old = rf.delta(rf.feed(e), d0)
    print("stretch loop:", old)
    assert old["feed_syncs"] >= 3 and old["feed_fallbacks"] >= 3, old   # what the old rule costs on this scene
    e.close()
