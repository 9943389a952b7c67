"""The pod records of the request-class-table evaluation launch
(csrc/ksim_batch.hip k_batch_top_commit, ksim_internal.h PodRec).

Evaluation launch i writes, once it knows where batch i starts, the records of
pods base + [0, 512) into H[i & 1] (request, class, valid), and launch i + 1
reads its 513 records from there instead of gathering them from the pod queue
behind the state's cursor; a flush writes them too and reqtab_begin fills H[1]
at a run's start.  Every case compares placements, evals, scheduled,
unschedulable, next_start and every node_state() column with the oracle and
checks that the run took the table."""
import functools

import pytest

from ksim import gen
from oracle.oracle import Oracle

import runfeedcases as rf

pytestmark = pytest.mark.gpu

B = rf.B
# records past the end on each side of both halves of the 2 B window
LENGTHS = (B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 1)
NARROW = 32
# The wide scene: 1,024 bare nodes cut down to 2 cores and 4 Gi each, where a
# batch commits all 256 pods (the B-pod run: 1 batch; the scene's 14 runs: 31
# batches, no cut, 3 truncations).  On gen.bare_cluster's own nodes (8 to 64
# cores) a bind of one of these pods rarely moves the node's integer score, so
# the next pod of its class prefers the same node and every batch but a run's
# last ends at a pair cut: at 1,024 / 2,048 / 4,096 / 8,192 nodes the B-pod
# run took 7 / 5 / 4 / 3 batches and the scene 221 / 170 / 74 / 57 with 207 /
# 156 / 60 / 43 cuts.
WIDE = 1024


def _counts(e):
    d = e.diag()
    return d["batches"], d["cuts"], d["truncations"]


def wide_cluster():
    c = gen.bare_cluster(WIDE, rf.SEED)
    c.alloc_cpu[:] = 2000
    c.alloc_mem[:] = 4 << 30
    return c


def _window_edges(cluster):
    """Every length on one handle, each followed by a run of 300 pods from
    where it ended (a stale H, both parities); the runs' (batches, cuts,
    truncations)."""
    pods = rf.queue(3 * B + 1 + rf.FOLLOW)
    n_nodes = cluster.n_nodes
    e = rf.engine(cluster, pods, rf.prof())
    out = []
    for n in LENGTHS:
        e.reset_cluster()
        ora = Oracle(cluster.copy_state(), rf.prof())
        for first, count in ((0, n), (n, rf.FOLLOW)):
            r0 = e.diag()["reqtab_runs"]
            rf.run_and_check(e, ora, pods, first, count, f"{n_nodes} nodes, {n} pods: run {first}+{count}")
            assert e.diag()["reqtab_runs"] == r0 + 1, (n, first)
            out.append(_counts(e))
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def _narrow_unforced():
    return tuple(_window_edges(rf.narrow_cluster(NARROW)))


@functools.lru_cache(maxsize=None)
def _wide_unforced():
    return tuple(_window_edges(wide_cluster()))


def _many_classes():
    """160 classes, 16 B + 1 pods on 96 nodes: the (batches, cuts, truncations)."""
    pods = rf.queue(16 * B + 1, 10, 16, tag=5)
    cluster = rf.narrow_cluster(96)
    e = rf.engine(cluster, pods, rf.prof())
    ora = Oracle(cluster.copy_state(), rf.prof())
    rf.run_and_check(e, ora, pods, 0, pods.n_pods, "160 classes")
    assert e.diag()["reqtab_runs"] == 1
    out = _counts(e)
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def _many_classes_unforced():
    return _many_classes()


def test_window_edges_narrow():
    """32 nodes: nearly every batch ends early, so most launches re-read most
    of the window."""
    runs = _narrow_unforced()
    print("narrow:", runs)
    # a batch binds each node once, and once more at a cut: at most 33 pods
    counts = [c for n in LENGTHS for c in (n, rf.FOLLOW)]
    assert all(b * (NARROW + 1) >= n for (b, _, _), n in zip(runs, counts)), runs
    assert sum(c for _, c, _ in runs) > 0, runs


def test_window_edges_wide():
    """1,024 small nodes: batches commit all 256 pods, so a block's pod is
    candidate 256, the last record of its window."""
    runs = _wide_unforced()
    print("wide:", runs)
    assert runs[2 * LENGTHS.index(B)] == (1, 0, 0), runs      # the B-pod run: one batch, whole
    assert runs[2 * LENGTHS.index(3 * B + 1)] == (4, 0, 0), runs


def test_both_paths_ran():
    """Over the file's scenes: batches that end at a pair cut, truncated ones,
    and batches without a cut."""
    runs = _narrow_unforced() + _wide_unforced() + (_many_classes_unforced(),)
    batches, cuts, trunc = (sum(r[k] for r in runs) for k in range(3))
    print("batches, cuts, truncations:", batches, cuts, trunc)
    assert cuts > 0 and trunc > 0 and batches - cuts > 0, (batches, cuts, trunc)


def test_non_zero_start():
    """A run from pod 37 on a handle whose previous run ended at pod 300."""
    pods = rf.queue(3 * B + 1 + rf.FOLLOW)
    cluster = rf.narrow_cluster(NARROW)
    e = rf.engine(cluster, pods, rf.prof())
    ora = Oracle(cluster.copy_state(), rf.prof())
    rf.run_and_check(e, ora, pods, 0, 300, "run 0+300")
    rf.run_and_check(e, ora, pods, 37, 2 * B + 3, "run 37+515")
    rf.run_and_check(e, ora, pods, B + 1, B, "run 257+256")
    assert e.diag()["reqtab_runs"] == 3
    e.close()


def test_many_classes():
    """160 classes: neighbouring candidates differ in class, and 2 C upkeep
    threads are live."""
    batches, cuts, trunc = _many_classes_unforced()
    print("160 classes:", batches, cuts, trunc)
    assert batches >= 17


def test_flush_writes_the_records(monkeypatch):
    """KSIM_FEED_FLUSH=1 (read at every run, as test_gpu_run_feed.py sets it):
    every stretch ends with a flush, whose records the next launch reads.
    Same placements (the oracle's) and the same batches, cuts and truncations."""
    narrow, many = _narrow_unforced(), _many_classes_unforced()
    monkeypatch.setenv("KSIM_FEED_FLUSH", "1")
    assert tuple(_window_edges(rf.narrow_cluster(NARROW))) == narrow
    assert _many_classes() == many


def test_timing_entry_points():
    """ksim_time_eval and ksim_time_kernels fill H for their own launches, and
    the handle then schedules the same range as the oracle does."""
    pods = rf.queue(3 * B + 1 + rf.FOLLOW)
    cluster = rf.narrow_cluster(NARROW)
    e = rf.engine(cluster, pods, rf.prof())
    name, ms = e.time_eval(37, reps=5)
    assert name == "k_batch_top_commit" and ms > 0, (name, ms)
    e.reset_cluster()
    t = e.time_kernels(37, 2 * B + 3)
    assert t["k_batch_top_commit"][1] > 2 and t["k_batch_chain_pairs"][1] > 2, t
    e.reset_cluster()
    ora = Oracle(cluster.copy_state(), rf.prof())
    r0 = e.diag()["reqtab_runs"]
    rf.run_and_check(e, ora, pods, 37, 2 * B + 3, "after the timing runs")
    assert e.diag()["reqtab_runs"] == r0 + 1
    e.close()
