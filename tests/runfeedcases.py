"""Scenes and helpers for the deferred-commit runs' host loop
(csrc/ksim_engine.cpp run_lazy; tests/test_gpu_run_feed.py).

The loop enqueues batches while none can start past the end of the run, from
the progress word the batches store to host memory.  A narrow cluster makes it
work hardest: a batch commits about as many pods as there are nodes, far fewer
than the 256 the enqueue rule has to assume, so the first stretch covers a
small part of the run and the loop tops the stream up many times."""
from __future__ import annotations

import functools

import numpy as np

from ksim import gen, profile
from ksim.engine import Engine
from oracle.oracle import Oracle

SEED = 0x46454544
B = 256                                             # pods per batch (ksim_batch_geometry out[0])
# every launch-count edge of the loop: one batch, a batch less / plus one pod,
# the tail graph's 4 batches and the 16-batch graph, each plus one pod
LENGTHS = (1, B - 1, B, B + 1, 4 * B, 4 * B + 1, 16 * B, 16 * B + 1)
FOLLOW = 300                                        # the second run on the same handle


def prof(pct: int = 100):
    return profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=pct))


def narrow_cluster(n_nodes: int, alloc_pods: int = 200):
    """gen.bare_cluster with room for more pods per node, so that most of a
    long queue still binds."""
    c = gen.bare_cluster(n_nodes, SEED)
    c.alloc_pods[:] = alloc_pods
    return c


@functools.lru_cache(maxsize=None)
def queue(n_pods: int, cpu_steps: int = 2, mem_steps: int = 2, tag: int = 0):
    """cpu_steps x mem_steps request classes (2 x 2: a run of 32 pods or more
    takes the request-class table; 10 x 16: a run below 1,280 pods does not)."""
    return gen.bare_pods(n_pods, SEED + tag, cpu_steps, mem_steps)


def engine(cluster, pods, pr, variant=None):
    e = Engine(0, variant=variant)
    e.set_profile(pr)
    e.set_cluster(cluster.copy_state())
    e.load_pods(pods)
    return e


def same_state(e, ora, tag):
    assert e.next_start == ora.next_start, tag
    es, os_ = e.node_state(), ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=f"{tag} {k}")


def same_run(got, want, tag):
    (c, st), (oc, ost) = got, want
    np.testing.assert_array_equal(c, oc, err_msg=tag)
    assert (st.evals, st.scheduled, st.unschedulable) == (ost.evals, ost.scheduled, ost.unschedulable), tag


def run_and_check(e, ora, pods, first, count, tag):
    """schedule_loaded(first, count) against the oracle's same range, with the
    node rows read back; returns the engine's stats."""
    got = e.schedule_loaded(first, count)
    same_run(got, ora.schedule(pods, first, count, nthreads=16), tag)
    same_state(e, ora, tag)
    return got[1]


def feed(e) -> dict:
    d = e.diag()
    return {k: d[k] for k in ("feed_syncs", "feed_past_end", "feed_fallbacks", "feed_topups", "feed_odd_ends",
                              "graph_captures", "reqtab_runs", "batches", "truncations", "cuts")}


def delta(after: dict, before: dict) -> dict:
    return {k: after[k] - before[k] for k in after}


def length_edges(cluster, pods, pr, lengths=LENGTHS, follow=FOLLOW):
    """Every length on one handle: reset, a run of that length, a second run
    of `follow` pods from where the first ended (no reset, so it starts from
    what the end launch left).  Returns the per-run diag deltas."""
    e = engine(cluster, pods, pr)
    out = []
    for n in lengths:
        e.reset_cluster()
        ora = Oracle(cluster.copy_state(), pr)
        for first, count in ((0, n), (n, follow)):
            d0 = feed(e)
            st = run_and_check(e, ora, pods, first, count, f"{n} pods: run {first}+{count}")
            d = delta(feed(e), d0)
            d["batches"] = st.batches
            d["pods"] = count
            out.append(d)
    e.close()
    return out
