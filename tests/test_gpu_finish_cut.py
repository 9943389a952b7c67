"""The evaluation launch's cut and its top-T finish (ksim_batch.hip
batch_top_commit_body, top_finish) against the oracle.

The cut: a scene of two pod classes under BalancedAllocation-heavy weights,
in which binding a pod of one class raises a node's score for the other, so
that some pod's exact choice is a node bound earlier in its batch: batch
i - 1 is cut at pod i*, which takes an earlier pod's node (that node's
overlay entry carries both requests).  With and without KSIM_FEED_FLUSH
(every stretch ending in the flush form of the launch).

The finish: its candidate array is filled by per-wave offsets, so the cases
are the lane counts at which those differ: 64 nodes (one wave holds every
key, the others none), 1,025 nodes (one lane with two keys) and 3 feasible
nodes of 2,000 (fewer candidates than the list is long).  On the
request-table launch and, where the flavor is built, on the launch without
the table (libksim_engine_ab128.so)."""
import os

import numpy as np
import pytest

from ksim import engine, gen, profile
from ksim.engine import Engine
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

MI = 1 << 20
SEED = 0x46494E43


def _run(cluster, pods, prof, tag, variant=None):
    e = Engine(0, variant=variant)
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    chosen, st = e.schedule_batch(pods)
    ora = Oracle(cluster.copy_state(), prof)
    ochosen, ost = ora.schedule(pods, nthreads=16)
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled) == (ost.evals, ost.scheduled), tag
    assert e.next_start == ora.next_start, tag
    es, os_ = e.node_state(), ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=f"{tag} {k}")
    d = e.diag()
    e.close()
    return st, d


def _two_classes(n):
    """Pods of two skewed classes, interleaved by a seeded stream: 1000m /
    256 Mi and 100m / 4 Gi."""
    pods = gen.bare_pods(n, SEED, 2, 1)
    big_cpu = pods.pods["req_cpu"] == 200
    for f, a, b in (("req_cpu", 1000, 100), ("req_mem", 256 * MI, 4096 * MI)):
        pods.pods[f] = np.where(big_cpu, a, b)
    pods.pods["nz_cpu"] = pods.pods["req_cpu"]
    pods.pods["nz_mem"] = pods.pods["req_mem"]
    return pods


@pytest.mark.parametrize("flush", [False, True])
def test_cut_takes_an_earlier_pods_node(monkeypatch, flush):
    if flush:
        monkeypatch.setenv("KSIM_FEED_FLUSH", "1")
    else:
        monkeypatch.delenv("KSIM_FEED_FLUSH", raising=False)
    cluster = gen.bare_cluster(300, SEED)
    pods = _two_classes(3000)
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    w = {p.name: (10 if p.name == "NodeResourcesBalancedAllocation" else 1) for p in sp.score_plugins()}
    st, d = _run(cluster, pods, profile.compile_profile(sp.with_weights(w)), f"cut flush={flush}")
    print("cut scene:", "batches", d["batches"], "cuts", d["cuts"], "truncations", d["truncations"],
          "reqtab_runs", d["reqtab_runs"])
    assert d["cuts"] > 0
    assert d["reqtab_runs"] == 1


def _finish_clusters():
    few = gen.bare_cluster(2000, SEED)
    few.alloc_pods[:] = 0                                     # no node takes a pod ...
    few.alloc_pods[[5, 1024, 1999]] = 110                     # ... but these three
    return {"64 nodes": gen.bare_cluster(64, SEED), "1025 nodes": gen.bare_cluster(1025, SEED),
            "3 feasible of 2000": few}


@pytest.mark.parametrize("variant", [None, "ab128"])
@pytest.mark.parametrize("name", ["64 nodes", "1025 nodes", "3 feasible of 2000"])
def test_finish_lane_counts(name, variant):
    if variant:
        path = os.path.join(os.path.dirname(engine.LIB_PATH), f"libksim_engine_{variant}.so")
        if not os.path.exists(path):
            pytest.fail(f"{path} missing: __graft_entry__.build() builds it")
    prof = profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=100))
    st, d = _run(_finish_clusters()[name], gen.bare_pods(600, SEED, 3, 3), prof, f"{name} {variant}", variant)
    assert d["reqtab_runs"] == (0 if variant else 1)
    assert st.batches >= 2
