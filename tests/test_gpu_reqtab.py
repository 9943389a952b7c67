"""The request-class table of the P100 deferred-commit batches.

Pods of a loaded queue that share their five request fields share a class,
and on a KEEP / DEF run of at least 8 pods per class k_batch_top_commit reads
each (class, node) verdict and score pair from a table (csrc/ksim_internal.h
ReqTab) instead of computing it per pod.  Every case compares placements,
evals, scheduled, next_start and every node_state() column with the oracle,
and asserts through diag() whether the run took the table: "reqtab_runs"
counts this engine's runs that did, and bits 27 / 28 of "variants" are the
table form's launch and its flush (process-wide, per library)."""
import numpy as np
import pytest

from ksim import abi, gen, profile
from ksim.encode import EncodedPods
from ksim.engine import Engine
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

MI = 1 << 20
GI = 1 << 30
SEED = 0x52455154


def _prof(weights=None):
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    if weights:
        sp = sp.with_weights(weights)
    return profile.compile_profile(sp)


def _bits(e):
    m = e.diag()["variants"]
    return {b for b in range(64) if m >> b & 1}


def _classes(pods):
    p = pods.pods
    return len({tuple(int(p[f][i]) for f in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem"))
                for i in range(len(p))})


def _same_state(e, ora, tag):
    assert e.next_start == ora.next_start, tag
    es, os_ = e.node_state(), ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=f"{tag} {k}")


def _check(cluster, pods, prof, tag, took, variant=None):
    """One engine run of the whole queue against the oracle; took: the runs
    that must have taken the table.  Returns the placements."""
    e = Engine(0, variant=variant)
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    chosen, st = e.schedule_batch(pods)
    ora = Oracle(cluster.copy_state(), prof)
    ochosen, ost = ora.schedule(pods, nthreads=16)
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled) == (ost.evals, ost.scheduled), tag
    _same_state(e, ora, tag)
    assert e.diag()["reqtab_runs"] == took, tag
    if took:
        assert {27, 28} <= _bits(e), tag
    e.close()
    return chosen


@pytest.mark.parametrize("n_nodes", [1, 64, 1023, 1025, 5000, 8192])
def test_node_range_takes_the_table(n_nodes):
    """Every lane count of the KEEP range: one node, one wave, one node short
    of and past a full block, the headline size, the range's last size."""
    pods = gen.bare_pods(1500, SEED, 3, 3)
    assert _classes(pods) == 9
    _check(gen.bare_cluster(n_nodes, SEED), pods, _prof(), f"nodes {n_nodes}", 1)


def test_past_the_keep_range_falls_back():
    _check(gen.bare_cluster(8193, SEED), gen.bare_pods(1500, SEED, 3, 3), _prof(), "nodes 8193", 0)


def test_cluster_that_fills():
    """40 nodes of 8 pods each under 600 pods of 4 classes: lists exhaust,
    batches truncate, consecutive batches guess the same nodes, i* lands on
    earlier guesses, nodes turn infeasible and 280 pods stay unschedulable."""
    cluster = gen.bare_cluster(40, SEED)
    cluster.alloc_pods[:] = 8
    pods = gen.bare_pods(600, SEED + 1, 2, 2)
    assert _classes(pods) == 4
    chosen = _check(cluster, pods, _prof(), "fills", 1)
    assert int((chosen >= 0).sum()) == 320


def _pods_256():
    pods = gen.bare_pods(3000, SEED + 2, 16, 16)
    assert _classes(pods) == 256
    return pods


def test_256_classes_take_the_table():
    _check(gen.bare_cluster(500, SEED), _pods_256(), _prof(), "256 classes", 1)


def test_257_classes_fall_back():
    pods = _pods_256()
    pods.pods["req_eph"][17] = 1                  # a class of its own
    assert _classes(pods) == 257
    _check(gen.bare_cluster(500, SEED), pods, _prof(), "257 classes", 0)


def test_short_config2_queue_falls_back():
    """700 config-2 pods carry 159 classes: fewer than 8 pods per class."""
    cluster, pods = gen.config2(n_nodes=500, n_pods=700)
    assert 8 * _classes(pods) > 700
    _check(cluster, pods, _prof(), "config2 700", 0)


def test_fit_special_cases():
    """A class with every request zero (Fit tests the pod count alone) and a
    class with an ephemeral-storage request on nodes whose ephemeral storage
    is set and nearly full (two such pods fit a node), among ordinary pods."""
    n = 100
    cluster = gen.bare_cluster(n, SEED)
    unit = 5 * GI
    cluster.alloc_eph[:] = 100 * GI
    cluster.req_eph[:] = 100 * GI - 2 * unit - 1
    base = gen.bare_pods(900, SEED + 3, 2, 2)
    p = base.pods
    kind = np.arange(900) % 3
    z = kind == 0                                 # no requests: the non-zero defaults alone
    for f in ("req_cpu", "req_mem"):
        p[f][z] = 0
    p["nz_cpu"][z] = 100
    p["nz_mem"][z] = 200 * MI
    p["req_eph"][kind == 1] = unit
    pods = EncodedPods(p, np.zeros(0, abi.LABEL_EXPR_DTYPE), np.zeros(0, abi.TERM_DTYPE), base.names)
    assert 5 < _classes(pods) <= 9
    chosen = _check(cluster, pods, _prof(), "fit shapes", 1)
    assert int((chosen[kind == 1] >= 0).sum()) == 2 * n   # the rest of the class found every node full


def _engine(cluster, prof, pods):
    e = Engine(0)
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    e.load_pods(pods)
    return e


def test_reset_between_runs():
    """run, reset_cluster, run: the second run's table is rebuilt from the
    restored snapshot, not left at the first run's end."""
    cluster, pods, prof = gen.bare_cluster(300, SEED), gen.bare_pods(1200, SEED + 4, 2, 2), _prof()
    e = _engine(cluster, prof, pods)
    c1, s1 = e.schedule_loaded(0, pods.n_pods)
    n1 = e.node_state()
    e.reset_cluster()
    c2, s2 = e.schedule_loaded(0, pods.n_pods)
    np.testing.assert_array_equal(c1, c2)
    assert (s1.evals, s1.scheduled) == (s2.evals, s2.scheduled)
    n2 = e.node_state()
    for k in n1:
        np.testing.assert_array_equal(n1[k], n2[k], err_msg=k)
    ora = Oracle(cluster.copy_state(), prof)
    oc, _ = ora.schedule(pods, nthreads=16)
    np.testing.assert_array_equal(c2, oc)
    _same_state(e, ora, "reset")
    assert e.diag()["reqtab_runs"] == 2
    e.close()


@pytest.mark.parametrize("sep", ["nb_add", "node_name"])
def test_stretches_between_other_pods(sep):
    """Batchable stretches separated by pods the table does not cover.  A pod
    that adds node bandwidth takes a per-pod cycle, which moves X between two
    table runs; a spec.nodeName pod is not trivial, so its whole run keeps
    the static-class kernels."""
    cluster, pods, prof = gen.bare_cluster(200, SEED), gen.bare_pods(1000, SEED + 5, 2, 2), _prof()
    for i in (300, 301, 650):
        if sep == "nb_add":
            pods.pods["nb_add"][i] = 1
        else:
            pods.pods["node_name"][i] = 7
    _check(cluster, pods, prof, f"stretches {sep}", 3 if sep == "nb_add" else 0)


def test_profile_change_between_runs():
    """Other score weights between two runs of one engine: the entries hold
    the two scores, not their weighted sum."""
    cluster, pods = gen.bare_cluster(300, SEED), gen.bare_pods(1200, SEED + 6, 2, 2)
    pa = _prof()
    pb = _prof({"NodeResourcesFit": 3, "NodeResourcesBalancedAllocation": 7})
    e = _engine(cluster, pa, pods)
    c1, _ = e.schedule_loaded(0, 600)
    e.set_profile(pb)
    e.load_pods(pods)                             # a profile change unloads the queue
    c2, _ = e.schedule_loaded(600, 600)
    oa = Oracle(cluster.copy_state(), pa)
    o1, _ = oa.schedule(pods, 0, 600, nthreads=16)
    mid = cluster.copy_state()
    for k, v in oa.node_state().items():
        getattr(mid, k)[:] = v
    ob = Oracle(mid, pb)
    ob.set_pod_seq(600)
    ob.set_next_start(oa.next_start)
    o2, _ = ob.schedule(pods, 600, 600, nthreads=16)
    np.testing.assert_array_equal(c1, o1)
    np.testing.assert_array_equal(c2, o2)
    _same_state(e, ob, "weights 3 / 7")
    assert e.diag()["reqtab_runs"] == 2
    e.close()


def test_run_ends_mid_batch_and_short_run():
    """300 pods (one batch and 44), then 100 pods (less than a batch)."""
    cluster, pods, prof = gen.bare_cluster(300, SEED), gen.bare_pods(400, SEED + 7, 2, 2), _prof()
    e = _engine(cluster, prof, pods)
    ora = Oracle(cluster.copy_state(), prof)
    for first, count in ((0, 300), (300, 100)):
        c, st = e.schedule_loaded(first, count)
        oc, ost = ora.schedule(pods, first, count, nthreads=16)
        np.testing.assert_array_equal(c, oc, err_msg=f"run {first}+{count}")
        assert (st.evals, st.scheduled) == (ost.evals, ost.scheduled)
        _same_state(e, ora, f"run {first}+{count}")
    assert e.diag()["reqtab_runs"] == 2
    e.close()


def test_ab_form_keys_every_pair():
    """The ab128 flavor (the table off alone) runs today's KEEP / DEF kernel
    and places every pod where the product does."""
    cluster, pods, prof = gen.bare_cluster(1025, SEED), gen.bare_pods(1500, SEED, 3, 3), _prof()
    got = _check(cluster, pods, prof, "product", 1)
    e = Engine(0, variant="ab128")
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    chosen, _ = e.schedule_batch(pods)
    assert e.diag()["reqtab_runs"] == 0
    assert not ({27, 28} & _bits(e)) and 4 in _bits(e)
    np.testing.assert_array_equal(chosen, got)
    e.close()
