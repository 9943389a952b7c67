"""The request-class table's patch entries, written by the pairs launch.

On a run that takes the request-class table (csrc/ksim_internal.h ReqTab)
batch i's evaluation launch no longer loads the rows of the nodes batch i-1
guessed: batch i-1's k_batch_chain_pairs, whose thread k holds that row with
pod k bound for its pair key, writes its entry for every class into the
ring (block B - 1 - c keys class c), and the evaluation launch reads one
2-byte entry per guess.  Only the node that takes two pods at a cut is keyed
in the evaluation launch.  Every case compares placements, evals, scheduled,
next_start and every node_state() column with the oracle, and asserts through
diag() that the run took the table ("reqtab_runs"), that bits 27 / 28 / 29 of
"variants" (the table form's launch, its flush, the pairs launch that writes
the patch entries; process-wide, per library) are set, and the batch counters
the case is built for."""
import numpy as np
import pytest

from ksim import abi, gen, profile
from ksim.encode import EncodedPods
from ksim.engine import Engine
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

MI = 1 << 20
GI = 1 << 30
SEED = 0x52455150
RT_BITS = {27, 28, 29}


def _prof():
    return profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=100))


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


def _check(cluster, pods, prof, tag, took=1, variant=None):
    """One engine run of the whole queue against the oracle; took: the runs
    that must have taken the table.  Returns the placements and the run's
    diag()."""
    e = Engine(0, variant=variant)
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    chosen, st = e.schedule_batch(pods)
    ora = Oracle(cluster.copy_state(), prof)
    ochosen, ost = ora.schedule(pods, nthreads=16)
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled) == (ost.evals, ost.scheduled), tag
    _same_state(e, ora, tag)
    d = e.diag()
    assert d["reqtab_runs"] == took, tag
    if took:
        assert RT_BITS <= _bits(e), tag
    e.close()
    return chosen, d


def _edge_case(alloc_pods):
    cluster = gen.bare_cluster(48, SEED)
    cluster.alloc_pods[:] = alloc_pods
    pods = gen.bare_pods(600, SEED, 2, 2)
    assert _classes(pods) == 4
    return cluster, pods


@pytest.mark.parametrize("alloc_pods", [2, 3])
def test_doubled_node_across_a_capacity_edge(alloc_pods):
    """48 nodes that the pod count alone bounds (2, then 3 pods each): one bind
    against two binds on a node flips the verdict of every class, so the entry
    of the node that takes pod k* and pod i* at a cut decides placements."""
    cluster, pods = _edge_case(alloc_pods)
    chosen, d = _check(cluster, pods, _prof(), f"edge {alloc_pods}")
    assert int((chosen >= 0).sum()) == 48 * alloc_pods
    assert d["cuts"] > 0 and d["truncations"] > 0, d


def test_one_class():
    """Only block B - 1 owns a class."""
    cluster = gen.bare_cluster(64, SEED)
    cluster.alloc_pods[:] = 8
    pods = gen.bare_pods(900, SEED, 1, 1)
    assert _classes(pods) == 1
    chosen, d = _check(cluster, pods, _prof(), "one class")
    assert int((chosen >= 0).sum()) == 64 * 8
    assert d["cuts"] + d["truncations"] > 0, d     # 64 nodes: no chain holds a batch's 256 pods


def test_256_classes():
    """Every block owns a class, blocks past a truncated chain's end among
    them.  Every node has the largest size (20 of the largest pods fit), so the
    pod count alone bounds it and exactly 2,000 pods schedule."""
    pods = gen.bare_pods(3000, SEED + 2, 16, 16)
    assert _classes(pods) == 256
    cluster = gen.bare_cluster(100, SEED)
    cluster.alloc_cpu[:] = 64000
    cluster.alloc_mem[:] = 256 * GI
    cluster.alloc_pods[:] = 20
    chosen, d = _check(cluster, pods, _prof(), "256 classes")
    assert int((chosen >= 0).sum()) == 2000
    assert d["truncations"] > 0, d


def _engine(cluster, prof, pods):
    e = Engine(0)
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    e.load_pods(pods)
    return e


def test_short_runs_and_tail():
    """300 pods (one batch and 44), then 100 pods (less than a batch): the
    blocks past the batch's pods still key their classes."""
    cluster, pods, prof = gen.bare_cluster(300, SEED), gen.bare_pods(400, SEED + 7, 2, 2), _prof()
    e = _engine(cluster, prof, pods)
    ora = Oracle(cluster.copy_state(), prof)
    for first, count in ((0, 300), (300, 100)):
        c, st = e.schedule_loaded(first, count)
        oc, ost = ora.schedule(pods, first, count, nthreads=16)
        np.testing.assert_array_equal(c, oc, err_msg=f"run {first}+{count}")
        assert (st.evals, st.scheduled) == (ost.evals, ost.scheduled)
        _same_state(e, ora, f"run {first}+{count}")
        assert e.diag()["batches"] >= (count + 255) // 256
    assert e.diag()["reqtab_runs"] == 2
    assert RT_BITS <= _bits(e)
    e.close()


def test_graph_single_launches_and_flushes():
    """6,000 pods of 4 classes on 300 nodes: a 16-batch graph, single launches
    and more than one flush, every one between two patch slots."""
    pods = gen.bare_pods(6000, SEED + 8, 2, 2)
    assert _classes(pods) == 4
    _, d = _check(gen.bare_cluster(300, SEED), pods, _prof(), "6000 pods")
    assert d["batches"] > 16, d


def test_unschedulable_guesses_inside_a_batch():
    """Pods with no feasible node (g1 == 0) among pods that bind: a class with
    every request zero and a class whose ephemeral-storage request fits twice
    per node, on 100 nodes."""
    n = 100
    cluster = gen.bare_cluster(n, SEED)
    unit = 5 * GI
    cluster.alloc_eph[:] = 100 * GI
    cluster.req_eph[:] = 100 * GI - 2 * unit - 1
    base = gen.bare_pods(900, SEED + 3, 2, 2)
    p = base.pods
    kind = np.arange(900) % 3
    z = kind == 0
    for f in ("req_cpu", "req_mem"):
        p[f][z] = 0
    p["nz_cpu"][z] = 100
    p["nz_mem"][z] = 200 * MI
    p["req_eph"][kind == 1] = unit
    pods = EncodedPods(p, np.zeros(0, abi.LABEL_EXPR_DTYPE), np.zeros(0, abi.TERM_DTYPE), base.names)
    assert 5 < _classes(pods) <= 9
    chosen, d = _check(cluster, pods, _prof(), "fit shapes")
    assert int((chosen[kind == 1] >= 0).sum()) == 2 * n
    assert int((chosen[kind == 1] < 0).sum()) == 300 - 2 * n
    assert d["batches"] > 0, d


def test_reset_and_rerun():
    """run, reset_cluster, run on one engine: no patch slot of the first run
    is read by the second."""
    cluster, pods = _edge_case(3)
    prof = _prof()
    e = _engine(cluster, prof, pods)
    c1, s1 = e.schedule_loaded(0, pods.n_pods)
    n1, d1 = e.node_state(), e.diag()
    e.reset_cluster()
    c2, s2 = e.schedule_loaded(0, pods.n_pods)
    np.testing.assert_array_equal(c1, c2)
    assert (s1.evals, s1.scheduled) == (s2.evals, s2.scheduled)
    n2, d2 = e.node_state(), e.diag()
    for k in n1:
        np.testing.assert_array_equal(n1[k], n2[k], err_msg=k)
    ora = Oracle(cluster.copy_state(), prof)
    oc, ost = ora.schedule(pods, nthreads=16)
    np.testing.assert_array_equal(c2, oc)
    assert (s2.evals, s2.scheduled) == (ost.evals, ost.scheduled)
    _same_state(e, ora, "reset")
    assert d2["reqtab_runs"] == 2
    assert (d1["batches"], d1["cuts"], d1["truncations"]) == (d2["batches"], d2["cuts"], d2["truncations"])
    assert RT_BITS <= _bits(e)
    e.close()


def test_ab128_flavor_has_no_patch_array():
    """The ab128 flavor (no table, so no patch entries) places every pod of
    the capacity-edge queue where the product does."""
    cluster, pods = _edge_case(2)
    prof = _prof()
    got, _ = _check(cluster, pods, prof, "product")
    e = Engine(0, variant="ab128")
    e.set_profile(prof)
    e.set_cluster(cluster.copy_state())
    chosen, _ = e.schedule_batch(pods)
    ora = Oracle(cluster.copy_state(), prof)
    oc, _ = ora.schedule(pods, nthreads=16)
    np.testing.assert_array_equal(chosen, oc)
    _same_state(e, ora, "ab128")
    assert e.diag()["reqtab_runs"] == 0
    assert not (RT_BITS & _bits(e)) and 4 in _bits(e)
    np.testing.assert_array_equal(chosen, got)
    e.close()
