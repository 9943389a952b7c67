"""Pods with container images on the batch paths (csrc/ksim_engine.cpp
pod_batchable: a pod whose uses are exactly one KSIM_USE_IMAGE is class 2; the
keys carry w_il * score beside the normalized parts, csrc/ksim_device.h
norm_part, from the static-table word's image field, stab_word, or from the
image class's count column, norm_raw), bit for bit against the oracle.

tests/test_image_cases.py proves on the CPU that the scenes of
tests/imagecases.py tell the wrong readings of the image part apart; here every
scene goes through schedule_batch at percentageOfNodesToScore 100 and 0, and
the path counters pin the route: no per-pod cycle for image pods within the
key bound, one per pod past it and on a sharded group.

Every comparison is exact: placements, evals, scheduled, next_start, every
node_state() column and class_count().  The oracle's run of a scene is computed
once per (scene, percentage, profile)."""
import functools

import numpy as np
import pytest

from ksim import profile
from ksim.engine import Engine, group_schedule_loaded
from ksim.shard import partition
from oracle.oracle import Oracle

import imagecases as ic

pytestmark = pytest.mark.gpu

PCTS = (100, 0)
NODE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)
QUEUE_LENGTHS = (1, 255, 256, 257, 513)


def _scene(key):
    """key: a scene name, ("sized", n_nodes, n_pods) or ("sigs",)."""
    if isinstance(key, str):
        return ic.scene(key)
    if key[0] == "sized":
        return ic.sized(key[1], key[2])
    return ic.many_signatures()


@functools.lru_cache(maxsize=None)
def _oracle(key, pct, il="scene"):
    s = _scene(key)
    cluster, pods = s.encoded
    prof = s.compiled(pct) if il == "scene" else s.compiled(pct, ic.make_profile(il))
    ora = Oracle(cluster.copy_state(), prof)
    chosen, st = ora.schedule(pods, nthreads=16)
    chosen.setflags(write=False)
    out = chosen, (st.evals, st.scheduled), ora.next_start, ora.node_state(), ora.class_count()
    ora.close()
    return out


def _same_state(e, want, tag):
    _, _, onext, ostate, ocount = want
    assert e.next_start == onext, tag
    es = e.node_state()
    assert set(es) == set(ostate), tag
    for k in es:
        np.testing.assert_array_equal(es[k], ostate[k], err_msg=f"{tag} {k}")
    np.testing.assert_array_equal(e.class_count(), ocount, err_msg=f"{tag} class_count")


def _same(e, chosen, st, want, tag):
    np.testing.assert_array_equal(chosen, want[0], err_msg=tag)
    assert (st.evals, st.scheduled) == want[1], tag
    _same_state(e, want, tag)


def _run(key, pct, variant=None):
    s = _scene(key)
    cluster, pods = s.encoded
    e = Engine(0, variant=variant)
    try:
        e.set_profile(s.compiled(pct))
        e.set_cluster(cluster.copy_state())
        chosen, st = e.schedule_batch(pods)
        _same(e, chosen, st, _oracle(key, pct), f"{s.name} pct {pct} {variant or ''}")
        return st
    finally:
        e.close()


def _assert_route(s, st, pct):
    n = len(s.queue)
    if s.route == "batch" or (s.route == "p100" and pct == 100):
        assert st.perpod_cycles == 0 and st.batches > 0, (s.name, pct, st.perpod_cycles, st.batches)
    elif s.route == "perpod":
        assert st.perpod_cycles == n, (s.name, pct, st.perpod_cycles)


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("name", ic.SCENES)
def test_scene(name, pct):
    """Every scene against the oracle; image pods within the key bound run no
    per-pod cycle (scalar + image pods: under 100 only), those past it one each."""
    s = ic.scene(name)
    st = _run(name, pct)
    _assert_route(s, st, pct)
    if len(s.nodes) > 100:
        # at percentage 0 such a scene runs in ADAPT: a window of K < N nodes
        assert profile.num_feasible_nodes_to_find(len(s.nodes), 0) < len(s.nodes), name


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_node_counts(n_nodes, pct):
    key = ("sized", n_nodes, 96)
    st = _run(key, pct)
    assert st.perpod_cycles == 0 and st.batches > 0, (n_nodes, pct, st.perpod_cycles)


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("n_pods", QUEUE_LENGTHS)
def test_queue_lengths(n_pods, pct):
    key = ("sized", 130, n_pods)
    st = _run(key, pct)
    assert st.perpod_cycles == 0 and st.batches > 0, (n_pods, pct, st.perpod_cycles)


def test_more_signatures_than_static_classes():
    """4,097 static signatures on 64 nodes, an image in each (2,049 image
    classes: a cluster holds at most 4,096 count classes): the pods past
    kStabMaxClasses have no static class and still run on the batch path
    (norm_raw)."""
    s = ic.many_signatures()
    cluster, pods = s.encoded
    assert len(ic.image_rows(cluster)) == 2049 and pods.n_pods == ic.STAB_MAX_CLASSES + 1
    assert ic.image_pods(pods).all()
    st = _run(("sigs",), 100)
    assert st.perpod_cycles == 0 and st.batches > 0


@pytest.mark.parametrize("name", ["three_parts", "fills_up"])
def test_without_the_static_table(name):
    """The flavor without the static-class table: every key reads the image
    class's count column."""
    st = _run(name, 100, variant="ab1")
    assert st.perpod_cycles == 0 and st.batches > 0


@pytest.mark.parametrize("pct", PCTS)
def test_sharded_group_runs_per_pod(pct):
    """An in-process shard group: image pods keep the per-pod path there."""
    s = ic.scene("three_parts")
    cluster, pods = s.encoded
    prof = s.compiled(pct)
    engines = []
    try:
        for base, cnt in partition(cluster.n_nodes, 3):
            e = Engine(0)
            e.set_shard(base, cluster.n_nodes)
            e.set_profile(prof)
            e.set_cluster(cluster.shard(base, cnt))
            e.load_pods(pods)
            engines.append(e)
        chosen, st = group_schedule_loaded(engines, 0, pods.n_pods)
        want = _oracle("three_parts", pct)
        np.testing.assert_array_equal(chosen, want[0])
        assert (st.evals, st.scheduled) == want[1]
        assert st.batches == 0                 # (a group's stats carry no per-pod count) no batch ran
        parts = [e.node_state() for e in engines]
        for k in parts[0]:
            np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), want[3][k], err_msg=k)
    finally:
        for e in engines:
            e.close()


# ---- lifetime ---------------------------------------------------------------------------
@pytest.mark.parametrize("pct", PCTS)
def test_node_delta_rebuilds_the_image_field(pct):
    """Half the queue, then nodes that hold the image join (every holder's
    score moves from 30 to 81), then the other half: the second run's keys
    follow the new counts, on the batch path both times."""
    s = ic.scene("delta")
    c0, p0 = s.encoded
    c1, p1 = s.encoded_after
    half = len(s.queue) // 2
    prof = s.compiled(pct)
    old_pos = ic.old_positions(c0, c1)
    ora = Oracle(c0.copy_state(), prof)
    e = Engine(0)
    try:
        e.set_profile(prof)
        e.set_cluster(c0.copy_state())
        e.load_pods(p0)
        a, st = e.schedule_loaded(0, half)
        oa, ost = ora.schedule(p0, 0, half)
        np.testing.assert_array_equal(a, oa)
        assert st.evals == ost.evals and st.perpod_cycles == 0 and st.batches > 0
        e.upsert_nodes(c1.copy_state(), old_pos)
        ora.upsert_nodes(c1.copy_state(), old_pos)
        e.load_pods(p1)
        b, st = e.schedule_loaded(half, len(s.queue) - half)
        ob, ost = ora.schedule(p1, half, len(s.queue) - half)
        np.testing.assert_array_equal(b, ob)
        assert st.evals == ost.evals and st.perpod_cycles == 0 and st.batches > 0
        assert (b >= c0.n_nodes).any()
        _same_state(e, (None, None, ora.next_start, ora.node_state(), ora.class_count()), f"delta pct {pct}")
    finally:
        e.close()
        ora.close()


@pytest.mark.parametrize("pct", PCTS)
def test_reset_cluster_between_runs(pct):
    """ksim_reset_cluster restores counts the image classes never moved: the
    second run repeats the first."""
    s = ic.scene("fills_up")
    cluster, pods = s.encoded
    want = _oracle("fills_up", pct)
    e = Engine(0)
    try:
        e.set_profile(s.compiled(pct))
        e.set_cluster(cluster.copy_state())
        e.load_pods(pods)
        for rep in range(2):
            chosen, st = e.schedule_loaded(0, pods.n_pods)
            _same(e, chosen, st, want, f"fills_up pct {pct} run {rep}")
            assert st.perpod_cycles == 0 and st.batches > 0
            e.reset_cluster()
            e.set_pod_seq(0)
            np.testing.assert_array_equal(e.class_count(), cluster.class_count)
    finally:
        e.close()


@pytest.mark.parametrize("pct", PCTS)
def test_profile_changes_the_image_weight(pct):
    """One handle, the same pods under ImageLocality weights 1, 5 and without
    the plugin: each run is the oracle's under that profile, on the batch path."""
    s = ic.scene("weight_five")
    cluster, pods = s.encoded
    e = Engine(0)
    runs = {}
    try:
        e.set_profile(s.compiled(pct))
        e.set_cluster(cluster.copy_state())
        for il in (1, 5, None):
            e.set_profile(s.compiled(pct, ic.make_profile(il)))
            e.reset_cluster()
            e.set_pod_seq(0)
            e.load_pods(pods)
            chosen, st = e.schedule_loaded(0, pods.n_pods)
            _same(e, chosen, st, _oracle("weight_five", pct, il), f"weight_five pct {pct} il {il}")
            assert st.perpod_cycles == 0 and st.batches > 0, (il, st.perpod_cycles)
            runs[il] = chosen
        assert (runs[1] != runs[5]).any() and (runs[1] != runs[None]).any()
    finally:
        e.close()
