"""ksim_update_node_rows flips the cluster facts the filter plans read, one at
a time: the first hard taint, the first PreferNoSchedule taint, the first
unschedulable node, an allocatable past the FAST key range, a label column that
stops being unique per node, one that stops being carried by every node.
ksim_set_cluster and ksim_update_node_rows compute those facts with one function
(csrc/ksim_snapshot.cpp cluster_facts); tests/test_gpu_fast_edges.py moves only
the reciprocals through the row update.

Per fact two tables over one vocabulary and layout: ``with`` (exactly one node
row carries the fact) and ``without`` (that row cleared).  The one whose nodes
hold the whole vocabulary is encoded and the other derived by editing its
arrays.  Each case runs both ways: engine A takes set_cluster(from) and
update_node_rows(to, [row]), engine B set_cluster(to), the oracle is built on
``to``; all three agree on fail_plugin and total of the first two pods'
cycles and on the whole queue's placements, at percentageOfNodesToScore 100
and 0.  The two oracles of a fact differ on some pod: 8 nodes and 16 pods
are enough for the fact to decide a placement."""
import copy
import functools

import numpy as np
import pytest

from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.engine import Engine
from ksim.model import (Container, LabelSelector, Node, Pod, PodAffinityTerm, Taint, TopologySpreadConstraint)
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

N_NODES, N_PODS, ROW = 8, 16, "n3"
SLOT, RACK = "example.com/slot", "example.com/rack"      # hostname-like (a value per node), zone-like (two values)


def _nodes(taint=None):
    return [Node(f"n{i}", labels={SLOT: f"s{i}", RACK: f"r{i // 4}"},
                 taints=[taint] if taint and f"n{i}" == ROW else [],
                 allocatable={"cpu": "8", "memory": "16Gi", "pods": "110"}) for i in range(N_NODES)]


def _queue(every_other=None):
    """16 equal pods; every_other(pod) dresses the even ones (half the queue)."""
    pods = []
    for k in range(N_PODS):
        p = Pod(f"p{k}", labels={"app": "plain"}, containers=[Container({"cpu": "500m", "memory": "1Gi"})])
        if every_other and k % 2 == 0:
            every_other(p)
        pods.append(p)
    return pods


def _edited(cluster, field, edit):
    """A copy of the encoded cluster with one array replaced (never in place:
    the copies share every other array)."""
    c = copy.copy(cluster)
    a = getattr(cluster, field).copy()
    edit(a, cluster.node_names.index(ROW))
    setattr(c, field, a)
    return c


def _anti(p):
    p.labels = {"app": "apart"}
    p.pod_anti_affinity_required = [PodAffinityTerm(SLOT, LabelSelector({"app": "apart"}))]


def _spread(p):
    p.labels = {"app": "even"}
    p.topology_spread = [TopologySpreadConstraint(1, RACK, "DoNotSchedule", LabelSelector({"app": "even"}))]


def _clear_taints(a, r):
    a[:, r] = 0


def _set_unschedulable(a, r):
    a[r] |= abi.NODE_UNSCHEDULABLE


def _set_wide(a, r):
    a[r] = 1 << 46


@functools.lru_cache(maxsize=None)
def _fact(name):
    """(with, without, pods) of a fact."""
    if name in ("hard_taint", "soft_taint"):
        effect = "NoSchedule" if name == "hard_taint" else "PreferNoSchedule"
        with_, _ = encode_cluster(_nodes(Taint("dedicated", "x", effect)))
        pods = encode_pods(with_, _queue())
        return with_, _edited(with_, "taints", _clear_taints), pods
    without, _ = encode_cluster(_nodes())
    if name == "unschedulable":
        pods = encode_pods(without, _queue())
        return _edited(without, "flags", _set_unschedulable), without, pods
    if name == "wide_allocatable":
        pods = encode_pods(without, _queue())
        return _edited(without, "alloc_cpu", _set_wide), without, pods
    if name == "unique_column":           # n3 takes n2's value: two nodes share a domain of the anti-affinity key
        pods = encode_pods(without, _queue(_anti))
        col, n2 = without.label_keys.index(SLOT), without.node_names.index("n2")

        def share(a, r):
            a[col, r] = a[col, n2]
        return _edited(without, "labels", share), without, pods
    assert name == "total_column"         # n3 loses the spread key
    pods = encode_pods(without, _queue(_spread))
    col = without.label_keys.index(RACK)

    def drop(a, r):
        a[col, r] = 0
    return _edited(without, "labels", drop), without, pods


FACTS = ("hard_taint", "soft_taint", "unschedulable", "wide_allocatable", "unique_column", "total_column")
PCTS = (100, 0)


def _table(name, side):
    with_, without, pods = _fact(name)
    return (with_ if side == "with" else without), pods


@functools.lru_cache(maxsize=None)
def _prof(pct):
    return profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=pct))


def _run(sched, cycle, pods):
    """The first two pods' cycles, then the whole queue: ([(fail_plugin, total)], placements)."""
    cyc = []
    for i in (0, 1):
        o = cycle(pods, i)
        cyc.append((np.array(o["fail_plugin"]), np.array(o["total"])))
    chosen = np.array(sched(pods)[0])
    return cyc, chosen


@functools.lru_cache(maxsize=None)
def _oracle(name, side, pct):
    cluster, pods = _table(name, side)
    ora = Oracle(cluster.copy_state(), _prof(pct))
    cyc, chosen = _run(ora.schedule, ora.cycle, pods)
    ora.close()
    chosen.setflags(write=False)
    return cyc, chosen


def _same(got, want, tag):
    for i, ((gf, gt), (wf, wt)) in enumerate(zip(got[0], want[0])):
        np.testing.assert_array_equal(gf, wf, err_msg=f"{tag} pod {i} fail_plugin")
        np.testing.assert_array_equal(gt, wt, err_msg=f"{tag} pod {i} total")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{tag} placements")


@pytest.mark.parametrize("direction", ["gains", "loses"])
@pytest.mark.parametrize("name", FACTS)
def test_row_update_flips_fact(name, direction):
    src, dst = ("without", "with") if direction == "gains" else ("with", "without")
    (from_, pods), (to, _) = _table(name, src), _table(name, dst)
    row = [to.node_names.index(ROW)]
    for pct in PCTS:
        want = _oracle(name, dst, pct)
        # the scene exercises the fact: it moves a placement
        assert (want[1] != _oracle(name, src, pct)[1]).any(), f"{name} pct {pct}: the fact decides no placement"
        a = Engine(0)
        a.set_profile(_prof(pct))
        a.set_cluster(from_.copy_state())
        a.update_node_rows(to.copy_state(), row)
        _same(_run(a.schedule_batch, a.eval_pod, pods), want, f"{name} {direction} pct {pct}: row update")
        a.close()
        b = Engine(0)
        b.set_profile(_prof(pct))
        b.set_cluster(to.copy_state())
        _same(_run(b.schedule_batch, b.eval_pod, pods), want, f"{name} {direction} pct {pct}: set_cluster")
        b.close()
