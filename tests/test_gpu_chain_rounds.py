"""The batch chain's tagged one-barrier rounds (ksim_chain.h chain_block;
tests/test_chain_tagged_protocol.py models the protocol) on the device:
placements, every node_state() column, next_start and the counters against
the oracle, in direct mode (the holders indexed by node id) and hash mode
(n_total > kChainDirect = 8192), on chains of one round and of many, on
batches of one pod, a full batch and a tail of one pod.  The long-chain and
the queue-length cases also run on the KSIM_CHAIN_DELAY flavor
(libksim_engine_chaindelay.so), which makes one wave late after every round's
barrier and another late before it registers for the next round."""
import os

import numpy as np
import pytest

from ksim import engine, gen, profile
from ksim.engine import Engine
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

GI = 1 << 30
DELAY = "chaindelay"
FLAVORS = [None, DELAY]


def _prof(pct=100):
    return profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=pct))


def _check(cluster, pods, prof, tag, variant=None):
    if variant:
        path = os.path.join(os.path.dirname(engine.LIB_PATH), f"libksim_engine_{variant}.so")
        if not os.path.exists(path):
            pytest.fail(f"{path} missing: __graft_entry__.build() builds it")
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
    e.close()
    return st


@pytest.fixture(scope="module")
def small():
    return gen.config2(600, 1500)


@pytest.mark.parametrize("pct", [100, 0])
def test_direct_mode_several_batches(small, pct):
    cluster, pods = small
    st = _check(cluster, pods, _prof(pct), f"pct {pct}")
    assert st.batches > 1500 // 256


def test_hash_mode():
    """8,300 nodes: past kChainDirect, the holders are hashed."""
    cluster, pods = gen.config2(8300, 600)
    st = _check(cluster, pods, _prof(), "hash")
    assert st.batches >= 3


@pytest.mark.parametrize("variant", FLAVORS)
def test_contention_long_chains_and_exhausted_lists(variant):
    """48 identical nodes (8 cores, 32 Gi, 110 pods) under 700 identical pods
    (100m, 256 Mi): within a batch every pod's list names the same nodes in the
    same order, so pod i's guess depends on all the pods before it (a chain as
    long as the list), and the pods past the list's length run out of entries
    with an incomplete list, which truncates the batch.  At this node size the
    cluster holds all 700 pods (80 per node by cpu), and the run before the
    round tags took 30 batches with 21 truncations (and 8 pair cuts)."""
    cluster = gen.bare_cluster(48, 7)
    cluster.alloc_cpu[:] = 8000
    cluster.alloc_mem[:] = 32 * GI
    pods = gen.bare_pods(700, 7, 1, 1)
    st = _check(cluster, pods, _prof(), "contention", variant)
    print("contention: batches", st.batches, "truncations", st.truncations)
    assert st.truncations > 0
    assert st.batches > 3
    assert st.scheduled == 700


@pytest.mark.parametrize("variant", FLAVORS)
@pytest.mark.parametrize("n", [1, 256, 257])
def test_queue_lengths(small, n, variant):
    """nb = 1, one full batch, and a full batch with a tail batch of one pod."""
    cluster, pods = small
    _check(cluster, pods.subset(0, n), _prof(), f"queue {n}", variant)
