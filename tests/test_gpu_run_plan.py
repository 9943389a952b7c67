"""The form of a run is decided once (csrc/ksim_engine.cpp plan_run) and a
handle's graphs live in one keyed cache (handle_graph, drop_graphs_if).

One scene per launch form: per-pod cycles (plain, with topology uses, with
topology uses read from persistent tables), three-launch batches (generic,
static-class, ADAPT), deferred-commit batches (without and with the
request-class table, ADAPT), topology batches, and one queue that holds three
forms in sequence.  Per scene:

  * ksim_time_kernels runs what ksim_schedule_loaded runs: the same node
    columns and next_start (both equal to the oracle's, whose placements
    schedule_loaded's are compared with; the C ABI has no call that reads the
    placements back after time_kernels), and the kernels it reports are the
    form's, as a literal set;
  * the cache contract: the first run captures its graphs, the same run again
    none; a weight-only profile change drops the per-pod graphs alone, a
    percentageOfNodesToScore change all of them.

Every expected kernel set and capture count below was printed by this file on
the library of the commit before plan_run and the cache existed
(profiles/run_plan/kernels_parent.txt, capture_counts.txt); this file passes on
that library too.  Queues are as short as the graph replays allow: 129 pods
(128 cycles and one), 16 batches and one pod, 17 topology batches and one pod;
the deferred-commit pair is captured at any length.  ADAPT needs K < N, so more
than 100 nodes: those scenes take runfeedcases' 300-node cluster."""
import functools

import numpy as np
import pytest

from ksim import profile
from ksim.encode import encode_cluster, encode_pods
from ksim.engine import lib
from oracle.oracle import Oracle

import fastcases
import runfeedcases as rf
import tbatchcases as tbc

pytestmark = pytest.mark.gpu

B = rf.B
CYCLES = 129                                        # kGraphCycles + 1
BATCHES = 16 * B + 1                                # kGraphBatches batches and one pod
TB_PODS = 17 * tbc.K_TB_PODS + 1                    # 17 full topology batches and one pod


def _bare(n_pods, cpu_steps=2, mem_steps=2, tag=0):
    """runfeedcases.queue, as a copy the scene may edit."""
    q = rf.queue(n_pods, cpu_steps, mem_steps, tag)
    return type(q)(q.pods.copy(), q.exprs, q.terms, q.names)


def _wide_alloc(cluster):
    """One allocatable past the FAST keys' range: generic keys for every run."""
    cluster.alloc_mem[0] = fastcases.NARROW
    return cluster


def _spread(nodes, n_pods, nb_add=False):
    cluster, _ = encode_cluster(nodes, [])
    pods = encode_pods(cluster, tbc.many_apps(n_pods))
    if nb_add:                                      # a bandwidth input keeps the pod off the topology batches
        pods.pods["nb_add"][:] = 1
    return cluster, pods


def _perpod_plain():
    pods = _bare(CYCLES)
    pods.pods["nb_add"][:] = 1
    return rf.narrow_cluster(24), pods, 100


def _perpod_topo():
    """One node without the zone label: the DoNotSchedule key is not on every
    node, so no pod reads its domain sums from a persistent table."""
    return _spread(tbc.zoned(47) + [tbc.node("n-nozone", None)], CYCLES) + (100,)


def _perpod_ptab():
    return _spread(tbc.zoned(48), CYCLES, nb_add=True) + (100,)


def _batch_generic():
    return _wide_alloc(rf.narrow_cluster(24)), _bare(BATCHES), 100


def _lazy_plain():
    """160 request classes, 300 pods: below 8 pods per class, no table."""
    return rf.narrow_cluster(24), _bare(300, 10, 16, tag=1), 100


def _lazy_table():
    return rf.narrow_cluster(24), _bare(300), 100


def _batch_stab():
    return rf.narrow_cluster(24), fastcases.with_zone_selector(_bare(BATCHES)), 100


def _adapt_generic():
    return _wide_alloc(rf.narrow_cluster(300, 110)), _bare(BATCHES, tag=3), 0


def _lazy_adapt():
    return rf.narrow_cluster(300, 110), _bare(300, tag=3), 0


def _tbatch():
    return _spread(tbc.zoned(48, cpu="64", mem="256Gi"), TB_PODS) + (100,)


MIXED = (300, 305, 900)                             # static-class batches | per-pod cycles | deferred-commit batches


def _mixed():
    pods = fastcases.with_zone_selector(_bare(MIXED[2]))
    pods.pods["sel_count"][MIXED[0]:] = 0
    pods.pods["nb_add"][MIXED[0]:MIXED[1]] = 1
    return rf.narrow_cluster(32), pods, 100


SCENES = {f.__name__[1:]: f for f in (_perpod_plain, _perpod_topo, _perpod_ptab, _batch_generic, _lazy_plain, _lazy_table,
                                      _batch_stab, _adapt_generic, _lazy_adapt, _tbatch, _mixed)}

CYCLE = {"k_filter_score", "k_select"}                # the no-window cycle: k_select binds as well, no k_bind launch
LAZY = {"k_batch_top_commit", "k_batch_chain_pairs"}
THREE = {"k_batch_top", "k_batch_chain_pairs", "k_batch_commit"}
# scene: (kernels time_kernels reports, captures of the first run, captures after a weight-only profile change)
EXPECT = {
    "perpod_plain": (CYCLE, 1, 1),
    "perpod_topo": (CYCLE | {"k_topo_prefilter"}, 1, 1),
    "perpod_ptab": (CYCLE, 1, 1),
    "batch_generic": (THREE, 1, 0),
    "lazy_plain": (LAZY, 2, 0),
    "lazy_table": (LAZY, 2, 0),
    "batch_stab": (THREE, 1, 0),
    "adapt_generic": ({"k_adapt_mask", "k_adapt_window", "k_adapt_top", "k_adapt_pairs", "k_adapt_commit"}, 1, 0),
    "lazy_adapt": ({"k_adapt_mask_commit", "k_adapt_top", "k_adapt_pairs"}, 2, 0),
    "tbatch": ({"k_tb_filter", "k_tb_select", "k_tb_merge", "k_tb_chain_pairs", "k_tb_commit"}, 1, 0),
    "mixed": (THREE | CYCLE | LAZY, 4, 1),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def compiled(pct, kind="base"):
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=pct)
    if kind == "weights":
        sp = sp.with_weights({"NodeResourcesFit": 2, "NodeResourcesBalancedAllocation": 1})
    return profile.compile_profile(sp)


def other_pct(pct):
    """Another percentageOfNodesToScore that keeps the scene's form: 99 keeps
    every node of a cluster below 100 nodes, 60 of 300 nodes is still ADAPT."""
    return 99 if pct == 100 else 60


@functools.lru_cache(maxsize=None)
def truth(name, pct=None, kind="base"):
    """The oracle's run of the whole queue, computed once per profile."""
    cluster, pods, pct0 = scene(name)
    ora = Oracle(cluster.copy_state(), compiled(pct0 if pct is None else pct, kind))
    chosen, st = ora.schedule(pods, 0, pods.n_pods, nthreads=16)
    chosen.setflags(write=False)
    return chosen, (st.evals, st.scheduled, st.unschedulable), ora.next_start, ora.node_state()


def _engine(name):
    cluster, pods, pct = scene(name)
    return rf.engine(cluster, pods, compiled(pct)), pods


def _captures(e):
    return e.diag()["graph_captures"]


def _same_state(e, want, tag):
    _, _, next_start, state = want
    assert e.next_start == next_start, tag
    got = e.node_state()
    for k in got:
        np.testing.assert_array_equal(got[k], state[k], err_msg=f"{tag} {k}")


def _run(e, pods, want, tag, first=0, count=None):
    """reset, schedule_loaded, compare with the oracle; the graphs captured."""
    e.reset_cluster()
    c0 = _captures(e)
    count = pods.n_pods - first if count is None else count
    chosen, st = e.schedule_loaded(first, count)
    if want is not None:
        np.testing.assert_array_equal(chosen, want[0], err_msg=tag)
        assert (st.evals, st.scheduled, st.unschedulable) == want[1], tag
        _same_state(e, want, tag)
    return _captures(e) - c0


@pytest.mark.parametrize("name", list(SCENES))
def test_timer_runs_the_form(name):
    e, pods = _engine(name)
    want = truth(name)
    _run(e, pods, want, f"{name}: schedule_loaded")
    e.reset_cluster()
    ran = e.time_kernels(0, pods.n_pods)
    print(f"kernels {name}: {sorted(ran)}")
    _same_state(e, want, f"{name}: time_kernels")
    assert set(ran) == EXPECT[name][0], (name, sorted(ran))
    e.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_capture_contract(name):
    cluster, pods, pct = scene(name)
    e, _ = _engine(name)
    first = _run(e, pods, truth(name), f"{name}: first")
    again = _run(e, pods, truth(name), f"{name}: again")
    e.set_profile(compiled(pct, "weights"))         # score weights alone: the batch paths read them from the device
    e.load_pods(pods)
    weights = _run(e, pods, truth(name, kind="weights"), f"{name}: weights")
    e.set_profile(compiled(other_pct(pct), "weights"))
    e.load_pods(pods)
    moved = _run(e, pods, truth(name, other_pct(pct), "weights"), f"{name}: percentage")
    print(f"captures {name}: first {first} again {again} weights {weights} percentage {moved}")
    assert first > 0 and (first, again, weights, moved) == (EXPECT[name][1], 0, EXPECT[name][2], first), name
    e.close()


def test_one_cut_recaptures_the_deferred_commit_pair(monkeypatch):
    """KSIM_ONE_CUT is an argument of the deferred-commit launches alone: the
    mixed queue's static-class and per-pod graphs stay."""
    e, pods = _engine("mixed")
    want = truth("mixed")
    first = _run(e, pods, want, "mixed")
    monkeypatch.setenv("KSIM_ONE_CUT", "1")
    cut = _run(e, pods, want, "mixed, one cut")
    same = _run(e, pods, want, "mixed, one cut again")
    monkeypatch.delenv("KSIM_ONE_CUT")
    back = _run(e, pods, want, "mixed, back")
    print(f"captures one_cut: first {first} toggled {cut} again {same} back {back}")
    assert (first, cut, same, back) == (4, 2, 0, 2)
    e.close()


def test_other_class_count_recaptures_the_table_pair():
    """A queue of the same size (its buffers are reused, so the reload drops
    nothing) with 2 request classes where the first had 4: the table's graphs
    hold the class count; the plain pair, which a 1-pod run takes, stays."""
    cluster, pods, pct = scene("lazy_table")
    other = _bare(pods.n_pods, 2, 1, tag=5)
    e, _ = _engine("lazy_table")
    counts = [_run(e, pods, None, "plain", 0, 1), _run(e, pods, truth("lazy_table"), "table")]
    r0 = e.diag()["reqtab_runs"]
    e.load_pods(other)
    ora = Oracle(cluster.copy_state(), compiled(pct))
    want = ora.schedule(other, 0, other.n_pods, nthreads=16)
    counts.append(_run(e, other, None, "plain, reloaded", 0, 1))
    e.reset_cluster()
    c0 = _captures(e)
    rf.same_run(e.schedule_loaded(0, other.n_pods), want, "table, reloaded")
    rf.same_state(e, ora, "table, reloaded")
    counts.append(_captures(e) - c0)
    print(f"captures class count: {counts}")
    assert counts == [2, 2, 0, 2] and e.diag()["reqtab_runs"] == r0 + 1
    e.close()


def test_two_kinds_capture_once_each():
    """The single-handle twin of test_group_two_kinds: the mixed queue's
    static-class stretch and its deferred-commit stretch, run in turn, capture
    their graphs once and keep them."""
    e, pods = _engine("mixed")
    stab, lazy = (0, MIXED[0]), (MIXED[1], MIXED[2] - MIXED[1])
    counts = [_run(e, pods, None, "kinds", *r) for r in (stab, lazy, stab, lazy)]
    print(f"captures two kinds: {counts}")
    assert counts == [1, 2, 0, 0]
    e.close()


SLOTS = ["k_topo_prefilter", "k_topo_min", "k_filter_score", "k_window", "k_extrema", "k_select", "k_bind",
         "k_batch_top", "k_batch_chain_pairs", "k_batch_commit",
         "k_adapt_mask", "k_adapt_window", "k_adapt_top", "k_adapt_pairs", "k_adapt_commit",
         "k_tb_filter", "k_tb_select", "k_tb_merge", "k_tb_chain_pairs", "k_tb_commit",
         "k_batch_top_commit", "k_batch_chain_pairs",
         "k_adapt_mask_commit", "k_adapt_cut0", "k_adapt_top", "k_adapt_pairs"]


def test_kernel_slots():
    L = lib()
    assert [L.ksim_kernel_name(k).decode() for k in range(26)] == SLOTS
    assert L.ksim_kernel_name(26) is None and L.ksim_kernel_name(-1) is None
    e, _ = _engine("lazy_plain")
    name, ms = e.time_eval(0, reps=3)
    assert name == "k_batch_top_commit" and ms > 0, (name, ms)
    e.close()
