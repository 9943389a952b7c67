"""The per-pod cycle (csrc/ksim_kernels.hip: k_filter_score, k_window,
k_extrema, k_select / bind_cycle, k_fw_normalize, the sharded k_wcount_sh ..
k_bind_sh) on the designed scenes of tests/cyclecases.py, bit for bit against
the C oracle, from a start and a pod sequence the test sets itself.
tests/test_cycle_cases.py proves on the CPU that tests/cycleref.py's plain
model equals that oracle on every scene, that the scenes tell twenty-four
wrong readings of the cycle from the right one and that each scene has the
property its name claims.

Every scene runs through every form it applies to:

  COMPAT (form 4)   Engine.eval_pod per pod, eval_pod_extenders where the scene
                    has extenders: every key of the result.  Windowed where
                    K < N, the no-window COMPAT cycle (k_extrema<true>) else.
  schedule_loaded   placements, stats, next_start, node state, class counts;
                    every pod a per-pod cycle, no batch.  Forms 1 to 3 by the
                    scene (cyclecases.cycle_form), form 6 for captured_run.
  time_kernels      the per-handle signal of the form: k_window and k_extrema
                    ran (form 1), k_extrema alone (form 2), neither (form 3).
  the "ab" flavor   the windowed cycle for plain pods (no use at all).
  node shards       form 5, group_schedule_loaded on every listed world, the
                    start and the pod sequence set on every member.
  fw_*              lists that leave out the maximum holder; fw_normalize of
                    every slot kind over lists of 1 to 2,049 entries against
                    cycleref.normalize and the oracle."""
import functools

import numpy as np
import pytest

from ksim.engine import Engine, KsimError, group_schedule_loaded
from ksim.shard import partition
from oracle.oracle import Oracle

import cyclecases
import cycleref

pytestmark = pytest.mark.gpu

KEYS = ("chosen", "status", "n_feasible", "n_evaluated", "n_processed", "k_to_find", "next_start")
ARRAYS = ("fail_plugin", "fail_detail", "scored", "raw", "norm", "total")
SCHEDULED = [n for n in cyclecases.ALL if cyclecases.scene(n).schedule]


def _engine(s, cluster=None, variant=None):
    e = Engine(0, variant=variant)
    e.set_profile(s.prof)
    e.set_cluster(cluster if cluster is not None else s.encoded[0].copy_state())
    e.set_next_start(s.s0)
    e.set_pod_seq(s.seq0)
    assert e.next_start == s.s0
    return e


def _oracle(s):
    ora = Oracle(s.encoded[0].copy_state(), s.prof)
    ora.set_next_start(s.s0)
    ora.set_pod_seq(s.seq0)
    return ora


def _run_oracle(s):
    ora = _oracle(s)
    chosen, st = ora.schedule(s.encoded[1], nthreads=16)
    chosen.setflags(write=False)
    return chosen, (st.evals, st.scheduled, st.unschedulable), ora.next_start, ora.node_state(), ora.class_count()


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """Oracle.schedule of a scene, computed once and shared."""
    return _run_oracle(cyclecases.scene(name))


def _check_run(tag, chosen, st, next_starts, states, classes, want):
    ochosen, ost, onext, ostate, oclasses = want
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled, st.unschedulable) == ost, tag
    assert all(x == onext for x in next_starts), (tag, next_starts, onext)
    for k, v in ostate.items():
        np.testing.assert_array_equal(np.concatenate([p[k] for p in states]), v, err_msg=f"{tag} {k}")
    np.testing.assert_array_equal(np.concatenate(classes, axis=1), oclasses, err_msg=f"{tag} class counts")


@pytest.mark.parametrize("name", cyclecases.ALL)
def test_compat_cycles(name):
    s = cyclecases.scene(name)
    _, pods = s.encoded
    e, ora = _engine(s), _oracle(s)
    ef, es = s.extender()
    for j in range(pods.n_pods):
        o = ora.cycle(pods, j, ef, es)
        g = e.eval_pod_extenders(pods, j, lambda _f: (ef, es)) if s.ext else e.eval_pod(pods, j)
        for k in KEYS:
            assert g[k] == o[k], (name, j, k, g[k], o[k])
        for k in ARRAYS:
            np.testing.assert_array_equal(g[k], o[k], err_msg=f"{name} pod {j} {k}")
    assert e.next_start == ora.next_start
    for k, v in ora.node_state().items():
        np.testing.assert_array_equal(e.node_state()[k], v, err_msg=f"{name} {k}")
    e.close()


@pytest.mark.parametrize("name", SCHEDULED)
def test_schedule_loaded(name):
    s = cyclecases.scene(name)
    _, pods = s.encoded
    e = _engine(s)
    chosen, st = e.schedule_batch(pods)
    print(name, s.form, "perpod", st.perpod_cycles, "batches", st.batches, "evals", st.evals, "next", e.next_start)
    _check_run(name, chosen, st, [e.next_start], [e.node_state()], [e.class_count()], _oracle_run(name))
    assert st.perpod_cycles == pods.n_pods and st.batches == 0, name
    if pods.n_pods >= cyclecases.GRAPH_CYCLES:
        assert e.diag()["graph_captures"] >= 1, name
    e.close()


@pytest.mark.parametrize("name", SCHEDULED)
def test_form_by_kernels(name):
    """Engine.time_kernels over the same queue on a fresh engine: which
    kernels ran tells the form; the run itself is compared as well."""
    s = cyclecases.scene(name)
    _, pods = s.encoded
    e = _engine(s)
    e.load_pods(pods)
    ran = e.time_kernels(0, pods.n_pods)
    window, extrema = cyclecases.FORM_KERNELS[s.form]
    print(name, s.form, sorted(ran))
    assert ("k_window" in ran) == window and ("k_extrema" in ran) == extrema, (name, s.form, sorted(ran))
    assert "k_filter_score" in ran and "k_select" in ran, (name, ran)
    _, _, onext, ostate, _ = _oracle_run(name)
    assert e.next_start == onext, name
    for k, v in ostate.items():
        np.testing.assert_array_equal(e.node_state()[k], v, err_msg=f"{name} {k}")
    e.close()


@pytest.mark.parametrize("name", cyclecases.AB)
def test_ab_flavor(name):
    """Plain pods (no use) whose normalized scores vary: the "ab" flavor sends
    them to the windowed cycle without the topology kernels."""
    s = cyclecases.without_ports(cyclecases.scene(name))
    _, pods = s.encoded
    assert s.form == "windowed"
    e = _engine(s, variant="ab")
    chosen, st = e.schedule_batch(pods)
    _check_run(name, chosen, st, [e.next_start], [e.node_state()], [e.class_count()], _run_oracle(s))
    assert st.perpod_cycles == pods.n_pods and st.batches == 0, name
    e.close()


@pytest.mark.parametrize("name,world", cyclecases.sharded())
def test_sharded(name, world):
    s = cyclecases.scene(name)
    cluster, pods = s.encoded
    tag = f"{name} {world} shards"
    engines = []
    for base, cnt in partition(s.n, world):
        e = Engine(0)
        e.set_shard(base, s.n)
        e.set_profile(s.prof)
        e.set_cluster(cluster.copy_state().shard(base, cnt))
        e.set_next_start(s.s0)                        # a global position, on every member
        e.set_pod_seq(s.seq0)
        e.load_pods(pods)
        engines.append(e)
    chosen, st = group_schedule_loaded(engines, 0, pods.n_pods)
    print(tag, "perpod", st.perpod_cycles, "batches", st.batches, "evals", st.evals)
    _check_run(tag, chosen, st, [e.next_start for e in engines], [e.node_state() for e in engines],
               [e.class_count() for e in engines], _oracle_run(name))
    assert st.perpod_cycles == pods.n_pods and st.batches == 0, tag
    for e in engines:
        e.close()


def test_sharded_handle_refuses_lists():
    s = cyclecases.scene("list_3_of_300")
    cluster, pods = s.encoded
    e = Engine(0)
    e.set_shard(0, s.n)
    e.set_profile(s.prof)
    e.set_cluster(cluster.copy_state().shard(0, 192))
    with pytest.raises(KsimError, match="unsharded"):
        e.load_pods(pods)
    e.close()


@pytest.mark.parametrize("name", ["cut_holds_best", "ipa_mixed_signs", "pts_rack_small", "pts_two_constraints"])
def test_fw_lists_without_the_maximum_holder(name):
    """fw_prefilter / fw_score over the feasible nodes but the holder of each
    normalized slot's maximum: the maxima come from the list alone."""
    s = cyclecases.scene(name)
    _, pods = s.encoded
    e, ora = _engine(s), _oracle(s)
    fe, fo = e.fw_prefilter(pods, 0), ora.fw_prefilter(pods, 0)
    np.testing.assert_array_equal(fe["fail_plugin"], fo["fail_plugin"])
    feasible = np.nonzero(fo["fail_plugin"] == cycleref.PASSED)[0]
    whole = _oracle(s)
    whole.fw_prefilter(pods, 0)
    full = whole.fw_score(feasible)
    holders = set()                                   # every holder of a normalized slot's maximum
    for x in (cyclecases.NA, cyclecases.TT, cyclecases.IPA, cyclecases.SPREAD):
        raw = full["raw"][x][feasible]
        if raw.max() > raw.min():
            holders |= {int(n) for n in feasible[raw == raw.max()]}
    assert holders and len(holders) < feasible.size // 2, name
    lst = np.array([n for n in feasible if int(n) not in holders], np.int32)[::-1]
    ge, go = e.fw_score(lst), ora.fw_score(lst)
    for k in ("scored", "raw", "norm", "total"):
        np.testing.assert_array_equal(ge[k], go[k], err_msg=f"{name} {k}")
    assert any((go["norm"][x][lst] != full["norm"][x][lst]).any() for x in range(len(cyclecases.KINDS))), name
    e.close()


FW_SIZES = (1, 1023, 1024, 1025, 2049)


def _fw_values(n, kind):
    """Scores whose extremum sits in the last entry (both ends for min-max)."""
    v = (np.arange(n, dtype=np.int64) * 37) % 91 + 5
    v[-1] = 400
    if kind == cycleref.MINMAX and n > 1:
        v[0] = -250
    return v


@pytest.mark.parametrize("name,sizes", [("chunk_2049_at2046_s0", FW_SIZES), ("ipa_mixed_signs", (1, 59, 60)),
                                        ("pts_rack_small", (1, 64, 101)), ("pts_all_ignored", (1, 60))])
def test_fw_normalize_lists(name, sizes):
    """k_fw_normalize (one block) over explicit lists, every slot kind, after
    an fw_score that set the PreScore facts: against cycleref.normalize with
    the model's IgnoredNodes and topologyScore flag, and against the oracle."""
    s = cyclecases.scene(name)
    _, pods = s.encoded
    run, inputs = cyclecases.truth(name)
    inp = inputs[0]
    e, ora = _engine(s), _oracle(s)
    feasible = np.nonzero(inp.feasible)[0].astype(np.int32)
    for x in (e, ora):
        x.fw_prefilter(pods, 0)
        x.fw_score(feasible)
    ignored = {n for n in feasible if inp.soft and not inp.system_default and
               any(int(u.value[n]) == 0 for u in inp.soft)}
    for n in sizes:
        nodes = np.arange(n, dtype=np.int32) if n > feasible.size else feasible[:n]
        for slot, kind in enumerate(cyclecases.KINDS):
            vals = _fw_values(n, kind)
            ign = [kind == cycleref.PTS and int(x) in ignored for x in nodes]
            want = cycleref.normalize(kind, [int(v) for v in vals], ign, [int(v) for v in vals], ign,
                                      inp.topology_score_nonempty, None)
            got = e.fw_normalize(slot, nodes, vals)
            np.testing.assert_array_equal(got, np.array(want, np.int64), err_msg=f"{name} n={n} slot {slot} {kind}")
            np.testing.assert_array_equal(got, ora.fw_normalize(slot, nodes, vals), err_msg=f"{name} n={n} {slot}")
    assert e.diag()["fw_normalize_device"] > 0
    e.close()
