"""What makes tests/test_gpu_cycle_edges.py mean something, checked on the CPU:

  - tests/cycleref.py's cycle equals the C oracle's in every key of its
    result (chosen, status, n_feasible, n_evaluated, n_processed, k_to_find,
    next_start, fail_plugin with its NOT_EVALUATED marks, scored, raw, norm,
    total) for every pod of every scene of tests/cyclecases.py, extenders
    included, and its sequential scheduler equals Oracle.schedule in
    placements, stats, next_start, node state and class counts;
  - every scene has the property its name claims and takes the launch form
    it is built for;
  - every wrong reading of cycleref.FAULTS changes an observable of at least
    one scene (the test prints the table);
  - cycleref.shard_view agrees with oracle/shard_model.py's window where the
    two overlap: the kept nodes of a shard, the run counts, the shares of the
    evaluations summing to the global count."""
import functools

import numpy as np
import pytest

from ksim.shard import partition
from oracle import shard_model
from oracle.oracle import Oracle

import cyclecases
import cycleref

OBSERVED = ("chosen", "status", "n_feasible", "n_evaluated", "n_processed", "next_start", "scored", "norm", "total")


def _oracle(s):
    cluster, _ = s.encoded
    ora = Oracle(cluster.copy_state(), s.prof)
    ora.set_next_start(s.s0)
    ora.set_pod_seq(s.seq0)
    return ora


@pytest.mark.parametrize("name", cyclecases.ALL)
def test_model_equals_oracle_cycle(name):
    s = cyclecases.scene(name)
    _, pods = s.encoded
    run, _ = cyclecases.truth(name)
    ora = _oracle(s)
    ef, es = s.extender()
    for j, r in enumerate(run.cycles):
        o = ora.cycle(pods, j, ef, es)
        for k in cycleref.RESULT_KEYS:
            assert o[k] == r[k], (name, j, k, o[k], r[k])
        for k in cycleref.ARRAY_KEYS:
            np.testing.assert_array_equal(o[k], r[k], err_msg=f"{name} pod {j} {k}")
    np.testing.assert_array_equal(ora.class_count(), run.class_count, err_msg=name)
    for k, v in ora.node_state().items():
        np.testing.assert_array_equal(v, run.state[k], err_msg=f"{name} {k}")


@pytest.mark.parametrize("name", [n for n in cyclecases.ALL if cyclecases.scene(n).schedule])
def test_schedule_equals_oracle_schedule(name):
    s = cyclecases.scene(name)
    _, pods = s.encoded
    run, _ = cyclecases.truth(name)
    ora = _oracle(s)
    chosen, st = ora.schedule(pods, nthreads=4)
    np.testing.assert_array_equal(chosen, run.chosen, err_msg=name)
    assert (st.evals, st.scheduled, st.unschedulable) == (run.evals, run.scheduled, run.unschedulable), name
    assert ora.next_start == run.next_start, name
    for k, v in ora.node_state().items():
        np.testing.assert_array_equal(v, run.state[k], err_msg=f"{name} {k}")
    np.testing.assert_array_equal(ora.class_count(), run.class_count, err_msg=name)


@pytest.mark.parametrize("name", cyclecases.ALL)
def test_scene_has_its_property_and_form(name):
    s = cyclecases.scene(name)
    run, _ = cyclecases.truth(name)
    assert s.claim(s, run.cycles), name
    assert 0 <= s.s0 and s.restated_form() == s.form, (name, s.restated_form())
    assert s.route == "port" and all(p.containers[0].ports for p in s.queue)
    compat = s.restated_form(compat=True)
    assert compat == ("windowed" if s.form == "windowed" else "nowin_unfused")


def test_every_form_has_scenes():
    forms = {}
    for name in cyclecases.ALL:
        s = cyclecases.scene(name)
        forms.setdefault(s.form, []).append(name)
        if len(s.queue) >= cyclecases.GRAPH_CYCLES:
            forms.setdefault("captured", []).append(name)
    forms["sharded"] = cyclecases.sharded()
    forms["compat"] = cyclecases.ALL
    for f in ("windowed", "nowin_unfused", "nowin_fused", "compat", "sharded", "captured"):
        print(f, len(forms.get(f, [])))
        assert forms.get(f), f
    # k_window's chunk grows from 1 to 2 at 1,025 scanned nodes, to 3 at 2,049
    assert {n for n, _, _ in cyclecases.CHUNKS} == {1024, 1025, 2049}
    assert -(-1024 // cyclecases.WINDOW_THREADS) == 1 and -(-1025 // cyclecases.WINDOW_THREADS) == 2
    assert {cyclecases.scene(f"threshold_{n}_pct{p}").form for n, p in cyclecases.THRESHOLDS[:2]} == {"nowin_fused"}
    assert cyclecases.scene("threshold_101_pct0").form == "windowed"
    assert cyclecases.scene("blocks65_pct0").n > 64 * 256


def test_float64_cases():
    """100 * (x / d) in float64 truncates below the integer quotient."""
    for x, d, go, integer in ((29, 50, 57, 58), (29, 100, 28, 29), (57, 100, 56, 57), (58, 100, 57, 58)):
        assert cycleref.normalize(cycleref.MINMAX, [0, x, d], [False] * 3, [0, x, d], [False] * 3, True, None)[1] == go
        assert cycleref.normalize(cycleref.MINMAX, [0, x, d], [False] * 3, [0, x, d], [False] * 3, True,
                                  "minmax_integer_division")[1] == integer


@functools.lru_cache(maxsize=None)
def _outcome(name, fault):
    if fault is None:
        return cyclecases.truth(name)[0]
    return cyclecases.reference(cyclecases.scene(name), fault)


def _differs(a, b) -> str:
    what = []
    for k in OBSERVED:
        n = sum(1 for x, y in zip(a.cycles, b.cycles) if not np.array_equal(x[k], y[k]))
        if n:
            what.append(k)
    return ", ".join(what)


# the large scenes tell nothing apart that a small one does not; leaving them out keeps this test quick
FAULT_SCENES = [n for n in cyclecases.ALL if cyclecases.scene(n).n <= 600 and n != "captured_run"]


def test_every_wrong_reading_is_caught():
    caught = {}
    for number, fault in enumerate(cycleref.FAULTS, 1):
        hits = []
        for name in FAULT_SCENES:
            d = _differs(_outcome(name, fault), _outcome(name, None))
            if d:
                hits.append(f"{name} ({d})")
        caught[fault] = hits
        more = f"; and {len(hits) - 4} more" if len(hits) > 4 else ""
        print(f"{number:2d} {fault:30s} {len(hits):2d} scenes: {'; '.join(hits[:4]) + more if hits else 'NOT CAUGHT'}")
    missed = [f for f, h in caught.items() if not h]
    assert not missed, f"no scene tells these readings from the reference: {missed}"
    # the scenes built for a reading do catch it
    for fault, name in (("k_plus_1_is_no_cut", "exactly_k_plus_1_s0"), ("cut_node_in_extrema", "cut_holds_best"),
                        ("extrema_over_all_feasible", "max_past_cut"), ("list_k_from_cluster", "list_150_of_300"),
                        ("list_start_mod_cluster", "list_3_of_300"), ("short_pod_advances_by_kept", "exactly_k"),
                        ("minmax_integer_division", "ipa_float64"), ("minmax_zero_diff_100", "ipa_all_equal"),
                        ("reverse_zero_max_0", "default_zero_max"), ("ignored_gets_100", "pts_hostname_fused"),
                        ("size_counts_past_cut", "pts_rack_wide"), ("dropped_in_extrema", "ext_drops_max_holder"),
                        ("single_node_scored", "one_feasible"), ("ties_to_lowest_index", "two_equal"),
                        ("pts_size_ignores_empty_value", "pts_system_default")):
        assert any(h.startswith(name + " ") for h in caught[fault]), (fault, name, caught[fault])


@pytest.mark.parametrize("name,world", cyclecases.sharded())
def test_shard_view(name, world):
    s = cyclecases.scene(name)
    run, inputs = cyclecases.truth(name)
    parts = partition(s.n, world)
    start = s.s0
    for j, (r, inp) in enumerate(zip(run.cycles, inputs)):
        views = [cycleref.shard_view(r, inp, start, parts, rk) for rk in range(world)]
        assert sum(v["evals"] for v in views) == r["n_evaluated"], (name, j)
        assert sorted(n for v in views for n in v["kept"]) == sorted(r["kept"])
        assert sum(v["owns_cut"] for v in views) == (r["cut"] >= 0)
        counts = np.array([[v["hi"], v["lo"]] for v in views])
        cutslots = []
        for rk, (base, cnt) in enumerate(parts):
            ok = np.asarray(inp.feasible[base:base + cnt])
            kend, cutslot = shard_model.window(counts, rk, s.n, s.k, base, cnt, start, ok)
            pos = (base + np.arange(cnt) - start) % s.n
            assert sorted(base + np.nonzero(ok & (pos < kend))[0]) == sorted(views[rk]["kept"]), (name, j, rk)
            assert (cutslot > 0) == views[rk]["owns_cut"], (name, j, rk)
            cutslots.append(cutslot)
        cutslot = max(cutslots)
        assert (cutslot if cutslot else s.n) == r["n_evaluated"]
        assert (start + (cutslot - 1 if cutslot else s.n)) % s.n == r["next_start"]
        assert all(v["next_start"] == r["next_start"] for v in views)
        start = r["next_start"]
