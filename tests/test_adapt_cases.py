"""What makes tests/test_gpu_adapt_edges.py mean something, checked on the CPU:

  - tests/adaptref.py's windows equal the windows of tests/fastref.py's
    schedule (adaptref.reference reads them off its cycles), of adaptref's own
    windowed schedule (the small rings, where the wrong readings are tried)
    and of the C oracle's cycles (n_processed, next_start, k_to_find) on
    every bare-pod scene of tests/adaptcases.py;
  - fastref.schedule equals Oracle.schedule on every bare-pod scene in both
    cluster shapes: placements, evals, next_start and node state;
  - every wrong reading of adaptref.FAULTS changes the placements, evals or
    next_start of at least one scene (the test prints which), and a flip past
    the cut changes nothing under the readings that speak of flips;
  - every scene has the property its name claims;
  - the restated choice of window form gives the form every scene is meant for.

The static-class scenes (list_*) are exempt from the Python restatement of the
placements: fastref restates trivial pods only.  Their windows are still
pinned: the bitmaps follow from the construction (roomy nodes of the selected
zone), and adaptref.windows over them gives the oracle's evals and next_start
(list_normv, whose bitmaps depend on taints and pools, is checked for its
claims alone and runs against the oracle on the GPU)."""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle

import adaptcases
import adaptref


@functools.lru_cache(maxsize=None)
def _reference(name, shape="fast"):
    s = adaptcases.scene(name)
    chosen, cols, nxt, evals, rows = adaptref.reference(s.shaped(shape), s.pods, adaptcases.compiled(s.pct),
                                                        next_start=s.s0)
    chosen.setflags(write=False)
    return chosen, cols, nxt, evals, rows


CYCLES_LARGE = 48                                    # pods walked cycle by cycle on the scenes of 16,384 nodes and more


@pytest.mark.parametrize("name", adaptcases.BARE)
def test_windows_equal_the_schedules_and_the_oracle_cycles(name):
    s = adaptcases.scene(name)
    prof = adaptcases.compiled(s.pct)
    chosen, cols, nxt, evals, rows = _reference(name)
    wins, last = s.windows()
    if not s.flips:                                  # no bit flips: the S0 bitmaps hold for the whole queue
        assert rows == wins, name
        assert last == nxt
        assert evals == sum(cut + 1 if cut >= 0 else s.n for _, cut in wins)
    if s.n < 1000:                                   # the windowed schedule the wrong readings are switched on in
        achosen, acols, anext, aevals, arows = adaptref.schedule(s.cluster, s.pods, prof, next_start=s.s0, trace=True)
        np.testing.assert_array_equal(achosen, chosen, err_msg=name)
        assert (anext, aevals, [r[:2] for r in arows]) == (nxt, evals, rows), name
        for k, v in cols.items():
            np.testing.assert_array_equal(acols[k], v, err_msg=f"{name} {k}")
    ora = Oracle(s.shaped("fast"), prof)
    ora.set_next_start(s.s0)
    walked = rows if s.n < 16384 else rows[:CYCLES_LARGE]   # (Oracle.schedule pins the whole queue below)
    for j, (start, cut) in enumerate(walked):
        o = ora.cycle(s.pods, j)
        tag = f"{name} pod {j}"
        assert o["k_to_find"] == s.k, tag
        assert o["n_processed"] == (cut if cut >= 0 else s.n), tag
        assert o["next_start"] == (rows[j + 1][0] if j + 1 < len(rows) else nxt), tag
        assert o["chosen"] == chosen[j], tag


@pytest.mark.parametrize("shape", ["fast", "generic"])
@pytest.mark.parametrize("name", adaptcases.BARE)
def test_reference_equals_oracle(name, shape):
    s = adaptcases.scene(name)
    chosen, cols, nxt, evals, _ = _reference(name, shape)
    ora = Oracle(s.shaped(shape), adaptcases.compiled(s.pct))
    ora.set_next_start(s.s0)
    ochosen, ost = ora.schedule(s.pods, nthreads=4)
    np.testing.assert_array_equal(ochosen, chosen, err_msg=f"{name} {shape}")
    assert (ora.next_start, ost.evals, ost.scheduled) == (nxt, evals, int((chosen >= 0).sum())), (name, shape)
    for k, v in ora.node_state().items():
        np.testing.assert_array_equal(v, cols[k], err_msg=f"{name} {shape} {k}")


def _outcome(name, fault=None):
    if fault is None:
        chosen, _, nxt, evals, _ = _reference(name)
        return chosen, nxt, evals
    s = adaptcases.scene(name)
    chosen, _, nxt, evals, _ = adaptref.schedule(s.cluster, s.pods, adaptcases.compiled(s.pct), next_start=s.s0,
                                                 window_fault=fault)
    return chosen, nxt, evals


def _differs(a, b) -> str:
    what = []
    if (a[0] != b[0]).any():
        what.append(f"{int((a[0] != b[0]).sum())} placements")
    if a[1] != b[1]:
        what.append("next_start")
    if a[2] != b[2]:
        what.append("evals")
    return ", ".join(what)


def test_every_wrong_reading_is_caught():
    caught = {}
    for number, fault in enumerate(adaptref.FAULTS, 1):
        hits = []
        for name in adaptcases.FAULT_SCENES:
            d = _differs(_outcome(name, fault), _outcome(name))
            if d:
                hits.append(f"{name} ({d})")
        caught[fault] = hits
        print(f"{number:2d} {fault:26s} {'; '.join(hits) if hits else 'NOT CAUGHT'}")
    missed = [f for f, h in caught.items() if not h]
    assert not missed, f"no scene tells these readings from the reference: {missed}"
    # the scenes built for a reading do catch it
    for fault, name in (("wrapped_low_bits_dropped", "kept_twice_guard"),
                        ("wrapped_high_bits_twice", "kept_twice_guard"),
                        ("stale_window", "flip_inside_window"), ("stale_cut_node", "flip_on_cut_node"),
                        ("binders_tested_alone", "two_binders_one_node"), ("k_plus_1_no_cut", "exactly_k_plus_1"),
                        ("short_pod_advances", "exactly_k"), ("empty_pod_not_counted", "none_feasible"),
                        ("wrap_by_words", "cut_in_wrapped_half")):
        assert any(h.startswith(name + " ") for h in caught[fault]), (fault, name, caught[fault])


@pytest.mark.parametrize("fault", ["stale_window", "stale_cut_node", "binders_tested_alone"])
def test_a_flip_past_the_cut_changes_nothing(fault):
    assert not _differs(_outcome("flip_past_cut", fault), _outcome("flip_past_cut"))


@pytest.mark.parametrize("name", list(adaptcases.SCENES))
def test_scene_has_the_property_it_claims(name):
    s = adaptcases.scene(name)
    claims = s.claims(s)
    print(name, claims)
    assert claims and all(v > 0 for v in claims.values()), claims
    assert 0 <= s.s0 < s.n and s.k < s.n


@pytest.mark.parametrize("name", list(adaptcases.SCENES))
def test_scene_runs_the_form_it_is_meant_for(name):
    s = adaptcases.scene(name)
    assert s.shapes
    for shape in s.shapes:
        assert s.form(shape) == s.forms[shape], (name, shape)
    if s.bare:
        from fastcases import is_narrow
        assert is_narrow(s.shaped("fast")) and not is_narrow(s.shaped("generic"))


def test_every_form_and_threshold_has_a_scene():
    forms = {}
    for name in adaptcases.SCENES:
        s = adaptcases.scene(name)
        for shape in s.shapes:
            forms.setdefault(s.forms[shape], []).append(f"{name}/{shape}")
    forms["sharded"] = [f"{n}/{w}" for n, w in adaptcases.SHARDED]
    for f in ("fused", "cut0_window", "cut0_top", "doubling", "sharded"):
        print(f, len(forms.get(f, [])))
        assert forms.get(f), f
    sc = adaptcases.scene
    words = lambda n: (sc(n).n + 63) // 64             # noqa: E731
    assert (words("doubling_8192"), words("doubling_8193")) == (128, 129)
    assert (words("cut0_counts_16384"), words("cut0_counts_16385")) == (256, 257)
    assert (sc("wide_top_8190").k, sc("wide_top_8192").k) == (4095, 4096)
    wide = sc("list_wide").claims(sc("list_wide"))
    assert wide["list"] > 0 and wide["fallback"] > 0      # at most / more than 4,096 kept nodes


@pytest.mark.parametrize("name,world", adaptcases.SHARDED)
def test_sharded_geometry(name, world):
    """Every group runs 64-aligned shards (the sharded ADAPT batch path) on a
    window that spans a shard boundary and wraps; the 600-node scenes with big
    pods leave a shard without a kept node for some pod; three shards end on a shorter one."""
    s = adaptcases.scene(name)
    g = adaptcases.shard_geometry(s, world)
    print(name, world, g)
    assert g["aligned shards"] and g["windows that span a shard boundary and wrap"] > 0
    assert g["last shard shorter"] or world == 2
    if s.n == adaptcases.SHARD_N and not s.flips:
        assert g["pods with no kept node on some shard"] > 0
    assert adaptcases.window_form(s.n, s.k, True, False, True) == "sharded"


@pytest.mark.parametrize("name", ["list_short", "list_mid", "list_wide"])
def test_static_class_windows(name):
    s = adaptcases.scene(name)
    ora = Oracle(s.shaped("static"), adaptcases.compiled(s.pct))
    ora.set_next_start(s.s0)
    chosen, st = ora.schedule(s.pods, nthreads=4)
    wins, last = s.windows()
    assert ora.next_start == last
    assert st.evals == sum(cut + 1 if cut >= 0 else s.n for _, cut in wins)
    assert (chosen >= 0).all()
    for j in range(s.pods.n_pods):                   # every pick a kept node of the pod's window
        start, cut = wins[j]
        off = (chosen[j] - start) % s.n
        assert s.masks[j][chosen[j]] and (cut < 0 or off < cut), (name, j)


def test_normv_scene_takes_the_kept_list_loops():
    """list_normv's bitmaps depend on taints and pools, so its windows are read
    off the oracle's cycles: pods whose normalized scores vary run the LDS-list
    loops of k_adapt_top's static-class keys, some with a wrapping window."""
    s = adaptcases.scene("list_normv")
    ora = Oracle(s.shaped("static"), adaptcases.compiled(s.pct))
    ora.set_next_start(s.s0)
    varies = adaptcases.norm_varies(s.cluster, s.pods)
    nt = adaptcases.top_threads(s.n, s.k, False, False)
    seen, wraps, start = {}, 0, s.s0
    for j in range(s.pods.n_pods):
        o = ora.cycle(s.pods, j)
        if varies[j]:
            f = adaptcases.list_form(o["n_processed"], min(o["n_feasible"], s.k), nt)
            seen[f] = seen.get(f, 0) + 1
            wraps += start + o["n_processed"] > s.n
        start = o["next_start"]
    print(seen, wraps)
    assert seen.get("list", 0) > 0 and wraps > 0 and nt == 256


def test_level_scenes_commit_whole_batches():
    """What the GPU test's batch counts stand on: on a level ring every bind
    lowers its node's total below every untouched node's of its kind, and the
    expected counts tell the forms apart."""
    import fastref
    s = adaptcases.scene("batch_tails_257")
    w = fastref.weights(adaptcases.compiled(s.pct))
    c = fastref.columns(s.cluster)
    for kind, sizes in ((adaptcases.SMALL, adaptcases.SIZES), (adaptcases.SMALL, adaptcases.LEVEL_SIZES),
                        (adaptcases.LARGE, adaptcases.LEVEL_SIZES)):
        cl = adaptcases.ring(64, np.full(64, kind), level=True)
        for name in "sb":
            if name == "b" and (kind == adaptcases.SMALL or sizes is adaptcases.SIZES):
                continue
            pods = adaptcases.queue(name, 3, sizes)
            cols = fastref.columns(cl)
            last = None
            for j in range(3):                       # the totals of a node as pods pile up on it: strictly falling
                ok, _, _, total = fastref.node_scores(cols, pods.pods[j], w)
                assert ok[0] and (last is None or total[0] < last), (kind, name, j)
                last = int(total[0])
                for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem"):
                    cols[f][0] += int(pods.pods[j][f])
                cols["num_pods"][0] += 1
    assert c["alloc_cpu"].size == adaptcases.TAILS_N
    for q in adaptcases.TAILS:
        t = adaptcases.scene(f"batch_tails_{q}")
        assert adaptcases.whole_batches(t, "generic") == -(-q // 256)
        assert adaptcases.whole_batches(t, "fast") >= -(-q // 256)
    slow = adaptcases.scene("slow_relaxation_4000")
    assert adaptcases.whole_batches(slow, "generic") == 1 and adaptcases.whole_batches(slow, "fast") == 3
    for name in ("doubling_8185", "doubling_8192"):
        assert adaptcases.whole_batches(adaptcases.scene(name), "generic") == 2


def test_relax_model():
    """relax agrees with windows where it says a pod is exact, needs one round
    on bitmaps without holes, and reports a fixpoint as the whole batch."""
    s = adaptcases.scene("slow_relaxation")
    left = adaptref.relax(s.masks, s.s0, s.k, adaptcases.K_WINDOW_ROUNDS)
    assert 0 < left < 256
    assert adaptref.relax(s.masks, s.s0, s.k, 1000) == 256
    assert adaptref.relax(s.masks, s.s0, s.k, 1) <= left
    dense = np.ones((256, 400), bool)
    assert adaptref.relax(dense, 5, 100, 1) == 256
