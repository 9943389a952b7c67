"""The ADAPT scan windows (csrc/ksim_adapt.hip) on the designed scenes of
tests/adaptcases.py, bit for bit against the C oracle: placements, evals,
scheduled, next_start and every node_state() column, from a start the test
sets (and reads back) itself.  tests/test_adapt_cases.py proves on the CPU
that these scenes tell twelve wrong readings of the window from the right one
and that each scene has the property its name claims.

A window form has no signal of its own per handle: adaptcases.window_form
restates the host's choice (launch_batch_adapt, launch_batch_adapt_lazy,
launch_adapt_sh_window) and the CPU test asserts every scene's form.  The
scenes per form ("fast": narrow cluster, deferred-commit FAST run; "generic":
one allocatable at 2^46, generic keys, three launches; "static": pods in
static classes, three launches):

  fused relaxation (window_block / find_cut inside k_adapt_top, WIN = 1)
      fast:    every small ring (ring101_* .. slow_relaxation*, shard_*,
               batch_tails_*), doubling_*, cut0_*_16384, wide_top_8190;
               slow_relaxation_4000, batch_tails_* and doubling_* take exactly
               the batches the relaxation's exact prefixes give
      generic: doubling_8193, cut0_*_16384
      static:  list_short, list_mid, list_normv
  k_adapt_cut0 + k_adapt_window (three launches)
      generic: cut0_*_16385, cut0_*_24576, cut0_*_24577
      static:  list_wide
  k_adapt_cut0 + the relaxation inside k_adapt_top (WIN = 2)
      fast:    cut0_*_16385, cut0_*_24576, cut0_*_24577, wide_top_8192
  pointer doubling (k_win_build, k_win_round_lds<8> x 2, k_win_final<64>)
      generic: every small ring, batch_tails_* (the radix-8 and stride-64
               tails: each run takes ceil(q / 256) batches, so every pod's
               window reaches the placements), doubling_8185 (scalar staging),
               doubling_8192 (uint4 staging, node 8,191; 260 pods in two
               batches), wide_top_8190, wide_top_8192
  node-sharded (k_adapt_unpack, k_adapt_cut0, k_adapt_window, k_adapt_top<SH>)
      shard_cut_in_wrapped_half, shard_exactly_k_plus_1,
      shard_flip_on_cut_node, cut0_wrapped_16385, each on 2 and 3 shards

The thresholds, a scene on each side: 128 / 129 words for generic keys
(doubling_8192 / doubling_8193), 256 / 257 words (cut0_*_16384 /
cut0_*_16385), K 4095 / 4096 (wide_top_8190 / wide_top_8192), 4,096 kept
nodes (list_wide's zone pods keep 3,333 or 3,334, its plain pods 4,500).
k_adapt_top's kept-node loops of the static-class FAST keys: list_short (the
stepping loop, one kept node per thread), list_mid (the LDS list), list_wide
(1,024 threads: one per thread, the list, the fallback), list_normv
(kPodNormVaries)."""
import functools
import math

import numpy as np
import pytest

from ksim.engine import Engine, group_schedule_loaded
from ksim.shard import partition
from oracle.oracle import Oracle

import adaptcases

pytestmark = pytest.mark.gpu

# the scenes on level rings: their batches commit whole
WHOLE = ["slow_relaxation_4000"] + [n for n in adaptcases.SCENES if n.startswith(("batch_tails_", "doubling_"))]
CASES = [(n, sh) for n in adaptcases.SCENES for sh in ("fast", "generic", "static")
         if (sh == "static") == n.startswith("list_")]


@functools.lru_cache(maxsize=None)
def _oracle(name, shape):
    """The oracle's run of a scene from its start, computed once: (placements,
    (evals, scheduled), next_start, node state)."""
    s = adaptcases.scene(name)
    ora = Oracle(s.shaped(shape), adaptcases.compiled(s.pct))
    ora.set_next_start(s.s0)
    chosen, st = ora.schedule(s.pods, nthreads=16)
    chosen.setflags(write=False)
    return chosen, (st.evals, st.scheduled), ora.next_start, ora.node_state()


@pytest.mark.parametrize("name,shape", CASES)
def test_scene(name, shape):
    s = adaptcases.scene(name)
    assert shape in s.shapes
    tag = f"{name} {shape} ({s.forms[shape]})"
    e = Engine(0)
    e.set_profile(adaptcases.compiled(s.pct))
    e.set_cluster(s.shaped(shape))
    e.set_next_start(s.s0)
    assert e.next_start == s.s0, tag
    chosen, st = e.schedule_batch(s.pods)
    ochosen, ost, onext, ostate = _oracle(name, shape)
    print(tag, "batches", st.batches, "perpod", st.perpod_cycles, "evals", st.evals, "next_start", e.next_start)
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled) == ost, tag
    assert e.next_start == onext, tag
    es = e.node_state()
    for k, v in ostate.items():
        np.testing.assert_array_equal(es[k], v, err_msg=f"{tag} {k}")
    assert st.perpod_cycles == 0 and st.batches > 0, tag
    if name in WHOLE:
        # a level ring: no pair cut and no broken window ends a batch, so the windows of every pod of
        # a batch reach the placements above.  The doubling form commits whole batches; the relaxation
        # commits the prefix it makes exact (adaptcases.relax_batches), all of the batch at a fixpoint
        assert st.batches == adaptcases.whole_batches(s, shape), tag
    if name.startswith("slow_relaxation") and shape == "fast":
        # a batch commits at most the prefix the relaxation makes exact (80 of the first 256 pods)
        assert st.batches >= adaptcases.relax_batches(s) > math.ceil(s.pods.n_pods / 256), tag
    e.close()


@pytest.mark.parametrize("name,world", adaptcases.SHARDED)
def test_sharded(name, world):
    """In-process groups of 64-aligned node shards through group_schedule_loaded."""
    s = adaptcases.scene(name)
    prof = adaptcases.compiled(s.pct)
    cluster = s.shaped("fast")
    tag = f"{name} {world} shards"
    engines = []
    for base, cnt in partition(s.n, world):
        assert base % 64 == 0
        e = Engine(0)
        e.set_shard(base, s.n)
        e.set_profile(prof)
        e.set_cluster(cluster.shard(base, cnt))
        e.set_next_start(s.s0)                        # a global position, on every shard
        e.load_pods(s.pods)
        engines.append(e)
    assert all(e.next_start == s.s0 for e in engines), tag
    chosen, st = group_schedule_loaded(engines, 0, s.pods.n_pods)
    ochosen, ost, onext, ostate = _oracle(name, "fast")
    print(tag, "batches", st.batches, "perpod", st.perpod_cycles, "evals", st.evals)
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled) == ost, tag
    assert all(e.next_start == onext for e in engines), tag
    parts = [e.node_state() for e in engines]
    for k, v in ostate.items():
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), v, err_msg=f"{tag} {k}")
    assert st.perpod_cycles == 0 and st.batches > 0, tag
    for e in engines:
        e.close()
