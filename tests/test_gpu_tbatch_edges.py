"""The topology batch kernels (csrc/ksim_tbatch.hip) and their host side
(tbatch_admit, tbatch_vuse, tbatch_runs in csrc/ksim_engine.cpp) on the
hand-built edge scenes of tests/tbatchcases.py, bit for bit against the
oracle.  tests/test_tbatch_cases.py proves on the CPU that each scene reaches
the edges it names; here every scene goes through the engine's routes.

  edge                                      scene                      pins
  ----------------------------------------  -------------------------  ------------------------------------------
  nf == 0, unschedulable pods in a run      nf_ladder_full_*           ksim_tbatch.hip:576 (stat), :1257 (commit)
  nf == 1: kStatOne, chosen unscored        nf_ladder, tiny_one_node   ksim_tbatch.hip:576-579, :1104
  has_soft = nf > 1                         nf_ladder                  ksim_tbatch.hip:530
  nf <= kTopT: topk_complete                many_apps_few_nodes_1..8   ksim_tbatch.hip:687, :742
  nf == kTopT + 1                           many_apps_few_nodes_9      ksim_tbatch.hip:687, :742
  an exhausted incomplete list cuts the     exhausted_list             ksim_tbatch.hip:906-908, :687, :742
    chain (the best node is on no list)
  IgnoredNodes: q.ign, nign, counted        ignored_and_unkeyed,       ksim_tbatch.hip:103-114, :331-334, :359, :539
    nf - nign == 1 and 0                    mostly_ignored
  the weight topo_log[nf - nign]            ignored_weight             ksim_tbatch.hip:531, :1146
  a node without a table-read key (id 0)    ignored_and_unkeyed        ksim_tbatch.hip:532; ksim_engine.cpp:4281
  a DoNotSchedule key some node lacks       ..._unkeyed_zoneless       ksim_engine.cpp:4276 (col_total), :779
  variant key of 1 .. 4 domains             variant_slots_1..4,        ksim_tbatch.hip:205, :240-260;
                                            many_apps_few_nodes_9      ksim_engine.cpp:4350-4351
  a slot with nf == 0 / nf == 1             variant_slots_3, _4        ksim_tbatch.hip:109-116, :502-517
  an unschedulable adder (slot 0)           variant_slots_3, _4        ksim_tbatch.hip:240 (wmax), :1257
  a foreign selector (self == 0)            variant_slots_*            ksim_tbatch.hip:206, :254
  two adders: no variant, the run ends      variant_two_adders         ksim_tbatch.hip:221; ksim_engine.cpp:4390
  5 and 17 domains (min(vdom, 15u))         variant_wide_5, _17        ksim_tbatch.hip:326; ksim_engine.cpp:4351
  partial last block (xr clamped)           block_edges_255, _257      ksim_tbatch.hip:281
  N = kTbMaxBlocks * 256, hold table        block_edges_16384          ksim_tbatch.hip:624-687, :884
  N = kTbMaxBlocks * 256 + 1: per-pod       block_edges_16385          ksim_engine.cpp:773, :2784
  more than kTopT nodes tie across blocks   block_edges_*              ksim_tbatch.hip:624-687 (k_tb_merge)
  runs of kTbPods - 1 .. 2 kTbPods + 1      run_lengths_*              ksim_tbatch.hip:59 (tb_count);
                                                                       ksim_engine.cpp:4380
  hard_small at / past kFuseMinValues       hard_hostname_255, _256    ksim_engine.cpp:4489, :4276
  a lone extremum holder an earlier pod     lone_holder                ksim_tbatch.hip:760-766 (hmin <= j), :1139
    of the app takes (hmin == j == 1)
  kTopoScoreNonEmpty flips in a batch       lone_holder_empty          ksim_tbatch.hip:1096, :1129
  one node; a tainted node; one wave        tiny_*                     ksim_tbatch.hip:435-620 (block_top_t)
  replicas: one-node range, a boundary      test_replicated_ranges     ksim_tbatch.hip:672 (xsend), :692, :719
    inside a block, ranges with no feasible
    node

Every route compares placements, evals, scheduled, next_start, every
node_state() column and class_count(), with no tolerance; the oracle's run of
a scene is computed once per percentageOfNodesToScore.

What the scenes were seen to tell apart: builds of ksim_tbatch.hip with one
line changed (topk_complete at nf <= kTopT + 1 in k_tb_merge or k_tb_gmerge;
topo_log[nf] for topo_log[nf - nign]; has_soft = nf > 2; IgnoredNodes counted
into the extrema; k_tb_merge's lane 63 without its block; tb_var_setup's
minimum without the adder's count; tb_keeps_extrema with hmax < j, hmin < j)
each fail a case here, and all but the tb_var_setup one pass
tests/test_gpu_tbatch.py.  Dropping the kTopoScoreNonEmpty check at line 1096
fails nothing: where the score map is empty every extremum is 0, so the moved
score leaves [gmin, gmax] and tb_keeps_extrema ends the batch anyway, or the
guessed node is outside the pod's feasible set and the newly non-empty map
moves every feasible node's normalized score alike."""
import functools

import numpy as np
import pytest

from ksim import engine
from ksim.engine import Engine, group_schedule_loaded
from oracle.oracle import Oracle

import tbatchcases as tc
from test_gpu_parity import _compare_cycle

pytestmark = pytest.mark.gpu

NAMES = list(tc.SCENES)
CYCLE_SCENES = [n for n in NAMES if n.startswith(("nf_ladder", "ignored_", "mostly_ignored", "tiny_", "variant_"))]


@functools.lru_cache(maxsize=None)
def _oracle(name, pct=100):
    """The oracle's run of the scene's queue, computed once: placements,
    (evals, scheduled), next_start, node state, class counts."""
    s = tc.scene(name)
    cluster, pods = s.encoded
    ora = Oracle(cluster.copy_state(), tc.compiled(s.kind, pct))
    chosen, st = ora.schedule(pods, nthreads=16)
    chosen.setflags(write=False)
    out = chosen, (st.evals, st.scheduled), ora.next_start, ora.node_state(), ora.class_count()
    ora.close()
    return out


def _same(e, chosen, st, name, pct, tag):
    ochosen, ost = _oracle(name, pct)[:2]
    np.testing.assert_array_equal(chosen, ochosen, err_msg=tag)
    assert (st.evals, st.scheduled) == ost, tag
    _same_state(e, name, pct, tag)


def _same_state(e, name, pct, tag):
    _, _, onext, ostate, ocount = _oracle(name, pct)
    assert e.next_start == onext, tag
    es = e.node_state()
    assert set(es) == set(ostate), tag
    for k in es:
        np.testing.assert_array_equal(es[k], ostate[k], err_msg=f"{tag} {k}")
    np.testing.assert_array_equal(e.class_count(), ocount, err_msg=f"{tag} class_count")


def _engine(name, pct=100, variant=None):
    s = tc.scene(name)
    cluster, _ = s.encoded
    e = Engine(0, variant=variant)
    e.set_profile(tc.compiled(s.kind, pct))
    e.set_cluster(cluster.copy_state())
    return e


def _run(name, pct=100, variant=None):
    """One handle's schedule_batch of the scene against the oracle; returns
    (stats, diag) for the caller's path assertions."""
    e = _engine(name, pct, variant)
    try:
        chosen, st = e.schedule_batch(tc.scene(name).encoded[1])
        _same(e, chosen, st, name, pct, f"{name} pct {pct} {variant or ''}")
        return st, e.diag()
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _product(name):
    """(batches, perpod_cycles, tb_variant_pods) of the product's run at pct 100."""
    st, d = _run(name)
    return st.batches, st.perpod_cycles, d["tb_variant_pods"]


def _assert_route(name, batches, perpod, plain=False):
    s = tc.scene(name)
    n = len(s.queue)
    if s.route == "perpod":
        assert perpod == n, (name, perpod, batches)
    else:
        assert perpod == 0 and batches > 0, (name, perpod, batches)
        if s.multi_plain if plain else s.multi:
            assert batches < n, (name, batches)


# ---- route 1: one handle, schedule_batch, pct 100 ---------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_schedule_batch(name):
    """The product: topology batches with zone variants.  The route is the
    scene's: no per-pod cycle and batches of several pods, or (16,385 nodes,
    a hostname key past kFuseMinValues, a DoNotSchedule key a node lacks) a
    per-pod cycle for every pod."""
    batches, perpod, vp = _product(name)
    _assert_route(name, batches, perpod)
    s = tc.scene(name)
    if s.variants is True:
        assert vp > 0, (name, vp)
    elif s.variants is False:
        assert vp == 0, (name, vp)


# ---- route 2: the flavor without zone variants --------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_without_zone_variants(name):
    """libksim_engine_ab64.so: the same placements with every run ending at a
    zone-keyed class conflict, so at least as many batches where the product
    takes variants."""
    st, d = _run(name, variant="ab64")
    assert d["tb_variant_pods"] == 0
    _assert_route(name, st.batches, st.perpod_cycles, plain=True)
    if tc.scene(name).variants:
        assert st.batches >= _product(name)[0], (name, st.batches, _product(name))


# ---- route 3: per-pod cycles, every output of every node -----------------------------------
@pytest.mark.parametrize("name", CYCLE_SCENES)
def test_per_pod_cycles(name):
    """Engine.eval_pod of every pod against Oracle.cycle: when a batch route
    fails, this tells a wrong filter or score from a wrong batch."""
    s = tc.scene(name)
    cluster, pods = s.encoded
    e = _engine(name)
    ora = Oracle(cluster.copy_state(), tc.compiled(s.kind))
    try:
        for j in range(pods.n_pods):
            _compare_cycle(e.eval_pod(pods, j), ora.cycle(pods, j), f"{name} pod {j}")
        _same_state(e, name, 100, name)
    finally:
        e.close()
        ora.close()


# ---- route 4: replicated handles with hand-picked ranges ------------------------------------
def _hostless_split():
    cluster, _ = tc.scene("ignored_and_unkeyed").encoded
    p = cluster.node_names.index("hostless")
    return [0, p, p + 1, cluster.n_nodes]


RANGES = [
    ("block_edges_257", [0, 1, 257]),                          # a one-node range
    ("block_edges_257", [0, 100, 250, 257]),                   # cuts inside block 0; a range across block 1's start
    ("many_apps_few_nodes_9", [0, 1, 9]),
    ("many_apps_few_nodes_9", [0, 8, 9]),
    ("exhausted_list", [0, 8, 9]),                             # the node on no list in a range of its own
    ("nf_ladder_full_one_app", [0, 1, 3]),
    ("variant_slots_3", [0, 1, 6]),
    ("lone_holder", [0, 1, 2, 12]),                            # the lone holder and its large rival, a range each
    ("ignored_and_unkeyed", None),                                 # the ignored node in a range of its own
    ("ignored_weight", [0, 3, 9]),                             # the labelled nodes in one range, the ignored in another
    ("tiny_one_wave", [0, 64, 128, 300]),                      # every feasible node in the middle replica
    ("block_edges_16384", [0, 1000, 2048, 4100, 8191, 8192, 12000, 16383, 16384]),
]


@pytest.mark.parametrize("name,bounds", RANGES, ids=[f"{n}-{k}" for k, (n, _) in enumerate(RANGES)])
def test_replicated_ranges(name, bounds):
    """Replicas of the whole snapshot on one device, each evaluating its node
    range (k_tb_merge's xsend record, k_tb_wmerge, k_tb_gmerge): the oracle's
    placements, and every replica ends with its node state and class counts."""
    bounds = bounds or _hostless_split()
    s = tc.scene(name)
    _, pods = s.encoded
    engines = []
    try:
        for lo, hi in zip(bounds, bounds[1:]):
            e = _engine(name)
            e.set_eval_range(lo, hi)
            e.load_pods(pods)
            engines.append(e)
        chosen, st = group_schedule_loaded(engines, 0, pods.n_pods)
        ochosen, ost, _, _, _ = _oracle(name)
        np.testing.assert_array_equal(chosen, ochosen)
        assert (st.evals, st.scheduled) == ost
        _assert_route(name, st.batches, st.perpod_cycles, plain=True)
        for r, e in enumerate(engines):
            _same_state(e, name, 100, f"{name} replica {r}")
    finally:
        for e in engines:
            e.close()


def test_world_of_one_communicator():
    """A replicated handle with a communicator of one rank (the RCCL exchange
    calls) on the nine-node scene: nf == kTopT + 1."""
    name = "many_apps_few_nodes_9"
    _, pods = tc.scene(name).encoded
    e = _engine(name)
    try:
        e.set_eval_range(0, 9)
        e.comm_init(0, 1, engine.comm_unique_id())
        e.load_pods(pods)
        chosen, st = e.schedule_loaded(0, pods.n_pods)
        _same(e, chosen, st, name, 100, name)
        assert st.perpod_cycles == 0 and 0 < st.batches < pods.n_pods
    finally:
        e.close()


# ---- route 5: percentageOfNodesToScore 0 -----------------------------------------------------
@pytest.mark.parametrize("name", ["nf_ladder", "many_apps_few_nodes_9", "block_edges_257"])
def test_adaptive_percentage(name):
    """Below 100 nodes numFeasibleNodesToFind is N and the topology batches
    run; at 257 nodes it is below N (ADAPT) and pod_on_batch sends the
    topology pods to the per-pod path."""
    st, d = _run(name, pct=0)
    n = len(tc.scene(name).queue)
    if tc.scene(name).encoded[0].n_nodes < 100:
        assert st.perpod_cycles == 0 and 0 < st.batches < n
    else:
        assert st.perpod_cycles == n
