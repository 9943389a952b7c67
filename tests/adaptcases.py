"""Designed scenes for the ADAPT scan windows (csrc/ksim_adapt.hip: find_cut,
window_block, k_adapt_cut0, k_adapt_window, the k_win_* doubling launches, the
kept-node loops of k_adapt_top, k_adapt_pairs' broken test).  Feasibility is
designed, not drawn: a node is full (its pod slots are used up), small-roomy
(cpu 2000m: only pods that request nothing fit) or large-roomy (cpu 64000m),
and a queue holds up to three pod sizes, "s" (requests nothing), "b"
(requests 4000m: large nodes only) and "h" (requests more than any node has),
so every pod's bitmap is known by construction.  Every scene sets
nextStartNodeIndex itself and carries the property its name claims as counts
over tests/adaptref.py's window model that must all be above zero.

tests/test_adapt_cases.py proves on the CPU that the scenes tell twelve wrong
readings of the window (adaptref.FAULTS) from the right one;
tests/test_gpu_adapt_edges.py runs them through every window form.

Two shapes per bare scene: "fast" (the cluster as built: narrow allocatables,
the FAST keys, deferred-commit runs) and "generic" (one full node's memory set
to 2^46: the cluster is no longer narrow, so the run takes the generic keys
and the three-launch batches; the node is full, so no pod ever scores it;
ring101_all_feasible has no full node and names a roomy one).

What the issue's list names and no legal input reaches: a cut in
k_adapt_cut0's virtual word 0.  The cut is the (K + 1)-th feasible node, and
the launch runs only past 256 words (K is then at least 819, 5 % of more than
16,384 nodes) or from K = 4,096, so the first word that can hold it is word 12
from the start, lane 6 of the first step; cut0_dense_* puts it there.

257 nodes give K = 123 under percentageOfNodesToScore 0 (48 % of 257), the
other small rings K = 100 or 144."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from ksim import gen, profile
from ksim.encode import EncodedCluster, EncodedPods

import adaptref
import fastcases
from fastcases import GI, MI, NARROW, best_effort, make_pods, requesting

SEED = 0x41445054
SIZES = {"s": best_effort(), "b": requesting(4000, GI), "h": requesting(10 ** 6, GI)}
FULL, SMALL, LARGE = 0, 1, 2
# level rings (ring(level=True)): every bind must move its node's score, see ring
LEVEL_SIZES = {"s": requesting(1000, 4 * GI), "b": requesting(4000, 4 * GI), "h": requesting(10 ** 6, GI)}

# csrc/ksim_adapt.hip's constants, restated for the form helper
K_WIN_SEQ_WORDS, K_WIN_FUSED_WORDS, K_TOP_WIDE_K, K_ADAPT_LIST, K_WINDOW_ROUNDS = 128, 256, 4096, 4096, 48
LAZY_MAX_NODES = 1 << 17


def window_form(n_nodes: int, k: int, fast: bool, lazy: bool, sharded: bool) -> str:
    """The host's choice of window form, restated from csrc/ksim_adapt.hip.
    Unsharded three-launch batches: launch_batch_adapt, lines 1276-1297
    (win_seq, win_fused, else k_adapt_cut0 + k_adapt_window); deferred-commit
    FAST runs: launch_batch_adapt_lazy, lines 1333-1352 (win_fused, else
    k_adapt_cut0 + k_adapt_top<.., 2>); node shards: launch_adapt_sh_window,
    lines 1391-1407 (always k_adapt_cut0 + k_adapt_window on the unpacked
    global bitmap).

    ``fast`` is LaunchArgs::fast.  The static-class scenes pass fast=False:
    run_stab is off under ADAPT, so their runs take the non-FAST template, and
    the FAST keys of a static class come from P.stab_fast inside it.  Those
    scenes need more than 8,192 nodes to stay off the doubling form."""
    words = (n_nodes + 63) // 64
    if sharded:
        return "sharded"
    fused = k < K_TOP_WIDE_K and words <= K_WIN_FUSED_WORDS
    if lazy:
        assert fast
        return "fused" if fused else "cut0_top"
    if not fast and words <= K_WIN_SEQ_WORDS:
        return "doubling"
    return "fused" if fused else "cut0_window"


def top_threads(n_nodes: int, k: int, fast: bool, lazy: bool) -> int:
    """k_adapt_top's block: 1,024 threads from K = 4,096 and behind the doubling windows."""
    return 1024 if k >= K_TOP_WIDE_K or window_form(n_nodes, k, fast, lazy, False) == "doubling" else 256


@dataclass
class Scene:
    name: str
    cluster: EncodedCluster
    pods: EncodedPods
    s0: int
    pct: int = 0
    bare: bool = True                              # trivial cpu / memory pods: tests/adaptref.py restates the run
    flips: bool = False                            # a bind of the queue fills a node
    generic_node: Optional[int] = None             # the node the generic shape widens (default: the first full node)
    masks: Optional[np.ndarray] = None             # the S0 bitmaps (bool, pods x nodes)
    claims: Callable[["Scene"], Dict[str, int]] = field(default=lambda s: {})
    # the window form the scene is meant for per shape (asserted against window_form)
    forms: Dict[str, str] = field(default_factory=dict)

    @property
    def n(self) -> int:
        return self.cluster.n_nodes

    @property
    def k(self) -> int:
        return profile.num_feasible_nodes_to_find(self.n, self.pct)

    @property
    def shapes(self) -> Tuple[str, ...]:
        return tuple(self.forms)

    def form(self, shape: str) -> str:
        fast = self.bare and shape == "fast"
        return window_form(self.n, self.k, fast, fast and self.n <= LAZY_MAX_NODES, False)

    def shaped(self, shape: str) -> EncodedCluster:
        """A private copy of the cluster in the given shape."""
        c = self.cluster.copy_state()
        if shape == "generic" and self.bare:
            node = self.generic_node
            if node is None:
                full = np.nonzero(self.cluster.num_pods >= self.cluster.alloc_pods)[0]
                assert full.size, f"{self.name}: the generic shape needs a full node"
                node = full[0]
            c.alloc_mem = self.cluster.alloc_mem.copy()
            c.alloc_mem[node] = NARROW
            assert not fastcases.is_narrow(c)
        return c

    def windows(self):
        return adaptref.windows(self.masks, self.s0, self.k)


def compiled(pct: int):
    return fastcases.compiled("w11", pct)


# ---- building blocks ---------------------------------------------------------------------
def ring(n: int, kinds: np.ndarray, slots: Optional[dict] = None, level: bool = False) -> EncodedCluster:
    """n nodes of the three kinds; roomy nodes carry unlike bound loads, so
    their scores differ.  slots: {node: free pod slots} on nodes left with no
    load at all (the best node of any window that holds one).

    level: the roomy nodes of a kind alike and empty (small 3000m, large
    16000m, 64 Gi both), for the scenes whose batches must commit whole.  A
    batch ends early where a pod's pick, re-keyed after an earlier pod of the
    batch bound there, still beats the later pod's own guess (the pair cut).
    On a level ring every bind lowers its node's total (a pod that requests
    nothing takes 3.3 cpu points of a small node, a LEVEL_SIZES pod 6 or more
    of any node), so a bound node falls behind every untouched node of its
    kind and a later pod's guess, its best untouched node, stands."""
    kinds = np.asarray(kinds)
    assert kinds.size == n
    c = gen.bare_cluster(n, SEED)
    i = np.arange(n)
    large = kinds == LARGE
    if level:
        assert not slots
        c.alloc_cpu[:] = np.where(large, 16000, 3000)
        c.alloc_mem[:] = 64 * GI
        c.alloc_pods[:] = 110
        c.num_pods[:] = np.where(kinds == FULL, 110, 0)
        return c
    c.alloc_cpu[:] = np.where(large, 64000, 2000)
    c.alloc_mem[:] = np.where(large, 256 * GI, 8 * GI)
    c.alloc_pods[:] = 110
    c.num_pods[:] = np.where(kinds == FULL, 110, i % 5)
    roomy = kinds != FULL
    c.req_cpu[:] = c.nz_cpu[:] = np.where(roomy, (1 + i * 37 % 9) * (c.alloc_cpu // 40), 0)
    c.req_mem[:] = c.nz_mem[:] = np.where(roomy, (1 + i * 11 % 7) * (c.alloc_mem // 40), 0)
    for node, free in (slots or {}).items():
        assert kinds[node] != FULL
        c.req_cpu[node] = c.nz_cpu[node] = c.req_mem[node] = c.nz_mem[node] = 0
        c.num_pods[node] = 110 - free
    return c


def queue(pattern: str, n_pods: int, sizes=None) -> EncodedPods:
    names = "sbh"
    order = [names.index(pattern[j % len(pattern)]) for j in range(n_pods)]
    return make_pods([(sizes or SIZES)[x] for x in names], order)


def kinds_at(n: int, s0: int, large=(), small=()) -> np.ndarray:
    """Full nodes but for the given offsets from s0."""
    kinds = np.full(n, FULL)
    kinds[(s0 + np.asarray(small, np.int64)) % n] = SMALL
    kinds[(s0 + np.asarray(large, np.int64)) % n] = LARGE
    return kinds


def spaced(count: int, span: int, first: int = 0) -> np.ndarray:
    """count offsets spread evenly over [first, first + span)."""
    assert 0 < count <= span
    return first + np.arange(count) * span // count


def pattern_kinds(n: int) -> np.ndarray:
    """Seven nodes in ten roomy, large and small alternating."""
    i = np.arange(n)
    return np.where(i * 7 % 10 < 7, np.where(i % 2 == 0, LARGE, SMALL), FULL)


def build(name, kinds, pattern, n_pods, s0, claims, pct=0, slots=None, flips=False, forms=None, level=False,
          sizes=None) -> Scene:
    c = ring(len(kinds), kinds, slots, level)
    pods = queue(pattern, n_pods, sizes)
    s = Scene(name, c, pods, s0, pct, flips=flips, claims=claims,
              masks=adaptref.masks_of(c, pods, compiled(pct)), forms=forms or {"fast": "fused", "generic": "doubling"})
    feasible = {"s": kinds != FULL, "b": kinds == LARGE, "h": np.zeros(len(kinds), bool)}
    for j in range(n_pods):                        # the bitmaps are the ones the construction means
        assert (s.masks[j] == feasible[pattern[j % len(pattern)]]).all(), (name, j)
    return s


def relax_batches(sc: Scene) -> int:
    """The batches of a deferred-commit run that no pair cut and no broken
    window shortens: each takes up to 256 pods and commits the prefix the
    relaxation makes exact (adaptref.relax), and the next starts from there."""
    cursor, s, batches = 0, sc.s0, 0
    while cursor < sc.pods.n_pods:
        m = sc.masks[cursor:cursor + adaptref.BATCH]
        exact = adaptref.relax(m, s, sc.k, K_WINDOW_ROUNDS)
        assert exact > 0
        s = adaptref.windows(m[:exact], s, sc.k)[1]
        cursor += exact
        batches += 1
    return batches


def whole_batches(sc: Scene, shape: str) -> int:
    """The batches a level scene's run takes: the doubling windows are exact
    for the whole batch, the relaxation for the prefix relax_batches follows."""
    if sc.form(shape) == "doubling":
        return -(-sc.pods.n_pods // adaptref.BATCH)
    return relax_batches(sc)


def _count(scene, pred) -> int:
    n = scene.n
    return sum(1 for (s, cut), ok in zip(scene.windows()[0], scene.masks) if pred(s, cut, ok, n))


def _wrapped(s, cut, ok, n) -> bool:
    return s + (cut if cut >= 0 else n) > n


# ---- small rings ---------------------------------------------------------------------------
def exactly_k() -> Scene:
    n = 129
    kinds = kinds_at(n, 0, large=spaced(100, n))
    # a roomy start behind a full node: a start that advanced past the last feasible node would move
    s0 = next(i for i in range(70, n) if kinds[i] != FULL and kinds[i - 1] == FULL)
    return build("exactly_k", kinds, "sb", 40, s0, lambda sc: {
        "pods with exactly K feasible nodes": int((sc.masks.sum(1) == sc.k).sum()),
        "pods without a cut": _count(sc, lambda s, cut, ok, n: cut < 0),
        "the start never moves": int(sc.windows()[1] == sc.s0 and len(sc.windows()[0]) == 40)})


def ring101_exactly_k() -> Scene:
    """101 nodes, K = 100 = N - 1: one full node (node 64, bit 0 of the second
    word, whose tail holds 37 nodes), so no pod has a cut."""
    n, s0 = 101, 90
    kinds = np.full(n, LARGE)
    kinds[64] = FULL
    return build("ring101_exactly_k", kinds, "sb", 40, s0, lambda sc: {
        "pods with exactly K = N - 1 feasible nodes": int((sc.masks.sum(1) == sc.k).all() and sc.k == sc.n - 1),
        "pods without a cut": _count(sc, lambda s, cut, ok, n: cut < 0),
        "the start never moves": int(sc.windows()[1] == sc.s0)})


def ring101_all_feasible() -> Scene:
    """101 nodes, every one roomy: the only ring of 101 with a (K + 1)-th
    feasible node.  Every cut is the node before the start, the last offset of
    the ring: in the start's own word below the start, or (start 64) the last
    node of the first word.  The start falls by one per pod, from 70 through
    bit 0 of the second word to bit 63 of the first.  No node is full, so the
    generic shape widens node 100's memory: it has room for the whole queue."""
    n, s0 = 101, 70
    sc = build("ring101_all_feasible", np.full(n, LARGE), "sb", 40, s0, lambda sc: {
        "cuts on the node before the start": _count(sc, lambda s, cut, ok, n: cut == n - 1),
        "of them in the start's own word below the start": _count(
            sc, lambda s, cut, ok, n: cut == n - 1 and adaptref.virtual_word(s, cut, n) == 2),
        "starts on bit 0 of the 37-node tail word": _count(sc, lambda s, cut, ok, n: s == 64),
        "starts in the first word": _count(sc, lambda s, cut, ok, n: s < 64)})
    sc.generic_node = 100
    return sc


def exactly_k_plus_1() -> Scene:
    n, s0 = 128, 63
    kinds = kinds_at(n, 0, large=spaced(101, n))
    return build("exactly_k_plus_1", kinds, "sb", 40, s0, lambda sc: {
        "pods with exactly K + 1 feasible nodes": int((sc.masks.sum(1) == sc.k + 1).sum() == 40),
        "pods whose cut is the last feasible node of the ring": _count(
            sc, lambda s, cut, ok, n: cut >= 0 and adaptref.offsets(ok, s)[-1] == cut)})


def none_feasible() -> Scene:
    n, s0 = 257, 200
    kinds = kinds_at(n, 0, small=spaced(180, n))
    return build("none_feasible", kinds, "sbssbbs", 42, s0, lambda sc: {
        "pods with no feasible node": int((sc.masks.sum(1) == 0).sum()),
        "such pods between two that have some": sum(
            1 for j in range(1, 41) if not sc.masks[j].any() and sc.masks[j - 1].any() and sc.masks[j + 1].any())})


def _start_scene(name, n, s0, extra) -> Scene:
    def claims(sc):
        out = {"windows with a cut": _count(sc, lambda s, cut, ok, n: cut >= 0),
               "windows that wrap": _count(sc, _wrapped)}
        out.update(extra(sc))
        return out
    return build(name, pattern_kinds(n), "ssb", 60, s0, claims)


def start_bit0() -> Scene:
    return _start_scene("start_bit0", 300, 128, lambda sc: {"the start is bit 0 of its word": int(sc.s0 % 64 == 0)})


def start_bit63() -> Scene:
    return _start_scene("start_bit63", 300, 191, lambda sc: {"the start is bit 63 of its word": int(sc.s0 % 64 == 63)})


def start_last_node() -> Scene:
    return _start_scene("start_last_node", 257, 256, lambda sc: {
        "the start is node N - 1, alone in its word": int(sc.s0 == sc.n - 1 and sc.n % 64 == 1)})


def start_on_infeasible() -> Scene:
    return _start_scene("start_on_infeasible", 300, 201, lambda sc: {
        "the start is a full node": int(not sc.masks[:, sc.s0].any())})


def cut_in_wrapped_half() -> Scene:
    """From node 150: 140 large nodes over offsets 0..277 (every node before
    the start's word comes round again), then nodes 128..149 all large, so pod
    0's 145th feasible node is node 132, below the start in the start's word."""
    n, s0 = 300, 150
    offs = np.concatenate([np.arange(0, 277, 2), [1], np.arange(278, 300)])
    return build("cut_in_wrapped_half", kinds_at(n, s0, large=offs), "sb", 24, s0, lambda sc: {
        "cuts in the start's own word below the start": _count(
            sc, lambda s, cut, ok, n: cut >= 0 and adaptref.virtual_word(s, cut, n) == (n + 63) // 64),
        "N is no multiple of 64": sc.n % 64})


def cut_is_last_node() -> Scene:
    n, s0 = 300, 10
    offs = np.concatenate([np.arange(0, 288, 2), [289]])
    return build("cut_is_last_node", kinds_at(n, s0, large=offs), "sb", 24, s0, lambda sc: {
        "cuts on node N - 1": _count(sc, lambda s, cut, ok, n: cut >= 0 and (s + cut) % n == n - 1),
        "N is no multiple of 64": sc.n % 64})


def kept_twice_guard() -> Scene:
    """Word 2 (nodes 128..191) all roomy round the start 150: five small nodes
    130..134, 59 large; 85 more large nodes elsewhere.  Big pods see exactly
    K = 144 nodes (no cut; counting nodes 150..191 again finds one), small pods
    149 (a cut at node 145, which dropping nodes 128..149 after the wrap loses)."""
    n, s0 = 300, 150
    kinds = np.full(n, FULL)
    kinds[128:192] = LARGE
    kinds[130:135] = SMALL
    rest = np.concatenate([np.arange(0, 128), np.arange(192, 300)])
    kinds[rest[::2][:85]] = LARGE

    def dense(s, cut, ok, n):
        w0 = (s >> 6) * 64
        return ok[s:min(w0 + 64, n)].sum() >= 8 and ok[w0:s].sum() >= 8
    return build("kept_twice_guard", kinds, "bs", 30, s0, lambda sc: {
        "starts with 8 or more feasible nodes on either side in their word": _count(sc, dense),
        "big pods see exactly K": int(sc.masks[0].sum() == sc.k),
        "small pods see more": int(sc.masks[1].sum() > sc.k)})


def _flip_scene(name, idx, free, n_pods, claims) -> Scene:
    """200 large nodes of 300 from node 40 on; the node at feasible rank idx
    from the start has ``free`` pod slots and no load, so the first pods whose
    window holds it bind there.  With 200 feasible nodes and K = 144, pod 0
    keeps ranks 0..143, pod 1 ranks 144..199 and 0..87 with its cut at rank
    88, pod 2 ranks 88..199 and 0..31."""
    n, s0 = 300, 40
    offs = np.sort(np.arange(200) * 3 // 2)        # 200 distinct offsets below 300
    x = int((s0 + offs[idx]) % n)
    sc = build(name, kinds_at(n, s0, large=offs), "s", n_pods, s0, claims, slots={x: free}, flips=True)
    sc.x = x
    return sc


def _trace(sc):
    return adaptref.schedule(sc.cluster, sc.pods, compiled(sc.pct), next_start=sc.s0, trace=True)


def flip_inside_window() -> Scene:
    def claims(sc):
        chosen, cols, _, _, rows = _trace(sc)
        return {"pod 0 fills the node": int(chosen[0] == sc.x and cols["num_pods"][sc.x] == 110),
                "later pods whose S0 window keeps it": sum(r[2] for r in rows)}
    return _flip_scene("flip_inside_window", 20, 1, 6, claims)


def flip_on_cut_node() -> Scene:
    """Two pods: the second's S0 cut is the node the first fills.  (A longer
    queue heals a window kept on that cut: the next pod starts on the filled
    node and skips it, so only the run's last start and evals tell.)"""
    def claims(sc):
        chosen, _, _, _, rows = _trace(sc)
        return {"pod 0 fills the node": int(chosen[0] == sc.x),
                "pods whose S0 cut is the filled node, nothing else flipped before it": sum(
                    1 for r in rows if r[3] and not r[2])}
    return _flip_scene("flip_on_cut_node", 88, 1, 2, claims)


def flip_past_cut() -> Scene:
    def claims(sc):
        chosen, _, _, _, rows = _trace(sc)
        return {"pod 0 fills the node": int(chosen[0] == sc.x), "flips past a cut": sum(r[4] for r in rows),
                "and none at or before one": int(sum(r[2] + r[3] for r in rows) == 0)}
    return _flip_scene("flip_past_cut", 100, 1, 2, claims)


def two_binders_one_node() -> Scene:
    def claims(sc):
        chosen, cols, _, _, rows = _trace(sc)
        return {"pods 0 and 1 bind the node and fill it": int(chosen[0] == sc.x and chosen[1] == sc.x and
                                                              cols["num_pods"][sc.x] == 110),
                "pod 2's S0 window keeps it": rows[2][2]}
    return _flip_scene("two_binders_one_node", 20, 2, 6, claims)


def slow_relaxation() -> Scene:
    """400 nodes, K = 100 (percentageOfNodesToScore 25): nodes 0..199 large and
    small alternating, nodes 200..399 large and full alternating.  Small pods
    see the first half dense and the second half every other node, big pods
    every other node everywhere, so a guessed start that lands in the wrong
    half is off by up to a window.  A deferred-commit batch commits at most the
    prefix the relaxation makes exact, so the run takes at least relax_batches
    batches.  (256 pods touch most of the 300 roomy nodes, so a later pod's
    eight candidates can all be taken and batches also end on that:
    slow_relaxation_4000 is the same ring ten times as long, where they do not.)"""
    return _slow("slow_relaxation", 400, 25)


def slow_relaxation_4000() -> Scene:
    """slow_relaxation's halves on 4,000 nodes, K = 100 still
    (percentageOfNodesToScore 2).  Few nodes of a window are touched, so no
    pair cut and no exhausted list ends a batch: a deferred-commit batch commits
    exactly the prefix the relaxation makes exact (relax_batches: three batches)
    and the doubling form the whole queue in one."""
    return _slow("slow_relaxation_4000", 4000, 2)


def _slow(name, n, pct) -> Scene:
    s0 = 37
    i = np.arange(n)
    kinds = np.where(i % 2 == 0, LARGE, np.where(i < n // 2, SMALL, FULL))
    return build(name, kinds, "ssbsbbsb", 256, s0, lambda sc: {
        "pods the relaxation leaves inexact after its rounds": 256 - adaptref.relax(sc.masks, sc.s0, sc.k,
                                                                                    K_WINDOW_ROUNDS),
        "batches past the one a whole commit takes": relax_batches(sc) - 1,
        "no bind fills a node": int(sum(r[2] + r[3] + r[4] for r in _trace(sc)[4]) == 0)}, pct=pct,
        level=True, sizes=LEVEL_SIZES)


TAILS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257)


TAILS_N = 2000


def batch_tails(q: int) -> Scene:
    """q pods that request nothing on a level ring of 2,000 nodes, nine in ten
    small-roomy, K = 680.  No bit flips and no pair cut ends a batch, so the
    window of every pod of the batch reaches the placements: the run takes
    ceil(q / 256) batches where the windows are exact for the whole batch
    (whole_batches), and a wrong window of any pod shows."""
    i = np.arange(TAILS_N)
    kinds = np.where(i % 10 == 3, FULL, SMALL)
    return build(f"batch_tails_{q}", kinds, "s", q, 1977, lambda sc: {
        "pods": sc.pods.n_pods, "windows that wrap": _count(sc, _wrapped) + int(q < 3),
        "no bind fills a node": int(sum(r[2] + r[3] + r[4] for r in _trace(sc)[4]) == 0)}, level=True)


# ---- the doubling form's limits ------------------------------------------------------------
def doubling(n: int) -> Scene:
    """Every fifth node roomy (large and small alternating), the start 200
    nodes before the end: K = 409 feasible nodes span 2,045 nodes, so a window
    in four wraps.  A level ring: the batches commit whole (whole_batches), so
    the tables' entries of the pods past the first 64 reach the placements."""
    i = np.arange(n)
    kinds = np.where(i % 10 == 0, LARGE, np.where(i % 5 == 0, SMALL, FULL))
    forms = {"fast": "fused", "generic": "doubling" if n <= 8192 else "fused"}
    return build(f"doubling_{n}", kinds, "ssb", 260, n - 200, lambda sc: {
        "windows that wrap": _count(sc, _wrapped), "bitmap words": (sc.n + 63) // 64}, forms=forms,
        level=True, sizes=LEVEL_SIZES)


# ---- k_adapt_cut0 ----------------------------------------------------------------------------
CUT0_PODS = 132                                    # 33 of k_adapt_cut0's four-pod blocks


def _cut0_forms(n: int) -> dict:
    return {"fast": "fused", "generic": "fused"} if n <= 16384 else {"fast": "cut0_top", "generic": "cut0_window"}


def _guess_words(sc):
    """The virtual word of every first-round cut (adaptref.guesses; -1: no cut)."""
    return [adaptref.virtual_word(s, cut, sc.n) if cut >= 0 else -1
            for s, cut in adaptref.guesses(sc.masks, sc.s0, sc.k)]


def cut0_counts(n: int) -> Scene:
    """K large nodes and one small: "s" pods see K + 1 nodes, "b" pods K, "h"
    pods none; the start is bit 0 of word 5 and pod 0 a "b" pod."""
    k = profile.num_feasible_nodes_to_find(n, 0)
    offs = spaced(k, n - 64, 64)
    return build(f"cut0_counts_{n}", kinds_at(n, 0, large=offs, small=[7]), "bshsb", CUT0_PODS, 320, lambda sc: {
        "pods with K + 1, K and no feasible nodes": int(sorted(set(sc.masks.sum(1).tolist())) == [0, sc.k, sc.k + 1]),
        "pods with none between two that have some": sum(
            1 for j in range(1, CUT0_PODS - 1)
            if not sc.masks[j].any() and sc.masks[j - 1].any() and sc.masks[j + 1].any()),
        "the start is bit 0 of its word": int(sc.s0 % 64 == 0),
        # ... so the wrapped word is masked to nothing: counting any of its bits again would give pod 0 a cut
        "pod 0 sees exactly K nodes from there and has no cut": int(
            sc.masks[0].sum() == sc.k and adaptref.guesses(sc.masks, sc.s0, sc.k)[0] == (sc.s0, -1)),
        "feasible nodes of pod 0 in the start's word": int(sc.masks[0][sc.s0:sc.s0 + 64].sum()),
        "first-round scans that reach the word after the last": sum(1 for v in _guess_words(sc) if v == -1)},
        forms=_cut0_forms(n))


def cut0_step_edge(n: int, v: int) -> Scene:
    """From bit 0 of word 5: K large nodes six apart (all before virtual word
    127), the next one in virtual word v = 127 (lane 63's second word of the
    first 128-word step) or 128 (the first word of the next step), then large
    nodes six apart for the later pods."""
    k = profile.num_feasible_nodes_to_find(n, 0)
    s0 = 320
    assert 6 * k < 127 * 64
    offs = np.concatenate([np.arange(k) * 6, [v * 64 + 5], np.arange(129 * 64, n - 64, 6)])
    return build(f"cut0_v{v}_{n}", kinds_at(n, s0, large=offs), "sb", CUT0_PODS, s0, lambda sc: {
        f"first-round cuts in virtual word {v}": sum(1 for x in _guess_words(sc) if x == v),
        "pod 0's among them": int(_guess_words(sc)[0] == v)}, forms=_cut0_forms(n))


def cut0_wrapped(n: int) -> Scene:
    """From bit 40 of word 5: K large nodes over the offsets before the start's
    word comes round again, then nodes 323..359 of that word (below the start)."""
    k = profile.num_feasible_nodes_to_find(n, 0)
    s0 = 360
    offs = np.concatenate([spaced(k, n - 40), np.arange(n - 37, n)])
    nw = (n + 63) // 64
    return build(f"cut0_wrapped_{n}", kinds_at(n, s0, large=offs), "sb", CUT0_PODS, s0, lambda sc: {
        "first-round cuts in virtual word n_words": sum(1 for x in _guess_words(sc) if x == nw),
        "pod 0's among them": int(_guess_words(sc)[0] == nw)}, forms=_cut0_forms(n))


def cut0_dense(n: int) -> Scene:
    """Every node roomy but one in 97: the cut 820 or 1,229 nodes from the
    start, in the earliest lane of the first step that can hold one."""
    i = np.arange(n)
    kinds = np.where(i % 97 == 0, FULL, np.where(i % 2 == 0, LARGE, SMALL))
    return build(f"cut0_dense_{n}", kinds, "s", CUT0_PODS, 320, lambda sc: {
        "first-round cuts in the first step": int(all(0 < x < 128 for x in _guess_words(sc))),
        "the earliest": int(min(x for x in _guess_words(sc) if x >= 0) == sc.k // 64)}, forms=_cut0_forms(n))


# ---- K = 4095 / 4096 --------------------------------------------------------------------------
def wide_top(n: int) -> Scene:
    i = np.arange(n)
    kinds = np.where(i % 97 == 0, FULL, np.where(i % 2 == 0, LARGE, SMALL))
    k = profile.num_feasible_nodes_to_find(n, 50)
    forms = {"fast": "fused" if k < K_TOP_WIDE_K else "cut0_top", "generic": "doubling"}
    return build(f"wide_top_{n}", kinds, "ssb", 260, n - 1000, lambda sc: {
        "K": int(sc.k == sc.n // 2), "windows that wrap": _count(sc, _wrapped),
        "threads per pod": top_threads(sc.n, sc.k, True, True)}, pct=50, forms=forms)


# ---- the kept-list forms of the static-class FAST keys ----------------------------------------
def list_form(kend: int, kept: int, nt: int) -> str:
    """Which loop of k_adapt_top's static-class FAST keys a window takes."""
    if kend <= 2 * nt:
        return "stepping"
    return "one_per_thread" if kept <= nt else "list" if kept <= K_ADAPT_LIST else "fallback"


def _selector_scene(name, n, pct, n_pods, full, want) -> Scene:
    """gen.bare_cluster's nodes (all roomy but ``full``), two pod sizes, every
    third pod with a zone selector: not trivial, so the run takes the generic
    launch with the static-class table, and the cluster is narrow, so its FAST
    keys.  The pods are too few to fill a node: the bitmaps are the roomy
    nodes, of the pod's zone where it selects one."""
    c = gen.bare_cluster(n, SEED + 1)
    c.num_pods[full] = c.alloc_pods[full]
    assert fastcases.is_narrow(c)
    order = np.arange(n_pods) % 2
    pods = fastcases.with_zone_selector(make_pods([requesting(100, 128 * MI), requesting(200, 256 * MI)], order))
    roomy = c.num_pods < c.alloc_pods
    zone = np.arange(n) % 3
    masks = np.array([roomy & (zone == (j // 3) % 3) if j % 3 == 0 else roomy for j in range(n_pods)])
    k = profile.num_feasible_nodes_to_find(n, pct)
    form = window_form(n, k, False, False, False)
    nt = top_threads(n, k, False, False)

    def claims(sc):
        seen: Dict[str, int] = {f: 0 for f in want}
        for (s, cut), ok in zip(sc.windows()[0], sc.masks):
            kend = cut if cut >= 0 else sc.n
            f = list_form(kend, min(int(ok.sum()), sc.k), nt)
            seen[f] = seen.get(f, 0) + 1
        assert set(seen) == set(want), (sc.name, seen)
        seen["windows that wrap"] = _count(sc, _wrapped)
        # a window that comes all the way round (no cut): word_range clips the start's word twice,
        # to the nodes from the start on in piece 1 and to those below it in piece 2
        seen["windows whose two pieces both hold the start's word"] = _count(
            sc, lambda s, cut, ok, n: cut < 0 and s % 64 != 0 and list_form(n, int(ok.sum()), nt) != "stepping")
        return seen
    return Scene(name, c, pods, n - 100, pct, bare=False, masks=masks, claims=claims, forms={"static": form})


def list_short() -> Scene:
    """K = 246 of 8,200; zone z2 is full but for its first 200 nodes.  Plain
    pods' windows are about 360 nodes long (the stepping loop), z0 / z1 pods'
    about 740 with 246 kept and z2 pods' the whole ring with 200 kept (one kept
    node per thread)."""
    return _selector_scene("list_short", 8200, 3, 90, np.arange(2, 8200, 3)[200:], ("stepping", "one_per_thread"))


def list_mid() -> Scene:
    """K = 820 of 8,200; zone z2 is full but for its first 600 nodes.  Every
    window is longer than 512 nodes, with 820 kept or (z2 pods, the whole
    ring) 600: the LDS list."""
    return _selector_scene("list_mid", 8200, 10, 90, np.arange(2, 8200, 3)[600:], ("list",))


def list_wide() -> Scene:
    """K = 4,500 of 10,000, a 1,024-thread top.  Zone z2 is full but for its
    first 900 nodes: plain pods keep 4,500 nodes (past the list: the
    fallback), z0 / z1 pods all 3,333 of their zone, z2 pods 900 (one per
    thread of 1,024)."""
    n = 10000
    z2 = np.arange(2, n, 3)
    return _selector_scene("list_wide", n, 45, 60, z2[900:], ("fallback", "list", "one_per_thread"))


def norm_varies(cluster, pods) -> np.ndarray:
    """Per pod what csrc/ksim_engine.cpp's pod_batchable calls ``varies`` under
    the default profile: a preferred node affinity term (NodeAffinity's raw
    score differs by node) or a PreferNoSchedule taint of the cluster the pod
    does not tolerate (TaintToleration's does)."""
    from ksim import abi
    p = pods.pods
    out = p["pref_term_count"] > 0
    for t in range(1, len(cluster.taint_effect)):
        if cluster.taint_effect[t] == abi.EFFECT_PREFER_NO_SCHEDULE:
            out = out | (((p["tol_prefer"][:, t >> 6] >> np.uint64(t & 63)) & np.uint64(1)) == 0)
    return out


def list_normv() -> Scene:
    """gen.config1's nodes and pods at 8,200 nodes, K = 820: taints, pools,
    preferred node affinity, PreferNoSchedule taints: static classes whose
    normalized scores vary over the nodes (kPodNormVaries)."""
    c, pods = gen.config1(n_nodes=8200, n_pods=120)
    assert fastcases.is_narrow(c)
    return Scene("list_normv", c, pods, 8100, 10, bare=False, forms={"static": "fused"}, claims=lambda sc: {
        "pods whose normalized scores vary (kPodNormVaries)": int(norm_varies(sc.cluster, sc.pods).sum()),
        "pods with preferred node affinity terms": int((sc.pods.pods["pref_term_count"] > 0).sum()),
        "pods with a selector or required affinity": int(((sc.pods.pods["sel_count"] > 0) |
                                                          (sc.pods.pods["req_term_count"] > 0)).sum())})


# ---- node shards ----------------------------------------------------------------------------------
SHARD_N = 600            # K = 276; two shards of 320 + 280 nodes, three of 256 + 256 + 88 (ksim.shard.partition)


def _regions(n, roomy) -> np.ndarray:
    """The roomy nodes small below node 330 and large from there on: big pods
    keep no node of the first shard of two or three."""
    kinds = np.full(n, FULL)
    roomy = np.asarray(roomy)
    kinds[roomy] = np.where(roomy < 330, SMALL, LARGE)
    return kinds


def shard_geometry(sc: Scene, world: int) -> Dict[str, int]:
    """What the issue asks of the sharded runs, over the scene's windows: a
    window that spans a shard boundary and wraps, a shard without a kept node
    for some pod, and with three shards a shorter last one."""
    from ksim.shard import partition
    parts = partition(sc.n, world)
    spans = empty = 0
    rows = adaptref.reference(sc.cluster, sc.pods, compiled(sc.pct), next_start=sc.s0)[4] if sc.flips \
        else sc.windows()[0]
    for (s, cut), ok in zip(rows, sc.masks):
        kend = cut if cut >= 0 else sc.n
        inside = np.zeros(sc.n, bool)
        inside[(s + np.arange(kend)) % sc.n] = True
        crossed = any(inside[b - 1] and inside[b] for b, _ in parts[1:])
        spans += int(crossed and s + kend > sc.n)
        empty += int(any(not (inside & ok)[b:b + c].any() for b, c in parts))
    return {"aligned shards": int(all(b % 64 == 0 for b, _ in parts)),
            "windows that span a shard boundary and wrap": spans, "pods with no kept node on some shard": empty,
            "last shard shorter": int(parts[-1][1] < parts[0][1])}


def shard_cut_in_wrapped_half() -> Scene:
    """cut_in_wrapped_half on 600 nodes from node 470: 272 roomy nodes on even
    offsets, then nodes 448..469 (the start's word below the start) all large:
    a small pod's 277th feasible node is node 452; a big pod sees 129 nodes,
    all from node 330 on."""
    n, s0 = SHARD_N, 470
    offs = np.concatenate([np.arange(0, 578, 2)[:272], np.arange(578, 600)])
    return build("shard_cut_in_wrapped_half", _regions(n, (s0 + offs) % n), "sb", 24, s0, lambda sc: {
        "cuts in the start's own word below the start": _count(
            sc, lambda s, cut, ok, n: cut >= 0 and adaptref.virtual_word(s, cut, n) == (n + 63) // 64),
        "pod 0's among them": int(adaptref.virtual_word(sc.s0, sc.windows()[0][0][1], sc.n) == 10)})


def shard_exactly_k_plus_1() -> Scene:
    n, s0 = SHARD_N, 191
    roomy = np.concatenate([spaced(177, 330), spaced(100, 270, 330)])
    return build("shard_exactly_k_plus_1", _regions(n, roomy), "sb", 24, s0, lambda sc: {
        "small pods with exactly K + 1 feasible nodes": int((sc.masks[0::2].sum(1) == sc.k + 1).all()),
        "big pods with fewer than K": int((sc.masks[1::2].sum(1) < sc.k).all())})


def shard_flip_on_cut_node() -> Scene:
    """flip_on_cut_node on 600 nodes: 400 roomy nodes, K = 276, so pod 1 starts
    at rank 276 and its S0 cut is rank 152, the node pod 0 fills."""
    n, s0 = SHARD_N, 100
    offs = spaced(400, n)
    x = int((s0 + offs[152]) % n)

    def claims(sc):
        chosen, _, _, _, rows = _trace(sc)
        return {"pod 0 fills the node": int(chosen[0] == x),
                "pods whose S0 cut is the filled node, nothing else flipped before it": sum(
                    1 for r in rows if r[3] and not r[2])}
    return build("shard_flip_on_cut_node", _regions(n, (s0 + offs) % n), "s", 2, s0, claims, slots={x: 1}, flips=True)


# ---- the registry -------------------------------------------------------------------------------
SMALL_RING = (ring101_exactly_k, ring101_all_feasible, exactly_k, exactly_k_plus_1, none_feasible, start_bit0, start_bit63, start_last_node,
              start_on_infeasible, cut_in_wrapped_half, cut_is_last_node, kept_twice_guard, flip_inside_window,
              flip_on_cut_node, flip_past_cut, two_binders_one_node, slow_relaxation)
CUT0_NODES = (16384, 16385, 24576, 24577)

SCENES: Dict[str, Callable[[], Scene]] = {f.__name__: f for f in SMALL_RING}
SCENES.update({f.__name__: f for f in (shard_cut_in_wrapped_half, shard_exactly_k_plus_1, shard_flip_on_cut_node)})
SCENES["slow_relaxation_4000"] = slow_relaxation_4000
SCENES.update({f"batch_tails_{q}": functools.partial(batch_tails, q) for q in TAILS})
SCENES.update({f"doubling_{n}": functools.partial(doubling, n) for n in (8185, 8192, 8193)})
for _n in CUT0_NODES:                              # every property on 257 and 385 words, fewer on 256 and 384
    SCENES[f"cut0_counts_{_n}"] = functools.partial(cut0_counts, _n)
    SCENES[f"cut0_wrapped_{_n}"] = functools.partial(cut0_wrapped, _n)
    if _n != 16384:
        SCENES[f"cut0_v128_{_n}"] = functools.partial(cut0_step_edge, _n, 128)
    if _n % 64:
        SCENES[f"cut0_v127_{_n}"] = functools.partial(cut0_step_edge, _n, 127)
        SCENES[f"cut0_dense_{_n}"] = functools.partial(cut0_dense, _n)
SCENES.update({f"wide_top_{n}": functools.partial(wide_top, n) for n in (8190, 8192)})
SCENES.update({f.__name__: f for f in (list_short, list_mid, list_wide, list_normv)})

BARE = [n for n in SCENES if not n.startswith("list_")]
STATIC = [n for n in SCENES if n.startswith("list_")]
# the scenes the wrong readings are tried on (the small rings: a reading costs a whole run per scene)
FAULT_SCENES = [f.__name__ for f in SMALL_RING]
# (scene, shards): in-process node-shard groups
SHARDED = [(name, world) for name in ("shard_cut_in_wrapped_half", "shard_exactly_k_plus_1",
                                      "shard_flip_on_cut_node", "cut0_wrapped_16385") for world in (2, 3)]


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    """The scene, built once; tests take shaped() copies of its cluster."""
    return SCENES[name]()
