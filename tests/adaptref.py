"""The ADAPT scan windows in plain numpy, with no cleverness: the model that
tests/adaptcases.py states its scenes' properties over, and the windowed
sequential scheduler whose wrong readings tests/test_adapt_cases.py tells
apart.

  windows(masks, s0, k)       the serial (start, cut) per pod and the final
                              start.  Pod j scans the ring from its start,
                              keeps the first k feasible nodes and stops at
                              the (k + 1)-th: cut is that node's offset from
                              the start (-1: at most k feasible nodes, all n
                              processed).  The next pod starts at start +
                              processed.
  relax(masks, s0, k, rounds) the guess-and-prefix-sum relaxation restated
                              (csrc/ksim_adapt.hip window_block): guess
                              s_j = s0 + j k, find every cut, re-derive the
                              starts as the prefix sum of the processed
                              counts, repeat; returns how many pods are exact
                              after ``rounds`` rounds.
  reference(...)              tests/fastref.py's schedule with the windows of
                              its cycles and the evaluated nodes summed.
  schedule(...)               tests/fastref.py's cycle (the same scores, keys
                              and binds) with the window spelled out, the
                              evaluated nodes (the processed ones and the cut
                              node) summed into ``evals``, and one
                              wrong reading of the window switched on by
                              ``window_fault`` (FAULTS).

Readings 9 to 11 speak of a batch: the engine computes a batch's bitmaps
under the state S0 the batch starts from.  The model's batches are the
queue's consecutive chunks of BATCH pods (the scenes that flip a bit hold at
most BATCH pods, so S0 is the scene's starting state)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ksim import profile
from oracle.shard_model import tb_keys

import fastref

BATCH = 256                                        # csrc/ksim_internal.h kBatchPods

FAULTS = (
    "cut_is_kth",               # 1: the cut is the K-th feasible node
    "k_plus_1_no_cut",          # 2: exactly K + 1 feasible nodes read as no cut
    "wrapped_low_bits_dropped", # 3: after the wrap the start's word below the start is dropped
    "wrapped_high_bits_twice",  # 4: after the wrap the start's word from the start on counts again
    "wrap_by_words",            # 5: offsets after the wrap from 64 * n_words, not n
    "start_plus_k",             # 6: the next start is the start plus K
    "short_pod_advances",       # 7: a pod with at most K feasible nodes advances the start
    "empty_pod_not_counted",    # 8: a pod with no feasible node leaves evals alone
    "stale_window",             # 9: the S0 window kept although a kept node was filled in the batch
    "stale_cut_node",           # 10: the same for the cut node (the off == cut clause)
    "binders_tested_alone",     # 11: two earlier binds on one node each tested alone
    "best_k_of_ring",           # 12: the kept set is the K best feasible nodes of the ring
)


def offsets(ok: np.ndarray, s: int) -> np.ndarray:
    """The feasible nodes' offsets from s in ring order."""
    n = ok.size
    return np.nonzero(ok[(np.arange(n) + s) % n])[0]


def window(ok: np.ndarray, s: int, k: int):
    """(cut, processed) of one pod: cut -1 and processed n without a (k + 1)-th feasible node."""
    fo = offsets(ok, s)
    if fo.size > k:
        return int(fo[k]), int(fo[k])
    return -1, ok.size


def windows(masks: np.ndarray, s0: int, k: int):
    """([(start, cut)] per pod, final start) of the serial scan over fixed bitmaps."""
    n = masks.shape[1]
    out, s = [], s0
    for ok in masks:
        cut, processed = window(ok, s, k)
        out.append((s, cut))
        s = (s + processed) % n
    return out, s


def guesses(masks: np.ndarray, s0: int, k: int):
    """The relaxation's first round: [(start, cut)] from the guessed starts s0 + j k."""
    n = masks.shape[1]
    return [((s0 + j * k) % n, window(ok, (s0 + j * k) % n, k)[0]) for j, ok in enumerate(masks)]


def relax(masks: np.ndarray, s0: int, k: int, rounds: int) -> int:
    """Pods with exact windows after ``rounds`` rounds of the relaxation."""
    nb, n = masks.shape
    s = [(s0 + j * k) % n for j in range(nb)]
    exact = 0
    for _ in range(rounds):
        proc = [window(masks[j], s[j], k)[1] for j in range(nb)]
        before = np.concatenate([[0], np.cumsum(proc)[:-1]])
        ns = [int((s0 + before[j]) % n) for j in range(nb)]
        changed = [j for j in range(nb) if ns[j] != s[j]]
        if not changed:
            return nb
        exact = changed[0]                         # pods before the first changed start: start and cut exact
        for j in range(exact, nb):
            s[j] = ns[j]
    return exact


def virtual_word(s: int, cut: int, n: int) -> int:
    """k_adapt_cut0's virtual word of the cut node: word (s >> 6) + v mod n_words,
    v = n_words for the bits of the start's own word below the start."""
    nw = (n + 63) // 64
    node = (s + cut) % n
    v = ((node >> 6) - (s >> 6)) % nw
    return nw if v == 0 and node < s else v


def _faulty_window(ok, s, k, fault):
    """(kept nodes, cut, processed, next start) under one reading of readings 1 to 8."""
    n = ok.size
    fo = offsets(ok, s)
    nodes = (fo + s) % n
    if fault == "wrapped_low_bits_dropped":
        keep = ~((nodes < s) & (nodes >= (s >> 6) * 64))
        fo, nodes = fo[keep], nodes[keep]
    elif fault == "wrapped_high_bits_twice":
        again = fo[fo < min((s >> 6) * 64 + 64, n) - s]
        fo = np.concatenate([fo, again + n])
        nodes = (fo + s) % n
    elif fault == "wrap_by_words":
        fo = np.where(nodes < s, nodes + 64 * ((n + 63) // 64) - s, fo)
    kk = k - 1 if fault == "cut_is_kth" else k
    has_cut = fo.size > kk + 1 if fault == "k_plus_1_no_cut" else fo.size > kk
    if has_cut:
        cut = processed = int(fo[kk])
        kept = nodes[:kk]
    else:
        cut, processed, kept = -1, n, nodes
    step = processed
    if fault == "start_plus_k" and has_cut:
        step = k
    if fault == "short_pod_advances" and not has_cut and fo.size:
        step = int(fo[-1]) + 1
    return np.unique(kept), cut, processed, (s + step) % n


def schedule(cluster, pods, prof, next_start: int = 0, window_fault: Optional[str] = None, seq0: int = 0,
             trace: bool = False):
    """The sequential scheduler with the scan window spelled out.  Returns
    (placements, node columns, next_start, evals, per-pod trace); the trace
    holds (start, cut, flips inside the S0 window, flip on the S0 cut node,
    flips past the S0 cut) when ``trace``."""
    assert window_fault is None or window_fault in FAULTS
    w = fastref.weights(prof)
    c = fastref.columns(cluster)
    n = c["alloc_cpu"].size
    k = profile.num_feasible_nodes_to_find(n, w["pct"])
    chosen = np.full(pods.n_pods, -1, np.int32)
    evals, rows = 0, []
    fields = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem")
    for j in range(pods.n_pods):
        p = pods.pods[j]
        if j % BATCH == 0:                          # a batch's S0, and what one earlier pod alone bound per node
            c0 = {f: v.copy() for f, v in c.items()}
            single = {f: np.zeros(n, np.int64) for f in fields}
            bound = np.zeros(n, bool)
        ok, _, _, total = fastref.node_scores(c, p, w)
        s = next_start
        view = ok
        if window_fault in ("stale_window", "stale_cut_node") or trace:
            ok0 = fastref.fit_ok(c0, p) if w["has_fit"] else np.ones(n, bool)
            cut0, _ = window(ok0, s, k)
            flipped = ((np.nonzero(ok0 & ~ok)[0] - s) % n)
            end0 = cut0 if cut0 >= 0 else n
            inside, on_cut = int((flipped < end0).sum()), int((flipped == cut0).sum())
            past = int(flipped.size - inside - on_cut)
            if window_fault == "stale_window" or (window_fault == "stale_cut_node" and on_cut and not inside):
                view = ok0                          # the span of the S0 window; the kept nodes still have to fit
            if trace:
                rows.append((s, window(ok, s, k)[0], inside, on_cut, past))
        if window_fault == "binders_tested_alone":
            alone = {f: c0[f] + single[f] if f in single else c0[f] for f in c0}
            alone["num_pods"] = c0["num_pods"] + bound
            view = fastref.fit_ok(alone, p) if w["has_fit"] else ok
        kept, cut, processed, nxt = _faulty_window(view, s, k, window_fault)
        if window_fault == "best_k_of_ring":
            kept = np.nonzero(ok)[0]
            if kept.size > k:
                lo = tb_keys(np.zeros(kept.size, np.int64), w["seed"], seq0 + j, kept)
                kept = kept[np.lexsort((lo, total[kept]))[-k:]]
        kept = kept[ok[kept]]
        if not (window_fault == "empty_pod_not_counted" and not ok.any()):
            evals += processed + (1 if cut >= 0 else 0)   # the cut node is evaluated too
        next_start = nxt
        pick = -1
        if kept.size == 1:
            pick = int(kept[0])
        elif kept.size > 1:
            lo = tb_keys(np.zeros(kept.size, np.int64), w["seed"], seq0 + j, kept)
            pick = int(kept[np.lexsort((lo, total[kept]))[-1]])
        chosen[j] = pick
        if pick >= 0:
            for f in fields:
                c[f][pick] += int(p[f])
                single[f][pick] = max(single[f][pick], int(p[f]))
            c["num_pods"][pick] += 1
            bound[pick] = True
    return chosen, c, next_start, evals, rows


def reference(cluster, pods, prof, next_start: int = 0, seq0: int = 0):
    """fastref.schedule's own run with the windows read off its cycles:
    (placements, node columns, next_start, evals, [(start, cut)] per pod)."""
    k = profile.num_feasible_nodes_to_find(cluster.n_nodes, fastref.weights(prof)["pct"])
    chosen, cols, last, cycles = fastref.schedule(cluster, pods, prof, next_start=next_start, seq0=seq0, trace=True)
    rows, evals, s = [], 0, next_start
    for _, ok, _, _ in cycles:
        cut, processed = window(ok, s, k)
        rows.append((s, cut))
        evals += processed + (1 if cut >= 0 else 0)
        s = (s + processed) % ok.size
    assert s == last
    return chosen, cols, last, evals, rows


def masks_of(cluster, pods, prof) -> np.ndarray:
    """Every pod's Fit bitmap under the cluster's state (bool, pods x nodes)."""
    w = fastref.weights(prof)
    c = fastref.columns(cluster)
    n = c["alloc_cpu"].size
    return np.array([fastref.fit_ok(c, p) if w["has_fit"] else np.ones(n, bool) for p in pods.pods])
