"""NodeResourcesFit and NodeResourcesBalancedAllocation for trivial pods, in
plain numpy int64 / float64: the reference of tests/test_gpu_fast_edges.py,
pinned by tests/test_fast_ref.py to the C oracle per scored node and cycle.

It restates what upstream computes (v1.26, from memory), not the engine's FAST
functions: no reciprocal, no correction step, no branch-free selects.

  fitsRequest                  the pod count first; a pod that requests nothing
                               (cpu, memory and ephemeral-storage all 0) is
                               checked against nothing else;
  leastRequestedScore          0 for a capacity of 0 or a request above it,
                               else (capacity - requested) * 100 / capacity in
                               integers, over the non-zero requests;
  leastResourceScorer          the weighted mean, in integers, over the
                               resources whose allocatable is not 0;
  balancedResourceScorer       float64 fractions of the requests, clamped at
                               1, over the resources whose allocatable is not
                               0; with two of them 1 - |f0 - f1| / 2, with one
                               1; times 100, truncated;
  prioritizeNodes / selectHost the weighted total, and the engine's stand-in
                               for the reservoir (oracle/shard_model.tb_keys).

A trivial pod passes every other filter, and every other score plugin gives it
the same normalized score on every node, so neither moves a pick.

``fault`` switches on one wrong reading of that arithmetic an implementation
could have (FAULTS), for the test that the scenes of tests/fastcases.py tell
each from the reference."""
from __future__ import annotations

from fractions import Fraction
from typing import Optional

import numpy as np

from ksim import abi, profile
from oracle.shard_model import tb_keys

FAULTS = ("uncorrected_quotient",       # trunc(n * RN(1 / d)), no residual step
          "round_to_nearest",           # a quotient rounded, not truncated
          "la_from_req",                # LeastAllocated over the requests, not the non-zero requests
          "ba_from_nz",                 # BalancedAllocation over the non-zero requests
          "no_clamp",                   # a fraction above 1 kept
          "ba_float32",                 # BalancedAllocation in float32
          "fit_checks_zero_request",    # a pod that requests nothing checked against cpu / memory / storage
          "pods_le",                    # num_pods <= alloc_pods
          "zero_alloc_averaged",        # an allocatable of 0 scores 0 and its weight still divides
          "overdrawn_not_zeroed",       # a request above the capacity keeps its (negative) quotient
          "missing_resource_not_100",   # BalancedAllocation with one resource: the other's fraction read as 0
          "mean_by_weight_sum",         # one resource present: its score times its weight over both weights
          "score_6bit",                 # scores kept in 6 bits: 64..100 wrap
          "stale_reciprocal")           # the quotient from RN(1 / d') of the allocatable d' the node had before

MAX_SCORE = 100


def weights(prof: abi.Profile) -> dict:
    """What the restatement reads of a compiled profile."""
    w = {"fit": 0, "ba": 0, "has_fit": False, "n_score": prof.n_score, "seed": int(prof.tiebreak_seed),
         "pct": int(prof.percentage_of_nodes_to_score)}
    for k in range(prof.n_score):
        name = abi.PLUGINS[prof.score[k]]
        if name == "NodeResourcesFit":
            w["fit"] += prof.score_weight[k] or 1
        if name == "NodeResourcesBalancedAllocation":
            w["ba"] += prof.score_weight[k] or 1
    w["has_fit"] = any(abi.PLUGINS[prof.filter[k]] == "NodeResourcesFit" for k in range(prof.n_filter))
    res = {int(prof.fit_res[i]): int(prof.fit_res_weight[i]) for i in range(prof.fit_n_res)}
    assert sorted(res) == [0, 1] and prof.ba_n_res == 2, "the restatement covers the {cpu, memory} strategies"
    w["cpu"], w["mem"] = res[0], res[1]
    return w


def _fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # one rounding


def _stale_quotient(n: int, d: int, d_prev: int) -> int:
    """The engine's three-operation quotient with the reciprocal of d_prev."""
    y = 1.0 / float(d_prev) if d_prev else 0.0
    q0 = float(n) * y
    return int(_fma(_fma(-q0, float(d), float(n)), y, q0))


def _quotient(n: np.ndarray, d: np.ndarray, fault: Optional[str], d_prev: Optional[np.ndarray]) -> np.ndarray:
    """n / d truncated, n >= 0 and d > 0 where it counts (d == 0 gives 0)."""
    ds = np.where(d == 0, 1, d)
    q = n // ds
    if fault == "uncorrected_quotient":
        q = np.trunc(n.astype(np.float64) * (1.0 / ds.astype(np.float64))).astype(np.int64)
    elif fault == "round_to_nearest":
        q = (2 * n + ds) // (2 * ds)
    elif fault == "stale_reciprocal" and d_prev is not None:
        q = q.copy()
        for i in np.nonzero((d_prev != d) & (d != 0) & (n >= 0))[0]:
            q[i] = _stale_quotient(int(n[i]), int(d[i]), int(d_prev[i]))
    return np.where(d == 0, 0, q)


def fit_ok(c, p, fault: Optional[str] = None) -> np.ndarray:
    """fitsRequest per node; c: the node columns (dict of arrays), p: one pod record."""
    pods_ok = (c["num_pods"] <= c["alloc_pods"]) if fault == "pods_le" else (c["num_pods"] + 1 <= c["alloc_pods"])
    rc, rm, re = int(p["req_cpu"]), int(p["req_mem"]), int(p["req_eph"])
    if rc == 0 and rm == 0 and re == 0 and fault != "fit_checks_zero_request":
        return pods_ok
    return (pods_ok & (rc <= c["alloc_cpu"] - c["req_cpu"]) & (rm <= c["alloc_mem"] - c["req_mem"]) &
            (re <= c["alloc_eph"] - c["req_eph"]))


def least_allocated(c, p, w, fault: Optional[str] = None, prev=None) -> np.ndarray:
    col = ("req_cpu", "req_mem") if fault == "la_from_req" else ("nz_cpu", "nz_mem")
    score, present = [], []
    for k, (a, f) in enumerate((("alloc_cpu", col[0]), ("alloc_mem", col[1]))):
        cap = c[a]
        want = c[f] + int(p[f])
        left = cap - want
        over = left < 0
        q = _quotient(np.where(over, 0, left) * MAX_SCORE, cap, fault, None if prev is None else prev[k])
        if fault == "overdrawn_not_zeroed":
            # C's division of the negative numerator (truncation toward zero)
            neg = -((-left * MAX_SCORE) // np.where(cap == 0, 1, cap))
            q = np.where(over & (cap != 0), neg, q)
        else:
            q = np.where(over, 0, q)
        score.append(q)
        present.append((cap != 0) | (fault == "zero_alloc_averaged"))
    wc = np.where(present[0], w["cpu"], 0)
    wm = np.where(present[1], w["mem"], 0)
    num = score[0] * wc + score[1] * wm
    den = wc + wm
    if fault == "mean_by_weight_sum":
        den = np.where(den != 0, w["cpu"] + w["mem"], 0)
    la = _quotient(num, den, fault if fault in ("uncorrected_quotient", "round_to_nearest") else None, None)
    if fault == "overdrawn_not_zeroed":
        la = np.where(den == 0, 0, np.where(num < 0, -((-num) // np.where(den == 0, 1, den)), la))
    return la


def balanced_allocation(c, p, fault: Optional[str] = None, prev=None) -> np.ndarray:
    col = ("nz_cpu", "nz_mem") if fault == "ba_from_nz" else ("req_cpu", "req_mem")
    ft = np.float32 if fault == "ba_float32" else np.float64
    fr = []
    for k, (a, f) in enumerate((("alloc_cpu", col[0]), ("alloc_mem", col[1]))):
        cap = c[a]
        want = c[f] + int(p[f])
        caps = np.where(cap == 0, 1, cap)
        if fault == "uncorrected_quotient":
            x = want.astype(np.float64) * (1.0 / caps.astype(np.float64))
        else:
            x = (want.astype(ft) / caps.astype(ft)).astype(ft)
            if fault == "stale_reciprocal" and prev is not None:
                x = x.copy()
                for i in np.nonzero((prev[k] != cap) & (cap != 0))[0]:
                    y = 1.0 / float(prev[k][i]) if prev[k][i] else 0.0
                    q0 = float(want[i]) * y
                    x[i] = _fma(_fma(-q0, float(cap[i]), float(want[i])), y, q0)
        if fault != "no_clamp":
            x = np.minimum(x, ft(1))
        fr.append(x.astype(ft))
    hc, hm = c["alloc_cpu"] != 0, c["alloc_mem"] != 0
    two = ((ft(1) - np.abs((fr[0] - fr[1]) / ft(2))) * ft(MAX_SCORE)).astype(ft)
    both = np.trunc(two).astype(np.int64)
    if fault == "missing_resource_not_100":
        f0 = np.where(hc, fr[0], ft(0)).astype(ft)
        f1 = np.where(hm, fr[1], ft(0)).astype(ft)
        return np.trunc(((ft(1) - np.abs((f0 - f1) / ft(2))) * ft(MAX_SCORE)).astype(ft)).astype(np.int64)
    return np.where(hc & hm, both, MAX_SCORE)


COLS = ("alloc_cpu", "alloc_mem", "alloc_eph", "alloc_pods", "req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem",
        "num_pods")


def columns(cluster) -> dict:
    """A private copy of the node columns the restatement reads and binds into."""
    return {k: np.array(getattr(cluster, k), np.int64) for k in COLS}


def node_scores(c, p, w, fault: Optional[str] = None, prev=None):
    """(ok, la, ba, total) of one pod on every node."""
    ok = fit_ok(c, p, fault) if w["has_fit"] else np.ones(c["alloc_cpu"].size, bool)
    la = least_allocated(c, p, w, fault, prev)
    ba = balanced_allocation(c, p, fault, prev)
    if fault == "score_6bit":
        la, ba = la & 0x3f, ba & 0x3f
    total = w["fit"] * la + w["ba"] * ba
    if w["n_score"] == 0:
        total = np.ones_like(total)
    return ok, la, ba, total


def schedule(cluster, pods, prof: abi.Profile, fault: Optional[str] = None, prev=None, first: int = 0,
             count: Optional[int] = None, next_start: int = 0, seq0: int = 0, trace: bool = False):
    """The sequential scheduler over pods [first, first + count): per pod the
    feasible nodes of the scan window, the best key among them, the bind, and
    seq0 + the pod's index as its tie-break sequence.  Returns (placements, node columns,
    next_start, per-cycle [(scored nodes, ok, la, ba)] when ``trace``)."""
    assert fault is None or fault in FAULTS
    w = weights(prof)
    c = columns(cluster)
    n = c["alloc_cpu"].size
    k_find = profile.num_feasible_nodes_to_find(n, w["pct"])
    count = pods.n_pods - first if count is None else count
    chosen = np.full(count, -1, np.int32)
    cycles = []
    for j in range(first, first + count):
        p = pods.pods[j]
        ok, la, ba, total = node_scores(c, p, w, fault, prev)
        order = (np.arange(n) + next_start) % n
        feas = order[ok[order]]
        if feas.size > k_find:                    # the (K + 1)-th feasible node ends the scan
            processed = int(np.nonzero(order == feas[k_find])[0][0])
            feas = feas[:k_find]
        else:
            processed = n
        next_start = (next_start + processed) % n
        pick = -1
        if feas.size == 1:
            pick = int(feas[0])
        elif feas.size > 1:
            # the total first, then the key's low part (a total past the key's 20 bits must not wrap)
            lo = tb_keys(np.zeros(feas.size, np.int64), w["seed"], seq0 + j, feas)
            pick = int(feas[np.lexsort((lo, total[feas]))[-1]])
        if trace:
            cycles.append((feas if feas.size > 1 else feas[:0], ok.copy(), la.copy(), ba.copy()))
        chosen[j - first] = pick
        if pick >= 0:
            for f in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem"):
                c[f][pick] += int(p[f])
            c["num_pods"][pick] += 1
    return chosen, c, next_start, cycles
