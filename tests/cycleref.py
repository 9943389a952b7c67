"""The back half of a per-pod scheduling cycle in plain Python: everything
between "which nodes pass the filters, and what does each score plugin say of
them" and "which node gets the pod, and where does the next pod's scan start"
(csrc/ksim_kernels.hip: k_window, k_extrema, k_select / bind_cycle, the
sharded k_wcount_sh .. k_bind_sh; csrc/ksim_device.h: normalize_value).

No cleverness: Python integers, ``float`` only where Go uses float64, numpy
only to hold the arrays.  Feasibility and the raw scores of every plugin but
PodTopologySpread are inputs (other suites own them; tests/cyclecases.py reads
them off the C oracle's Filter / Score of every node and checks them against
what the scene was built to give); the model derives the rest:

  K (numFeasibleNodesToFind), the cut, processed, evaluated, the kept list, nf
  the per-slot extrema over the kept list
  IgnoredNodes, the registered pairs and topologyNormalizingWeight per
  ScheduleAnyway constraint from the kept, non-ignored nodes
  PodTopologySpread's raw scores (scoreForCount, math.Round)
  the NormalizeScore forms: Default, DefaultReverse, PodTopologySpread, the
  min-max form in float64 with Go's truncation, its empty-topologyScore
  pass-through
  the weighted totals, the extender scores, the single-feasible-node shortcut
  selectHost under oracle.shard_model.tb_keys
  the next start modulo the scan length
  the error outcome of a PreFilterResult name the snapshot lacks

``finish`` is one cycle, ``schedule`` a sequential scheduler over a queue that
applies each bind, ``shard_view`` what rank r of a node partition must report.
``FAULTS`` names the wrong readings of all this that ``fault=`` switches on;
tests/test_cycle_cases.py proves that the scenes of tests/cyclecases.py tell
every one of them from the right reading."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle.shard_model import NODE_MASK, tb_keys

MAX_NODE_SCORE = 100
MIN_FEASIBLE_NODES_TO_FIND = 100
MIN_FEASIBLE_NODES_PERCENTAGE_TO_FIND = 5

PASSED, NOT_EVALUATED, FAIL_EXTENDER = 0xFF, 0xFE, 0xFD
STATUS_SCHEDULED, STATUS_UNSCHEDULABLE, STATUS_ERROR = 0, 1, 2
CHOSEN_ERROR = -2

# NormalizeScore forms of a score slot
NONE, DEFAULT, REVERSE, PTS, MINMAX = "none", "default", "reverse", "pts", "minmax"

FAULTS = (
    # window
    "cut_is_kth_feasible",            # 1  the cut is the K-th feasible node, not the (K + 1)-th
    "k_plus_1_is_no_cut",             # 2  exactly K + 1 feasible nodes read as no cut
    "advance_by_evaluated",           # 3  the next start advances by evaluated (cut + 1), not processed
    "short_pod_advances_by_kept",     # 4  a pod with at most K feasible nodes advances the start by its feasible nodes
    "scan_from_node_0",               # 5  the scan ignores the start (node order)
    "list_k_from_cluster",            # 6  with a PreFilterResult list, K comes from the cluster's node count
    "list_start_mod_cluster",         # 7  with a list, the start is taken and advanced modulo the cluster's node count
    # extrema
    "extrema_over_all_feasible",      # 8  extrema over every feasible node of the ring
    "cut_node_in_extrema",            # 9  the cut node enters the extrema
    "ignored_in_pts_extrema",         # 10 IgnoredNodes enter PodTopologySpread's min / max
    "size_counts_past_cut",           # 16 topologyNormalizingWeight's size counts feasible nodes past the cut
    "size_counts_ignored",            # 16 ... or ignored ones
    "dropped_in_extrema",             # 18 an extender-dropped node still enters the extrema
    "dropped_in_nf",                  # 18 ... or nf
    # normalize
    "ignored_gets_100",               # 11 an ignored node gets 100, not 0
    "pts_without_minimum",            # 12 PodTopologySpread normalized as 100 (max - v) / max
    "minmax_integer_division",        # 13 the min-max form by integer division
    "minmax_zero_diff_100",           # 14 the min-max form gives 100 on a zero difference
    "reverse_zero_max_0",             # 15 DefaultReverse gives 0 on a zero maximum
    # select
    "ties_to_lowest_index",           # 17 ties go to the lowest node index (no hash)
    "single_node_scored",             # 19 one feasible node is scored like any other
    # readings the code suggests
    "weight_zero_is_zero",            # a weight of 0 multiplies by 0 (the framework reads it as 1)
    "pts_score_truncated",            # math.Round read as a truncating conversion
    "pts_size_ignores_empty_value",   # a system-defaulted constraint's size leaves out the pair of unlabelled nodes
)


def num_feasible_nodes_to_find(n: int, pct: int) -> int:
    if n < MIN_FEASIBLE_NODES_TO_FIND or pct >= 100:
        return n
    adaptive = pct
    if adaptive <= 0:
        adaptive = max(50 - n // 125, MIN_FEASIBLE_NODES_PERCENTAGE_TO_FIND)
    return max(n * adaptive // 100, MIN_FEASIBLE_NODES_TO_FIND)


@dataclass
class SoftUse:
    """One ScheduleAnyway constraint of the pod."""
    value: np.ndarray                  # [N] value id of the key on each node, 0: the node lacks the key
    count: np.ndarray                  # [N] pods on the node that match the selector
    max_skew: int
    hostname: bool                     # keyed by kubernetes.io/hostname: the node's own count, size nf - ignored
    counted: Optional[np.ndarray] = None   # [N] nodes whose pods count (the inclusion policies); None: all


@dataclass
class Inputs:
    """What one pod's cycle starts from (node positions are global)."""
    n_nodes: int
    feasible: np.ndarray               # [N] bool: the node passes every filter
    raw: np.ndarray                    # [S][N] raw score of each slot (the PodTopologySpread slot is derived)
    kinds: Sequence[str]               # [S] NormalizeScore form of each slot
    weights: Sequence[int]             # [S]
    scan: Optional[Sequence[int]] = None   # PreFilterResult node positions (None: every node)
    unknown: bool = False              # the PreFilterResult names a node the snapshot lacks
    soft: Sequence[SoftUse] = ()
    system_default: bool = False       # system-defaulted constraints: requireAllTopologies is false
    topology_score_nonempty: bool = False
    ext_fail: Optional[np.ndarray] = None
    ext_score: Optional[np.ndarray] = None
    fail_plugin: Optional[np.ndarray] = None   # [N] the filter verdict to report for a scanned node


def _round_half_away(x: float) -> int:
    """Go's math.Round."""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _go_div(a: int, b: int) -> int:
    """Go's integer division: truncated toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _missing_key(inp: Inputs, node: int) -> bool:
    return any(int(u.value[node]) == 0 for u in inp.soft)


def _pts(inp: Inputs, kept: List[int], size_nodes: List[int], fault: Optional[str]):
    """initPreScoreState + Score of PodTopologySpread over the kept list.
    Returns (ignored set, sizes, raw score function)."""
    require_all = not inp.system_default
    ignored = {n for n in kept if require_all and _missing_key(inp, n)}
    basis = [n for n in size_nodes if fault == "size_counts_ignored" or
             not (require_all and _missing_key(inp, n))]
    sizes, present = [], []
    for u in inp.soft:
        if u.hostname:
            present.append(None)
            sizes.append(len(basis))
            continue
        vals = {int(u.value[n]) for n in basis}
        present.append({int(u.value[n]) for n in kept if n not in ignored})
        if fault == "pts_size_ignores_empty_value":
            vals.discard(0)
        sizes.append(len(vals))
    weight = [math.log(float(sz + 2)) for sz in sizes]
    dom: List[Optional[Dict[int, int]]] = []
    for u, pres in zip(inp.soft, present):
        if pres is None:
            dom.append(None)
            continue
        d = {v: 0 for v in pres}
        for n in range(inp.n_nodes):
            if require_all and _missing_key(inp, n):
                continue
            if u.counted is not None and not u.counted[n]:
                continue
            v = int(u.value[n])
            if v in d:
                d[v] += int(u.count[n])
        dom.append(d)

    def raw(node: int) -> int:
        if node in ignored:
            return 0
        score = 0.0
        for u, w, d in zip(inp.soft, weight, dom):
            v = int(u.value[node])
            if v == 0:
                continue
            cnt = int(u.count[node]) if d is None else d.get(v, 0)
            score += float(cnt) * w + float(u.max_skew - 1)
        return int(score) if fault == "pts_score_truncated" else _round_half_away(score)

    return ignored, sizes, raw


def normalize(kind: str, vals: List[int], ign: List[bool], ext_vals: List[int], ext_ign: List[bool],
               nonempty: bool, fault: Optional[str]) -> List[int]:
    """NormalizeScore of one slot over the scored list; the extrema are taken
    over ``ext_vals`` (the scored list itself but under a wrong reading)."""
    if kind == NONE:
        return list(vals)
    if kind in (DEFAULT, REVERSE):
        mx = max([0] + ext_vals)
        if mx == 0:
            if kind == REVERSE:
                return [0 if fault == "reverse_zero_max_0" else MAX_NODE_SCORE] * len(vals)
            return list(vals)
        out = [_go_div(MAX_NODE_SCORE * v, mx) for v in vals]
        return [MAX_NODE_SCORE - x for x in out] if kind == REVERSE else out
    if kind == PTS:
        counted = [v for v, g in zip(ext_vals, ext_ign) if not g or fault == "ignored_in_pts_extrema"]
        mn = min(counted) if counted else (1 << 63) - 1
        mx = max([0] + counted)
        out = []
        for v, g in zip(vals, ign):
            if g:
                out.append(MAX_NODE_SCORE if fault == "ignored_gets_100" else 0)
            elif mx == 0:
                out.append(MAX_NODE_SCORE)
            elif fault == "pts_without_minimum":
                out.append(_go_div(MAX_NODE_SCORE * (mx - v), mx))
            else:
                out.append(_go_div(MAX_NODE_SCORE * (mx + mn - v), mx))
        return out
    assert kind == MINMAX
    if not nonempty:
        return list(vals)
    mn, mx = min(ext_vals), max(ext_vals)
    diff = mx - mn
    out = []
    for v in vals:
        if diff <= 0:
            out.append(MAX_NODE_SCORE if fault == "minmax_zero_diff_100" else 0)
        elif fault == "minmax_integer_division":
            out.append(_go_div(MAX_NODE_SCORE * (v - mn), diff))
        else:
            out.append(int(float(MAX_NODE_SCORE) * (float(v - mn) / float(diff))))
    return out


def tb_lo(seed: int, pod_seq: int, nodes: Sequence[int]) -> List[int]:
    """The tie-break word of selectHost's (total, lo) order: tb_keys of a zero total."""
    arr = np.asarray(list(nodes), np.int64)
    return [int(k) for k in tb_keys(np.zeros(arr.size, np.int64), seed, pod_seq, arr)]


def finish(inp: Inputs, next_start: int, pct: int, seed: int, pod_seq: int, fault: Optional[str] = None) -> dict:
    """One cycle.  The result has every key of Oracle.cycle's (but
    fail_detail) and, for the scenes' claims: kept (the scored list in scan
    order), cut (node or -1), ring (every feasible node of the scan, in scan
    order), ignored, sizes, extrema ([S] (min, max) over the scored list)."""
    assert fault is None or fault in FAULTS, fault
    N, S = inp.n_nodes, len(inp.kinds)
    scan = list(range(N)) if inp.scan is None else [int(x) for x in inp.scan]
    listed = inp.scan is not None
    NS = 0 if inp.unknown else len(scan)
    K = num_feasible_nodes_to_find(N if listed and fault == "list_k_from_cluster" else NS, pct)
    out = dict(chosen=-1, status=STATUS_UNSCHEDULABLE, k_to_find=K,
               fail_plugin=np.full(N, NOT_EVALUATED, np.uint8), scored=np.zeros(N, np.uint8),
               raw=np.zeros((max(S, 1), N), np.int64), norm=np.zeros((max(S, 1), N), np.int64),
               total=np.zeros(N, np.int64), kept=[], cut=-1, ring=[], ignored=set(), sizes=[], extrema=[])
    mod = N if listed and fault == "list_start_mod_cluster" else NS
    start = 0
    if NS > 0:
        start = 0 if fault == "scan_from_node_0" else (next_start % mod) % NS
    order = [scan[(start + i) % NS] for i in range(NS)]
    ring = [n for n in order if inp.feasible[n]]
    limit = K - 1 if fault == "cut_is_kth_feasible" else K
    kept: List[int] = []
    cut, evaluated, failed = -1, 0, 0
    no_cut = fault == "k_plus_1_is_no_cut" and len(ring) == K + 1
    for n in order:
        evaluated += 1
        out["fail_plugin"][n] = PASSED if inp.feasible[n] else \
            (0 if inp.fail_plugin is None else inp.fail_plugin[n])
        if not inp.feasible[n]:
            failed += 1
        elif len(kept) < limit:
            kept.append(n)
        elif no_cut:
            continue
        else:
            cut = n
            break
    processed = len(kept) + failed if cut >= 0 else evaluated
    advance = evaluated if fault == "advance_by_evaluated" else processed
    if fault == "short_pod_advances_by_kept" and cut < 0:
        advance = len(kept)
    nxt = next_start if NS == 0 else (next_start + advance) % mod
    dropped: List[int] = []
    if inp.ext_fail is not None:
        for n in kept:
            if inp.ext_fail[n]:
                out["fail_plugin"][n] = FAIL_EXTENDER
                dropped.append(n)
        kept = [n for n in kept if not inp.ext_fail[n]]
    nf = len(kept) + (len(dropped) if fault == "dropped_in_nf" else 0)
    out.update(n_feasible=nf, n_evaluated=evaluated, n_processed=processed, next_start=nxt, kept=kept, cut=cut,
               ring=ring)
    if inp.unknown:
        out.update(chosen=CHOSEN_ERROR, status=STATUS_ERROR)
        return out
    if not kept:
        return out
    if nf == 1 and fault != "single_node_scored":
        out.update(chosen=kept[0], status=STATUS_SCHEDULED)
        return out

    # the nodes a wrong reading lets into the extrema / the sizes beside the scored list
    extra: List[int] = []
    if fault == "extrema_over_all_feasible":
        extra = [n for n in ring if n not in kept and n not in dropped]
    elif fault == "cut_node_in_extrema" and cut >= 0:
        extra = [cut]
    elif fault == "dropped_in_extrema":
        extra = list(dropped)
    size_nodes = kept + ([n for n in ring if n not in kept and n not in dropped]
                         if fault == "size_counts_past_cut" else [])
    ignored, sizes, pts_raw = (set(), [], None)
    if inp.soft:
        ignored, sizes, pts_raw = _pts(inp, kept, size_nodes, fault)
    require_all = not inp.system_default
    totals = [0] * len(kept)
    for s in range(S):
        kind = inp.kinds[s]
        if kind == PTS and inp.soft:
            score = pts_raw
            ign_of = lambda n: n in ignored or (n in extra and require_all and _missing_key(inp, n))  # noqa: E731
        else:
            score = lambda n, s=s: int(inp.raw[s][n])                                               # noqa: E731
            ign_of = lambda n: False                                                                # noqa: E731
        vals = [score(n) for n in kept]
        ext_nodes = kept + extra
        ext_vals = vals + [score(n) for n in extra]
        nm = normalize(kind, vals, [ign_of(n) for n in kept], ext_vals, [ign_of(n) for n in ext_nodes],
                        inp.topology_score_nonempty, fault)
        w = int(inp.weights[s])
        if w == 0 and fault != "weight_zero_is_zero":
            w = 1
        for j, n in enumerate(kept):
            out["raw"][s][n] = vals[j]
            out["norm"][s][n] = nm[j]
            totals[j] += nm[j] * w
        live = [v for v, n in zip(vals, kept) if not ign_of(n)] if kind == PTS else vals
        out["extrema"].append((min(live), max(live)) if live else None)
    if S == 0 and inp.ext_score is None:
        totals = [1] * len(kept)
    if inp.ext_score is not None:
        totals = [t + int(inp.ext_score[n]) for t, n in zip(totals, kept)]
    los = tb_lo(seed, pod_seq, kept)
    best = None
    for j, n in enumerate(kept):
        out["total"][n] = totals[j]
        out["scored"][n] = 1
        key = (totals[j], -n) if fault == "ties_to_lowest_index" else (totals[j], los[j])
        if best is None or key > best[0]:
            best = (key, n)
    out.update(chosen=best[1], status=STATUS_SCHEDULED, ignored=ignored, sizes=sizes)
    return out


RESULT_KEYS = ("chosen", "status", "n_feasible", "n_evaluated", "n_processed", "k_to_find", "next_start")
ARRAY_KEYS = ("fail_plugin", "scored", "raw", "norm", "total")

STATE_COLUMNS = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "num_pods")


@dataclass
class Run:
    """What ``schedule`` leaves behind."""
    chosen: np.ndarray
    evals: int
    scheduled: int
    unschedulable: int
    next_start: int
    state: Dict[str, np.ndarray]
    class_count: np.ndarray
    cycles: List[dict] = field(default_factory=list)


def schedule(cluster, pods, inputs_of: Callable[[int], Inputs], bound: Callable[[int, int], None], pct: int,
             seed: int, next_start: int = 0, pod_seq: int = 0, fault: Optional[str] = None,
             on_cycle: Optional[Callable[[int, dict], None]] = None) -> Run:
    """The sequential scheduler over the queue ``pods`` (ksim.encode.EncodedPods)
    from the state of ``cluster``.  ``inputs_of(j)`` gives pod j's inputs under
    the binds so far; ``bound(j, node)`` tells whoever computes them of a bind.
    The model applies each bind to its own copy of the node state: the pod's
    requests, the pod count and the pod's count-class adds."""
    state = {k: np.array(getattr(cluster, k), np.int64 if k != "num_pods" else np.int32) for k in STATE_COLUMNS}
    classes = np.array(cluster.class_count, np.int32)
    chosen = np.full(pods.n_pods, -1, np.int32)
    run = Run(chosen, 0, 0, 0, next_start, state, classes)
    for j in range(pods.n_pods):
        r = finish(inputs_of(j), run.next_start, pct, seed, pod_seq + j, fault)
        if on_cycle is not None:
            on_cycle(j, r)
        run.cycles.append(r)
        run.evals += r["n_evaluated"]
        run.next_start = r["next_start"]
        chosen[j] = r["chosen"]
        if r["status"] != STATUS_SCHEDULED:
            run.unschedulable += 1                  # a cycle that ends in an error is counted here too
            continue
        run.scheduled += 1
        node, p = r["chosen"], pods.pods[j]
        for k in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem"):
            state[k][node] += int(p[k])
        state["num_pods"][node] += 1
        for a in pods.adds[int(p["add_first"]):int(p["add_first"]) + int(p["add_count"])]:
            classes[int(a["cls"]), node] += int(a["count"])
        bound(j, node)
    return run


def shard_view(result: dict, inp: Inputs, start: int, parts: Sequence[Tuple[int, int]], r: int) -> dict:
    """What rank r of the node partition ``parts`` ((base, count) per rank)
    must report of a cycle on the whole cluster (no PreFilterResult list: a
    sharded handle refuses them) that started at ``start``: the kept nodes it
    holds, its share of the evaluated nodes (the shares sum to n_evaluated)
    and the common next start.  hi / lo: its feasible nodes at or after the
    start and before it (the two run counts the shards exchange)."""
    base, cnt = parts[r]
    mine = range(base, base + cnt)
    N = inp.n_nodes
    evaluated = result["n_evaluated"]
    return dict(kept=[n for n in result["kept"] if n in mine],
                evals=sum(1 for n in mine if (n - start) % N < evaluated),
                next_start=result["next_start"],
                hi=sum(1 for n in mine if inp.feasible[n] and n >= start),
                lo=sum(1 for n in mine if inp.feasible[n] and n < start),
                owns_cut=result["cut"] in mine, owns_chosen=result["chosen"] in mine)


__all__ = ["FAULTS", "Inputs", "SoftUse", "Run", "finish", "schedule", "shard_view", "num_feasible_nodes_to_find",
           "tb_lo", "NODE_MASK"]
