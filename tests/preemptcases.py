"""Hand-made clusters for DefaultPreemption's dry run (ksim_preempt,
csrc/ksim_preempt.hip): one case per level of pickOneNodeForPreemption's
cascade, the ``want`` cut of the candidate list at every geometry of
k_preempt_pick's 1,024 per-thread chunks, and a few shapes of the per-node
victim selection (tests/test_preemption.py on the CPU,
tests/test_gpu_preempt_edges.py on the device).

Nodes are identical (10 CPUs, no taints, no labels but the hostname), every
bound pod and the one preemptor request CPU only, and the bound-pod table is
written out row by row as (node, priority, start, cpu milli).  ``criteria``
restates the rules of the header comment of ksim_preempt
(include/ksim_engine.h) in plain Python over that table, with no code shared
with the oracle or objref.

A candidate always has a victim: a potential node failed NodeResourcesFit
with all its pods on it, so reprieving every lower-priority pod would restore
exactly that state.  "A node that needs no victims" is therefore a node the
preemptor fits on as it is; it is not a potential node, is never picked, and
does not count in n_potential (the cases ``fits_somewhere``,
``int32_min_victim`` and ``empty_node``)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from ksim import abi, profile
from ksim.model import Container, Node, Pod

ALLOC_CPU = 10000                            # milli-CPU of every node
I32_MIN = -(2 ** 31)
LEVELS = ("high", "sum", "nv", "early", "position")
PICK_THREADS = 1024                          # k_preempt_pick's block


@dataclass
class Case:
    name: str
    n_nodes: int
    rows: List[Tuple[int, int, int, int]]    # bound pods: (node, priority, start, cpu milli), table order
    preemptor: Tuple[int, int]               # (priority, cpu milli)
    args: Tuple[int, int] = (10, 100)        # minCandidateNodesPercentage, minCandidateNodesAbsolute
    level: Optional[str] = None              # the cascade level meant to decide (LEVELS), if any
    winner: Optional[int] = None             # the node meant to win (-1: none)
    want: Optional[int] = None               # the cut meant (pick geometry)
    best_rank: Optional[int] = None          # node-order rank of the uniquely best candidate (pick geometry)
    note: str = ""


# ---- the rules, restated -----------------------------------------------------------
@dataclass
class Verdict:
    potential: List[int]
    want: int
    kept: Dict[int, tuple]                   # node -> (high, sum, nv, -early, position), first `want` candidates
    victims: Dict[int, List[int]]            # node -> table rows, reprieve order (kept candidates)
    all_candidates: List[int]                # every candidate, node order (before the cut)
    pick: int
    result: tuple = field(default=())        # (nominated, victims, n_potential, n_candidates)


def criteria(case: Case) -> Verdict:
    prio_p, cpu_p = case.preemptor
    by_node: Dict[int, List[int]] = {}
    for i, (node, _, _, _) in enumerate(case.rows):
        by_node.setdefault(node, []).append(i)
    used = [sum(case.rows[i][3] for i in by_node.get(n, [])) for n in range(case.n_nodes)]
    # potential nodes: NodeResourcesFit fails (the pod does not fit beside what is there)
    potential = [n for n in range(case.n_nodes) if used[n] + cpu_p > ALLOC_CPU]
    pct, mabs = case.args
    want = min(max(len(potential) * pct // 100, mabs), len(potential))
    kept, victims, cands = {}, {}, []
    for n in potential:
        # SelectVictimsOnNode: remove every lower-priority pod, then reprieve
        # most important first (priority desc, start asc, table order)
        lower = sorted((i for i in by_node.get(n, []) if case.rows[i][1] < prio_p),
                       key=lambda i: (-case.rows[i][1], case.rows[i][2], i))
        load = used[n] - sum(case.rows[i][3] for i in lower)
        if load + cpu_p > ALLOC_CPU:
            continue
        v = []
        for i in lower:
            if load + case.rows[i][3] + cpu_p > ALLOC_CPU:
                v.append(i)
            else:
                load += case.rows[i][3]
        cands.append(n)
        if len(kept) >= want:
            continue
        high = case.rows[v[0]][1] if v else I32_MIN
        total = sum(case.rows[i][1] + 2 ** 31 for i in v)
        early = min((case.rows[i][2] for i in v if case.rows[i][1] == high), default=2 ** 63 - 1)
        kept[n] = (high, total, len(v), -early, len(kept))
        victims[n] = v
    pick = min(kept, key=lambda n: kept[n]) if kept else -1
    res = (pick, victims.get(pick, []), len(potential), len(kept))
    return Verdict(potential, want, kept, victims, cands, pick, res)


def deciding_level(v: Verdict) -> Optional[str]:
    """The first tuple position where the winner and the runner-up differ."""
    if len(v.kept) < 2:
        return None
    order = sorted(v.kept, key=lambda n: v.kept[n])
    a, b = v.kept[order[0]], v.kept[order[1]]
    return LEVELS[next(k for k in range(5) if a[k] != b[k])]


def tie_width(v: Verdict, level: str) -> int:
    """How many kept candidates tie with the winner on every level above ``level``."""
    k = LEVELS.index(level)
    w = v.kept[v.pick]
    return sum(1 for t in v.kept.values() if t[:k] == w[:k])


# ---- the cascade ---------------------------------------------------------------------
def _fill(n_nodes, per_node, special: Dict[int, list]):
    """rows: ``per_node`` [(prio, start, cpu)] on every node but the ones in ``special``."""
    rows = []
    for n in range(n_nodes):
        for prio, start, cpu in special.get(n, per_node):
            rows.append((n, prio, start, cpu))
    return rows


def cascade_cases() -> List[Case]:
    P = (1000, 8000)                         # the preemptor: any pod over 2,000m beside it is a victim
    out = []
    # 0. the pod fits on node 5 as it is: not a potential node; among the others the
    #    highest victim priority decides
    out.append(Case("fits_somewhere", 10,
                    _fill(10, [(50, 100, 2500)], {5: [(50, 100, 1500)], 7: [(20, 100, 2500)], 2: [(900, 1, 2500)]}),
                    P, level="high", winner=7,
                    note="node 5 needs no victims: it passes the filter, so it is no candidate"))
    # 1. lowest highest-victim priority; the winner is worse on every later level
    out.append(Case("level_high", 12,
                    _fill(12, [(50, 100, 2500)], {8: [(20, 5, 2500), (20, 6, 2500), (10, 7, 2500)]}),
                    P, level="high", winner=8))
    # 2. equal high (50), equal count: the sum decides; the winner's start is the earliest (worst)
    out.append(Case("level_sum", 12,
                    _fill(12, [(50, 100, 2500), (40, 100, 2500)], {9: [(50, 1, 2500), (10, 100, 2500)]}),
                    P, level="sum", winner=9))
    # 3. equal high (0), equal sum (2^31): {0} against {0, -2^31}; fewer victims win
    out.append(Case("level_nv", 12,
                    _fill(12, [(0, 100, 2500), (I32_MIN, 100, 2500)], {6: [(0, 1, 2500)]}),
                    P, level="nv", winner=6))
    # 4. equal high, sum, count: the latest earliest-start among the highest-priority
    #    victims; the winner's lower-priority victim started first of all and must not count
    out.append(Case("level_early", 12,
                    _fill(12, [(50, 100, 2500), (10, 150, 2500)], {4: [(10, 5, 2500), (50, 300, 2500)],
                                                                  10: [(50, 200, 2500), (10, 150, 2500)]}),
                    P, level="early", winner=4))
    # 5. everything ties: the first candidate in node order (node 0 is no candidate:
    #    its pods outrank the preemptor)
    out.append(Case("level_position", 12,
                    _fill(12, [(50, 100, 2500)], {0: [(2000, 100, 2500)]}),
                    P, level="position", winner=1))
    # a victim of priority -2^31 (high == the INT32_MIN "no victims" sentinel) and a node needing no victims
    out.append(Case("int32_min_victim", 9,
                    _fill(9, [(0, 100, 2500)], {3: [(I32_MIN, 100, 2500)], 6: []}),
                    P, level="high", winner=3))
    # reprieve: on node 2 the two most important lower-priority pods stay, the
    # victims come out in importance order (not table order)
    out.append(Case("reprieve", 8,
                    _fill(8, [(60, 100, 5200)], {2: [(20, 9, 1500), (30, 8, 2500), (40, 7, 2500), (50, 6, 2500)]}),
                    (1000, 5000), level="high", winner=2))
    # node 1's pods all have priority >= the preemptor's (equal counts as not lower)
    out.append(Case("all_outrank", 8,
                    _fill(8, [(50, 100, 2500)], {1: [(1000, 1, 2500), (1001, 1, 2500)], 0: [(1000, 5, 9000)]}),
                    P, level="position", winner=2))
    # node 3 holds no bound pod
    out.append(Case("empty_node", 8, _fill(8, [(50, 100, 2500)], {3: [], 5: [(40, 100, 2500)]}),
                    P, level="high", winner=5))
    # the pod is larger than a node: every node is potential, none a candidate
    out.append(Case("nothing_helps", 8, _fill(8, [(50, 100, 2500)], {}), (1000, ALLOC_CPU + 1), winner=-1))
    return out


# ---- the cut ---------------------------------------------------------------------------
GEOMETRY_N = (1, 1023, 1024, 1025, 2049, 3000)


def _wants(n: int) -> List[int]:
    """want = 1, N, and (chunk >= 2) cuts strictly inside one thread's chunk:
    near the middle of the node range and in the last chunk that holds more
    than one node."""
    chunk = (n + PICK_THREADS - 1) // PICK_THREADS
    w = {1, n}
    if chunk == 1:
        if n // 2 + 5 < n:
            w.add(n // 2 + 5)
    else:
        mid = (n // 2) // chunk * chunk                  # first node of a middle thread's chunk
        last = (n - 2) // chunk * chunk                  # first node of the last chunk with two nodes in range
        for base in (mid, last):
            for k in range(1, chunk):
                if base + k < n:
                    w.add(base + k)                      # nodes base .. base + k - 1 kept, base + k cut: same thread
        if n == 3000:
            w = {x for x in w if x % 2 == 1 or x in (1, n)}
    return sorted(w)


def inside_a_chunk(n: int, want: int) -> bool:
    chunk = (n + PICK_THREADS - 1) // PICK_THREADS
    return 0 < want < n and (want - 1) // chunk == want // chunk


def geometry_cases() -> List[Case]:
    """Every node a candidate with one victim (50, start 100); the best
    candidate's victim has priority 10.  At rank want - 1 it is picked; at
    rank want it is cut and the first node wins the tie."""
    out = []
    for n in GEOMETRY_N:
        for want in _wants(n):
            for rank in (want - 1, want):
                if rank >= n:
                    continue
                rows = [(v, 10 if v == rank else 50, 100, 5000) for v in range(n)]
                args = (100, 0) if want == n else (0, want)
                out.append(Case(f"cut_n{n}_want{want}_{'in' if rank < want else 'out'}", n, rows, (1000, 6000), args,
                                winner=rank if rank < want else 0, want=want, best_rank=rank))
    return out


@functools.lru_cache(maxsize=None)
def all_cases() -> Dict[str, Case]:
    cs = cascade_cases() + geometry_cases()
    table = {c.name: c for c in cs}
    assert len(table) == len(cs)
    return table


def cascade_ids() -> List[str]:
    return [c.name for c in cascade_cases()]


def geometry_ids() -> List[str]:
    return [c.name for c in geometry_cases()]


# ---- a two-call sequence on one table ---------------------------------------------------
SEQUENCE = Case("sequence", 8,
                _fill(8, [(60, 100, 5200)], {2: [(20, 9, 1500), (30, 8, 2500), (40, 7, 2500), (50, 6, 2500)]}),
                (1000, 9000))
SEQUENCE_PREEMPTORS = ((1000, 9000), (35, 5000))         # high priority first, then a low one


# ---- objects and encodings ---------------------------------------------------------------
def objects(case: Case):
    """(nodes, bound pods, start_time, order, preemptor) as model objects."""
    nodes = [Node(name=f"n{i:04d}", labels={"kubernetes.io/hostname": f"n{i:04d}"},
                  allocatable={"cpu": f"{ALLOC_CPU}m", "memory": "64Gi", "pods": "110"}) for i in range(case.n_nodes)]
    bound, start, order = [], {}, {}
    for i, (node, prio, st, cpu) in enumerate(case.rows):
        name = f"b{i}"
        bound.append(Pod(name, node_name=nodes[node].name, priority=prio, containers=[Container({"cpu": f"{cpu}m"})]))
        start[name] = st
        order[name] = i
    return nodes, bound, start, order, preemptor_pod(case.preemptor)


def preemptor_pod(pc: Tuple[int, int]) -> Pod:
    return Pod("preemptor", priority=pc[0], containers=[Container({"cpu": f"{pc[1]}m"})])


@functools.lru_cache(maxsize=8)
def _cluster(n_nodes: int, load: tuple):
    """The encoded cluster of ``n_nodes`` nodes holding pods of these (node, cpu):
    priorities and start times are no part of it, so the cut cases of one N share it."""
    from ksim.encode import encode_cluster
    case = Case("", n_nodes, [(n, 0, 0, c) for n, c in load], (0, 0))
    nodes, bound, _, _, _ = objects(case)
    cluster, _ = encode_cluster(nodes, bound)
    assert list(cluster.node_names) == [n.name for n in nodes]   # nodeTree order == list order (one zone)
    return cluster


def encoded(case: Case, preemptor: Optional[Tuple[int, int]] = None):
    """(cluster, bound-pod table, encoded preemptor, compiled profile).  The
    table is the case's rows as they stand."""
    from ksim.encode import encode_pods
    cluster = _cluster(case.n_nodes, tuple((r[0], r[3]) for r in case.rows))
    rows = np.array(case.rows, np.int64).reshape(-1, 4)
    req = np.zeros((len(case.rows), abi.PREEMPT_REQ), np.int64)
    req[:, 0] = rows[:, 3]
    table = abi.BoundPods(rows[:, 0], rows[:, 1], rows[:, 2], req)
    enc = encode_pods(cluster, [preemptor_pod(preemptor or case.preemptor)])
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=100, preemption=profile.PreemptionArgs(*case.args))
    return cluster, table, enc, profile.compile_profile(sp)
