"""Multi-preemptor scenes for the batched DefaultPreemption dry run
(ksim_preempt_many; csrc/ksim_preempt.hip k_preempt_many_nodes, k_preempt_pick's
row blocks, k_preempt_many_victims), each on one cluster, and a small Python
model of the call whose wrong readings (FAULTS) the scenes must tell from the
right one: tests/test_preempt_many_cases.py on the CPU,
tests/test_gpu_preempt_many.py on the device.

Every row of a call is ksim_preempt_full's dry run without nominated groups, so
the reference of a row is the reference of that single call:
  Fit-only scenes   tests/preemptcases.py ``Case`` rows with a list of
                    (priority, cpu) preemptors: ``preemptcases.criteria`` per
                    row, and ``fit_dry_run`` below, which restates the rules once
                    more with budgets (filterPodsWithPDBViolation) and keeps the
                    victim flags of every node, as the call's model needs them;
  object scenes     tests/preemptfullcases.py ``FullScene`` builders (host
                    ports, counted volumes, volume groups, budgets, and the uses
                    no Filter reads): ``preemptfullref.dry_run`` per row.
All scenes are under 4,096 nodes, where a launch group takes 64 rows
(``many_rows`` restates ksim_preempt_many_rows)."""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import preemptcases as pc
import preemptfullcases as fc
import preemptfullref
import preemptpdbref
from ksim.model import (LabelSelector, Pod, PodAffinityTerm, PodDisruptionBudget, TopologySpreadConstraint,
                        WeightedPodAffinityTerm)

MAX_ROWS = 64                                    # KSIM_PREEMPT_MANY_ROWS
SLAB_BYTES = 256 << 20                           # the bound include/ksim_engine.h states
NODE_BYTES = 32                                  # one node's result record
SENTINEL = ("unwritten",)
FAULTS = ("shared_flags",                        # one victim-flag array for every row of a launch group
          "row0_priority",                       # row 0's priority used for every row
          "grouped_order",                       # the answers come back in form-grouped order
          "second_group_dropped",                # the second launch group is never launched
          "first_group_repeated",                # ... or the first one's rows are launched again in its place
          "victims_cut_64",                      # the victims step stops after one stride of 64
          "violating_order_lost")                # victims in CSR order, the violating ones not first


def many_rows(n_nodes: int, n_bound: int) -> int:
    per = NODE_BYTES * max(n_nodes, 0) + max(n_bound, 0)
    return max(1, min(MAX_ROWS, SLAB_BYTES // per)) if per > 0 else MAX_ROWS


@dataclass
class Answer:
    result: tuple                                # (node or -1, victims, n_potential, n_candidates, n_pdb_violations)
    flags: Dict[int, Dict[int, int]]             # node -> {table row: flag}: bit 0 victim, bit 1 violating


# ---- Fit and budgets, restated with the flags kept -------------------------------------------------
def fit_dry_run(case: pc.Case, preemptor: Tuple[int, int], budgets=None) -> Answer:
    """``budgets``: (allowed per budget, budget ids per table row) or None."""
    prio_p, cpu_p = preemptor
    by_node: Dict[int, List[int]] = {}
    for i, row in enumerate(case.rows):
        by_node.setdefault(row[0], []).append(i)
    cpu = lambda i: case.rows[i][3]                                          # noqa: E731
    flags, cands, n_pot = {}, [], 0
    for n in range(case.n_nodes):
        mine = sorted(by_node.get(n, []), key=lambda i: (-case.rows[i][1], case.rows[i][2], i))
        used = sum(cpu(i) for i in mine)
        if used + cpu_p <= pc.ALLOC_CPU:
            continue
        n_pot += 1
        lower = [i for i in mine if case.rows[i][1] < prio_p]
        f = {i: 0 for i in mine}
        flags[n] = f
        load = used - sum(cpu(i) for i in lower)
        if load + cpu_p > pc.ALLOC_CPU:
            continue
        viol = set()
        if budgets:
            left = list(budgets[0])
            for i in lower:                                                  # a fresh copy per node
                for b in budgets[1][i]:
                    left[b] -= 1
                    if left[b] < 0:
                        viol.add(i)
        victims = []
        for part in ([i for i in lower if i in viol], [i for i in lower if i not in viol]):
            for i in part:
                if load + cpu(i) + cpu_p > pc.ALLOC_CPU:
                    victims.append(i)
                else:
                    load += cpu(i)
                f[i] = (1 if victims and victims[-1] == i else 0) | (2 if i in viol else 0)
        nviol = sum(1 for i in victims if i in viol)
        top = max(case.rows[i][1] for i in victims)
        early = min(case.rows[i][2] for i in victims if case.rows[i][1] == top)
        key = (nviol, case.rows[victims[0]][1], sum(case.rows[i][1] + 2 ** 31 for i in victims), len(victims), -early)
        cands.append((n, key, victims))
    pct, mabs = case.args
    want = min(max(n_pot * pct // 100, mabs), n_pot)
    kept = []
    for c in cands if want > 0 else []:
        if len(kept) >= want and any(k[1][0] == 0 for k in kept):
            break
        kept.append(c)
    if not kept:
        return Answer((-1, [], n_pot, 0, 0), flags)
    node, key, victims = min(kept, key=lambda c: c[1] + (kept.index(c),))
    return Answer((node, victims, n_pot, len(kept), key[0]), flags)


# ---- the call, modelled -----------------------------------------------------------------------------
def victims_of(flags: Dict[int, int], csr: List[int], order_lost: bool = False) -> List[int]:
    if order_lost:
        return [i for i in csr if flags.get(i, 0) & 1]
    return [i for i in csr if flags.get(i, 0) == 3] + [i for i in csr if flags.get(i, 0) == 1]


def call_model(rows, answer: Callable[[int, int], Answer], form: Callable[[int], int], csr: Callable[[int], List[int]],
               fault: Optional[str] = None, rows_per_group: int = MAX_ROWS) -> list:
    """ksim_preempt_many over ``rows`` [(pod, priority)]: the rows of form 0
    (ports / free) and 1 (volume) run in launch groups of ``rows_per_group``, each
    row on flag and result slabs of its own, the victims read back from the
    row's flags; the rows of form 2 are single dry runs.  One 5-tuple per row,
    in the caller's order."""
    assert fault is None or fault in FAULTS
    n = len(rows)
    prio = [rows[0][1] if fault == "row0_priority" else p for _, p in rows]
    groups = []
    for f in (0, 1):
        members = [i for i in range(n) if form(rows[i][0]) == f]
        groups += [members[k:k + rows_per_group] for k in range(0, len(members), rows_per_group)]
    outs = [SENTINEL] * n
    for gi, g in enumerate(groups):
        if fault == "second_group_dropped" and gi == 1:
            continue
        src = groups[0] if fault == "first_group_repeated" and gi == 1 else g
        ans = [answer(rows[src[k % len(src)]][0], prio[src[k % len(src)]]) for k in range(len(g))]
        shared: Dict[int, Dict[int, int]] = {}
        for a in ans:                                                        # later rows overwrite earlier ones
            for node, f in a.flags.items():
                shared.setdefault(node, {}).update(f)
        for k, i in enumerate(g):
            node = ans[k].result[0]
            flags = (shared if fault == "shared_flags" else ans[k].flags).get(node, {})
            v = victims_of(flags, csr(node), fault == "violating_order_lost") if node >= 0 else []
            if fault == "victims_cut_64":
                v = v[:64]
            outs[i] = (node, v) + tuple(ans[k].result[2:])
    single = [i for i in range(n) if form(rows[i][0]) == 2]
    for i in single:
        outs[i] = tuple(answer(rows[i][0], prio[i]).result)
    if fault == "grouped_order":
        outs = [outs[i] for g in groups for i in g] + [outs[i] for i in single]
    return outs


# ---- scenes --------------------------------------------------------------------------------------------
@dataclass
class ManyScene:
    name: str
    rows: List[Tuple[int, int]]                      # (pending pod, priority), the caller's order
    n_nodes: int
    n_bound: int
    answer: Callable[[int, int], Answer]             # the row's reference, with what flags it knows
    form: Callable[[int], int]                       # 0 ports / free, 1 volume, 2 the single-pod launches
    csr: Callable[[int], List[int]]                  # a node's table rows, most important first
    build: Callable[[], object]                      # -> Built: cluster, enc, table, prof (for the engine)
    case: Optional[pc.Case] = None                   # Fit-only scenes
    preemptors: Tuple[Tuple[int, int], ...] = ()
    budgets: object = None                           # Fit-only: (allowed, ids per row); object scenes: the PDBs
    aims: Tuple[str, ...] = ()                       # the faults the scene is there to tell

    def reference(self) -> list:
        return call_model(self.rows, self.answer, self.form, self.csr)


@dataclass
class Built:
    cluster: object
    enc: object
    table: object
    prof: object


def _case_csr(case: pc.Case):
    def csr(node):
        mine = [i for i, r in enumerate(case.rows) if r[0] == node]
        return sorted(mine, key=lambda i: (-case.rows[i][1], case.rows[i][2], i))
    return csr


def fit_scene(name, case: pc.Case, preemptors, picks, budgets=None, aims=()) -> ManyScene:
    """``picks``: per row the index into ``preemptors``."""
    preemptors = tuple(preemptors)

    @functools.lru_cache(maxsize=None)
    def answer(pod, prio):
        return fit_dry_run(case, (prio, preemptors[pod][1]), budgets)

    def build():
        from ksim import abi
        from ksim.encode import encode_pods
        cluster, table, _, prof = pc.encoded(case)
        pods = [dataclasses.replace(pc.preemptor_pod(p), name=f"p{k}") for k, p in enumerate(preemptors)]
        if budgets:
            import numpy as np
            off = np.concatenate([[0], np.cumsum([len(x) for x in budgets[1]])]).astype(np.int32)
            table = abi.BoundPods(table.node, table.priority, table.start_time, table.req, pdb_allowed=budgets[0],
                                  pdb_off=off, pdb_ids=[b for x in budgets[1] for b in x])
        return Built(cluster, encode_pods(cluster, pods), table, prof)

    return ManyScene(name, [(k, preemptors[k][0]) for k in picks], case.n_nodes, len(case.rows), answer,
                     lambda pod: 0, _case_csr(case), build, case, preemptors, budgets, tuple(aims))


RACE = ((1000, 9000), (35, 5000), (45, 5000), (10, 9000), (2000, 9000))   # on preemptcases.SEQUENCE


def victims_case(v: int) -> pc.Case:
    """Node 0 holds ``v`` pods of 100m below the preemptor (9,950m: every one is a
    victim), node 1 one pod that outranks it."""
    rows = [(0, 10 + j % 7, 100 + j % 3, 100) for j in range(v)] + [(1, 2000, 100, 9000)]
    return pc.Case(f"victims_{v}", 2, rows, (1000, 9950), (100, 0))


def edge_case(n: int, target: int) -> pc.Case:
    """``n`` nodes with one 5-CPU pod each; the pod of node ``target`` has the lowest priority."""
    rows = [(v, 10 if v == target else 50, 100, 5000) for v in range(n)]
    return pc.Case(f"edge_{n}_{target}", n, rows, (1000, 6000), (100, 0))


def _every_third_guarded(case: pc.Case):
    """One budget that allows nothing over every third row."""
    return ([0], [[0] if i % 3 == 0 else [] for i in range(len(case.rows))])


# ---- the object scene: every route in one call -------------------------------------------------------------
IMAGE = "registry.example/many:v1"
X = fc.X


def mixed() -> fc.FullScene:
    """Four 16-CPU nodes at EBS limit 2.  n0 (za) holds 15 CPUs in three pods
    (a0 holds port 8000 and volume s and is app=x, a1 holds t and is guarded by
    the budget), n1 (zb) one pod that outranks everybody, n2 (za) two pods (d0
    holds port 8001, d1 is app=x and guarded), n3 (zb) one pod with two
    volumes.  The pending pods, one per route: Fit only; a host port; a counted
    volume; both; a volume whose PV reaches n0 and n3 only (the veto takes n2,
    the Fit-only row's node, out of the candidates); then
    ScheduleAnyway spread, preferred pod affinity and an image, which no Filter
    reads; then hostname anti-affinity and DoNotSchedule spread, which take the
    single-pod launches."""
    s = fc.FullScene("mixed")
    lim = {fc.EBS_KEY: "2"}
    for name, zone in (("n0", "za"), ("n1", "zb"), ("n2", "za"), ("n3", "zb")):
        s.znode(name, zone, lim)
    s.nodes[0].images = [([IMAGE], 500 * 1024 * 1024)]
    s.bpod("a0", "n0", 10, [("ebs", "s")], cpu="6000m", port=8000, labels=X)
    s.bpod("a1", "n0", 8, [("ebs", "t")], cpu="6000m", labels={"tier": "db"})
    s.bpod("a2", "n0", 5, cpu="3000m")
    s.bpod("c0", "n1", 2000, cpu="15900m")
    s.bpod("d0", "n2", 20, cpu="8000m", port=8001)
    s.bpod("d1", "n2", 3, cpu="7500m", labels={"app": "x", "tier": "db"})
    s.bpod("e0", "n3", 30, [("ebs", "u"), ("ebs", "v")], cpu="15950m")
    big = "4000m"
    s.preemptor(cpu=big)                                                       # 0: Fit only
    s.pending[0].name = "fit"
    mk = lambda name, **kw: _named(s.preemptor(**kw), name)                    # noqa: E731
    mk("port", ports=(8000,))                                                  # 1
    mk("volume", vols=[("ebs", "x")])                                          # 2
    mk("port_volume", vols=[("ebs", "y")], ports=(8001,))                      # 3
    mk("pinned", vols=[("ebs", "z")], cpu=big)                                 # 4: the static veto
    s.pin("ebs", "z", ["n0", "n3"])
    soft = TopologySpreadConstraint(1, fc.ZONE, "ScheduleAnyway", LabelSelector(dict(X)))
    mk("soft_spread", cpu=big, labels={"app": "w"}, spread=[soft])             # 5 (no term of another pod selects it)
    p = mk("preferred", cpu=big)                                               # 6
    p.pod_affinity_preferred = [WeightedPodAffinityTerm(10, PodAffinityTerm(fc.ZONE, LabelSelector(dict(X))))]
    p = mk("image", cpu=big)                                                   # 7
    p.containers[0].image = IMAGE
    mk("anti", cpu=big, terms=[fc.anti()])                                     # 8: single
    mk("hard_spread", cpu=big, labels=X, spread=[fc.hard(skew=5)])             # 9: single
    s.budgets = [PodDisruptionBudget("db", selector=LabelSelector({"tier": "db"}), disruptions_allowed=0)]
    return s


def _named(p: Pod, name: str) -> Pod:
    p.name = name
    return p


MIXED_FORM = (0, 0, 1, 1, 1, 0, 0, 0, 2, 2)          # the route of each pending pod of mixed()
MIXED_ROWS = ((8, 1000), (0, 1000), (2, 1000), (1, 1000), (9, 1000), (3, 1000), (5, 1000), (4, 1000), (6, 1000),
              (7, 1000), (0, 9), (2, 25), (1, 15), (8, 9), (4, 25), (0, 1000))


def object_scene(name, sc: fc.FullScene, rows, forms, budgets: bool, aims=()) -> ManyScene:
    pdbs = list(sc.budgets) if budgets else []

    @functools.lru_cache(maxsize=None)
    def built():
        from ksim.preemption import bound_table
        b = fc.build(sc)
        table = bound_table(b.cluster, sc.bound, sc.start, b.cluster.topo, full_adds=True,
                            vol_limits=b.cluster.vol_limits, pdbs=pdbs) if budgets else b.table
        return Built(b.cluster, b.enc, table, b.prof), b

    @functools.lru_cache(maxsize=None)
    def answer(pod, prio):
        b = built()[1]
        got = preemptfullref.dry_run(b.nodes, sc.pvs, sc.pvcs, sc.bound, sc.start, sc.order, sc.pending[pod], prio,
                                     sc.args, None, filter_order=sc.filter_order, classes=sc.classes, pdbs=pdbs)
        res = preemptpdbref.as_indices(got, built()[0].cluster.node_names, sc.order)
        flags = {}
        if res[0] >= 0:                                  # the violating victims lead the list
            flags[res[0]] = {v: (3 if k < res[4] else 1) for k, v in enumerate(res[1])}
        return Answer(res, flags)

    def csr(node):
        name_of = built()[0].cluster.node_names[node]
        mine = [p for p in sc.bound if p.node_name == name_of]
        mine.sort(key=lambda p: (-p.priority, sc.start[p.name], sc.order[p.name]))
        return [sc.order[p.name] for p in mine]

    return ManyScene(name, list(rows), len(sc.nodes), len(sc.bound), answer, lambda pod: forms[pod], csr,
                     lambda: built()[0], budgets=pdbs, aims=tuple(aims))


# ---- the catalogue -----------------------------------------------------------------------------------------
def _geometry(n: int) -> pc.Case:
    """A preemptcases geometry case of ``n`` nodes whose ``want`` cut falls inside a pick chunk, the best candidate kept."""
    return next(c for c in pc.geometry_cases() if c.n_nodes == n and pc.inside_a_chunk(n, c.want) and
                c.best_rank < c.want)


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, ManyScene]:
    seq = pc.SEQUENCE
    out = [
        fit_scene("race", seq, RACE, [0, 1, 2, 3, 4, 1, 0], aims=("shared_flags", "row0_priority")),
        fit_scene("race_reversed", seq, RACE, [0, 1, 4, 3, 2, 1, 0][::-1] + [1, 0], aims=("shared_flags",)),
        fit_scene("one_row", seq, RACE, [1]),
        fit_scene("two_rows", seq, RACE, [1, 0], aims=("shared_flags",)),
        fit_scene("no_rows", seq, RACE, []),
        fit_scene("nobody_beside_everybody", seq, RACE, [3, 4], aims=("row0_priority",)),
    ]
    for n in (63, 64, 65, 130):
        out.append(fit_scene(f"rows_{n}", seq, RACE, [k % 5 for k in range(n)],
                             aims=(("second_group_dropped",) if n > 64 else ()) +
                             (("first_group_repeated",) if n == 130 else ())))
    for v in (63, 64, 65):
        c = victims_case(v)
        out.append(fit_scene(f"victims_{v}", c, [c.preemptor, (12, 9950)], [0, 1, 0],
                             aims=("victims_cut_64",) if v > 64 else ()))
        out.append(fit_scene(f"victims_{v}_guarded", c, [c.preemptor, (12, 9950)], [0, 1, 0], _every_third_guarded(c),
                             aims=("violating_order_lost",)))
    for n, target in ((1, 0), (255, 254), (256, 255), (257, 255), (257, 256)):
        c = edge_case(n, target)
        out.append(fit_scene(c.name, c, [c.preemptor, (30, 6000), (5, 6000)], [0, 1, 2, 1]))
    for n in (1025, 2049):
        c = _geometry(n)
        out.append(fit_scene(f"cut_{n}", c, [c.preemptor, (20, 6000), (60, 6000)], [0, 1, 2, 0]))
    sc = mixed()
    out.append(object_scene("mixed", sc, MIXED_ROWS, MIXED_FORM, False, aims=("grouped_order", "row0_priority")))
    out.append(object_scene("mixed_guarded", sc, MIXED_ROWS, MIXED_FORM, True, aims=("grouped_order",)))
    table = {s.name: s for s in out}
    assert len(table) == len(out)
    return table


def scene_ids() -> List[str]:
    return list(scenes())
