"""Scenes for the batched dry run of pods that read domain tables
(ksim_preempt_many_dom; csrc/ksim_preempt.hip k_preempt_many_dom,
k_preempt_many_mins, k_preempt_many_dom_nodes), and a Python model of the call
whose wrong readings (FAULTS) the scenes must tell from the right one:
tests/test_preempt_many_dom_cases.py on the CPU,
tests/test_gpu_preempt_many_dom.py on the device.

Every scene is a tests/preemptfullcases.py ``FullScene`` with several
preemptors, and a row's reference is ``preemptfullref.dry_run`` for its (pod,
priority), as in tests/preemptmanycases.py ``object_scene``.

The call gives every domain row a PreFilter state of its own.  To say what a
row answers when it reads another row's state, ``dry_run`` below restates the
dry run once more over an explicit ``State`` (the domain tables with their
presence marks, the critical-path minima, the affinity totals and flag, the
nodes PodTopologySpread counts), for the pods the scenes' domain rows are made
of: CPU requests, labels, DoNotSchedule constraints, required pod affinity and
anti-affinity terms over match_labels selectors, no tolerations.  The CPU test
holds it against the reference for every such row.  Rows it does not cover
(volumes, ports: ``simple`` is false) keep the reference's answer under every
wrong reading of the state; the wrong readings of the grouping cover all rows.

Launch groups: forms 0 (ports / free) and 1 (volume) as in ksim_preempt_many,
then 2 (affinity / spread) and 3 (the same beside counted volumes), 64 rows
each in every scene here (``dom_rows`` restates ksim_preempt_many_dom_rows)."""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import preemptfullcases as fc
import preemptfullref
import preemptmanycases as mc
import preemptpdbref
from ksim.model import LabelSelector, PodAffinityTerm, Taint, TopologySpreadConstraint

MAX_ROWS, SLAB_BYTES, NODE_BYTES, MAX_USES = mc.MAX_ROWS, mc.SLAB_BYTES, mc.NODE_BYTES, 16
SENTINEL = mc.SENTINEL
ZONE, HOST, REGION = fc.ZONE, fc.HOST, "topology.kubernetes.io/region"
X, Y, Q, DB = fc.X, fc.Y, {"app": "q"}, fc.DB
NONE_LEFT = 2 ** 31 - 1                            # math.MaxInt32: no (other) present domain
FAULTS = ("row0_tables",                           # every row of a group reads row 0's domain tables
          "row0_afftot",                           # row 0's affinity totals and flag are shared
          "row0_minima",                           # row 0's critical-path minima are shared
          "tables_not_zeroed",                     # the previous group's sums stay in the slab
          "presence_mark_dropped",                 # the minimum runs over absent pairs
          "row0_eligibility",                      # the nodes PodTopologySpread counts are row 0's
          "grouped_order",                         # the answers come back in form-grouped order
          "second_group_dropped",                  # a launch group is never launched
          "first_group_repeated")                  # ... or the one before it is launched again in its place


def dom_rows(n_nodes: int, n_bound: int, n_values: int) -> int:
    per = NODE_BYTES * max(n_nodes, 0) + max(n_bound, 0) + 8 * MAX_USES * max(n_values, 0)
    return max(1, min(MAX_ROWS, SLAB_BYTES // per)) if per > 0 else MAX_ROWS


# ---- the dry run over an explicit PreFilter state ---------------------------------------------------
def milli(q: str) -> int:
    return int(q[:-1]) if q.endswith("m") else int(round(float(q) * 1000))


def _cpu(p) -> int:
    return sum(milli(c.requests.get("cpu", "0")) for c in p.containers)


@dataclass
class Use:
    kind: str                                      # "hard", "anti" or "aff"
    key: str
    sel: Dict[str, str]
    skew: int = 0
    honor_taints: bool = False


def uses_of(p) -> List[Use]:
    out = [Use("hard", c.topology_key, dict(c.label_selector.match_labels), c.max_skew, c.node_taints_policy == "Honor")
           for c in p.topology_spread if c.when_unsatisfiable == "DoNotSchedule"]
    out += [Use("anti", t.topology_key, dict(t.label_selector.match_labels)) for t in p.pod_anti_affinity_required]
    out += [Use("aff", t.topology_key, dict(t.label_selector.match_labels)) for t in p.pod_affinity_required]
    return out


def simple(p) -> bool:
    """A pod ``dry_run`` below covers, with at least one use that reads a domain table."""
    return bool(uses_of(p)) and not p.pvc_claims and not any(c.ports for c in p.containers) and not p.tolerations \
        and not p.node_selector and not p.required_terms and \
        all(c.when_unsatisfiable == "DoNotSchedule" and c.node_affinity_policy is None for c in p.topology_spread)


def _match(sel: Dict[str, str], labels: Dict[str, str]) -> bool:
    return all(labels.get(k) == v for k, v in sel.items())


def _tainted(node) -> bool:
    return any(t.effect in ("NoSchedule", "NoExecute") for t in node.taints)


@dataclass
class State:
    """What the PreFilter pass leaves for one pod, use by use."""
    tables: List[Dict[str, List[int]]]             # value -> [count, presence marks]
    minima: List[Tuple[int, Optional[str], int]]   # hard uses: (min1, one arg-min's value, min2)
    afftot: List[int]
    flag: bool                                     # len(affinityCounts) > 0
    elig: List[Dict[str, bool]]                    # hard uses: node name -> its pods count


def minima_of(table: Dict[str, List[int]], marks: bool = True) -> Tuple[int, Optional[str], int]:
    present = sorted((c, v) for v, (c, m) in table.items() if m > 0 or not marks)
    if not present:
        return (NONE_LEFT, None, NONE_LEFT)
    return (present[0][0], present[0][1], present[1][0] if len(present) > 1 else NONE_LEFT)


def prefilter(sc, pod, elig_of=None, marks: bool = True) -> State:
    """k_topo_prefilter's rule for ``pod``.  ``elig_of``: the pod whose
    constraints say which nodes count (a wrong reading; default ``pod``)."""
    uses, eu = uses_of(pod), uses_of(elig_of or pod)
    per_node = {n.name: [q for q in sc.bound if q.node_name == n.name] for n in sc.nodes}
    hard_keys = [u.key for u in eu if u.kind == "hard"]
    st = State([{} for _ in uses], [(0, None, 0)] * len(uses), [0] * len(uses), False, [{} for _ in uses])
    for i, u in enumerate(uses):
        honor = eu[i].honor_taints if i < len(eu) and eu[i].kind == "hard" else False
        for n in sc.nodes:
            v = n.labels.get(u.key)
            cnt = sum(1 for q in per_node[n.name] if _match(u.sel, q.labels))
            if u.kind == "hard":
                ok = all(k in n.labels for k in hard_keys) and not (honor and _tainted(n))
                st.elig[i][n.name] = ok and v is not None
                if v is None:
                    continue
                e = st.tables[i].setdefault(v, [0, 0])             # (an absent pair: a zero entry without a mark)
                if ok:
                    e[0] += cnt
                    e[1] += 1
            elif v is not None:
                st.tables[i].setdefault(v, [0, 0])[0] += cnt
                if u.kind == "aff":
                    st.afftot[i] += cnt
                    st.flag |= cnt > 0
        if u.kind == "hard":
            st.minima[i] = minima_of(st.tables[i], marks)
    return st


def _ipa(uses, self_aff, flag, node, count) -> str:
    """interpodaffinity Filter -> "", "affinity" or "anti"; count(i): use i's entry for the node."""
    missing = exist = False
    pods_exist = True
    for i, u in enumerate(uses):
        has = u.key in node.labels
        if u.kind == "aff":
            if not has:
                missing = True
            elif count(i) <= 0:
                pods_exist = False
        if u.kind == "anti" and has and count(i) > 0:
            exist = True
    if missing:
        return "affinity"
    if any(u.kind == "aff" for u in uses) and not pods_exist and not (not flag and self_aff):
        return "affinity"
    return "anti" if exist else ""


def dry_run(sc, pod, prio: int, st: State, nodes=None) -> tuple:
    """SelectVictimsOnNode on every potential node and the pick, over ``st``:
    (node index or -1, victims as table rows, potential nodes, candidates kept, 0).
    ``nodes``: the scene's nodes in the cluster's (nodeTree) order, which the
    node indices and the candidates' order follow."""
    order = list(sc.filter_order)
    uses = uses_of(pod)
    self_m = [_match(u.sel, pod.labels) for u in uses]
    self_aff = all(s for u, s in zip(uses, self_m) if u.kind == "aff")
    need = _cpu(pod)
    cands, n_pot = [], 0
    for ni, n in enumerate(sc.nodes if nodes is None else nodes):
        mine = sorted((q for q in sc.bound if q.node_name == n.name),
                      key=lambda q: (-q.priority, sc.start[q.name], sc.order[q.name]))
        val = [n.labels.get(u.key) for u in uses]
        entry = [st.tables[i].get(val[i], [0, 0])[0] if val[i] is not None else 0 for i in range(len(uses))]
        # the status: the first failing filter in the profile's order
        first = None
        for pl in order:
            if pl == "TaintToleration" and _tainted(n):
                first = pl
            elif pl == "NodeResourcesFit" and sum(_cpu(q) for q in mine) + need > milli(n.allocatable["cpu"]):
                first = pl
            elif pl == "PodTopologySpread":
                for i, u in enumerate(uses):
                    if u.kind == "hard" and first is None:
                        if val[i] is None:
                            first = "missing"
                        elif entry[i] + self_m[i] - st.minima[i][0] > u.skew:
                            first = pl
            elif pl == "InterPodAffinity" and _ipa(uses, self_aff, st.flag, n, lambda i: entry[i]):
                first = pl if _ipa(uses, self_aff, st.flag, n, lambda i: entry[i]) == "anti" else "affinity"
            if first is not None:
                break
        if first not in ("NodeResourcesFit", "PodTopologySpread", "InterPodAffinity"):
            continue
        # the trial state: the node's own entries move, and per constraint the minimum over the other domains stands
        moved = list(entry)
        elig = [u.kind == "hard" and st.elig[i].get(n.name, False) for i, u in enumerate(uses)]
        others = [0] * len(uses)
        for i, u in enumerate(uses):
            if u.kind == "hard":
                m1, at, m2 = st.minima[i]
                others[i] = m2 if elig[i] and val[i] == at else m1
        outside = any(u.kind == "aff" and val[i] is not None and st.afftot[i] - entry[i] > 0 for i, u in enumerate(uses))
        load = sum(_cpu(q) for q in mine)

        def move(q, sign):
            nonlocal load
            load += sign * _cpu(q)
            for i, u in enumerate(uses):
                if _match(u.sel, q.labels) and (elig[i] if u.kind == "hard" else True):
                    moved[i] += sign

        def fails() -> bool:
            if "NodeResourcesFit" in order and load + need > milli(n.allocatable["cpu"]):
                return True
            if "PodTopologySpread" in order:
                for i, u in enumerate(uses):
                    if u.kind != "hard":
                        continue
                    crit = min(moved[i], others[i]) if elig[i] else others[i]
                    if val[i] is None or moved[i] + self_m[i] - crit > u.skew:
                        return True
            if "InterPodAffinity" in order:
                flag = outside or any(u.kind == "aff" and val[i] is not None and moved[i] > 0 for i, u in enumerate(uses))
                return _ipa(uses, self_aff, flag, n, lambda i: moved[i]) != ""
            return False
        n_pot += 1
        lower = [q for q in mine if q.priority < prio]
        for q in lower:
            move(q, -1)
        if fails():
            continue
        victims = []
        for q in lower:
            move(q, 1)
            if fails():
                move(q, -1)
                victims.append(q)
        if victims:
            top = victims[0].priority
            early = min(sc.start[q.name] for q in victims if q.priority == top)
            key = (0, top, sum(q.priority + 2 ** 31 for q in victims), len(victims), -early)
        else:
            key = (0, -2 ** 31, 0, 0, -(2 ** 63 - 1))
        cands.append((ni, key, [sc.order[q.name] for q in victims]))
    pct, mabs = sc.args
    want = min(max(n_pot * pct // 100, mabs), n_pot)
    kept = cands[:want]
    if not kept:
        return (-1, [], n_pot, 0, 0)
    node, _, victims = min(kept, key=lambda c: c[1] + (c[0],))
    return (node, victims, n_pot, len(kept), 0)


def _summed(a: State, b: State) -> List[Dict[str, List[int]]]:
    """Row a's tables on a slab that still holds row b's sums, use by use."""
    out = []
    for i, t in enumerate(a.tables):
        t = {v: list(e) for v, e in t.items()}
        for v, e in (b.tables[i].items() if i < len(b.tables) else ()):
            cur = t.setdefault(v, [0, 0])
            cur[0] += e[0]
            cur[1] += e[1]
        out.append(t)
    return out


# ---- the call, modelled -----------------------------------------------------------------------------
def call_model(sc, rows, reference: Callable[[int, int], tuple], form: Callable[[int], int],
               fault: Optional[str] = None, rows_per_group: int = MAX_ROWS, nodes=None) -> list:
    """ksim_preempt_many_dom over ``rows`` [(pod, priority)]: per form, launch
    groups of ``rows_per_group`` rows; a covered domain row's answer is
    ``dry_run`` over the state the (wrong) reading hands it, every other row's
    the reference's.  One 5-tuple per row, in the caller's order."""
    assert fault is None or fault in FAULTS
    n = len(rows)
    groups = []
    for f in (0, 1, 2, 3):
        members = [i for i in range(n) if form(rows[i][0]) == f]
        groups += [members[k:k + rows_per_group] for k in range(0, len(members), rows_per_group)]
    state = functools.lru_cache(maxsize=None)(lambda pod: prefilter(sc, sc.pending[pod]))
    outs = [SENTINEL] * n
    for gi, g in enumerate(groups):
        if fault == "second_group_dropped" and gi == 1:
            continue
        src = groups[gi - 1] if fault == "first_group_repeated" and gi >= 1 else g
        for k, i in enumerate(g):
            pod, prio = rows[src[k % len(src)]]
            p = sc.pending[pod]
            if form(pod) < 2 or not simple(p) or fault in (None, "grouped_order", "second_group_dropped",
                                                           "first_group_repeated"):
                outs[i] = reference(pod, prio)
                continue
            st, p0 = state(pod), sc.pending[rows[g[0]][0]]
            st0 = state(rows[g[0]][0]) if simple(p0) else st
            if fault == "row0_tables":
                pad = [{} for _ in st.tables]
                st = dataclasses.replace(st, tables=(st0.tables + pad)[:len(st.tables)])
            elif fault == "row0_afftot":
                pad = [0] * len(st.afftot)
                st = dataclasses.replace(st, afftot=(st0.afftot + pad)[:len(st.afftot)], flag=st0.flag)
            elif fault == "row0_minima":
                pad = [(0, None, 0)] * len(st.minima)
                st = dataclasses.replace(st, minima=(st0.minima + pad)[:len(st.minima)])
            elif fault == "tables_not_zeroed" and gi >= 1 and form(rows[groups[gi - 1][0]][0]) >= 2:
                prev = groups[gi - 1]
                if k < len(prev) and simple(sc.pending[rows[prev[k]][0]]):
                    tables = _summed(st, state(rows[prev[k]][0]))
                    st = dataclasses.replace(st, tables=tables, minima=[
                        minima_of(t) if u.kind == "hard" else m for t, u, m in zip(tables, uses_of(p), st.minima)])
            elif fault == "presence_mark_dropped":
                st = prefilter(sc, p, marks=False)
            elif fault == "row0_eligibility" and simple(p0):
                st = prefilter(sc, p, elig_of=p0)
            outs[i] = dry_run(sc, p, prio, st, nodes)
    if fault == "grouped_order":
        outs = [outs[i] for g in groups for i in g]
    return outs


# ---- scenes --------------------------------------------------------------------------------------------
@dataclass
class DomScene:
    name: str
    sc: fc.FullScene
    rows: List[Tuple[int, int]]                      # (pending pod, priority), the caller's order
    aims: Tuple[str, ...] = ()                       # the wrong readings the scene is there to tell
    budgets: bool = False
    _built: list = field(default_factory=list)

    def built(self):
        if not self._built:
            from ksim.preemption import bound_table
            b = fc.build(self.sc)
            if not b.cluster.vol_limits.families:            # no volume table: the engine takes no holdings
                b.table.vol_off = b.table.vol_uses = None
            if self.budgets:
                b.table = bound_table(b.cluster, self.sc.bound, self.sc.start, b.cluster.topo, full_adds=True,
                                      vol_limits=b.cluster.vol_limits, pdbs=list(self.sc.budgets))
            self._built.append(b)
        return self._built[0]

    def form(self, pod: int) -> int:
        """The launch group's form of a pending pod, from its compiled uses and the scene's filter list."""
        from ksim import abi
        b = self.built()
        p = b.enc.pods[pod]
        kinds = [int(k) for k in b.enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]]
        order = self.sc.filter_order
        dom = ("InterPodAffinity" in order and any(k in (abi.USE_IPA_AFFINITY, abi.USE_IPA_ANTI,
                                                          abi.USE_IPA_EXISTING_ANTI) for k in kinds)) or \
            ("PodTopologySpread" in order and abi.USE_PTS_HARD in kinds)
        vol = abi.USE_VOLUME in kinds
        return (3 if vol else 2) if dom else (1 if vol else 0)

    def answer(self, pod: int, prio: int) -> tuple:
        return _answer(self, pod, prio)

    def reference(self) -> list:
        return [self.answer(pod, prio) for pod, prio in self.rows]

    def model(self, fault: Optional[str] = None) -> list:
        return call_model(self.sc, self.rows, self.answer, self.form, fault, nodes=self.built().nodes)


@functools.lru_cache(maxsize=None)
def _answer(s: DomScene, pod: int, prio: int) -> tuple:
    sc, b = s.sc, s.built()
    pdbs = list(sc.budgets) if s.budgets else []
    got = preemptfullref.dry_run(b.nodes, sc.pvs, sc.pvcs, sc.bound, sc.start, sc.order, sc.pending[pod], prio, sc.args,
                                 None, filter_order=sc.filter_order, classes=sc.classes, pdbs=pdbs)
    return preemptpdbref.as_indices(got, b.cluster.node_names, sc.order)


DomScene.__hash__ = lambda self: id(self)            # noqa: E731  (the cache's key: one object per scene)
DomScene.__eq__ = lambda self, other: self is other  # noqa: E731


def _zoned(name: str, zones: Dict[str, int], cpu: str = "10", **extra) -> fc.FullScene:
    """Nodes n0000.. zone by zone (preemptaffcases' layout), 10 CPUs each."""
    s = fc.FullScene(name, **extra)
    for z, k in zones.items():
        for _ in range(k):
            lab = {ZONE: z} if z else {}
            s.node(f"n{len(s.nodes):04d}", None, lab, cpu)
    return s


def _rows(s: fc.FullScene, rows) -> None:
    """(node, priority, start, cpu milli, labels) rows in table order."""
    for k, (v, prio, start, cpu, labels) in enumerate(rows):
        s.bpod(f"b{k}", f"n{v:04d}", prio, cpu=f"{cpu}m", start=start, labels=labels)


def _spread(key=ZONE, skew=1, labels=X, **policies) -> TopologySpreadConstraint:
    return TopologySpreadConstraint(skew, key, "DoNotSchedule", LabelSelector(dict(labels)), **policies)


def _pre(s: fc.FullScene, name: str, **kw):
    p = s.preemptor(**kw)
    p.name = name
    return p


def selectors_differ() -> fc.FullScene:
    """za x2, zb x2; maxSkew 1 on the zone.  app=x: za = 2 (node 0: priorities
    20 and 10), zb = 0.  app=y: za = 0, zb = 2 (node 2: 20 and 10).  The x
    preemptor fails the skew on za and takes node 0's two x pods, the y
    preemptor the mirror image on node 2; node 3 is full of a pod that outranks
    both.  A row that reads the other's tables sees the skew on the wrong zone."""
    s = _zoned("selectors_differ", {"za": 2, "zb": 2})
    _rows(s, [(0, 20, 100, 1000, X), (0, 10, 100, 1000, X), (2, 20, 100, 1000, Y), (2, 10, 100, 1000, Y),
              (3, 2000, 100, 9950, None)])
    _pre(s, "x", labels=X, spread=[_spread()])
    _pre(s, "y", labels=Y, spread=[_spread(labels=Y)])
    return s


def affinity_only_here() -> fc.FullScene:
    """Required zone affinity.  Pod 0 (app=w) wants app=db, which lives on nodes
    2 and 3 (zb, priority 2000); node 2 is short of CPU beside its hog (5), the
    victim.  Pod 1 (app=q) wants app=q: the only q pod (10) sits on node 0 (za)
    beside a hog (5), nothing outside.  With both out no q pod is left anywhere,
    the pod matches its own term and passes; the q pod back fits, the hog does
    not.  With pod 0's totals the state "nobody matches" is never seen: node 0
    fails with everybody out and is no candidate."""
    s = _zoned("affinity_only_here", {"za": 2, "zb": 2})
    _rows(s, [(0, 10, 100, 1000, Q), (0, 5, 100, 8950, None), (1, 2000, 100, 9950, None),
              (2, 2000, 100, 1000, DB), (2, 5, 100, 8950, None), (3, 2000, 100, 9950, DB)])
    _pre(s, "wants_db", labels={"app": "w"}, aff=[PodAffinityTerm(ZONE, LabelSelector(dict(DB)))])
    _pre(s, "wants_q", labels=Q, aff=[PodAffinityTerm(ZONE, LabelSelector(dict(Q)))])
    return s


def minima_differ() -> fc.FullScene:
    """Five nodes of one region, zones za x2, zb x2, zc.  app=x by zone: za = 2,
    zb = 1, zc = 1, the two minima tie (tests/preemptspreadcases.py tied_minima).
    app=y by region: the only domain holds 4, so there is no other minimum
    (MaxInt32) and the skew is the pod's own 1 whatever moves (only_domain).
    Node 2 is short of CPU for both 4-CPU preemptors: the hog goes.  A y row on
    the x row's minima (1, 1) sees 4 + 1 - 1 > 1 on every node."""
    s = fc.FullScene("minima_differ")
    for z in ("za", "za", "zb", "zb", "zc"):
        s.node(f"n{len(s.nodes):04d}", None, {ZONE: z, REGION: "r1"}, "10")
    _rows(s, [(0, 10, 100, 1000, X), (1, 2000, 100, 9500, X), (2, 30, 100, 1000, X), (2, 20, 100, 8000, None),
              (3, 2000, 100, 9500, None), (4, 2000, 100, 9500, X),
              (0, 2000, 100, 500, Y), (1, 2000, 100, 100, Y), (2, 2000, 100, 500, Y), (4, 2000, 100, 100, Y)])
    _pre(s, "x", cpu="4000m", labels=X, spread=[_spread()])
    _pre(s, "y", cpu="4000m", labels=Y, spread=[_spread(REGION, labels=Y)])
    return s


def honor_beside_ignore() -> fc.FullScene:
    """The layout of tests/preemptspreadcases.py tainted_node_moves_nothing (no
    TaintToleration in the profile; node 0 tainted, its two x pods below the
    preemptor), with the same selector twice.  Under nodeTaintsPolicy Honor node
    0 counts nowhere: za = 3, zb = 2, and node 1 without its priority-30 pod
    brings za to 2: the victim.  Under the default it counts: za = 5, and no
    node's removals bring za to 3.  Pod 2 spreads over the hostname with Honor:
    node 0's pair is absent, the minimum (1) runs over nodes 1 to 4 and node 1
    (2) gives up the same pod; without the presence mark the minimum is 0."""
    s = _zoned("honor_beside_ignore", {"za": 3, "zb": 2}, filter_order=fc.without("TaintToleration"))
    s.nodes[0].taints = [Taint("dedicated", "batch", "NoSchedule")]
    _rows(s, [(0, 10, 100, 1000, X), (0, 20, 100, 1000, X), (1, 2000, 100, 1000, X), (1, 30, 90, 1000, X),
              (2, 2000, 100, 1000, X), (3, 2000, 100, 9500, X), (4, 2000, 100, 9500, X)])
    _pre(s, "honor", labels=X, spread=[_spread(node_taints_policy="Honor")])
    _pre(s, "ignore", labels=X, spread=[_spread()])
    _pre(s, "hosts", labels=X, spread=[_spread(HOST, node_taints_policy="Honor")])
    return s


def host_spread(n: int) -> fc.FullScene:
    """maxSkew 1 on the hostname over app=x on ``n`` nodes (a table of n values):
    every node holds one x pod that outranks the preemptor, the last one two more
    (20 and 10): both go."""
    s = _zoned(f"host_spread_{n}", {"z0": n})
    rows = [(v, 2000, 100, 1000, X) for v in range(n)] + [(n - 1, 20, 100, 1000, X), (n - 1, 10, 100, 1000, X)]
    _rows(s, rows)
    _pre(s, "hosts", labels=X, spread=[_spread(HOST)])
    _pre(s, "hosts_anti", labels=Y, terms=[fc.anti()], cpu="9000m")
    return s


def many_zones(z: int) -> fc.FullScene:
    """``z`` zones of one node (z + 1 value ids with the absent one: 128 ids are
    staged in LDS, 129 are not), one x pod below the preemptor on every node and
    a second one on the last: maxSkew 1 fails there alone, and either goes."""
    s = _zoned(f"zones_{z}", {f"z{k:03d}": 1 for k in range(z)})
    _rows(s, [(v, 10 + v % 5, 100, 1000, X) for v in range(z)] + [(z - 1, 3, 100, 1000, X)])
    _pre(s, "zones", labels=X, spread=[_spread()])
    _pre(s, "zones_aff", labels=Y, aff=[PodAffinityTerm(ZONE, LabelSelector(dict(X)))], cpu="9500m")
    return s


def one_node() -> fc.FullScene:
    s = _zoned("one_node", {"za": 1})
    _rows(s, [(0, 10, 100, 1000, X), (0, 5, 100, 1000, None)])
    _pre(s, "anti", terms=[fc.anti()])
    _pre(s, "spread", labels=X, spread=[_spread(HOST)])
    return s


def two_priorities() -> fc.FullScene:
    """Node 0 holds x pods of priority 20 and 10 and a bystander (5); node 1 is
    full.  Hostname anti-affinity against app=x at priority 1000 takes both x
    pods; an x pod with maxSkew 2 over the hostname (node 1 counts 0) at
    priority 15 takes the second alone: one node, two victim lists."""
    s = _zoned("two_priorities", {"za": 2})
    _rows(s, [(0, 20, 100, 1000, X), (0, 10, 100, 1000, X), (0, 5, 100, 1000, None), (1, 2000, 100, 9950, None)])
    _pre(s, "anti", terms=[fc.anti()])
    _pre(s, "spread", labels=X, spread=[_spread(HOST, 2)])
    return s


def routes() -> fc.FullScene:
    """tests/preemptmanycases.py mixed() (pods 0 to 9: Fit only, a port, volumes,
    the static veto, uses no Filter reads, hostname anti-affinity, DoNotSchedule
    spread) with the StatefulSet replica as pod 10 (a volume, hostname
    anti-affinity and a zone spread: the full form) and a zone anti-affinity
    pod as pod 11."""
    s = mc.mixed()
    s.name = "routes"
    _pre(s, "replica", vols=[("ebs", "r")], cpu="4000m", labels=X, terms=[fc.anti()], spread=[fc.hard(skew=5)])
    _pre(s, "zone_anti", cpu="4000m", terms=[fc.anti(ZONE)])
    return s


ROUTES_ROWS = ((8, 1000), (0, 1000), (10, 1000), (2, 1000), (1, 1000), (9, 1000), (3, 1000), (11, 1000), (5, 1000),
               (4, 1000), (10, 9), (6, 1000), (7, 1000), (0, 9), (9, 25), (2, 25), (1, 15), (8, 9), (10, 25), (4, 25),
               (11, 9), (0, 1000))


def _alternating(n: int) -> List[Tuple[int, int]]:
    """Rows of pods 0 and 1 in turn; from row 64 on the other way round, so row
    64 + k (place k of the second group) has another selector than row k."""
    return [((i + (i >= MAX_ROWS)) % 2, 1000) for i in range(n)]


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, DomScene]:
    sd, hb = selectors_differ(), honor_beside_ignore()
    out = [
        DomScene("selectors_differ", sd, [(0, 1000), (1, 1000), (1, 15), (0, 15)], aims=("row0_tables",)),
        DomScene("affinity_only_here", affinity_only_here(), [(0, 1000), (1, 1000)], aims=("row0_afftot",)),
        DomScene("minima_differ", minima_differ(), [(0, 1000), (1, 1000)], aims=("row0_minima",)),
        DomScene("honor_beside_ignore", hb, [(1, 1000), (0, 1000), (2, 1000)],
                 aims=("row0_eligibility", "presence_mark_dropped")),
        DomScene("one_node", one_node(), [(0, 1000), (1, 1000), (0, 7)]),
        DomScene("two_priorities", two_priorities(), [(0, 1000), (1, 15), (1, 1000), (0, 15)]),
        DomScene("routes", routes(), list(ROUTES_ROWS), aims=("grouped_order", "second_group_dropped")),
        DomScene("routes_guarded", routes(), list(ROUTES_ROWS), aims=("grouped_order",), budgets=True),
    ]
    for n in (1, 2, 63, 64, 65, 130):
        out.append(DomScene(f"rows_{n}", sd, _alternating(n),
                            aims=(("tables_not_zeroed", "second_group_dropped", "first_group_repeated")
                                  if n > 64 else ())))
    for n in (255, 256, 257):
        be = fc.block_edge(n)
        out.append(DomScene(be.name, be, [(0, 1000), (0, 8), (0, 12), (0, 1000)]))
    for n in (255, 256, 257, 300):
        out.append(DomScene(f"host_spread_{n}", host_spread(n), [(0, 1000), (1, 1000), (0, 15)]))
    for z in (127, 128):
        out.append(DomScene(f"zones_{z}", many_zones(z), [(0, 1000), (1, 1000), (0, 5)]))
    table = {s.name: s for s in out}
    assert len(table) == len(out)
    return table


def scene_ids() -> List[str]:
    return list(scenes())
