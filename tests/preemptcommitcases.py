"""Scenes and a plain model for ksim_preempt_commit (csrc/ksim_preempt.hip, the
k_commit_* kernels; csrc/ksim_preempt_host.cpp).

The model (``Model``) is the bound table as a Python list of caller rows in the
table's order, an eviction as a deletion from that list, and the snapshot as
dicts.  ``flat()`` writes the list out as the arrays the device keeps (per-node
offsets, the position -> caller row index, the rows' columns and the three
lists as CSRs) and ``view()`` reads arrays back per node, so a wrong reading of
the compaction (FLAWS) is a wrong way to get from the arrays before a commit to
the arrays after it.  tests/test_preempt_commit_cases.py shows on the CPU that
the model scenes tell every such reading from the model;
tests/test_gpu_preempt_commit.py runs the engine on the engine scenes below and
compares with the model's snapshot and with the rebuild form.

Model scenes are rows written by hand: (node, priority, start, cpu, adds, budget
ids, volume holdings).  Engine scenes are model objects (tests/preemptfullcases.py
FullScene) with ``steps``: the bound pods each commit evicts, by name."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

FLAWS = ("order_not_kept",            # the hole is filled with the table's last row
         "off_not_moved",             # the nodes' offsets stay where they were
         "dead_entries_left",         # the lists' entries are not compacted, only their offsets
         "entries_from_new_offset",   # a survivor's entries are read at its new offset of the old array
         "victims_compacted",         # later victims are numbered by position among the survivors
         "nz_not_returned",           # the non-zero requests stay on the node
         "last_holder_skipped",       # the last holder of a shared volume leaves it attached
         "last_holder_twice",         # two victims sharing a volume both detach it
         "dead_evictable_again",      # a row evicted before is taken again
         "budget_ids_shifted")        # the budget lists keep their old offsets: a survivor reads its predecessor's


class Refused(Exception):
    def __init__(self, entry: int, why: str):
        super().__init__(f"entry {entry}: {why}")
        self.entry, self.why = entry, why


@dataclass
class Row:
    node: int
    prio: int
    start: int
    cpu: int = 100
    adds: Tuple[Tuple[int, int], ...] = ()        # (class, count)
    pids: Tuple[int, ...] = ()                    # budget ids
    vols: Tuple[Tuple[int, int, int], ...] = ()   # (class or -1, family, count)
    nz_cpu: Optional[int] = None                  # the record's non-zero requests (None: cpu / 200 MB)
    nz_mem: int = 200
    nb: int = 0                                   # the record's bandwidth add


LISTS = ("adds", "pids", "vols")


@dataclass
class Flat:
    """The device's arrays."""
    off: List[int]
    index: List[int]
    cols: List[tuple]                             # per position (prio, start, cpu)
    loff: Dict[str, List[int]]
    lent: Dict[str, list]


class Model:
    def __init__(self, n_nodes: int, rows: Sequence[Row], flaw: Optional[str] = None, lists: Sequence[str] = LISTS):
        assert flaw is None or flaw in FLAWS
        self.n_nodes, self.rows, self.flaw, self.lists = n_nodes, list(rows), flaw, tuple(lists)
        # util.MoreImportantPod per node, then table order
        self.table = sorted(range(len(rows)), key=lambda i: (rows[i].node, -rows[i].prio, rows[i].start, i))
        self.dead = set()
        self.arr = self.flat()
        self.node = [dict(cpu=0, nz_cpu=0, nz_mem=0, num_pods=0, nb=0) for _ in range(n_nodes)]
        self.cnt: Dict[Tuple[int, int], int] = {}          # (class, node) -> count
        self.att: Dict[Tuple[int, int], int] = {}          # (family, node) -> attached volumes
        for r in rows:
            self._move(r, 1)

    # ---- the snapshot ------------------------------------------------------------------------
    def _move(self, r: Row, sign: int, last_holder: str = "rule") -> None:
        v = self.node[r.node]
        v["cpu"] += sign * r.cpu
        if not (sign < 0 and self.flaw == "nz_not_returned"):
            v["nz_cpu"] += sign * (r.cpu if r.nz_cpu is None else r.nz_cpu)
            v["nz_mem"] += sign * r.nz_mem
        v["num_pods"] += sign
        v["nb"] += sign * r.nb
        for cls, count in r.adds:
            self.cnt[(cls, r.node)] = self.cnt.get((cls, r.node), 0) + sign * count
        for cls, fam, count in r.vols:
            if cls < 0:
                self.att[(fam, r.node)] = self.att.get((fam, r.node), 0) + sign * count
                continue
            old = self.cnt.get((cls, r.node), 0)
            self.cnt[(cls, r.node)] = old + sign
            edge = old == 0 if sign > 0 else old == 1      # volume_bind: the first holder attaches, the last detaches
            if sign < 0 and self.flaw == "last_holder_skipped":
                edge = False
            if sign < 0 and self.flaw == "last_holder_twice":
                edge = old <= 2
            if edge:
                self.att[(fam, r.node)] = self.att.get((fam, r.node), 0) + sign

    def snapshot(self) -> dict:
        return dict(node=[dict(v) for v in self.node], cnt={k: c for k, c in self.cnt.items() if c},
                    att={k: c for k, c in self.att.items() if c})

    # ---- the table as arrays -------------------------------------------------------------------
    def flat(self) -> Flat:
        off = [0] * (self.n_nodes + 1)
        for i in self.table:
            off[self.rows[i].node + 1] += 1
        for v in range(self.n_nodes):
            off[v + 1] += off[v]
        loff, lent = {}, {}
        for name in self.lists:
            loff[name], lent[name] = [0], []
            for i in self.table:
                lent[name].extend(getattr(self.rows[i], name))
                loff[name].append(len(lent[name]))
        return Flat(off, list(self.table), [(self.rows[i].prio, self.rows[i].start, self.rows[i].cpu) for i in self.table],
                    loff, lent)

    def view(self) -> List[List[tuple]]:
        """Per node its rows in table order: (caller row, prio, start, cpu, adds, pids, vols), read from the arrays."""
        a, out = self.arr, []
        for v in range(self.n_nodes):
            rows = []
            for k in range(a.off[v], a.off[v + 1]):
                if k >= len(a.index):
                    rows.append(("past the end", k))
                    continue
                ent = tuple(tuple(a.lent[n][a.loff[n][k]:a.loff[n][k + 1]]) if n in a.loff else None for n in LISTS)
                rows.append((a.index[k],) + a.cols[k] + ent)
            out.append(rows)
        return out

    def victims_below(self, node: int, prio: int) -> List[int]:
        """The rows of ``node`` a preemptor of priority ``prio`` may evict, as a later dry run numbers them."""
        got = [r[0] for r in self.view()[node] if r[0] != "past the end" and r[1] < prio]
        if self.flaw == "victims_compacted":
            got = [r - sum(d < r for d in self.dead) for r in got]
        return got

    # ---- the commit -------------------------------------------------------------------------------
    def commit(self, victims: Sequence[int], cpus: Optional[Sequence[int]] = None) -> None:
        """``cpus``: the records' cpu requests (None: the rows' own)."""
        seen = set()
        for i, r in enumerate(victims):                    # everything is checked before anything moves
            if not 0 <= r < len(self.rows):
                raise Refused(i, "row outside the table")
            if r in self.dead and self.flaw != "dead_evictable_again":
                raise Refused(i, "row already evicted")
            if r in seen:
                raise Refused(i, "row named twice")
            if cpus is not None and cpus[i] != self.rows[r].cpu:
                raise Refused(i, "requests differ")
            seen.add(r)
        before = self.arr
        for r in victims:
            self._move(self.rows[r], -1)
        gone = [before.index.index(r) for r in victims if r in self.table]
        for r in victims:
            if r in self.table:
                self.table.remove(r)                       # the eviction: a deletion from the list
            self.dead.add(r)
        self.arr = self._compact(before, sorted(gone), self.flat())

    def _compact(self, a: Flat, gone: List[int], good: Flat) -> Flat:
        """The arrays after the commit.  ``good``: the list written out again."""
        f = self.flaw
        if f == "order_not_kept":
            index, cols = list(a.index), list(a.cols)
            ent = {n: [a.lent[n][a.loff[n][k]:a.loff[n][k + 1]] for k in range(len(a.index))] for n in a.loff}
            for k in reversed(gone):                       # the last row into the hole
                for arr in [index, cols] + list(ent.values()):
                    arr[k] = arr[-1]
                    arr.pop()
            loff, lent = {}, {}
            for n in ent:
                loff[n], lent[n] = [0], []
                for e in ent[n]:
                    lent[n].extend(e)
                    loff[n].append(len(lent[n]))
            return Flat(good.off, index, cols, loff, lent)
        if f == "off_not_moved":
            return Flat(a.off, good.index, good.cols, good.loff, good.lent)
        if f == "dead_entries_left":
            return Flat(good.off, good.index, good.cols, good.loff, dict(a.lent))
        if f == "entries_from_new_offset":
            lent = {n: [a.lent[n][e] for e in range(len(good.lent[n]))] for n in good.loff}
            return Flat(good.off, good.index, good.cols, good.loff, lent)
        if f == "budget_ids_shifted" and "pids" in a.loff:
            loff = dict(good.loff)
            loff["pids"] = a.loff["pids"][:len(good.index) + 1]
            lent = dict(good.lent)
            lent["pids"] = list(a.lent["pids"])
            return Flat(good.off, good.index, good.cols, loff, lent)
        return good


# ---- model scenes: rows written by hand ---------------------------------------------------------------------
@dataclass
class ModelScene:
    name: str
    n_nodes: int
    rows: List[Row]
    steps: List[List[int]]                        # the rows each commit names
    probes: List[Tuple[int, int]]                 # (node, priority) of the later dry runs
    tells: Tuple[str, ...] = ()
    lists: Tuple[str, ...] = LISTS

    def result(self, flaw: Optional[str] = None) -> list:
        """After every step: the snapshot, the table per node, the probes' victims; a refused step by its reason."""
        m = Model(self.n_nodes, self.rows, flaw, self.lists)
        out = []
        for step in self.steps:
            try:
                m.commit(step)
                out.append((m.snapshot(), m.view(), [m.victims_below(*p) for p in self.probes]))
            except Refused as e:
                out.append(("refused", e.entry, e.why, m.snapshot(), m.view()))
        return out


def _middle_of_three_nodes() -> ModelScene:
    """Three nodes; the middle node's only two rows go, so its range is empty
    between two others.  Rows with no entries beside rows with several."""
    rows = [Row(0, 10, 100, adds=((0, 1), (1, 2)), pids=(0,)), Row(0, 5, 100),
            Row(1, 9, 100, adds=((0, 1),), pids=(0, 1)), Row(1, 7, 100, adds=((2, 1), (3, 1), (4, 1))),
            Row(2, 8, 100, pids=(1,)), Row(2, 6, 100, adds=((1, 1),), pids=(0,))]
    return ModelScene("middle_of_three_nodes", 3, rows, [[3, 2]], [(0, 100), (1, 100), (2, 100), (2, 7)],
                      tells=("off_not_moved", "dead_entries_left", "entries_from_new_offset",
                             "victims_compacted", "budget_ids_shifted", "nz_not_returned"))


def _two_commits() -> ModelScene:
    """Two commits in a row, the second by original numbers; then the first one's row again."""
    rows = [Row(0, 10 - i, 100 + i, adds=((i % 3, 1),), pids=(i % 2,)) for i in range(6)]
    return ModelScene("two_commits", 1, rows, [[1], [4, 0], [1]], [(0, 100)],
                      tells=("victims_compacted", "dead_evictable_again", "order_not_kept", "dead_entries_left"))


def _only_two_holders() -> ModelScene:
    """Rows 0 and 1 are the only holders of volume class 7 (family 0) on node 0
    and leave together: attached falls by exactly one.  Row 2 holds two volumes
    of its own, row 3 shares class 8 with row 4, which stays."""
    rows = [Row(0, 5, 100, vols=((7, 0, 1),)), Row(0, 4, 100, vols=((7, 0, 1),)), Row(0, 3, 100, vols=((-1, 0, 2),)),
            Row(0, 2, 100, vols=((8, 1, 1),)), Row(0, 1, 100, vols=((8, 1, 1),))]
    return ModelScene("only_two_holders", 1, rows, [[0, 1], [3], [2]], [(0, 100)],
                      tells=("last_holder_skipped", "last_holder_twice", "dead_entries_left"))


def _first_and_last() -> ModelScene:
    """The table's first and last rows, with empty nodes on either side of both."""
    rows = [Row(1, 3, 100, adds=((0, 1),)), Row(1, 2, 100), Row(3, 3, 100, adds=((1, 1),)), Row(3, 2, 100, adds=((2, 5),))]
    return ModelScene("first_and_last", 5, rows, [[0, 3]], [(1, 100), (3, 100)],
                      tells=("off_not_moved", "entries_from_new_offset", "victims_compacted"))


def _everything() -> ModelScene:
    rows = [Row(i % 2, i, 100, adds=((i, 1),), pids=(0,)) for i in range(5)]
    return ModelScene("everything", 2, rows, [[4, 0, 2, 1, 3]], [(0, 100), (1, 100)], tells=("off_not_moved",))


def _only_adds_set() -> ModelScene:
    rows = [Row(0, 3, 100, adds=((0, 1),), pids=(1,)), Row(0, 2, 100, adds=((1, 1), (2, 1)), pids=(0,)),
            Row(0, 1, 100, adds=((3, 1),))]
    return ModelScene("only_adds_set", 1, rows, [[0]], [(0, 100)], tells=("dead_entries_left",), lists=("adds",))


@functools.lru_cache(maxsize=None)
def model_scenes() -> Dict[str, ModelScene]:
    made = (_middle_of_three_nodes(), _two_commits(), _only_two_holders(), _first_and_last(), _everything(),
            _only_adds_set())
    return {s.name: s for s in made}


# ---- engine scenes: model objects --------------------------------------------------------------------------
from preemptfullcases import DB, HOST, X, Y, ZONE, FullScene, anti, hard, sched_profile   # noqa: E402
from preemptvolcases import EBS_KEY                                                       # noqa: E402

TILE = 1024                                       # ksim.preemption.COMMIT_TILE (checked by the CPU test)


@dataclass
class CommitScene(FullScene):
    steps: List[List[str]] = field(default_factory=list)       # the bound pods each commit evicts
    wide: bool = False                                           # too wide for the object-level reference

    def bp(self, name, on, prio, vols=(), cpu="100m", start=100, port=0, labels=None, terms=(), mem="1Mi"):
        p = self.bpod(name, on, prio, vols, cpu, start, port, labels, terms)
        p.containers[0].requests["memory"] = mem
        return p

    def pend(self, name, prio=1000, **kw):
        p = self.preemptor(**kw)
        p.name, p.priority = name, prio
        return p


def seam(n_rows: int) -> CommitScene:
    """``n_rows`` rows on nodes n1, n3 and n4 of five (n0 and n2 stay empty),
    each node's rows in mixed priorities so the table order is not the caller's.
    Every third row carries app=x (and, every ninth, tier=t and env=e too: rows
    with three or four class adds beside rows with none); rows 1 mod 5 sit
    under a budget.  Commit 1: the table's first row, its last row and every
    seventh row; commit 2: every row of n3 that is left (or, for one row, nothing
    more).  Pending: a plain pod, one with anti-affinity terms (the classes), one
    of priority 4 (few victims)."""
    from ksim.model import LabelSelector, PodDisruptionBudget
    s = CommitScene(f"seam_{n_rows}", wide=n_rows > 70)
    for v in range(5):
        s.node(f"n{v}", {"pods": "4000"}, cpu="2")
    homes = ("n1", "n3", "n4")
    for i in range(n_rows):
        lab = {}
        if i % 3 == 0:
            lab["app"] = "x"
        if i % 9 == 0:
            lab.update(tier="t", env="e")
        if i % 5 == 1:
            lab["guard"] = "g"
        s.bp(f"b{i}", homes[i % 3 if n_rows > 2 else 0], 1 + (i * 7) % 10, cpu="1m", start=100 + (i * 13) % 50,
             labels=lab or None)
    s.pend("plain", cpu="1995m")
    s.pend("picky", cpu="1990m", terms=[anti(), anti(HOST, tier="t"), anti(HOST, env="e")])
    s.pend("low", prio=4, cpu="1999m")
    s.budgets = [PodDisruptionBudget("g", selector=LabelSelector({"guard": "g"}), disruptions_allowed=1)]
    order = sorted(range(n_rows), key=lambda i: (homes.index(s.bound[i].node_name), -s.bound[i].priority,
                                                 s.start[f"b{i}"], i))
    first = sorted({order[0], order[-1]} | set(order[3::7]))
    s.steps = [[f"b{i}" for i in first]]
    rest = [f"b{i}" for i in range(n_rows) if s.bound[i].node_name == "n3" and i not in first]
    if rest:
        s.steps.append(rest)
    return s


def whole_table() -> CommitScene:
    """Every row of the table in one commit; then a dry run finds nobody to evict."""
    s = CommitScene("whole_table")
    s.node("n0", cpu="1")
    s.node("n1", cpu="1")
    for i in range(5):
        s.bp(f"b{i}", f"n{i % 2}", 5 + i, cpu="300m", labels=X if i % 2 else None)
    s.pend("plain", cpu="900m")
    s.pend("picky", cpu="100m", terms=[anti()])
    s.steps = [[f"b{i}" for i in (3, 0, 4, 1, 2)]]
    return s


def volumes() -> CommitScene:
    """n0, EBS limit 3.  b0 and b1 are the only two holders of volume s: they
    leave together and attached falls by exactly one.  b2 and b3 share t and only
    b2 leaves: no change.  b4 holds two volumes of its own (a classless count
    of two) and leaves in the second commit; b5 holds one and stays.  n1: c0 and
    c1 share u, evicted in the same commit as b0 and b1 (several nodes, one call).
    Pending: a pod with a new EBS volume; one that mounts t."""
    s = CommitScene("volumes")
    s.znode("n0", "za", {EBS_KEY: "3"})
    s.znode("n1", "zb", {EBS_KEY: "3"})
    s.bp("b0", "n0", 10, [("ebs", "s")])
    s.bp("b1", "n0", 9, [("ebs", "s")])
    s.bp("b2", "n0", 8, [("ebs", "t")])
    s.bp("b3", "n0", 7, [("ebs", "t")])
    s.bp("b4", "n0", 6, [("ebs", "p"), ("ebs", "q")])
    s.bp("b5", "n0", 5, [("ebs", "r")])
    s.bp("c0", "n1", 10, [("ebs", "u")], labels=X)
    s.bp("c1", "n1", 9, [("ebs", "u")])
    s.bp("c2", "n1", 8, [("ebs", "w"), ("ebs", "y"), ("ebs", "z")])
    s.pend("newvol", vols=[("ebs", "x")])
    s.pend("mounts_t", vols=[("ebs", "t"), ("ebs", "x2")], terms=[anti()])
    s.steps = [["b1", "c0", "b0", "c1", "b2"], ["b4"]]
    return s


def only_adds() -> CommitScene:
    """No budgets and no volumes: only the class adds are set on the rows."""
    s = CommitScene("only_adds")
    for v in range(3):
        s.node(f"n{v}", cpu="1")
    for i in range(9):
        s.bp(f"b{i}", f"n{i % 3}", 3 + i % 4, cpu="300m", labels=X if i % 2 else None, port=8080 if i == 4 else 0)
    s.pend("picky", cpu="500m", terms=[anti()])
    s.pend("ported", cpu="100m", ports=(8080,))
    s.steps = [["b4", "b0"], ["b7"]]
    return s


def plain() -> CommitScene:
    """Requests alone (the oracle's dry run takes these): 4 nodes, two of them
    empty, victims on both others in one call, two commits."""
    s = CommitScene("plain")
    for v in range(4):
        s.node(f"n{v}", cpu="2")
    for i in range(12):
        s.bp(f"b{i}", "n1" if i % 2 else "n3", 2 + (i * 5) % 9, cpu="300m", start=100 + i % 4)
    s.pend("big", cpu="1500m")
    s.pend("small", prio=6, cpu="700m")
    s.steps = [["b1", "b4", "b6"], ["b0", "b11"]]
    return s


def chain() -> CommitScene:
    """Three pending pods in priority order on two zoned nodes of 1 CPU, every
    bound pod 400m.  n0 (za): a0 (priority 1, app=x), a1 (2, under the budget).
    n1 (zb): c0 (5), c1 (6, under the budget).
    A (1000, 300m): both nodes fail Fit; on n0 a1 is reprieved (400 + 300) and a0
    is the victim, on n1 c0: n0's victim ranks lower.  A is nominated on n0 and
    a0 is committed.
    B (900, 500m, app=x, DoNotSchedule maxSkew 1 over the zone for app=x): on the
    untouched snapshot its answer is (n0, [a0]) as well.  After the commit, with
    A nominated on n0 (300 + 400 + 500 > 1000): a1 out, 800 fits, a1 back does
    not: (n0, [a1]).  Had the commit left a0 in the table the victims would be
    [a1, a0]; had it left a0 in za's count of app=x the skew (1 + 1 - 0 > 1)
    would fail n0 with nobody to evict for it, and B would go to n1.
    C (800, 300m, hostname anti-affinity against app=y): after B's commit n0
    holds A and B alone (800 + 300 > 1000, nobody to evict); on n1 c1 is
    reprieved and c0 is the victim."""
    from ksim.model import LabelSelector, PodDisruptionBudget
    s = CommitScene("chain")
    s.znode("n0", "za", cpu="1")
    s.znode("n1", "zb", cpu="1")
    s.bp("a0", "n0", 1, cpu="400m", labels=X)
    s.bp("a1", "n0", 2, cpu="400m", labels={"guard": "g"})
    s.bp("c0", "n1", 5, cpu="400m")
    s.bp("c1", "n1", 6, cpu="400m", labels={"guard": "g"})
    s.pend("A", prio=1000, cpu="300m")
    s.pend("B", prio=900, cpu="500m", labels=X, spread=[hard(ZONE, 1)])
    s.pend("C", prio=800, cpu="300m", terms=[anti(**Y)])
    s.budgets = [PodDisruptionBudget("g", selector=LabelSelector({"guard": "g"}), disruptions_allowed=1)]
    return s


_ENGINE = (lambda: seam(1), lambda: seam(63), lambda: seam(64), lambda: seam(65), lambda: seam(TILE - 2),
           lambda: seam(TILE - 1), lambda: seam(TILE), lambda: seam(TILE + 1), lambda: seam(2 * TILE),
           whole_table, volumes, only_adds, plain)


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, CommitScene]:
    out = {}
    for make in _ENGINE:
        s = make()
        out[s.name] = s
    return out


def scene_ids() -> List[str]:
    return list(scenes())


# ---- the scenes compiled --------------------------------------------------------------------------------------
@dataclass
class Built:
    sc: CommitScene
    cluster: object
    enc: object                                   # the pending pods, then one record per bound pod
    table: object
    prof: object
    n_pending: int
    pos: Dict[str, int]                           # node name -> cluster position

    def record(self, row: int) -> int:
        """The pod record of table row ``row`` in ``enc``."""
        return self.n_pending + row

    def rows_of(self, names: Sequence[str]) -> List[int]:
        return [self.sc.order[n] for n in names]


def survivors_table(b: Built, alive: Sequence[int]):
    """ksim.preemption.bound_table over the rows ``alive`` (caller numbers, ascending) of the scene."""
    from ksim.preemption import bound_table
    sc = b.sc
    has_vols = b.cluster.vol_limits is not None and b.table.vol_off is not None
    return bound_table(b.cluster, [sc.bound[i] for i in alive], sc.start, b.cluster.topo, full_adds=True,
                       pdbs=sc.budgets or None, vol_limits=b.cluster.vol_limits if has_vols else None)


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    """The scene compiled once: the pending pods and a record per bound pod in
    one pod set (every class exists before any record's adds are taken), the
    bound pods' records carrying their holdings as the limits compile counted
    them, then the table with every list the scene has."""
    from ksim import profile
    from ksim.encode import encode_cluster, encode_pods
    from ksim.preemption import bound_table
    from ksim.volumes import VolumeIndex
    sc = scenes()[name] if name != "chain" else chain()
    index = VolumeIndex.from_nodes(sc.nodes, sc.pvs, sc.pvcs)
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    has_vols = bool(sc.pvs)
    if has_vols:
        vl = index.volume_limits(sc.nodes, sc.bound, sc.pending)
        vl.pod_uses.update(vl.bound_uses)          # a bound pod's record: what the compile counted for it
        cluster.set_volume_limits(vl)
    enc = encode_pods(cluster, list(sc.pending) + list(sc.bound), volumes=index)
    table = bound_table(cluster, sc.bound, sc.start, cluster.topo, full_adds=True, pdbs=sc.budgets or None,
                        vol_limits=cluster.vol_limits if has_vols else None)
    assert table.n == len(sc.bound)
    pos = {n: i for i, n in enumerate(cluster.node_names)}
    return Built(sc, cluster, enc, table, profile.compile_profile(sched_profile(sc.filter_order, sc.args)),
                 len(sc.pending), pos)


def model_of(b: Built) -> Model:
    """The model over the compiled scene's own arrays: the table's rows, and of each bound pod's record what an eviction moves."""
    from ksim import abi
    t, enc, rows = b.table, b.enc, []
    for i in range(t.n):
        rec = enc.pods[b.record(i)]
        adds = tuple((int(a["cls"]), int(a["count"])) for a in
                     enc.adds[int(rec["add_first"]):int(rec["add_first"]) + int(rec["add_count"])])
        vols = tuple((int(u["cls"]), int(u["col"]), int(u["arg"])) for u in
                     enc.uses[int(rec["use_first"]):int(rec["use_first"]) + int(rec["use_count"])] if u["kind"] == abi.USE_VOLUME)
        pids = () if t.pdb_off is None else tuple(int(x) for x in t.pdb_ids[t.pdb_off[i]:t.pdb_off[i + 1]])
        assert int(rec["req_cpu"]) == int(t.req[i, 0])
        rows.append(Row(int(t.node[i]), int(t.priority[i]), int(t.start_time[i]), int(rec["req_cpu"]), adds, pids, vols,
                        int(rec["nz_cpu"]), int(rec["nz_mem"]), int(rec["nb_add"])))
    return Model(b.cluster.n_nodes, rows)
