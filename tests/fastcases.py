"""Engineered narrow clusters for the FAST key arithmetic (csrc/ksim_device.h
fast_fit_ok, fast_least_allocated, fast_balanced_allocation, div_rn,
u52_to_f64, req_entry): every allocatable cpu and memory is below 2^46, so the
engine takes the reciprocal quotients, and the values sit where those can go
wrong.  tests/test_fast_ref.py proves on the CPU that each wrong reading of
tests/fastref.FAULTS moves a placement of some scene;
tests/test_gpu_fast_edges.py runs the scenes through every path that
evaluates the FAST key.

The scenes are small (16 to 64 nodes, at most 600 pods in classes of at least
8 pods) and built straight on the EncodedCluster arrays.  What makes a
placement sensitive to one score point is LeastAllocated itself: the pods are
small against the nodes, so the nodes' totals level out within a point of each
other and stay there, and a node that reads one point low or high takes a
different share of the queue."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from ksim import abi, gen, profile
from ksim.encode import EncodedCluster, EncodedPods

import fastref

MI = 1 << 20
GI = 1 << 30
PI = 1 << 50
NARROW = 1 << 46
SEED = 0x46415354


@dataclass
class Scene:
    name: str
    cluster: EncodedCluster
    pods: EncodedPods
    # (alloc_cpu, alloc_mem) the nodes had before the last update (fastref's stale_reciprocal)
    prev: Optional[Tuple[np.ndarray, np.ndarray]] = None
    # the property the scene's name claims, as counts that must all be above zero
    claims: Dict[str, int] = field(default_factory=dict)
    seq0: int = 0                                  # the tie-break sequence of the queue's first pod

    def __post_init__(self):
        c = self.cluster
        assert 16 <= c.n_nodes <= 64 and self.pods.n_pods <= 600, self.name
        assert is_narrow(c), self.name
        assert min(class_sizes(self.pods).values()) >= 8, (self.name, class_sizes(self.pods))


def is_narrow(c) -> bool:
    return bool(((c.alloc_cpu >= 0) & (c.alloc_cpu < NARROW) & (c.alloc_mem >= 0) & (c.alloc_mem < NARROW)).all())


def class_sizes(pods) -> dict:
    p = pods.pods
    out: dict = {}
    for i in range(len(p)):
        k = tuple(int(p[f][i]) for f in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem"))
        out[k] = out.get(k, 0) + 1
    return out


def make_pods(classes, order) -> EncodedPods:
    """classes: [(req_cpu, req_mem, req_eph, nz_cpu, nz_mem)]; order: class index per pod."""
    order = np.asarray(order)
    pods = np.zeros(order.size, abi.POD_DTYPE)
    tab = np.array(classes, np.int64)
    for k, f in enumerate(("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem")):
        pods[f] = tab[order, k]
    pods["node_name"] = -1
    return EncodedPods(pods, np.zeros(0, abi.LABEL_EXPR_DTYPE), np.zeros(0, abi.TERM_DTYPE),
                       [("default", f"pod-{j:05d}") for j in range(order.size)])


def draw(n: int, weights, tag: int) -> np.ndarray:
    """n class indices, class k drawn weights[k] times in sum(weights) (a fixed stream)."""
    table = np.repeat(np.arange(len(weights)), weights)
    return table[gen.below(gen.stream(SEED, tag, n), table.size)]


def best_effort():
    return (0, 0, 0, 100, 200 * MI)               # no requests: the non-zero defaults alone


def requesting(cpu, mem, eph=0):
    return (cpu, mem, eph, cpu, mem)


def uncorrected_wrong(d: int, k: int) -> bool:
    """trunc(n * RN(1 / d)) != n // d at the exact quotient n = k d."""
    return int(float(k * d) * (1.0 / float(d))) != k


@functools.lru_cache(maxsize=None)
def boundary_m(min_wrong: int = 20, skip: int = 0) -> int:
    """The (skip + 1)-th m below 2^46 / 100 whose allocatable d = 100 m has at
    least min_wrong exact quotients k in 50..99 that the uncorrected product
    truncates to k - 1."""
    m = (NARROW - 1) // 100
    while True:
        if sum(uncorrected_wrong(100 * m, k) for k in range(50, 100)) >= min_wrong:
            if skip == 0:
                return m
            skip -= 1
        m -= 1


# ---- quotient boundaries -------------------------------------------------------
def quotient_boundary() -> Scene:
    """16 nodes of memory 100 m just below 2^46, cpu 2^46 - 1 / 7910m / 31750m.
    Class A requests memory m, so on a node loaded with t m the remaining
    memory is exactly (99 - t) hundredths: an exact quotient, for this m one the
    uncorrected product truncates a point low on many t.  Class B requests
    m + 1 (its quotient, and that of every later pod on its node, lies just
    under the integer) and class C m - 1 (a B and a C bring a node back)."""
    n = 16
    m = boundary_m()
    c = gen.bare_cluster(n, SEED)
    c.alloc_mem[:] = 100 * m
    c.alloc_cpu[:] = np.array([NARROW - 1, 7910, 31750, NARROW - 1] * 4, np.int64)
    t = np.array([0, 3, 7, 12, 1, 4, 9, 15, 2, 6, 11, 20, 5, 8, 14, 30], np.int64)
    c.req_mem[:] = c.nz_mem[:] = t * m
    c.num_pods[:] = t
    c.alloc_pods[:] = 110
    classes = [requesting(10, m), requesting(10, m + 1), requesting(10, m - 1), requesting(25, m)]
    pods = make_pods(classes, draw(600, [12, 1, 1, 2], 1))
    exact = wrong = under = 0
    for node in range(n):
        d = int(c.alloc_mem[node])
        for cls in classes:
            left = (d - int(c.nz_mem[node]) - cls[4]) * 100
            exact += left % d == 0
            wrong += left % d == 0 and uncorrected_wrong(d, left // d)
            under += 0 < d - left % d <= 100
    return Scene("quotient_boundary", c, pods,
                 claims={"exact quotients": exact, "exact quotients the uncorrected product truncates low": wrong,
                         "quotients within 100 / d below an integer": under})


def ba_boundary() -> Scene:
    """BalancedAllocation where (1 - |fc - fm| / 2) 100 lands on or next to an
    integer in float64: decimal allocatables (cpu 10000m, 7910m, 31750m,
    memory 100 m') under requests of whole hundredths, so the fractions differ
    by whole hundredths and the product is k, k - one ulp or k + one ulp: the
    truncation tells these apart, a float32 evaluation does not.  Nodes 0, 3,
    4 and 7 start on loads found by search to give class 0 such scores."""
    n = 16
    m = boundary_m(skip=3) // 1024                 # memory 100 m: about 64 Gi, still no power of two
    c = gen.bare_cluster(n, SEED + 1)
    c.alloc_mem[:] = 100 * m
    cpu = np.array([10000, 7910, 31750, 10000], np.int64)
    c.alloc_cpu[:] = np.tile(cpu, 4)
    hundredth = c.alloc_cpu // 100                 # 79 and 317 are not exact hundredths: those nodes sit off the grid
    tc = np.array([34, 5, 10, 35, 2, 8, 13, 8, 30, 2, 7, 40, 11, 4, 6, 9], np.int64)
    tm = np.array([52, 0, 4, 55, 34, 8, 1, 40, 3, 30, 7, 5, 11, 12, 6, 0], np.int64)
    c.req_cpu[:] = c.nz_cpu[:] = tc * hundredth
    c.req_mem[:] = c.nz_mem[:] = tm * m
    c.num_pods[:] = 1
    classes = [requesting(100, m), requesting(200, m), requesting(100, 2 * m), requesting(79, m)]
    pods = make_pods(classes, draw(600, [3, 2, 2, 1], 2))
    below = above = 0
    for node in range(n):
        for cls in classes:
            fc = min((int(c.req_cpu[node]) + cls[0]) / int(c.alloc_cpu[node]), 1.0)
            fm = min((int(c.req_mem[node]) + cls[1]) / int(c.alloc_mem[node]), 1.0)
            x = (1 - abs((fc - fm) / 2)) * 100
            if x != round(x) and abs(x - round(x)) <= np.spacing(x):
                below += x < round(x)
                above += x > round(x)
    return Scene("ba_boundary", c, pods, claims={"scores one ulp below an integer": below,
                                                 "scores one ulp above an integer": above})


# ---- zero allocatable, overdrawn capacity, nz != req ---------------------------------
def zero_and_overdrawn() -> Scene:
    """24 small nodes (cpu 1000m..2000m, memory 2..4 Gi, 9..14 pods) under
    BestEffort pods (they request nothing, so Fit tests their pod count alone
    and they land on anything) and a few small requesting pods:
      0..2    allocatable cpu 0 / memory 0 / both 0
      3, 4    requested cpu / memory above allocatable (only zero-request pods fit)
      5, 6    non-zero requested above allocatable, requested below (score 0, feasible)
      7       requested memory 300 Pi, 8 requested memory 4 Pi + 1 Gi, 9 requested
              cpu 2^53 + 2^52: sums at and past 2^52 on allocatables below 2^46
      10..13  bound BestEffort load (non-zero requested, nothing requested)
      14..23  plain rivals, balanced and unbalanced bound load
    The queue is longer than the pod slots, so every node fills and the last
    pods find none."""
    n = 24
    c = gen.bare_cluster(n, SEED + 2)
    i = np.arange(n)
    c.alloc_cpu[:] = np.where(i % 2 == 0, 1000, 2000)
    c.alloc_mem[:] = np.where(i % 3 == 0, 2 * GI, 4 * GI)
    c.alloc_pods[:] = 9 + i % 6
    c.alloc_cpu[0], c.alloc_mem[1] = 0, 0
    c.alloc_cpu[2], c.alloc_mem[2] = 0, 0
    c.req_mem[0] = c.nz_mem[0] = GI               # the one resource present is in use
    c.req_cpu[1] = c.nz_cpu[1] = 400
    c.req_cpu[3] = c.nz_cpu[3] = int(c.alloc_cpu[3]) + 500
    c.req_mem[4] = c.nz_mem[4] = int(c.alloc_mem[4]) + GI
    c.nz_cpu[5], c.req_cpu[5] = int(c.alloc_cpu[5]) + 300, 200
    c.nz_mem[6], c.req_mem[6] = int(c.alloc_mem[6]) + 700 * MI, GI
    c.req_mem[7] = c.nz_mem[7] = 300 * PI
    c.req_mem[8] = c.nz_mem[8] = 4 * PI + GI
    c.req_cpu[9] = c.nz_cpu[9] = (1 << 53) + (1 << 52)
    for k in (10, 11, 12, 13):
        c.nz_cpu[k], c.nz_mem[k] = 100 * (k - 9), 200 * MI * (k - 9)
    for k in range(14, 24):
        c.req_cpu[k] = c.nz_cpu[k] = 100 * (k % 5)
        c.req_mem[k] = c.nz_mem[k] = 256 * MI * (k % 4)
    c.num_pods[:] = 1
    c.num_pods[2] = 0
    classes = [best_effort(), requesting(50, 100 * MI), requesting(100, 64 * MI), (0, 0, 0, 100, 100 * MI)]
    pods = make_pods(classes, draw(400, [6, 2, 1, 1], 3))
    slots = int((c.alloc_pods - c.num_pods).sum())
    return Scene("zero_and_overdrawn", c, pods, claims={
        "zero allocatables": int((c.alloc_cpu == 0).sum() + (c.alloc_mem == 0).sum()),
        "requested above allocatable": int(((c.req_cpu > c.alloc_cpu) | (c.req_mem > c.alloc_mem)).sum()),
        "non-zero requested above allocatable, requested below": int(
            (((c.nz_cpu > c.alloc_cpu) & (c.req_cpu <= c.alloc_cpu) & (c.alloc_cpu > 0)) |
             ((c.nz_mem > c.alloc_mem) & (c.req_mem <= c.alloc_mem) & (c.alloc_mem > 0))).sum()),
        "requested at or past 2^52": int(((c.req_mem >= 1 << 52) | (c.req_cpu >= 1 << 52)).sum()),
        "nodes whose columns differ": int(((c.nz_cpu != c.req_cpu) | (c.nz_mem != c.req_mem)).sum()),
        "pods past the pod slots": pods.n_pods - slots})


# ---- pod count, ephemeral storage, near ties of unlike nodes --------------------------
def limits_and_ties() -> Scene:
    """32 nodes of unlike sizes (cpu 4..64 cores, 7910m and 31750m among them,
    memory 16..256 Gi) loaded to the same fractions, so unlike quotients tie;
    allowed pods 0, 1, 2 and 3 on eight of them; ephemeral storage set on all
    and nearly full on eight (two more storage pods fit).  Pods request about
    a hundredth of the smallest node."""
    n = 32
    c = gen.bare_cluster(n, SEED + 3)
    i = np.arange(n)
    c.alloc_cpu[:] = np.array([4000, 7910, 16000, 31750, 64000, 8000, 32000, 12000], np.int64)[i % 8]
    c.alloc_mem[:] = np.array([16, 32, 64, 128, 256, 48, 96, 24], np.int64)[(i // 2) % 8] * GI
    c.alloc_pods[:] = 40
    c.alloc_pods[[4, 5, 12, 13, 20, 21, 28, 29]] = [0, 1, 2, 3, 0, 1, 2, 3]
    unit = 5 * GI
    c.alloc_eph[:] = 100 * GI
    c.req_eph[:] = 10 * GI
    c.req_eph[i % 4 == 3] = 100 * GI - 2 * unit - 1
    load = np.array([0, 10, 25, 40], np.int64)[i % 4]
    c.req_cpu[:] = c.nz_cpu[:] = c.alloc_cpu * load // 100
    c.req_mem[:] = c.nz_mem[:] = c.alloc_mem * load // 100
    c.nz_cpu[i % 5 == 0] += 300                    # bound BestEffort pods on some
    c.nz_mem[i % 5 == 0] += 600 * MI
    classes = [requesting(50, 128 * MI), requesting(100, 64 * MI), requesting(40, 256 * MI, unit), best_effort(),
               requesting(60, 200 * MI)]
    pods = make_pods(classes, draw(600, [3, 2, 1, 1, 2], 4))
    # the rivals: under Fit / BalancedAllocation weights 2 / 1 one LeastAllocated point weighs 2, so a node
    # that loses one falls strictly below every unlike node whose total is now less than 2 below its own
    w = fastref.weights(compiled("w21"))
    ok, _, _, total = fastref.node_scores(fastref.columns(c), pods.pods[0], w)
    rivals = sum(1 for a in range(n) for b in range(n)
                 if ok[a] and ok[b] and (c.alloc_cpu[a], c.alloc_mem[a]) != (c.alloc_cpu[b], c.alloc_mem[b])
                 and 0 <= total[a] - total[b] < 2)
    return Scene("limits_and_ties", c, pods, claims={
        "unlike nodes less than one LeastAllocated point apart at weights 2 / 1": rivals,
        "allowed pods 0..3": int(len(set(c.alloc_pods.tolist()) & {0, 1, 2, 3}) == 4),
        "storage nearly full": int((c.alloc_eph - c.req_eph < 3 * unit).sum()),
        "unlike allocatables": len(set(zip(c.alloc_cpu.tolist(), c.alloc_mem.tolist())))})


# ---- a reciprocal's lifetime ---------------------------------------------------------
LIFETIME_ROWS = (2, 7, 13)


def lifetime_allocatables(c):
    """(rows, alloc_cpu, alloc_mem) of the UpdateNode step: three nodes move to
    other allocatables below 2^46, 2.5 to 7.5 % down (memory still a multiple
    of 100; cpu 7910m and 31750m 130m up).  A quotient near k from the old
    reciprocal is low by about k times the square of that step, up to 0.5
    points here."""
    rows = np.array(LIFETIME_ROWS, np.int32)
    cpu, mem = c.alloc_cpu.copy(), c.alloc_mem.copy()
    for k, r in enumerate(LIFETIME_ROWS):
        m = int(mem[r]) // 100
        mem[r] = 100 * (m - (k + 1) * (m // 40))
        cpu[r] = cpu[r] - (cpu[r] >> 5) - k if cpu[r] > 1 << 40 else cpu[r] + 130
    return rows, cpu, mem


def reciprocal_lifetime() -> Scene:
    """quotient_boundary as its own queue leaves it under the "w11" profile
    (tests/fastref.py's run), then three nodes' allocatables moved: a quotient
    from the reciprocal of the allocatable a node had before is what a stale
    inv_cpu / inv_mem gives.  The queue goes on at sequence 600, as it does on
    an engine that ran quotient_boundary first."""
    s = scene("quotient_boundary")
    _, cols, _, _ = fastref.schedule(s.cluster, s.pods, compiled("w11"))
    c = s.cluster.copy_state()
    for f in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem"):
        setattr(c, f, cols[f].copy())
    c.num_pods = cols["num_pods"].astype(np.int32)
    prev = (c.alloc_cpu.copy(), c.alloc_mem.copy())
    _, c.alloc_cpu, c.alloc_mem = lifetime_allocatables(c)
    moved = int(((prev[0] != c.alloc_cpu) | (prev[1] != c.alloc_mem)).sum())
    return Scene("reciprocal_lifetime", c, lifetime_queue(), prev=prev, seq0=s.pods.n_pods,
                 claims={"nodes whose allocatable moved": moved})


def lifetime_queue(tag: int = 5, n_pods: int = 240) -> EncodedPods:
    m = boundary_m()
    classes = [requesting(10, m), requesting(25, m), requesting(10, m + 1)]
    return make_pods(classes, draw(n_pods, [5, 2, 1], tag))


SCENES: Dict[str, Callable[[], Scene]] = {f.__name__: f for f in (
    quotient_boundary, ba_boundary, zero_and_overdrawn, limits_and_ties, reciprocal_lifetime)}


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    """The scene, built once; tests take copy_state() of its cluster."""
    return SCENES[name]()


# ---- profiles --------------------------------------------------------------------------
BIG_WEIGHT = 1 << 14                               # fast_def's bound: not the compiled-in shape


def scheduler_profile(kind: str, pct: int = 100) -> profile.SchedulerProfile:
    """"w11" / "w21" / "w12": Fit / BalancedAllocation score weights, the
    default shape; "res21": LeastAllocated resource weights cpu 2, memory 1;
    "big": a Fit score weight of 2^14; "nofit": no NodeResourcesFit filter, so
    pods land on full nodes and the sums are unbounded (all three leave the
    default shape)."""
    sp = profile.SchedulerProfile(percentage_of_nodes_to_score=pct)
    if kind == "nofit":
        sp.plugins["filter"].enabled = [p for p in sp.plugins["filter"].enabled
                                        if profile.original_name(p.name) != "NodeResourcesFit"]
    elif kind == "res21":
        sp.fit = profile.FitArgs(resources=[("cpu", 2), ("memory", 1)])
    elif kind == "big":
        sp = sp.with_weights({"NodeResourcesFit": BIG_WEIGHT, "NodeResourcesBalancedAllocation": 3})
    elif kind != "w11":
        fit, ba = {"w21": (2, 1), "w12": (1, 2)}[kind]
        sp = sp.with_weights({"NodeResourcesFit": fit, "NodeResourcesBalancedAllocation": ba})
    return sp


DEFAULT_SHAPE = ("w11", "w21", "w12")
OTHER_SHAPES = ("res21", "big", "nofit")


def compiled(kind: str, pct: int = 100) -> abi.Profile:
    return profile.compile_profile(scheduler_profile(kind, pct))


# ---- larger forms of a scene ------------------------------------------------------------
def tiled(s: Scene, n_nodes: int = 8193) -> EncodedCluster:
    """The scene's nodes repeated to at least n_nodes nodes (whole copies)."""
    reps = -(-n_nodes // s.cluster.n_nodes)
    c = gen.bare_cluster(reps * s.cluster.n_nodes, SEED)
    for f in ("alloc_cpu", "alloc_mem", "alloc_eph", "alloc_pods", "req_cpu", "req_mem", "req_eph", "nz_cpu",
              "nz_mem", "num_pods"):
        getattr(c, f)[:] = np.tile(getattr(s.cluster, f), reps)
    assert is_narrow(c)
    return c


def repeated(pods: EncodedPods, n_pods: int) -> EncodedPods:
    """The queue repeated to n_pods pods."""
    idx = np.arange(n_pods) % pods.n_pods
    return EncodedPods(pods.pods[idx].copy(), pods.exprs, pods.terms,
                       [("default", f"pod-{j:05d}") for j in range(n_pods)])


def with_zone_selector(pods: EncodedPods, every: int = 3) -> EncodedPods:
    """Every ``every``-th pod with a node selector on its zone (bare_cluster's
    label column 1, values z0..z2 = ids 1..3): those pods are not trivial, so
    their run takes the static-class keys."""
    exprs = np.zeros(3, abi.LABEL_EXPR_DTYPE)
    exprs["col"], exprs["op"], exprs["nvals"] = 1, abi.OP_IN, 1
    exprs["vals"][:, 0] = [1, 2, 3]
    p = pods.pods.copy()
    j = np.arange(len(p))
    sel = j % every == 0
    p["sel_first"][sel] = (j[sel] // every) % 3
    p["sel_count"][sel] = 1
    return EncodedPods(p, exprs, pods.terms, pods.names)
