"""Hand-built scenes for pods with container images on the batch paths
(csrc/ksim_engine.cpp pod_batchable, csrc/ksim_device.h stab_word / norm_raw /
norm_part): ksim.model nodes with status.images, pods whose containers name
images, so the encoder gives each pod one KSIM_USE_IMAGE use.

tests/test_image_cases.py proves on the CPU that the scenes reach the image
scores they claim and that each wrong reading of FAULTS moves a placement of
some scene; tests/test_gpu_image_batch.py runs them through the engine.

Within a scene the nodes are identical in resources unless its text says
otherwise, so ImageLocality alone orders them until LeastAllocated answers.
An image's size is chosen for the score it must give: with the image on
``holders`` of ``n`` nodes a holder's sum is int(size * holders / n), clamped to
[23 MB, 1000 MB x containers] and scaled to 0..100."""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

from ksim import profile
from ksim.encode import encode_cluster, encode_pods
from ksim.topology import normalized_image_name
from ksim.model import (Container, Node, NodeSelectorTerm, Pod, PreferredTerm, Requirement, Taint, Toleration)

MB = 1024 * 1024
MIN_T = 23 * MB
MAX_T = 1000 * MB
KEY_TOTAL_LIMIT = 1 << 20          # csrc/ksim_device.h kKeyTotalLimit
STAB_MAX_CLASSES = 4096            # csrc/ksim_engine.cpp kStabMaxClasses
BATCH_PODS = 256                   # csrc/ksim_device.h KSIM_BATCH_PODS


def image_score(total: int, containers: int = 1) -> int:
    """imagelocality.calculatePriority."""
    mx = MAX_T * containers
    s = min(max(total, MIN_T), mx)
    return (100 * (s - MIN_T)) // (mx - MIN_T)


def size_for(score: int, holders: int, n: int, containers: int = 1) -> int:
    """The smallest size whose holders score exactly ``score`` for a pod of
    ``containers`` containers naming only this image among the listed ones."""
    assert 0 < score <= 100
    mx = MAX_T * containers
    want = MIN_T + -(-score * (mx - MIN_T) // 100)         # the least sum with that score
    size = -(-want * n // holders)
    while image_score(int(float(size) * (float(holders) / float(n))), containers) < score:
        size += 1
    assert image_score(int(float(size) * (float(holders) / float(n))), containers) == score
    return size


def make_node(i: int, images=(), cpu="16", mem="64Gi", taints=(), labels=None, extra=None) -> Node:
    alloc = {"cpu": cpu, "memory": mem, "pods": "110"}
    alloc.update(extra or {})
    lab = {"kubernetes.io/hostname": f"n{i:04d}"}
    lab.update(labels or {})
    return Node(name=f"n{i:04d}", labels=lab, taints=list(taints), allocatable=alloc,
                images=[([normalized_image_name(name)], int(size)) for name, size in images])


def make_pod(j: int, images, cpu="500m", mem="2Gi", extra=None, preferred=(), tag="p") -> Pod:
    req = {"cpu": cpu, "memory": mem}
    cs = [Container(dict(req) if k == 0 else {}, image=im) for k, im in enumerate(images)]
    if extra:
        cs[0].requests.update(extra)
    return Pod(name=f"{tag}-{j:05d}", containers=cs, preferred_terms=list(preferred))


def make_profile(il: Optional[int] = 1, weights: Optional[Dict[str, int]] = None) -> profile.SchedulerProfile:
    """The default profile with ImageLocality at weight ``il`` (None: not in
    the score list) and ``weights`` over the other score plugins."""
    sp = profile.SchedulerProfile()
    if il is None:
        sp.plugins["score"].enabled = [p for p in sp.plugins["score"].enabled
                                       if profile.original_name(p.name) != "ImageLocality"]
        return sp.with_weights(weights or {})
    return sp.with_weights({"ImageLocality": il, **(weights or {})})


@dataclass
class Scene:
    name: str
    nodes: List[Node]
    queue: List[Pod]
    sp: profile.SchedulerProfile = field(default_factory=make_profile)
    # every pod of the queue: "batch" (both modes), "p100" (the batch path at
    # percentageOfNodesToScore 100 only: scalar requests), "perpod" (past the
    # key bound), None (a mixed queue: no path counter is pinned)
    route: Optional[str] = "batch"
    # image scores some node must take for some pod of the queue
    scores: tuple = ()
    # a node delta after the first half of the queue: nodes appended
    more_nodes: List[Node] = field(default_factory=list)

    @functools.cached_property
    def encoded(self):
        cluster, _ = encode_cluster(self.nodes)
        pods = encode_pods(cluster, self.queue)
        return cluster, pods

    @functools.cached_property
    def encoded_after(self):
        """The snapshot after the delta and the queue encoded against it, the
        classes in the first snapshot's order (ids carry over the delta)."""
        assert self.more_nodes
        c0, _ = self.encoded
        cluster, _ = encode_cluster(self.nodes + self.more_nodes, classes_from=c0.topo)
        pods = encode_pods(cluster, self.queue)
        return cluster, pods

    def compiled(self, pct: int, sp: Optional[profile.SchedulerProfile] = None):
        sp = copy.deepcopy(sp or self.sp)
        sp.percentage_of_nodes_to_score = pct
        return profile.compile_profile(sp, self.encoded[0].scalar_names)


def image_rows(cluster) -> List[int]:
    """The count classes that are image classes, in id order."""
    return sorted(cid for key, cid in cluster.topo.ids.items() if key[0] == "image")


def image_pods(pods) -> np.ndarray:
    """Per pod: whether its uses are exactly one image use."""
    from ksim import abi
    p = pods.pods
    out = np.zeros(len(p), bool)
    for i in range(len(p)):
        if p["use_count"][i] == 1 and pods.uses["kind"][p["use_first"][i]] == abi.USE_IMAGE:
            out[i] = True
    return out


# ---- scenes ---------------------------------------------------------------------
def score_values() -> Scene:
    """12 identical nodes.  One-container images give their holders 1, 63, 64,
    99 and 100; two-container pods name two of them (2000 MB clamp: about half
    the points), three-container pods a listed image between two unlisted ones,
    and one image no node lists stands beside a listed one."""
    n = 12
    targets = {"one": 1, "lo": 63, "hi": 64, "most": 99, "full": 100}
    holders = {"one": [0, 1], "lo": [2, 3], "hi": [4, 5], "most": [6, 7], "full": [8, 9]}
    imgs: Dict[int, list] = {i: [] for i in range(n)}
    for nm, s in targets.items():
        size = size_for(s, len(holders[nm]), n)
        for i in holders[nm]:
            imgs[i].append((f"reg.io/{nm}:v1", size))
    # a pair for two-container pods: node 10 lists a (99 of 2 containers' range), node 11 lists b (64)
    imgs[10].append(("reg.io/pa", size_for(99, 1, n, 2)))
    imgs[11].append(("reg.io/pb", size_for(64, 1, n, 2)))
    nodes = [make_node(i, imgs[i]) for i in range(n)]
    queue = []
    j = 0
    for rep in range(6):
        for nm in targets:
            queue.append(make_pod(j, [f"reg.io/{nm}:v1"], cpu="800m", mem="3Gi")); j += 1
        queue.append(make_pod(j, ["reg.io/pa", "reg.io/pb"], cpu="1600m", mem="6Gi")); j += 1
        queue.append(make_pod(j, ["reg.io/pa", "reg.io/nowhere"], cpu="800m", mem="3Gi")); j += 1
        queue.append(make_pod(j, ["reg.io/nowhere", "reg.io/full:v1", "other.io/nowhere"], cpu="800m", mem="3Gi")); j += 1
        queue.append(make_pod(j, ["reg.io/lo:v1", "reg.io/hi:v1", "reg.io/most:v1"], cpu="800m", mem="3Gi")); j += 1
    return Scene("score_values", nodes, queue, scores=(0, 1, 63, 64, 99, 100))


def saturation() -> Scene:
    """Two-container pods see 99 on node 0, 64 on node 1 and 63 on node 2 (the
    other five nodes 0): a field cut to 6 bits reads 35 / 0 / 63, one saturated
    at 63 reads three equal scores.  The pods are large (a tenth of a node), so
    LeastAllocated moves the choice down the ladder within a few binds."""
    n = 8
    nodes = [make_node(0, [("q.io/a", size_for(99, 1, n, 2))]),
             make_node(1, [("q.io/b", size_for(64, 1, n, 2))]),
             make_node(2, [("q.io/c", size_for(63, 1, n, 2))])] + [make_node(i) for i in range(3, n)]
    queue = []
    for j in range(40):
        trio = [["q.io/a", "q.io/b"], ["q.io/b", "q.io/c"], ["q.io/c", "q.io/a"]][j % 3]
        queue.append(make_pod(j, trio, cpu="1600m", mem="6Gi"))
    return Scene("saturation", nodes, queue, scores=(0, 63, 64, 99))


def ties() -> Scene:
    """Every node lists the image: equal image scores, equal resources, so the
    tie-break hash picks, and one image-less pod in three keeps the FAST-class
    pods in the same runs."""
    n = 9
    size = size_for(70, n, n)
    nodes = [make_node(i, [("t.io/all", size)]) for i in range(n)]
    queue = [make_pod(j, ["t.io/all"] if j % 3 else [""], cpu="100m", mem="256Mi") for j in range(60)]
    return Scene("ties", nodes, queue, route=None, scores=(70,))


def fills_up() -> Scene:
    """140 nodes (ADAPT keeps fewer than all), the image on four of them at 90
    points; 300 pods of a twentieth of a node each: the holders fill while the
    chain still guesses them, so pair keys, the re-key and the cut all run, and
    the queue spans two batches."""
    n = 140
    hold = [3, 50, 77, 139]
    size = size_for(90, len(hold), n)
    nodes = [make_node(i, [("f.io/app:2", size)] if i in hold else []) for i in range(n)]
    queue = [make_pod(j, ["f.io/app:2"], cpu="800m", mem="3Gi") for j in range(300)]
    return Scene("fills_up", nodes, queue, scores=(0, 90))


def three_parts() -> Scene:
    """130 nodes: every fifth carries a PreferNoSchedule taint, every third the
    label the pods prefer (weights 3 and 7 over two terms), every fourth the
    image (40 points) and every seventh a second one (75): TaintToleration,
    NodeAffinity and ImageLocality vary together in one key."""
    n = 130
    h1 = [i for i in range(n) if i % 4 == 0]
    h2 = [i for i in range(n) if i % 7 == 0]
    s1, s2 = size_for(40, len(h1), n), size_for(75, len(h2), n)
    nodes = []
    for i in range(n):
        im = ([("x.io/one", s1)] if i % 4 == 0 else []) + ([("x.io/two", s2)] if i % 7 == 0 else [])
        nodes.append(make_node(i, im, taints=[Taint("soft", "yes", "PreferNoSchedule")] if i % 5 == 0 else [],
                               labels={"disk": "ssd" if i % 3 == 0 else "hdd", "rack": f"r{i % 6}"}))
    pref = [PreferredTerm(3, NodeSelectorTerm([Requirement("disk", "In", ["ssd"])])),
            PreferredTerm(7, NodeSelectorTerm([Requirement("rack", "In", ["r1", "r2"])]))]
    queue = []
    for j in range(270):
        queue.append(make_pod(j, ["x.io/one"] if j % 2 else ["x.io/two"], cpu="400m", mem="1Gi",
                              preferred=pref if j % 3 else pref[:1]))
    return Scene("three_parts", nodes, queue, scores=(0, 40, 75))


def scalar_image() -> Scene:
    """Pods with a hugepages request and an image: no static class, the
    generic key reads the image class's count column (norm_raw)."""
    n = 120
    hold = [i for i in range(n) if i % 6 == 1]
    size = size_for(55, len(hold), n)
    nodes = [make_node(i, [("s.io/db", size)] if i in hold else [], extra={"hugepages-2Mi": "2Gi"})
             for i in range(n)]
    queue = [make_pod(j, ["s.io/db"], cpu="500m", mem="1Gi", extra={"hugepages-2Mi": "256Mi"}) for j in range(120)]
    return Scene("scalar_image", nodes, queue, route="p100", scores=(0, 55))


def weight_five() -> Scene:
    """ImageLocality at weight 5: 20 image points outweigh what a few binds cost
    the holder in LeastAllocated, which weight 1 does not."""
    n = 110
    hold = [i for i in range(n) if i % 10 == 0]
    size = size_for(20, len(hold), n)
    nodes = [make_node(i, [("w.io/svc", size)] if i in hold else []) for i in range(n)]
    queue = [make_pod(j, ["w.io/svc"], cpu="400m", mem="1Gi") for j in range(150)]
    return Scene("weight_five", nodes, queue, sp=make_profile(5), scores=(0, 20))


def _bound(il: int, name: str, route: str) -> Scene:
    n = 101
    hold = [i for i in range(n) if i % 9 == 2]
    size = size_for(100, len(hold), n)
    nodes = [make_node(i, [("b.io/big", size)] if i in hold else []) for i in range(n)]
    queue = [make_pod(j, ["b.io/big"], cpu="2", mem="8Gi") for j in range(96)]
    return Scene(name, nodes, queue, sp=make_profile(il), route=route, scores=(0, 100))


def bound_below() -> Scene:
    """100 * (w_fit + w_ba + w_il) = 100 * (1 + 1 + 10483) = 1,048,500: the last
    sum below 2^20.  TaintToleration and NodeAffinity stay in the profile at
    weight 1 and vary for no pod, so they are outside the sum."""
    s = _bound(KEY_TOTAL_LIMIT // 100 - 2, "bound_below", "batch")
    assert 100 * (2 + KEY_TOTAL_LIMIT // 100 - 2) < KEY_TOTAL_LIMIT
    return s


def bound_above() -> Scene:
    """One more: 1,048,600 >= 2^20, every image pod takes the per-pod path."""
    s = _bound(KEY_TOTAL_LIMIT // 100 - 1, "bound_above", "perpod")
    assert 100 * (2 + KEY_TOTAL_LIMIT // 100 - 1) >= KEY_TOTAL_LIMIT
    return s


def delta() -> Scene:
    """104 nodes, the image on 8 of them (30 points).  After half the queue 16
    nodes join that all hold it: with 24 of 120 holders every holder scores 81,
    the old ones too."""
    n = 104
    hold = [i for i in range(n) if i % 13 == 5]
    size = size_for(30, len(hold), n)
    assert image_score(int(float(size) * (24.0 / 120.0))) == 81
    nodes = [make_node(i, [("d.io/cache", size)] if i in hold else []) for i in range(n)]
    more = [make_node(n + i, [("d.io/cache", size)]) for i in range(16)]
    queue = [make_pod(j, ["d.io/cache"], cpu="400m", mem="1Gi") for j in range(120)]
    return Scene("delta", nodes, queue, more_nodes=more, scores=(0, 30))


BUILDERS: Dict[str, Callable[[], Scene]] = {f.__name__: f for f in (
    score_values, saturation, ties, fills_up, three_parts, scalar_image, weight_five, bound_below, bound_above,
    delta)}
SCENES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    s = BUILDERS[name]()
    assert s.name == name
    return s


# ---- generated sizes (tests/test_gpu_image_batch.py) ------------------------------
@functools.lru_cache(maxsize=None)
def sized(n_nodes: int, n_pods: int, n_images: int = 5) -> Scene:
    """``n_nodes`` identical nodes, ``n_images`` images on residue classes of
    the node index with different scores, ``n_pods`` pods naming them in turn
    (every fourth pod two of them)."""
    imgs: Dict[int, list] = {i: [] for i in range(n_nodes)}
    for k in range(n_images):
        hold = [i for i in range(n_nodes) if i % (k + 2) == 0]
        size = size_for(15 + 17 * k, len(hold), n_nodes)
        for i in hold:
            imgs[i].append((f"g.io/i{k}", size))
    nodes = [make_node(i, imgs[i]) for i in range(n_nodes)]
    queue = []
    for j in range(n_pods):
        names = [f"g.io/i{j % n_images}"] + ([f"g.io/i{(j + 2) % n_images}"] if j % 4 == 0 else [])
        queue.append(make_pod(j, names, cpu="300m", mem="1Gi"))
    return Scene(f"sized_{n_nodes}_{n_pods}", nodes, queue)


MAX_CLASSES = 4096                 # include/ksim_engine.h KSIM_MAX_CLASSES: count classes per cluster


@functools.lru_cache(maxsize=None)
def many_signatures(n_sigs: int = STAB_MAX_CLASSES + 1, n_nodes: int = 64) -> Scene:
    """One pod per static signature, every one with an image.  A cluster holds
    at most KSIM_MAX_CLASSES = 4,096 count classes, so 4,097 image classes
    cannot exist; the signatures are 2,049 image sets (a listed image, seven of
    them by residue, beside an unlisted one of the set's own) times whether the
    pod tolerates the PreferNoSchedule taint every fifth node carries.  The
    pods past kStabMaxClasses have no static class."""
    n_img = (n_sigs + 1) // 2
    assert n_img <= MAX_CLASSES
    imgs: Dict[int, list] = {i: [] for i in range(n_nodes)}
    for k in range(7):
        hold = [i for i in range(n_nodes) if i % 7 == k]
        size = size_for(20 + 12 * k, len(hold), n_nodes, 2)
        for i in hold:
            imgs[i].append((f"m.io/i{k}", size))
    nodes = [make_node(i, imgs[i], cpu="64", mem="512Gi", extra={"pods": "200"},
                       taints=[Taint("soft", "yes", "PreferNoSchedule")] if i % 5 == 0 else [])
             for i in range(n_nodes)]
    queue = []
    for j in range(n_sigs):
        k = j % n_img
        p = make_pod(j, [f"m.io/i{k % 7}", f"own.io/u{k}"], cpu="50m", mem="64Mi")
        if j >= n_img:
            p.tolerations = [Toleration(key="soft", operator="Exists")]
        queue.append(p)
    return Scene(f"many_signatures_{n_sigs}", nodes, queue)


# ---- wrong readings ------------------------------------------------------------------
def _with_rows(cluster, f):
    c = cluster.copy_state()
    for r in image_rows(cluster):
        c.class_count[r] = f(c.class_count[r])
    return c


def _first_class(cluster, pods):
    """Every image pod reads the first image class's row."""
    q = copy.copy(pods)
    q.uses = pods.uses.copy()
    from ksim import abi
    q.uses["cls"][q.uses["kind"] == abi.USE_IMAGE] = image_rows(cluster)[0]
    return q


# name -> (cluster, pods, compiled profile) the faulty engine would in effect run, at pct
FAULTS: Dict[str, Callable[[Scene, int], tuple]] = {
    "image_term_dropped": lambda s, pct: (s.encoded[0], s.encoded[1], s.compiled(pct, make_profile(None))),
    "field_six_bits": lambda s, pct: (_with_rows(s.encoded[0], lambda r: r & 63), s.encoded[1], s.compiled(pct)),
    "field_saturates_63": lambda s, pct: (_with_rows(s.encoded[0], lambda r: np.minimum(r, 63)), s.encoded[1],
                                          s.compiled(pct)),
    "classes_shared_across_images": lambda s, pct: (s.encoded[0], _first_class(*s.encoded), s.compiled(pct)),
    "weight_read_as_one": lambda s, pct: (s.encoded[0], s.encoded[1], s.compiled(pct, make_profile(1))),
}


def old_positions(c0, c1) -> np.ndarray:
    """ksim_upsert_nodes' old_pos: where each node of c1 stands in c0, or -1."""
    at = {nm: i for i, nm in enumerate(c0.node_names)}
    return np.array([at.get(nm, -1) for nm in c1.node_names], np.int32)


def stale_after_delta(s: Scene):
    """The snapshot after the delta with the image rows of the one before it
    (the new nodes 0): what a static table that outlived the delta holds."""
    c0, _ = s.encoded
    c1, _ = s.encoded_after
    c = c1.copy_state()
    for r in image_rows(c0):
        c.class_count[r] = 0
        c.class_count[r, :c0.n_nodes] = c0.class_count[r]
    return c
