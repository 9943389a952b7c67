"""Small node volume limit scenes for tests/test_vollimit_ref.py (CPU) and
tests/test_gpu_vollimits.py: model objects (nodes, PVs, PVCs, bound and pending
pods), hand-written verdicts for the small ones, and two array-level scenes for
the device's 64-bit comparison.  Node counts 1, 64, 65, 257 and 300 cover the
wave and 256-thread block edges of the per-node kernels."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

from ksim.model import Container, Node, PersistentVolume, PersistentVolumeClaim, Pod

EBS_KEY, GCE_KEY, AZ_KEY = "attachable-volumes-aws-ebs", "attachable-volumes-gce-pd", "attachable-volumes-azure-disk"
SOURCES = {"ebs": "awsElasticBlockStore", "gce": "gcePersistentDisk", "azure": "azureDisk"}


@dataclass
class Scene:
    name: str
    nodes: List[Node] = field(default_factory=list)
    pvs: List[PersistentVolume] = field(default_factory=list)
    pvcs: List[PersistentVolumeClaim] = field(default_factory=list)
    bound: List[Pod] = field(default_factory=list)
    pending: List[Pod] = field(default_factory=list)
    # hand-written: pod name -> {node name: failing limit plugins}, against the bound pods alone;
    # nodes left out pass every limit plugin
    expect: Optional[Dict[str, Dict[str, Set[str]]]] = None
    shared: bool = False                  # some volume is held by two or more pods
    _claims: Dict[Tuple[str, str], str] = field(default_factory=dict)

    def node(self, name: str, alloc: Optional[Dict[str, str]] = None, labels: Optional[Dict[str, str]] = None,
             cpu: str = "16") -> str:
        a = {"cpu": cpu, "memory": "64Gi", "pods": "110"}
        a.update(alloc or {})
        lab = {"kubernetes.io/hostname": name}
        lab.update(labels or {})
        self.nodes.append(Node(name=name, labels=lab, allocatable=a))
        return name

    def claim(self, kind: str, vid: str) -> str:
        """The claim bound to volume ``vid`` of ``kind`` (ebs / gce / azure, or
        csi:<driver>); one PV and claim per volume."""
        key = (kind, vid)
        if key not in self._claims:
            k = len(self.pvs)
            if kind.startswith("csi:"):
                pv = PersistentVolume(name=f"pv{k}", source="csi", source_id=vid, csi_driver=kind[4:])
            else:
                pv = PersistentVolume(name=f"pv{k}", source=SOURCES[kind], source_id=vid)
            pv.claim_ref = ("default", f"c{k}")
            self.pvs.append(pv)
            self.pvcs.append(PersistentVolumeClaim(name=f"c{k}", namespace="default", volume_name=pv.name))
            self._claims[key] = f"c{k}"
        return self._claims[key]

    def pod(self, name: str, vols=(), on: str = "", cpu: str = "100m", claims_twice: bool = False) -> Pod:
        claims = [self.claim(k, v) for k, v in vols]
        if claims_twice:
            claims = claims + claims[:1]
        p = Pod(name=name, containers=[Container({"cpu": cpu, "memory": "64Mi"})], pvc_claims=claims, node_name=on)
        (self.bound if on else self.pending).append(p)
        return p


def one_node() -> Scene:
    s = Scene("one_node")
    s.node("n0", {EBS_KEY: "2"})
    s.pod("b0", [("ebs", "a")], on="n0")
    s.pod("p_attached", [("ebs", "a")])                       # 1 + 0 <= 2
    s.pod("p_two_new", [("ebs", "b"), ("ebs", "c")])          # 1 + 2 > 2
    s.pod("p_one_new", [("ebs", "d")])                        # 1 + 1 <= 2
    s.pod("p_plain")
    s.expect = {"p_attached": {}, "p_two_new": {"n0": {"EBSLimits"}}, "p_one_new": {}, "p_plain": {}}
    s.shared = True
    return s


def over_limit() -> Scene:
    """A node already over its limit: the in-tree plugin rejects a pod whose
    disk is attached there, the CSI one lets it in."""
    s = Scene("over_limit")
    s.node("n0", {EBS_KEY: "1", "attachable-volumes-csi-x": "1"})
    s.node("n1", {EBS_KEY: "3", "attachable-volumes-csi-x": "3"})
    s.pod("b0", [("ebs", "a"), ("csi:x", "h0")], on="n0")
    s.pod("b1", [("ebs", "b"), ("csi:x", "h1")], on="n0")
    s.pod("p_ebs_attached", [("ebs", "a")])
    s.pod("p_csi_attached", [("csi:x", "h0")])
    s.pod("p_csi_new", [("csi:x", "h2")])
    s.pod("p_both", [("ebs", "b"), ("csi:x", "h1")])
    s.expect = {"p_ebs_attached": {"n0": {"EBSLimits"}}, "p_csi_attached": {},
                "p_csi_new": {"n0": {"NodeVolumeLimits"}}, "p_both": {"n0": {"EBSLimits"}}}
    s.shared = True
    return s


def limit_zero() -> Scene:
    s = Scene("limit_zero")
    s.node("n0", {GCE_KEY: "0", "attachable-volumes-csi-x": "0"})
    s.node("n1")
    s.node("n2", {"attachable-volumes-csi-x": "1"})
    s.pod("p_gce", [("gce", "d0")])
    s.pod("p_csi", [("csi:x", "h0")])
    s.pod("p_csi2", [("csi:x", "h1"), ("csi:x", "h2")])
    s.expect = {"p_gce": {"n0": {"GCEPDLimits"}}, "p_csi": {"n0": {"NodeVolumeLimits"}},
                "p_csi2": {"n0": {"NodeVolumeLimits"}, "n2": {"NodeVolumeLimits"}}}
    return s


def csi_missing_key() -> Scene:
    """A node without the CSI key next to nodes with it; driver y publishes no
    key anywhere and has no family."""
    s = Scene("csi_missing_key")
    s.node("n0", {"attachable-volumes-csi-x": "1"})
    s.node("n1")
    s.node("n2", {"attachable-volumes-csi-x": "2"})
    s.pod("p_x2", [("csi:x", "h0"), ("csi:x", "h1")])
    s.pod("p_y9", [("csi:y", f"y{k}") for k in range(9)])
    s.pod("p_x1", [("csi:x", "h2")])
    s.expect = {"p_x2": {"n0": {"NodeVolumeLimits"}}, "p_y9": {}, "p_x1": {}}
    return s


def claim_twice() -> Scene:
    s = Scene("claim_twice")
    s.node("n0", {AZ_KEY: "1"})
    s.pod("p_twice", [("azure", "d0")], claims_twice=True)      # one volume, listed twice: 0 + 1 <= 1
    s.pod("p_two", [("azure", "d1"), ("azure", "d2")])
    s.expect = {"p_twice": {}, "p_two": {"n0": {"AzureDiskLimits"}}}
    return s


def alloc_override() -> Scene:
    """allocatable above and below the default 39, next to a node without the key."""
    s = Scene("alloc_override")
    s.node("n_above", {EBS_KEY: "50"})
    s.node("n_default")
    s.node("n_below", {EBS_KEY: "3"})
    s.pod("p40", [("ebs", f"v{k}") for k in range(40)])
    s.pod("p4", [("ebs", f"w{k}") for k in range(4)])
    s.expect = {"p40": {"n_default": {"EBSLimits"}, "n_below": {"EBSLimits"}}, "p4": {"n_below": {"EBSLimits"}}}
    return s


def instance_types() -> Scene:
    s = Scene("instance_types")
    it, beta = "node.kubernetes.io/instance-type", "beta.kubernetes.io/instance-type"
    s.node("n_c5", labels={it: "c5.large"})
    s.node("n_t3", labels={beta: "t3.small"})
    s.node("n_m4", labels={it: "m4.large"})
    s.node("n_both", labels={it: "m4.large", beta: "c5.large"})      # the first label wins: 39
    s.node("n_z1d", labels={it: "x.z1d.large"})                      # a search, not a full match: 25
    s.pod("p26", [("ebs", f"v{k}") for k in range(26)])
    s.pod("p25", [("ebs", f"w{k}") for k in range(25)])
    s.expect = {"p26": {"n_c5": {"EBSLimits"}, "n_t3": {"EBSLimits"}, "n_z1d": {"EBSLimits"}}, "p25": {}}
    return s


def same_node_sharers() -> Scene:
    """Two pods of one node hold the same disk: it is attached once."""
    s = Scene("same_node_sharers")
    s.node("n0", {EBS_KEY: "2"})
    s.pod("b0", [("ebs", "s")], on="n0")
    s.pod("b1", [("ebs", "s")], on="n0")
    s.pod("p_t", [("ebs", "t")])                               # 1 + 1 <= 2
    s.pod("p_tu", [("ebs", "t"), ("ebs", "u")])                # 1 + 2 > 2
    s.expect = {"p_t": {}, "p_tu": {"n0": {"EBSLimits"}}}
    s.shared = True
    return s


def unbind_holders() -> Scene:
    """Removals: a second holder leaves while the first stays (the disk stays
    attached), then the only holder of another disk leaves (it goes)."""
    s = Scene("unbind_holders")
    s.node("n0", {EBS_KEY: "2"})
    s.pod("b0", [("ebs", "a")], on="n0")
    s.pod("p_a", [("ebs", "a")])                               # placed: 1 + 0
    s.pod("p_b", [("ebs", "b")])                               # placed: 1 + 1
    s.pod("p_c", [("ebs", "c")])                               # 2 + 1 > 2 until p_b leaves
    s.expect = {"p_a": {}, "p_b": {}, "p_c": {}}
    s.shared = True
    return s


def two_families() -> Scene:
    s = Scene("two_families")
    s.node("n0", {EBS_KEY: "2", GCE_KEY: "2"})
    s.pod("b0", [("ebs", "a"), ("gce", "g")], on="n0")
    s.pod("p_b", [("ebs", "b")])                               # 1 + 1 <= 2: the GCE disk is not EBS's
    s.pod("p_gh", [("gce", "h"), ("gce", "i")])                # 1 + 2 > 2
    s.expect = {"p_b": {}, "p_gh": {"n0": {"GCEPDLimits"}}}
    return s


def shared_three(n_nodes: int = 65) -> Scene:
    """A volume held by three pods across two nodes (two bound, one pending),
    and a second holder that leaves while the first stays."""
    s = Scene(f"shared_three_{n_nodes}")
    for i in range(n_nodes):
        s.node(f"n{i:03d}", {EBS_KEY: "2", "attachable-volumes-csi-x": "2"})
    s.pod("b0", [("ebs", "s"), ("ebs", "a")], on="n000")
    s.pod("b1", [("ebs", "s")], on="n001")
    s.pod("b2", [("csi:x", "hs"), ("csi:x", "h1")], on=f"n{n_nodes - 1:03d}")
    s.pod("p_s", [("ebs", "s"), ("ebs", "b")])                 # n000: 2 + 1 > 2; n001: 1 + 1 <= 2; else 0 + 2 <= 2
    s.pod("p_s2", [("ebs", "s")])
    s.pod("p_hs", [("csi:x", "hs"), ("csi:x", "h2")])          # last node: 2 + 1 > 2
    s.pod("p_plain")
    s.pod("p_hs2", [("csi:x", "hs")])
    s.expect = {"p_s": {"n000": {"EBSLimits"}}, "p_s2": {}, "p_hs": {f"n{n_nodes - 1:03d}": {"NodeVolumeLimits"}},
                "p_plain": {}, "p_hs2": {}}
    s.shared = True
    return s


def all_families(n_nodes: int = 64) -> Scene:
    """All eight families at once, and one pod with 16 uses: a shared and an
    own volume in each family."""
    s = Scene(f"all_families_{n_nodes}")
    drivers = ["d0", "d1", "d2", "d3", "d4"]
    kinds = ["ebs", "gce", "azure"] + [f"csi:{d}" for d in drivers]
    for i in range(n_nodes):
        alloc = {EBS_KEY: str(1 + i % 3), GCE_KEY: str(1 + i % 2), AZ_KEY: "2"}
        for k, d in enumerate(drivers):
            if (i + k) % 4:                                    # every fourth node lacks the key
                alloc[f"attachable-volumes-csi-{d}"] = str(1 + (i + k) % 3)
        s.node(f"n{i:03d}", alloc)
    for k, kind in enumerate(kinds):
        s.pod(f"b{k}", [(kind, "shared")], on=f"n{(5 * k) % n_nodes:03d}")
    s.pod("p16", [(kind, v) for kind in kinds for v in ("shared", "own")])
    for k, kind in enumerate(kinds):
        s.pod(f"p_{k}", [(kind, "shared"), (kind, f"o{k}")])
        s.pod(f"q_{k}", [(kind, f"q{k}")])
    s.pod("p_plain")
    s.shared = True
    return s


def mixed(n_nodes: int, seed: int, shared: bool) -> Scene:
    """A generated queue: volume pods of EBS, GCE PD and two CSI drivers mixed
    with plain (batchable) pods, limits of 0 to 2 so that many nodes refuse a
    pod and some pods fit nowhere.  Without
    ``shared`` every volume has one holder and every CSI pod brings new volumes."""
    rng = np.random.default_rng(seed)
    s = Scene(f"mixed_{n_nodes}_{'shared' if shared else 'own'}")
    for i in range(n_nodes):
        alloc = {EBS_KEY: str(int(rng.integers(0, 3))), GCE_KEY: str(int(rng.integers(0, 2)))}
        if i % 5:
            alloc["attachable-volumes-csi-x"] = str(int(rng.integers(0, 3)))
        if i % 3 == 0:
            alloc["attachable-volumes-csi-y"] = str(int(rng.integers(0, 2)))
        s.node(f"n{i:03d}", alloc, cpu="4")
    kinds = ["ebs", "gce", "csi:x", "csi:y"]
    n_bound = max(1, n_nodes // 3)
    for j in range(n_bound):
        kind = kinds[int(rng.integers(0, 4))]
        vid = f"s{int(rng.integers(0, 6))}" if shared else f"b{j}"
        s.pod(f"b{j}", [(kind, vid)], on=f"n{int(rng.integers(0, n_nodes)):03d}")
    n_pending = min(3 * n_nodes, 40)
    for j in range(n_pending):
        r = int(rng.integers(0, 10))
        if r < 3:
            s.pod(f"q{j}", cpu="200m")
            continue
        vols = []
        one_kind = kinds[int(rng.integers(0, 4))] if r < 7 else None   # often every volume of one family
        for k in range(int(rng.integers(1, 4))):
            kind = one_kind or kinds[int(rng.integers(0, 4))]
            vid = f"s{int(rng.integers(0, 6))}" if shared and rng.integers(0, 2) else f"p{j}_{k}"
            vols.append((kind, vid))
        s.pod(f"q{j}", vols, cpu="200m")
    s.shared = shared
    return s


def object_scenes() -> List[Scene]:
    return [one_node(), over_limit(), limit_zero(), csi_missing_key(), claim_twice(), alloc_override(),
            instance_types(), same_node_sharers(), unbind_holders(), two_families(), shared_three(65), all_families(64), mixed(1, 11, True), mixed(64, 12, False),
            mixed(65, 13, True), mixed(257, 14, False), mixed(300, 15, True)]


# ---- array-level scenes: the device's comparison at the int32 edge ---------------------
INT32_MAX = 2**31 - 1


@dataclass
class RawScene:
    """Tables handed to ksim_set_volume_limits as they are, one classless use
    per pod: (family, count) -> the nodes that must fail."""
    name: str
    family_plugin: List[str]
    limit: List[List[int]]
    attached: List[List[int]]
    pods: List[Tuple[int, int, List[int]]]       # (family, count, failing node positions)


def raw_scenes() -> List[RawScene]:
    big = INT32_MAX - 2
    return [
        # node 0: no limit (the sentinel) next to an attached count near INT32_MAX - 1: never fails;
        # node 1: limit INT32_MAX - 1, attached INT32_MAX - 2: one more fits, two more do not
        # (a 32-bit sum would wrap and pass); node 2: small numbers
        RawScene("csi_near_int32_max", ["NodeVolumeLimits"], [[INT32_MAX, INT32_MAX - 1, 3]], [[big, big, 2]],
                 [(0, 1, []), (0, 2, [1, 2]), (0, 5, [1, 2])]),
        RawScene("ebs_near_int32_max", ["EBSLimits"], [[INT32_MAX, INT32_MAX - 1, 3]], [[big, big, 3]],
                 [(0, 1, [2]), (0, 2, [1, 2])]),
    ]


# ---- the header's formula over the compiled tables --------------------------------------
PLUGIN_NAMES = ("EBSLimits", "GCEPDLimits", "NodeVolumeLimits", "AzureDiskLimits")


class HeaderModel:
    """include/ksim_engine.h "Node volume limits" read literally in numpy over
    limit, attached, the class counts and a pod's uses [(family, cls, arg)]:
    what the device must compute from the same tables."""

    def __init__(self, family_plugin, limit, attached, class_count):
        self.plugin = [str(x) for x in family_plugin]          # plugin names per family
        self.limit = np.array(limit, np.int64)
        self.attached = np.array(attached, np.int64)
        self.cnt = {c: np.array(v, np.int64) for c, v in class_count.items()}

    def failing(self, uses) -> Dict[str, np.ndarray]:
        """plugin name -> bool[N], for the plugins owning a family the pod has a use of."""
        out: Dict[str, np.ndarray] = {}
        for f in sorted({u[0] for u in uses}):
            new = np.zeros(self.limit.shape[1], np.int64)
            for fam, cls, arg in uses:
                if fam == f:
                    new += (self.cnt[cls] == 0) if cls >= 0 else arg
            over = (self.attached[f] + new > self.limit[f]) & (self.limit[f] != INT32_MAX)
            if self.plugin[f] == "NodeVolumeLimits":
                over &= new > 0
            out[self.plugin[f]] = out.get(self.plugin[f], False) | over
        return out

    def bind(self, uses, node: int, sign: int) -> None:
        for f, cls, arg in uses:
            if cls < 0:
                self.attached[f, node] += sign * arg
                continue
            old = int(self.cnt[cls][node])
            self.cnt[cls][node] = old + sign
            if (sign > 0 and old == 0) or (sign < 0 and old == 1):
                self.attached[f, node] += sign
