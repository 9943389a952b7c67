"""Node volume limits at the object level: the reference of
tests/test_vollimit_ref.py and tests/test_gpu_vollimits.py.  The C oracle knows
no volume limits, so this is a restatement of its own, over ksim.model objects
(pods, nodes, PVs, PVCs) and Python sets of unique volume names.  It follows
upstream v1.26.2 nodevolumelimits/non_csi.go and csi.go, restated from memory:

  scope      volumes reached through a persistentVolumeClaim bound to a PV;
             csiNode is nil (no CSINode objects) and CSI migration is off, so an
             in-tree PV counts with its in-tree plugin only and NodeVolumeLimits
             counts PVs with spec.csi;
  families   attachable-volumes-aws-ebs (EBSLimits, volumeID), -gce-pd
             (GCEPDLimits, pdName), -azure-disk (AzureDiskLimits, diskName) and
             attachable-volumes-csi-<driver> (NodeVolumeLimits,
             <driver>/<volumeHandle>) for the drivers some node publishes;
  limit      in-tree: the node's allocatable value of the key, else 39 / 16 /
             16, EBS 25 when the instance-type label (node.kubernetes.io/ first,
             then beta.kubernetes.io/) matches ^[cmr]5.*|t3|z1d (a regexp
             search); CSI: allocatable, a node without the key has no limit;
  filter     per family f of the plugin the pod has a volume of: existing = the
             distinct family-f names over the node's pods, new = the pod's
             family-f names not among them; in-tree fails when
             existing + new > limit, CSI when new > 0 and existing + new > limit.

Nothing is kept between questions but "which pods are on which node": every
count is recomputed from the pods' volumes.  No code is shared with
ksim.volumes or the engine.

``fault`` switches on one wrong reading an implementation could have (FAULTS),
for the test that the scenes of tests/vollimitcases.py tell each from the
reference."""
from __future__ import annotations

import re
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple

from ksim.model import Node, PersistentVolume, PersistentVolumeClaim, Pod, quantity_value

FAULTS = ("shared_twice",              # a volume held by two pods of a node counts twice
          "intree_new0_pass",          # in-tree: a pod whose disks are all attached passes an over-limit node
          "csi_rule_intree",           # in-tree families by the CSI rule (new > 0; no key, no limit)
          "intree_rule_csi",           # CSI families fail with new == 0 as well
          "default_over_allocatable",  # the in-tree default even when allocatable has the key
          "nitro_default_wrong",       # 39 whatever the instance type
          "missing_csi_key_zero",      # a node without the CSI key has limit 0
          "unbind_never",              # a removed pod's volumes stay attached
          "unbind_while_held",         # a removed pod's volumes leave though another pod holds them
          "cross_family",              # a family's existing count includes the node's other families
          "limit_ge")                  # fails when existing + new >= limit

PLUGINS = ("EBSLimits", "GCEPDLimits", "NodeVolumeLimits", "AzureDiskLimits")
EBS, GCE, AZURE = "attachable-volumes-aws-ebs", "attachable-volumes-gce-pd", "attachable-volumes-azure-disk"
CSI_PREFIX = "attachable-volumes-csi-"
_IN_TREE = {"awsElasticBlockStore": (EBS, "EBSLimits"), "gcePersistentDisk": (GCE, "GCEPDLimits"),
            "azureDisk": (AZURE, "AzureDiskLimits")}
_DEFAULT = {EBS: 39, GCE: 16, AZURE: 16}
_NITRO = re.compile("^[cmr]5.*|t3|z1d")
NO_LIMIT = None


def owner(family: str) -> str:
    for key, plugin in _IN_TREE.values():
        if key == family:
            return plugin
    return "NodeVolumeLimits"


class VolLimitRef:
    def __init__(self, nodes: Sequence[Node], pvs: Iterable[PersistentVolume], pvcs: Iterable[PersistentVolumeClaim],
                 fault: Optional[str] = None):
        assert fault is None or fault in FAULTS
        self.nodes = {n.name: n for n in nodes}
        self.order = [n.name for n in nodes]
        self.pvs = {v.name: v for v in pvs}
        self.pvcs = {(c.namespace, c.name): c for c in pvcs}
        self.fault = fault
        self.published = {k[len(CSI_PREFIX):] for n in nodes for k in n.allocatable if k.startswith(CSI_PREFIX)}
        self.on: Dict[str, List[Pod]] = {n.name: [] for n in nodes}   # the only state: pods per node
        # what the two unbind faults remember (a correct reading remembers nothing)
        self._ghost: Dict[str, List[Tuple[str, str]]] = {n.name: [] for n in nodes}
        self._dropped: Dict[str, Set[Tuple[str, str]]] = {n.name: set() for n in nodes}

    # ---- a pod's counted volumes -------------------------------------------------
    def volumes(self, pod: Pod) -> Set[Tuple[str, str]]:
        """{(family, unique name)} through the pod's bound claims."""
        out: Set[Tuple[str, str]] = set()
        for claim in pod.pvc_claims:
            pvc = self.pvcs.get((pod.namespace, claim))
            if pvc is None or not pvc.volume_name or pvc.volume_name not in self.pvs:
                continue
            pv = self.pvs[pvc.volume_name]
            if pv.source in _IN_TREE:
                out.add((_IN_TREE[pv.source][0], pv.source_id))
            elif pv.source == "csi" and pv.csi_driver in self.published:
                out.add((CSI_PREFIX + pv.csi_driver, f"{pv.csi_driver}/{pv.source_id}"))
        return out

    # ---- placement ----------------------------------------------------------------
    def place(self, pod: Pod, node: str) -> None:
        self.on[node].append(pod)
        self._dropped[node] -= self.volumes(pod)

    def remove(self, pod: Pod, node: str) -> None:
        self.on[node].remove(pod)
        if self.fault == "unbind_never":
            self._ghost[node].extend(sorted(self.volumes(pod)))
        if self.fault == "unbind_while_held":
            self._dropped[node] |= self.volumes(pod)

    # ---- per node -------------------------------------------------------------------
    def limit(self, family: str, node: str) -> Optional[int]:
        n = self.nodes[node]
        in_tree = family in _DEFAULT
        if family in n.allocatable and not (in_tree and self.fault == "default_over_allocatable"):
            return int(quantity_value(n.allocatable[family]))
        if not in_tree:
            return 0 if self.fault == "missing_csi_key_zero" else NO_LIMIT
        if self.fault == "csi_rule_intree":
            return NO_LIMIT
        if family == EBS and self.fault != "nitro_default_wrong":
            itype = n.labels.get("node.kubernetes.io/instance-type") or n.labels.get("beta.kubernetes.io/instance-type") or ""
            if itype and _NITRO.search(itype):
                return 25
        return _DEFAULT[family]

    def existing(self, family: str, node: str):
        """The family's volumes on the node: a set, or a list under the faults that miscount."""
        names: List[Tuple[str, str]] = []
        for p in self.on[node]:
            names.extend(sorted(self.volumes(p)))
        names.extend(self._ghost[node])
        if self.fault != "cross_family":
            names = [v for v in names if v[0] == family]
        if self.fault == "shared_twice":
            return names
        return set(names) - self._dropped[node]

    def attached(self, family: str, node: str) -> int:
        return len(self.existing(family, node))

    def failing(self, pod: Pod, node: str) -> Set[str]:
        """The limit plugins whose Filter fails the pod on the node."""
        out: Set[str] = set()
        mine = self.volumes(pod)
        for family in sorted({v[0] for v in mine}):
            have = self.existing(family, node)
            new = len({v for v in mine if v[0] == family} - set(have))
            lim = self.limit(family, node)
            if lim is NO_LIMIT:
                continue
            in_tree = family in _DEFAULT
            if self.fault == "csi_rule_intree":
                in_tree = False
            if self.fault == "intree_rule_csi":
                in_tree = True
            if in_tree and new == 0 and self.fault == "intree_new0_pass":
                continue
            if not in_tree and new == 0:
                continue
            total = len(have) + new
            if total > lim or (self.fault == "limit_ge" and total >= lim):
                out.add(owner(family))
        return out

    def verdicts(self, pod: Pod) -> Dict[str, Set[str]]:
        return {n: self.failing(pod, n) for n in self.order}
