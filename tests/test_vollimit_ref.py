"""Node volume limits on the CPU: the object-level reference
(tests/vollimitref.py) against hand-written verdicts, the host compile
(ksim.volumes.VolumeIndex.volume_limits) against the reference on every scene,
placement step and node -- the compile read through the header's formula in
numpy (vollimitcases.HeaderModel) -- and every wrong reading the reference can
switch on changes a verdict of some scene."""
import numpy as np
import pytest

from ksim import abi
from ksim.encode import encode_cluster, encode_pods
from ksim.volumes import VolumeIndex

import vollimitcases as cases
from vollimitref import FAULTS, PLUGINS, VolLimitRef

SCENES = cases.object_scenes()


def script(sc):
    """The scene's steps from the (correct) reference: ("ask", pod) records
    every node's verdict, ("place" / "remove", pod, node) moves a pod.  Each
    pending pod is asked, then placed on the first node that passes every limit
    plugin, scanning from a start that moves with the step; then the placed
    pods leave in placement order, every pending pod that is on no node asked
    again after each."""
    ref = VolLimitRef(sc.nodes, sc.pvs, sc.pvcs)
    for b in sc.bound:
        ref.place(b, b.node_name)
    steps, placed = [], []
    n = len(sc.nodes)
    for k, p in enumerate(sc.pending):
        steps.append(("ask", p))
        v = ref.verdicts(p)
        for r in range(n):
            name = ref.order[(7 * k + r) % n]
            if not v[name]:
                steps.append(("place", p, name))
                ref.place(p, name)
                placed.append((p, name))
                break
    asked = sc.pending if n <= 65 else sc.pending[:8]
    there = {p.name for p, _ in placed}
    for p, name in (placed if n <= 65 else placed[:6]):
        steps.append(("remove", p, name))
        there.discard(p.name)
        for q in asked:                   # a pod is only ever scheduled while it is on no node
            if q.name not in there:
                steps.append(("ask", q))
    return steps


def replay(sc, steps, fault=None):
    """The verdicts a (possibly faulty) reference gives along ``steps``."""
    ref = VolLimitRef(sc.nodes, sc.pvs, sc.pvcs, fault)
    for b in sc.bound:
        ref.place(b, b.node_name)
    out = []
    for st in steps:
        if st[0] == "ask":
            out.append(ref.verdicts(st[1]))
        elif st[0] == "place":
            ref.place(st[1], st[2])
        else:
            ref.remove(st[1], st[2])
    return out, ref


SCRIPTS = {sc.name: script(sc) for sc in SCENES}
ANSWERS = {sc.name: replay(sc, SCRIPTS[sc.name])[0] for sc in SCENES}     # computed once, shared, never changed


@pytest.mark.parametrize("sc", [s for s in SCENES if s.expect is not None], ids=lambda s: s.name)
def test_reference_matches_hand_written_verdicts(sc):
    ref = VolLimitRef(sc.nodes, sc.pvs, sc.pvcs)
    for b in sc.bound:
        ref.place(b, b.node_name)
    assert set(sc.expect) == {p.name for p in sc.pending}
    for p in sc.pending:
        want = {n.name: set(sc.expect[p.name].get(n.name, ())) for n in sc.nodes}
        assert ref.verdicts(p) == want, p.name


def compiled(sc):
    index = VolumeIndex.from_nodes(sc.nodes, sc.pvs, sc.pvcs)
    vl = index.volume_limits(sc.nodes, sc.bound, sc.pending)
    cls = {key: k for k, key in enumerate(vl.shared)}
    model = cases.HeaderModel([abi.PLUGINS[int(x)] for x in vl.family_plugin], vl.limit, vl.attached,
                              {cls[key]: v for key, v in vl.shared.items()})
    uses = {name: [(f, -1 if sh is None else cls[(f, sh)], c) for f, sh, c in u] for name, u in vl.pod_uses.items()}
    return vl, model, uses


@pytest.mark.parametrize("sc", SCENES, ids=lambda s: s.name)
def test_compile_matches_reference_at_every_step(sc):
    vl, model, uses = compiled(sc)
    pos = {n.name: i for i, n in enumerate(sc.nodes)}
    assert vl.node_names == [n.name for n in sc.nodes] and len(vl.families) <= abi.MAX_VOL_FAMILIES
    assert all(len(u) <= abi.MAX_USES for u in uses.values())
    # a class only for volumes two or more pods hold; at most one classless use per family
    for u in uses.values():
        own = [f for f, c, _ in u if c < 0]
        assert len(own) == len(set(own)) and all(a == 1 for _, c, a in u if c >= 0)
    answers = iter(ANSWERS[sc.name])
    for st in SCRIPTS[sc.name]:
        u = uses.get((st[1].namespace, st[1].name), [])
        if st[0] == "ask":
            want = next(answers)
            got = model.failing(u)
            for pl in PLUGINS:
                w = np.array([pl in want[n.name] for n in sc.nodes])
                assert np.array_equal(got.get(pl, np.zeros(len(sc.nodes), bool)), w), (st[1].name, pl)
        else:
            model.bind(u, pos[st[2]], 1 if st[0] == "place" else -1)
    # the attached counts equal the reference's recount of the final placement
    _, ref = replay(sc, SCRIPTS[sc.name])
    for f, key in enumerate(vl.families):
        assert [int(x) for x in model.attached[f]] == [ref.attached(key, n.name) for n in sc.nodes], key
    assert all((v >= 0).all() for v in model.cnt.values())


def test_scenes_cover_the_listed_ground():
    by = {s.name: s for s in SCENES}
    assert {len(s.nodes) for s in SCENES} >= {1, 64, 65, 257, 300}
    vl, _, uses = compiled(by["all_families_64"])
    assert len(vl.families) == 8 and sorted(set(int(x) for x in vl.family_plugin)) == [
        abi.PL_EBS_LIMITS, abi.PL_GCEPD_LIMITS, abi.PL_NODE_VOLUME_LIMITS, abi.PL_AZURE_DISK_LIMITS]
    assert len(uses[("default", "p16")]) == 16
    vl, _, uses = compiled(by["claim_twice"])
    assert uses[("default", "p_twice")] == [(0, -1, 1)]
    vl, _, _ = compiled(by["csi_missing_key"])
    assert vl.families == ["attachable-volumes-csi-x"] and list(vl.limit[0]) == [1, abi.INT32_MAX, 2]
    vl, _, _ = compiled(by["instance_types"])
    assert list(vl.limit[0]) == [25, 25, 39, 39, 25]
    vl, _, _ = compiled(by["alloc_override"])
    assert list(vl.limit[0]) == [50, 39, 3]
    vl, _, _ = compiled(by["shared_three_65"])
    assert sorted(int(v.sum()) for v in vl.shared.values()) == [1, 2]   # hs: one bound holder; s: two, on two nodes


@pytest.mark.parametrize("fault", FAULTS)
def test_every_wrong_reading_changes_a_verdict(fault):
    hit = [sc.name for sc in SCENES if len(sc.nodes) <= 65
           and replay(sc, SCRIPTS[sc.name], fault)[0] != ANSWERS[sc.name]]
    assert hit, f"no scene tells {fault} from the reference"


@pytest.mark.parametrize("rs", cases.raw_scenes(), ids=lambda r: r.name)
def test_array_scenes_by_the_header_formula(rs):
    model = cases.HeaderModel(rs.family_plugin, rs.limit, rs.attached, {})
    for f, count, bad in rs.pods:
        got = model.failing([(f, -1, count)])[rs.family_plugin[f]]
        assert list(np.flatnonzero(got)) == bad, (f, count)


def test_encode_compiles_uses_and_keeps_refusing_the_rest():
    """The compile through ksim.encode: volume pods get KSIM_USE_VOLUME uses
    (family in col, a class for shared volumes, no class adds for them); without
    the compile the same pods stay flagged KSIM_POD_HAS_VOLUMES."""
    sc = cases.shared_three(65)
    index = VolumeIndex.from_nodes(sc.nodes, sc.pvs, sc.pvcs)
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    flagged = encode_pods(cluster, sc.pending, volumes=index)
    assert [bool(f & abi.POD_HAS_VOLUMES) for f in flagged.pods["flags"]] == [True, True, True, False, True]
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    vl = index.volume_limits(sc.nodes, sc.bound, sc.pending)
    cluster.set_volume_limits(vl)
    enc = encode_pods(cluster, sc.pending, volumes=index)
    assert not (enc.pods["flags"] & abi.POD_HAS_VOLUMES).any()
    vol = enc.uses[enc.uses["kind"] == abi.USE_VOLUME]
    assert len(vol) == 6 and set(int(c) for c in vol["col"]) == {0, 1}
    vol_cls = {int(c) for c in vol["cls"] if c >= 0}
    assert len(vol_cls) == 2 and not vol_cls & {int(c) for c in enc.adds["cls"]}
    assert cluster.vol_limits.node_names == cluster.node_names
    for c in vol_cls:                         # the bound holders' counts went into the cluster's class table
        assert cluster.class_count[c].sum() in (1, 2)


def test_ingest_document_compiles_and_keeps_refusing_the_rest():
    """The hand-written ResourcesForImport document: pods on EBS and CSI PVs
    join the queue with KSIM_USE_VOLUME uses (one claim bound by the PV
    controller at load); the inline-disk pod and the pod with an unbound
    WaitForFirstConsumer claim of an EBS-provisioning class are still reported."""
    import json
    import os
    from ksim import ingest
    with open(os.path.join(os.path.dirname(__file__), "golden", "vollimits", "import_volumes.json")) as f:
        snap = ingest.load(json.load(f))
    assert [(n, why.split(":")[0]) for _, n, why in snap.unsupported] == [("inline-disk", "volumes"),
                                                                          ("wait-ebs", "volumes")]
    assert "count against node limits" in snap.unsupported[1][2]
    assert snap.volumes.pvcs[("default", "c-ebs-0")].volume_name == "pv-ebs-0"
    cluster, pods, _ = ingest.encode(snap)
    vl = cluster.vol_limits
    assert vl.families == ["attachable-volumes-aws-ebs", "attachable-volumes-csi-disk.csi.example.com"]
    a, b = cluster.node_names.index("node-a"), cluster.node_names.index("node-b")
    assert (vl.limit[0, a], vl.limit[0, b], vl.limit[1, a], vl.limit[1, b]) == (1, 2, 1, 0)
    assert (vl.attached[0, a], vl.attached[0, b]) == (1, 0) and not vl.attached[1].any()
    assert not (pods.pods["flags"] & abi.POD_HAS_VOLUMES).any()
    vol = pods.uses[pods.uses["kind"] == abi.USE_VOLUME]
    assert len(vol) == 6                      # one per volume pod: three EBS, two CSI, the shared disk
    shared = vol[vol["cls"] >= 0]
    assert len(shared) == 1 and cluster.class_count[int(shared["cls"][0])][a] == 1
