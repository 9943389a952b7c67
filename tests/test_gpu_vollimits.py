"""Node volume limits on the GPU (EBSLimits, GCEPDLimits, NodeVolumeLimits,
AzureDiskLimits; KSIM_USE_VOLUME uses and ksim_set_volume_limits) against the
object-level reference tests/vollimitref.py and the C oracle.

The oracle knows no volume limits, so it takes part in two restatements:
  gate     before each cycle the oracle's nodes get a scalar column whose
           allocatable is 0 where the reference fails the pod and huge
           elsewhere (through its node-update call), and the oracle's copy of
           the pod, its volume uses stripped, requests 1 of it: the same
           feasible set, so placements, counters and node state must agree;
  columns  scenes where no volume is shared: each family is a scalar column
           (allocatable = limit, requested = attached, the pod requests its
           count), which needs no reference at all.
Per-node codes compose the oracle's codes for the stripped pod (a second
oracle kept on the engine's placements, evaluating every node) with the
reference's verdict for the four plugins: the first failure in profile order
wins."""
import dataclasses
import json
import os

import numpy as np
import pytest

from ksim import abi, ingest, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.engine import Engine, KsimError
from ksim.volumes import MSG_VOLUME_LIMIT, VolumeIndex
from ksim.wrapped import filter_message
from oracle.oracle import Oracle

import vollimitcases as cases
from vollimitref import PLUGINS, VolLimitRef

pytestmark = pytest.mark.gpu

GATE = "example.com/gate"
HUGE = 1 << 40
FIELDS = ("chosen", "status", "n_feasible", "n_evaluated", "n_processed", "k_to_find", "next_start")
DEFAULT_ORDER = profile.SchedulerProfile().filter_order()
LIMITS_FIRST = list(PLUGINS) + [p for p in DEFAULT_ORDER if p not in PLUGINS]
WITHOUT = [p for p in DEFAULT_ORDER if p not in PLUGINS]
ORDERS = {"default": DEFAULT_ORDER, "limits_first": LIMITS_FIRST, "without": WITHOUT}
BY_NAME = {s.name: s for s in cases.object_scenes()}


def sched_profile(order, pct):
    plugins = profile.convert_for_simulator({"filter": profile.PluginSet([profile.Plugin(n) for n in order],
                                                                         [profile.Plugin("*")])})
    return profile.SchedulerProfile(plugins=plugins, percentage_of_nodes_to_score=pct)


def strip_volume_uses(enc, scalar_req=None):
    """The oracle's copy of the pods: KSIM_USE_VOLUME uses taken out, and
    scalar_req[i] (column -> amount) requested instead."""
    pods = enc.pods.copy()
    keep = []
    for i in range(len(pods)):
        first, count = int(pods[i]["use_first"]), int(pods[i]["use_count"])
        rows = [k for k in range(first, first + count) if enc.uses[k]["kind"] != abi.USE_VOLUME]
        pods[i]["use_first"], pods[i]["use_count"] = len(keep), len(rows)
        keep.extend(rows)
        for col, amount in (scalar_req[i] if scalar_req else {}).items():
            pods[i]["scalar_req"][col] = amount
            pods[i]["flags"] |= abi.POD_HAS_SCALAR
    return dataclasses.replace(enc, pods=pods, uses=enc.uses[keep].copy() if keep else enc.uses[:0].copy())


def own_tables(cluster):
    c = cluster.copy_state()
    c.alloc_scalar = cluster.alloc_scalar.copy()
    return c


class Rig:
    """One scene encoded for the engine (with the limits compile) and for the
    gated oracle, plus the reference holding the bound pods."""

    def __init__(self, sc, order=DEFAULT_ORDER, pct=0, scalars=(GATE,)):
        self.sc = sc
        # every attachable-volumes-* key of a node is a scalar column already: a scene that
        # fills all of them lends the gate one (no pod requests those columns)
        published = {k for n in sc.nodes for k in n.allocatable if k not in ("cpu", "memory", "pods")}
        if len(published) + len(scalars) > abi.MAX_SCALAR:
            scalars = ()
        self.sp = sched_profile(order, pct)
        self.order = order
        self.index = VolumeIndex.from_nodes(sc.nodes, sc.pvs, sc.pvcs)
        self.cluster, _ = encode_cluster(sc.nodes, sc.bound, extra_scalar=list(scalars))
        self.vl = self.index.volume_limits(sc.nodes, sc.bound, sc.pending)
        self.cluster.set_volume_limits(self.vl)
        self.vl = self.cluster.vol_limits                       # in the cluster's node order
        self.enc = encode_pods(self.cluster, sc.pending, volumes=self.index)
        assert not (self.enc.pods["flags"] & abi.POD_HAS_VOLUMES).any()
        self.prof = profile.compile_profile(self.sp, self.cluster.scalar_names)
        self.names = self.cluster.node_names
        self.pos = {n: i for i, n in enumerate(self.names)}
        self.ref = VolLimitRef([n for name in self.names for n in sc.nodes if n.name == name], sc.pvs, sc.pvcs)
        for b in sc.bound:
            self.ref.place(b, b.node_name)

    def engine(self):
        eng = Engine(0)
        eng.set_profile(self.prof)
        eng.set_cluster(own_tables(self.cluster))
        return eng

    def failing(self, pod):
        """plugin -> bool[N] by the reference, only the plugins of the profile."""
        v = self.ref.verdicts(pod)
        return {pl: np.array([pl in v[n] for n in self.names]) for pl in PLUGINS if pl in self.order}

    def recount(self):
        return np.array([[self.ref.attached(key, n) for n in self.names] for key in self.vl.families], np.int32)

    def expected_codes(self, pod, fail, detail):
        """The oracle's codes of the stripped pod composed with the reference."""
        fail, detail = fail.copy(), detail.copy()
        for pl, bad in sorted(self.failing(pod).items(), key=lambda kv: self.order.index(kv[0]), reverse=True):
            q = self.order.index(pl)
            first = bad & ((fail == abi.PASSED) | (fail > q))
            fail[first], detail[first] = q, 0
        return fail, detail


class GateOracle:
    """The oracle stepping a rig's queue one cycle at a time behind the gate column."""

    def __init__(self, rig):
        self.rig = rig
        names = rig.cluster.scalar_names
        self.col = names.index(GATE) if GATE in names else 0
        self.cluster = own_tables(rig.cluster)
        self.cluster.alloc_scalar[self.col, :] = HUGE
        self.enc = strip_volume_uses(rig.enc, [{self.col: 1}] * rig.enc.n_pods)
        self.ora = Oracle(self.cluster, rig.prof)
        self.all = np.arange(self.cluster.n_nodes, dtype=np.int32)

    def cycle(self, i):
        closed = np.zeros(self.cluster.n_nodes, bool)
        for bad in self.rig.failing(self.rig.sc.pending[i]).values():
            closed |= bad
        self.cluster.alloc_scalar[self.col, :] = np.where(closed, 0, HUGE)
        self.ora.upsert_nodes(self.cluster, self.all)
        return self.ora.cycle(self.enc, i)


def run_reference_queue(rig):
    """The queue on the gated oracle alone: (chosen per pod, per-cycle results)."""
    gate = GateOracle(rig)
    out = []
    for i, pod in enumerate(rig.sc.pending):
        o = gate.cycle(i)
        out.append(o)
        if o["chosen"] >= 0:
            rig.ref.place(pod, rig.names[o["chosen"]])
    return gate, out


# ---- per-node codes, placements and state, cycle by cycle -------------------------------
STEP_CASES = [("over_limit", "default", 0), ("shared_three_65", "default", 0), ("shared_three_65", "limits_first", 100),
              ("all_families_64", "limits_first", 0), ("all_families_64", "without", 0),
              ("mixed_1_shared", "default", 0), ("mixed_65_shared", "default", 100),
              ("mixed_257_own", "limits_first", 0), ("mixed_300_shared", "default", 0),
              ("mixed_300_shared", "without", 100)]


@pytest.mark.parametrize("scene,order,pct", STEP_CASES)
def test_compat_cycles_codes_placements_and_state(scene, order, pct):
    rig = Rig(BY_NAME[scene], ORDERS[order], pct)
    eng = rig.engine()
    gate = GateOracle(rig)
    # the stripped pod's codes on every node: an oracle that evaluates all of
    # them (percentageOfNodesToScore 100), kept on the engine's placements
    plain = strip_volume_uses(rig.enc)
    codes = Oracle(own_tables(rig.cluster), profile.compile_profile(sched_profile(ORDERS[order], 100),
                                                                      rig.cluster.scalar_names))
    limit_hits = 0
    np.testing.assert_array_equal(eng.volume_attached(), rig.recount())
    for i, pod in enumerate(rig.sc.pending):
        e, o = eng.eval_pod(rig.enc, i), gate.cycle(i)
        for f in FIELDS:
            assert e[f] == o[f], f"pod {i} {pod.name}: {f} engine={e[f]} gated oracle={o[f]}"
        c = codes.cycle(plain, i)
        want_fail, want_detail = rig.expected_codes(pod, c["fail_plugin"], c["fail_detail"])
        seen = e["fail_plugin"] != abi.NOT_EVALUATED
        np.testing.assert_array_equal(e["fail_plugin"][seen], want_fail[seen], err_msg=f"pod {i} fail_plugin")
        np.testing.assert_array_equal(e["fail_detail"][seen], want_detail[seen], err_msg=f"pod {i} fail_detail")
        limit_hits += int(sum(((e["fail_plugin"] == rig.order.index(pl)) & seen).sum()
                              for pl in PLUGINS if pl in rig.order))
        if c["chosen"] >= 0:
            codes.forget(plain, i, c["chosen"])
        if e["chosen"] >= 0:
            codes.assume(plain, i, e["chosen"])
            rig.ref.place(pod, rig.names[e["chosen"]])
        if len(rig.names) <= 65:                               # the table after every cycle
            np.testing.assert_array_equal(eng.volume_attached(), rig.recount(), err_msg=f"after pod {i}")
    es, os_ = eng.node_state(), gate.ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=k)
    np.testing.assert_array_equal(eng.volume_attached(), rig.recount())
    if order == "without":
        assert limit_hits == 0
    elif scene != "mixed_1_shared":
        assert limit_hits > 0, "the scene never met a limit"
        plugin = next(pl for pl in PLUGINS if pl in rig.order)
        assert filter_message(rig.cluster, plugin, 0) == MSG_VOLUME_LIMIT == "node(s) exceed max volume count"


# ---- whole queues through ksim_schedule_loaded: stretches of batchable and volume pods ----
@pytest.mark.parametrize("scene", ["mixed_64_own", "mixed_65_shared", "mixed_257_own", "mixed_300_shared",
                                   "all_families_64"])
@pytest.mark.parametrize("pct", [0, 100])
def test_loaded_queue_against_gated_oracle(scene, pct):
    rig = Rig(BY_NAME[scene], DEFAULT_ORDER, pct)
    eng = rig.engine()
    chosen, st = eng.schedule_batch(rig.enc)
    gate, cycles = run_reference_queue(rig)
    np.testing.assert_array_equal(chosen, [o["chosen"] for o in cycles])
    assert eng.next_start == gate.ora.next_start
    assert st.scheduled == sum(o["chosen"] >= 0 for o in cycles)
    assert st.unschedulable == sum(o["chosen"] < 0 for o in cycles)
    assert st.evals == sum(o["n_evaluated"] for o in cycles)
    es, os_ = eng.node_state(), gate.ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=k)
    np.testing.assert_array_equal(eng.volume_attached(), rig.recount())
    has_vol = [bool(rig.vl.pod_uses.get((p.namespace, p.name))) for p in rig.sc.pending]
    assert any(has_vol) and not all(has_vol)                   # the run split into stretches
    # the table is part of what ksim_reset_cluster restores; the same queue again
    eng.reset_cluster()
    np.testing.assert_array_equal(eng.volume_attached(), rig.vl.attached)
    # ... in three calls, the getter against a recount of the placements so far after each
    fresh = Rig(BY_NAME[scene], DEFAULT_ORDER, pct)
    n = rig.enc.n_pods
    for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
        part, _ = eng.schedule_loaded(a, b - a)
        np.testing.assert_array_equal(part, chosen[a:b])
        for p, c in zip(fresh.sc.pending[a:b], part):
            if c >= 0:
                fresh.ref.place(p, fresh.names[c])
        np.testing.assert_array_equal(eng.volume_attached(), fresh.recount(), err_msg=f"after pods [{a}, {b})")
    np.testing.assert_array_equal(eng.volume_attached(), rig.recount())


@pytest.mark.parametrize("scene", ["mixed_64_own", "mixed_257_own"])
@pytest.mark.parametrize("pct", [0, 100])
def test_unshared_scenes_as_scalar_columns(scene, pct):
    """No volume is shared: each family restated as a scalar resource column
    for the oracle, which then runs the whole queue by itself."""
    sc = BY_NAME[scene]
    probe = Rig(sc, DEFAULT_ORDER, pct)
    F = len(probe.vl.families)
    assert F >= 3 and not probe.vl.shared
    cols = [f"example.com/vol{f}" for f in range(F)]
    rig = Rig(sc, DEFAULT_ORDER, pct, scalars=cols)
    ocluster = own_tables(rig.cluster)
    req = []
    for p in sc.pending:
        want = {}
        for f, _, count in rig.vl.pod_uses.get((p.namespace, p.name), []):
            k = rig.cluster.scalar_names.index(cols[f])
            want[k] = want.get(k, 0) + count
        req.append(want)
    for f in range(F):
        k = rig.cluster.scalar_names.index(cols[f])
        lim = rig.vl.limit[f].astype(np.int64)
        ocluster.alloc_scalar[k, :] = np.where(lim == abi.INT32_MAX, HUGE, lim)
        ocluster.req_scalar[k, :] = rig.vl.attached[f]
    oenc = strip_volume_uses(rig.enc, req)
    ora = Oracle(ocluster, rig.prof)
    want, ost = ora.schedule(oenc)
    eng = rig.engine()
    chosen, st = eng.schedule_batch(rig.enc)
    np.testing.assert_array_equal(chosen, want)
    assert (st.scheduled, st.unschedulable, st.evals) == (ost.scheduled, ost.unschedulable, ost.evals)
    assert eng.next_start == ora.next_start and (chosen < 0).any() and (chosen >= 0).any()
    es, os_ = eng.node_state(), ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=k)
    for p, c in zip(sc.pending, chosen):
        if c >= 0:
            rig.ref.place(p, rig.names[c])
    np.testing.assert_array_equal(eng.volume_attached(), rig.recount())


# ---- the device's comparison at the int32 edge ---------------------------------------------
@pytest.mark.parametrize("rs", cases.raw_scenes(), ids=lambda r: r.name)
def test_array_scenes_on_the_device(rs):
    sc = cases.Scene("raw")
    for k in range(len(rs.limit[0])):
        sc.node(f"n{k}")
    for k, _ in enumerate(rs.pods):
        sc.pod(f"p{k}")
    cluster, _ = encode_cluster(sc.nodes)
    enc = encode_pods(cluster, sc.pending)
    uses = np.zeros(len(rs.pods), abi.TOPO_USE_DTYPE)
    pods = enc.pods.copy()
    for k, (f, count, _) in enumerate(rs.pods):
        uses[k]["cls"], uses[k]["arg"], uses[k]["col"], uses[k]["kind"] = -1, count, f, abi.USE_VOLUME
        pods[k]["use_first"], pods[k]["use_count"] = k, 1
    assert enc.uses.size == 0
    enc = dataclasses.replace(enc, pods=pods, uses=uses)
    sp = profile.SchedulerProfile()
    eng = Engine(0)
    eng.set_profile(profile.compile_profile(sp))
    eng.set_cluster(cluster)
    order = [n.name for n in sc.nodes]
    perm = [order.index(n) for n in cluster.node_names]
    plug = [abi.PLUGIN_ID[p] for p in rs.family_plugin]
    eng.set_volume_limits(plug, np.array(rs.limit)[:, perm], np.array(rs.attached)[:, perm])
    model = cases.HeaderModel(rs.family_plugin, rs.limit, rs.attached, {})
    for k, (f, count, bad) in enumerate(rs.pods):
        r = eng.fw_prefilter(enc, k)                           # every node, nothing bound
        q = sp.filter_order().index(rs.family_plugin[f])
        got = sorted(perm[i] for i in np.flatnonzero(r["fail_plugin"] == q))
        assert got == bad == list(np.flatnonzero(model.failing([(f, -1, count)])[rs.family_plugin[f]])), (k, got)
        assert (r["fail_plugin"][[i for i in range(len(perm)) if perm[i] not in bad]] == abi.PASSED).all()
    # a bind next to the edge: attached INT32_MAX - 2 takes one more volume and gives it back
    node = perm.index(0)
    eng.assume(enc, 0, node)
    assert eng.volume_attached()[0, node] == rs.attached[0][0] + 1
    eng.forget(enc, 0, node)
    np.testing.assert_array_equal(eng.volume_attached(), np.array(rs.attached)[:, perm])


# ---- getter and state: assume / forget, framework-driven passes -----------------------------
def test_assume_forget_round_trips_and_second_holder():
    rig = Rig(BY_NAME["shared_three_65"])
    eng = rig.engine()
    idx = {p.name: i for i, p in enumerate(rig.sc.pending)}
    before = rig.recount()
    np.testing.assert_array_equal(eng.volume_attached(), before)
    counts = eng.class_count()
    # p_s on an empty node: two disks arrive and leave
    node = rig.pos["n010"]
    eng.assume(rig.enc, idx["p_s"], node)
    rig.ref.place(rig.sc.pending[idx["p_s"]], "n010")
    got = eng.volume_attached()
    np.testing.assert_array_equal(got, rig.recount())
    assert got[0, node] == 2
    eng.forget(rig.enc, idx["p_s"], node)
    rig.ref.remove(rig.sc.pending[idx["p_s"]], "n010")
    np.testing.assert_array_equal(eng.volume_attached(), before)
    # p_s2 is a second holder of disk s on n000 (b0 has it): the disk stays attached both ways
    node = rig.pos["n000"]
    eng.assume(rig.enc, idx["p_s2"], node)
    np.testing.assert_array_equal(eng.volume_attached(), before)
    assert (eng.class_count() != counts).sum() == 1
    eng.forget(rig.enc, idx["p_s2"], node)
    np.testing.assert_array_equal(eng.volume_attached(), before)
    np.testing.assert_array_equal(eng.class_count(), counts)
    # the first holder leaves while the second stays: still attached; then the second: gone
    node = rig.pos["n020"]
    eng.assume(rig.enc, idx["p_s"], node)
    eng.assume(rig.enc, idx["p_s2"], node)
    eng.forget(rig.enc, idx["p_s"], node)
    assert eng.volume_attached()[0, node] == 1
    eng.forget(rig.enc, idx["p_s2"], node)
    np.testing.assert_array_equal(eng.volume_attached(), before)
    eng.assume(rig.enc, idx["p_hs"], node)
    eng.reset_cluster()
    np.testing.assert_array_equal(eng.volume_attached(), rig.vl.attached)
    np.testing.assert_array_equal(eng.class_count(), counts)


def _finish_cycle(rig, eng, ora, plain, i, e):
    """Score the feasible nodes on both sides and assume the pod on the best one."""
    feas = np.flatnonzero(e["fail_plugin"] == abi.PASSED).astype(np.int32)
    assert feas.size > 1                      # a single feasible node is not scored
    es, os_ = eng.fw_score(feas), ora.fw_score(feas)
    for k in ("raw", "norm", "total"):
        np.testing.assert_array_equal(es[k][..., feas], os_[k][..., feas], err_msg=f"pod {i} {k}")
    node = int(feas[np.argmax(es["total"][feas])])
    eng.assume(rig.enc, i, node)
    ora.assume(plain, i, node)
    rig.ref.place(rig.sc.pending[i], rig.names[node])
    np.testing.assert_array_equal(eng.volume_attached(), rig.recount())


def test_framework_prefilter_and_score():
    """ksim_fw_prefilter answers every node with the composed codes and
    ksim_fw_score scores the feasible ones as the oracle scores the stripped
    pod (volume pods go through the device Score path)."""
    rig = Rig(BY_NAME["shared_three_65"])
    eng = rig.engine()
    plain = strip_volume_uses(rig.enc)
    ora = Oracle(own_tables(rig.cluster), rig.prof)
    idx = {p.name: i for i, p in enumerate(rig.sc.pending)}
    differs = []
    for name in ("p_s", "p_hs", "p_plain", "p_s2"):
        i, pod = idx[name], rig.sc.pending[idx[name]]
        e, o = eng.fw_prefilter(rig.enc, i), ora.fw_prefilter(plain, i)
        want_fail, want_detail = rig.expected_codes(pod, o["fail_plugin"], o["fail_detail"])
        np.testing.assert_array_equal(e["fail_plugin"], want_fail, err_msg=name)
        np.testing.assert_array_equal(e["fail_detail"], want_detail, err_msg=name)
        differs.append(bool((want_fail != o["fail_plugin"]).any()))
        _finish_cycle(rig, eng, ora, plain, i, e)
    assert differs[:3] == [True, True, False]
    es, os_ = eng.node_state(), ora.node_state()
    for k in es:
        np.testing.assert_array_equal(es[k], os_[k], err_msg=k)


def test_framework_nominated_pass_leaves_the_table():
    """ksim_fw_filter_nominated assumes the nominated pods, filters the cycle's
    pod and forgets them: p_c fits n0 alone (1 + 1 <= 2), next to the
    nominated second holder of disk a as well, not next to nominated p_b."""
    sc = cases.unbind_holders()
    for k in (1, 2):                                            # more than one feasible node, so the cycle scores
        sc.node(f"n{k}", {cases.EBS_KEY: "2"})
    rig = Rig(sc)
    eng = rig.engine()
    plain = strip_volume_uses(rig.enc)
    ora = Oracle(own_tables(rig.cluster), rig.prof)
    idx = {p.name: i for i, p in enumerate(rig.sc.pending)}
    i, n0 = idx["p_c"], rig.pos["n0"]
    before, counts = eng.volume_attached(), eng.class_count()
    e, o = eng.fw_prefilter(rig.enc, i), ora.fw_prefilter(plain, i)
    assert list(e["fail_plugin"]) == [abi.PASSED] * 3 == list(o["fail_plugin"])
    q = rig.order.index("EBSLimits")
    for members, want in (([idx["p_b"]], q), ([idx["p_a"]], abi.PASSED), ([idx["p_a"], idx["p_b"]], q)):
        fp, fd = eng.fw_filter_nominated(rig.enc, [(n0, members)])
        ofp, _ = ora.fw_filter_nominated(plain, [(n0, members)])
        assert (int(fp[0]), int(fd[0]), int(ofp[0])) == (want, 0, abi.PASSED), members
    fp, _ = eng.fw_filter_nominated(rig.enc, [(n0, [idx["p_b"]]), (rig.pos["n1"], [idx["p_a"]])])
    assert list(fp) == [q, abi.PASSED]                          # n0: 2 + 1 > 2; n1 held nothing: 1 + 1 <= 2
    _finish_cycle(rig, eng, ora, plain, i, e)
    after = rig.recount()
    assert after.sum() == before.sum() + 1                      # p_c's own disk, nothing of the nominated pods
    np.testing.assert_array_equal(eng.volume_attached(), after)
    np.testing.assert_array_equal(eng.class_count(), counts)


# ---- ingest ---------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "vollimits", "import_volumes.json")


def test_ingest_schedules_volume_pods_within_the_limits():
    with open(GOLDEN) as f:
        snap = ingest.load(json.load(f))
    # unchanged: the inline-disk pod and the pod with an unbound delay-binding EBS-class claim
    assert sorted(n for _, n, _ in snap.unsupported) == ["inline-disk", "wait-ebs"]
    pending = [p.name for p in snap.pending]
    assert {"ebs-0", "ebs-1", "ebs-2", "ebs-shared", "csi-0", "csi-1", "plain"} == set(pending)
    cluster, pods, prof = ingest.encode(snap)
    assert not (pods.pods["flags"] & abi.POD_HAS_VOLUMES).any()
    eng = Engine(0)
    eng.set_profile(prof)
    eng.set_cluster(cluster)
    chosen, st = eng.schedule_batch(pods)
    placed = {name: (cluster.node_names[c] if c >= 0 else None) for name, c in zip(pending, chosen)}
    # node-a takes one EBS disk (allocatable 1) and already holds vol-shared; node-b takes two;
    # the CSI driver allows one volume on node-a and none on node-b
    ref = VolLimitRef(snap.nodes, snap.volumes.pvs.values(), snap.volumes.pvcs.values())
    for b in snap.bound:
        ref.place(b, b.node_name)
    for p in snap.pending:                                      # queue order: each placement passed at its turn
        node = placed[p.name]
        if node is None:
            assert all(ref.verdicts(p).values()), p.name
        else:
            assert not ref.failing(p, node), (p.name, node)
            ref.place(p, node)
    assert placed["plain"] is not None and placed["ebs-shared"] is not None
    assert sorted(placed[n] for n in ("ebs-0", "ebs-1", "ebs-2") if placed[n]) == ["node-b", "node-b"]
    assert sum(placed[n] is None for n in ("ebs-0", "ebs-1", "ebs-2")) == 1
    assert sorted(str(placed[n]) for n in ("csi-0", "csi-1")) == ["None", "node-a"]
    vl = cluster.vol_limits
    np.testing.assert_array_equal(eng.volume_attached(),
                                  [[ref.attached(k, n) for n in cluster.node_names] for k in vl.families])
    assert (eng.volume_attached() <= vl.limit).all()


# ---- refusals ---------------------------------------------------------------------------------
def _refused(code, text, call, *args, **kw):
    with pytest.raises(KsimError) as e:
        call(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals_name_their_cause():
    rig = Rig(BY_NAME["over_limit"])
    E_INVALID, E_UNSUPPORTED = -1, -5
    # a volume use without a table
    bare = own_tables(rig.cluster)
    bare.vol_limits = None
    eng = Engine(0)
    eng.set_profile(rig.prof)
    eng.set_cluster(bare)
    _refused(E_INVALID, "volume use without a volume table", eng.eval_pod, rig.enc, 0)
    _refused(E_INVALID, "volume use without a volume table", eng.load_pods, rig.enc)
    _refused(E_INVALID, "no volume table", eng.volume_attached)
    # a family index >= n_families
    eng = rig.engine()
    bad = dataclasses.replace(rig.enc, uses=rig.enc.uses.copy())
    bad.uses["col"][bad.uses["kind"] == abi.USE_VOLUME] = len(rig.vl.families)
    _refused(E_INVALID, "volume use family out of range", eng.eval_pod, bad, 0)
    _refused(E_INVALID, "n_families out of range", eng.set_volume_limits, [abi.PL_EBS_LIMITS] * 9,
             np.zeros((9, eng.n_nodes)), np.zeros((9, eng.n_nodes)))
    _refused(E_INVALID, "not a volume limit plugin", eng.set_volume_limits, [abi.PL_NODE_PORTS],
             np.zeros((1, eng.n_nodes)), np.zeros((1, eng.n_nodes)))
    # the three preemption dry runs for a preemptor with a volume use
    eng = rig.engine()
    _refused(E_UNSUPPORTED, "KSIM_USE_VOLUME", eng.preempt, rig.enc, 0, 10)
    _refused(E_UNSUPPORTED, "KSIM_USE_VOLUME", eng.preempt, rig.enc, 0, 10, groups=[(0, [1])])
    _refused(E_UNSUPPORTED, "KSIM_USE_VOLUME", eng.preempt, rig.enc, 0, 10, hard_spread=True)
    # the packed sweep takes one run of FAST batches only: a queue with volume pods is none
    p100 = Rig(BY_NAME["over_limit"], DEFAULT_ORDER, 100)
    sw = p100.engine()
    sw.load_pods(p100.enc)
    _refused(E_UNSUPPORTED, "packed sweep", sw.sweep_loaded, [p100.prof, p100.prof])
    # node deltas while a table is set
    c = own_tables(rig.cluster)
    _refused(E_UNSUPPORTED, "ksim_upsert_nodes while a volume table is set", eng.upsert_nodes, c,
             np.arange(c.n_nodes, dtype=np.int32))
    _refused(E_UNSUPPORTED, "ksim_update_node_rows while a volume table is set", eng.update_node_rows, c, [0])
    _refused(E_UNSUPPORTED, "ksim_remove_node while a volume table is set", eng.remove_node, 0)
    # replicated and shard handles
    _refused(E_UNSUPPORTED, "cannot be replicated", eng.set_eval_range, 0, eng.n_nodes)
    sh = Engine(0)
    sh.set_profile(rig.prof)
    sh.set_shard(0, rig.cluster.n_nodes)
    _refused(E_UNSUPPORTED, "shard or replicated handle", sh.set_cluster, own_tables(rig.cluster))
    rep = Engine(0)
    rep.set_profile(rig.prof)
    rep.set_cluster(bare)
    rep.set_eval_range(0, rep.n_nodes)
    _refused(E_UNSUPPORTED, "shard or replicated handle", rep.set_volume_limits, rig.vl.family_plugin, rig.vl.limit,
             rig.vl.attached)
    # a new snapshot drops the table
    eng.set_cluster(bare)
    _refused(E_INVALID, "volume use without a volume table", eng.eval_pod, rig.enc, 0)
    assert eng.L.ksim_abi_version() == 12
