"""Who owns the handle's memory (csrc/ksim_mem.h; ksim_host.h BoundPods,
LazyBufs, AshBufs): nothing is lost when a handle is destroyed, when a cluster
replaces another on the same handle, or when a list of the bound-pod table is
set again, and nothing dropped on the way is still read.

Free device memory is ``torch.cuda.mem_get_info`` after a device synchronize.
torch finds the device only when it is loaded before the engine library (the
library then binds to the HIP runtime torch brought; bench.py does the same),
so each case runs in a fresh child process that loads torch first.  What a
cycle computes (placements, the dry runs' answers, node state) is
compared with the first cycle's, so a buffer dropped too early or reused
wrongly shows as a wrong answer.

One cycle (``_use``) touches every allocation family of a handle once:
profile; clusters of n nodes (n = 64, 96) with a loaded queue, with and
without volume limits; a deferred-commit run that takes the request-class
table; a P100 three-launch run on the static-class table; a two-lane packed
sweep; a topology-batch run; an ADAPT run; one framework cycle (PreFilter,
Score, NormalizeScore on the device, Reserve); the extender round trip; bound
pods with adds, budgets and volumes; a single dry run, preempt_many,
preempt_many_dom, preempt_commit; match_terms.  ADAPT keeps fewer than all
nodes only on clusters of more than 100 nodes (numFeasibleNodesToFind's floor),
so that one run takes 128 nodes.

The permitted fall of free memory in each comparison is the largest fall the
parent commit's library showed in it (profiles/handle_memory/README.md holds
both libraries' readings): the runtime's own allocation granularity, nothing
else.  Every reading is printed before it is compared."""
import functools
import multiprocessing as mp
import traceback

import numpy as np
import pytest

import fastcases
import matchcases
import preemptcommitcases as cc
import runfeedcases as rf
import tbatchcases as tbc
from ksim import abi, profile
from ksim.encode import encode_cluster, encode_pods
from ksim.engine import Engine
from preemptfullcases import EBS_KEY, HOST, X, ZONE, anti, hard, sched_profile

pytestmark = pytest.mark.gpu

SIZES = (64, 96)
ADAPT_NODES = 128
# The largest fall (bytes) of free memory the parent's library showed in each
# comparison; profiles/handle_memory/README.md.
MARGIN_CYCLES = 0
MARGIN_REPLACE = 0
MARGIN_LISTS = 0


def _free() -> int:
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


# ---- the scenes, compiled once ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _profiles():
    base = profile.SchedulerProfile(percentage_of_nodes_to_score=100)
    other = base.with_weights({"NodeResourcesFit": 2, "NodeResourcesBalancedAllocation": 1})
    return (profile.compile_profile(base), profile.compile_profile(other),
            profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=0)))


@functools.lru_cache(maxsize=None)
def _queues(n: int):
    """(cluster, pods) per run kind on n nodes."""
    table = rf.narrow_cluster(n), rf.queue(300)                          # 4 request classes: the table
    stab = rf.narrow_cluster(n), fastcases.with_zone_selector(rf.queue(300))
    tb_cluster, _ = encode_cluster(tbc.zoned(n, cpu="64", mem="256Gi"), [])
    tb = tb_cluster, encode_pods(tb_cluster, tbc.many_apps(tbc.K_TB_PODS + 8))
    adapt = rf.narrow_cluster(ADAPT_NODES, 110), rf.queue(300, tag=3)
    return {"table": table, "stab": stab, "tbatch": tb, "adapt": adapt}


@functools.lru_cache(maxsize=None)
def _bound(n: int) -> cc.Built:
    """n zoned 2-CPU nodes at EBS limit 3, two 900m bound pods on each (every
    fourth holding a volume, every third app=x, some under a budget), and four
    pending pods: requests alone, hostname anti-affinity, DoNotSchedule spread
    over the zone (domain rows), a new EBS volume."""
    from ksim.model import LabelSelector, PodDisruptionBudget
    from ksim.preemption import bound_table
    from ksim.volumes import VolumeIndex
    s = cc.CommitScene(f"memory_{n}")
    for v in range(n):
        s.znode(f"n{v:03d}", f"z{v % 3}", {EBS_KEY: "3"}, cpu="2")
    for v in range(n):
        lab = dict(X) if v % 3 == 0 else ({"guard": "g"} if v % 5 == 1 else None)
        s.bp(f"a{v}", f"n{v:03d}", 1 + v % 7, [("ebs", f"v{v}")] if v % 4 == 0 else (), cpu="900m", labels=lab)
        s.bp(f"b{v}", f"n{v:03d}", 2 + v % 5, cpu="900m", start=100 + v % 9)
    s.pend("plain", cpu="1500m")
    s.pend("picky", cpu="1200m", terms=[anti(HOST)])
    s.pend("spread", cpu="1200m", labels=X, spread=[hard(ZONE, 2)])
    s.pend("newvol", cpu="1200m", vols=[("ebs", "x")])
    s.budgets = [PodDisruptionBudget("g", selector=LabelSelector({"guard": "g"}), disruptions_allowed=1)]
    index = VolumeIndex.from_nodes(s.nodes, s.pvs, s.pvcs)
    cluster, _ = encode_cluster(s.nodes, s.bound)
    vl = index.volume_limits(s.nodes, s.bound, s.pending)
    vl.pod_uses.update(vl.bound_uses)
    cluster.set_volume_limits(vl)
    enc = encode_pods(cluster, list(s.pending) + list(s.bound), volumes=index)
    table = bound_table(cluster, s.bound, s.start, cluster.topo, full_adds=True, pdbs=s.budgets, vol_limits=cluster.vol_limits)
    assert table.n == 2 * n and table.vol_off is not None and table.pdb_off is not None
    return cc.Built(s, cluster, enc, table, profile.compile_profile(sched_profile(s.filter_order, s.args)), len(s.pending),
                    {name: i for i, name in enumerate(cluster.node_names)})


@functools.lru_cache(maxsize=None)
def _match_problem():
    return matchcases.random_problem("memory", 7)


# ---- what a handle does -----------------------------------------------------------------------------------------
def _schedule(eng, cluster, pods, kernel: str) -> list:
    """set_cluster, load_pods, schedule_loaded; the run's placements and state,
    and (ksim_time_kernels runs what schedule_loaded runs) that it took the
    launch form ``kernel`` belongs to."""
    eng.set_cluster(cluster.copy_state())
    eng.load_pods(pods)
    chosen, st = eng.schedule_loaded(0, pods.n_pods)
    state = eng.node_state()
    eng.reset_cluster()
    ran = eng.time_kernels(0, pods.n_pods)
    assert kernel in ran, (kernel, sorted(ran))
    return [chosen.tolist(), (st.scheduled, st.unschedulable, st.evals), eng.next_start] + [state[k].tolist() for k in sorted(state)]


def _dry_runs(eng, b) -> list:
    idx = list(range(b.n_pending))
    prio = [p.priority for p in b.sc.pending]
    single = [eng.preempt(b.enc, i, q, full=True, with_pdb=True) for i, q in zip(idx, prio)]
    many = eng.preempt_many(b.enc, idx, prio, with_pdb=True)
    dom = eng.preempt_many(b.enc, idx, prio, with_pdb=True, domains=True)
    assert single == many == dom
    return dom


def _preemption(eng, b) -> list:
    """The bound table with its three lists, the dry runs, one commit of the
    plain pod's victims, the dry runs again."""
    eng.set_profile(b.prof)
    eng.set_cluster(b.cluster)
    eng.set_bound_pods(b.table)
    before = _dry_runs(eng, b)
    assert before[0][0] >= 0 and before[0][1]                           # the plain pod evicts somebody
    rows = before[0][1]
    eng.preempt_commit(b.enc, rows, [b.record(r) for r in rows])
    after = _dry_runs(eng, b)
    assert after != before
    return [before, after, eng.node_state()["num_pods"].tolist(), eng.volume_attached().tolist()]


def _framework_cycle(eng, pods) -> list:
    fe = eng.fw_prefilter(pods, 0)
    feas = np.nonzero(fe["fail_plugin"] == abi.PASSED)[0]
    se = eng.fw_score(feas)
    bent = se["raw"][0][feas].copy()
    bent[-1] += 7                                                        # not the scored list's scores: the device path
    norm = eng.fw_normalize(0, feas, bent)
    eng.assume(pods, 0, int(feas[0]))
    ext = eng.eval_pod_extenders(pods, 1, lambda r: (None, np.arange(r["fail_plugin"].size, dtype=np.int64) % 7))
    return [feas.tolist(), se["total"].tolist(), norm.tolist(), ext["chosen"], ext["total"].tolist()]


def _use(eng, n: int) -> list:
    p100, weights, adapt = _profiles()
    q = _queues(n)
    out = []
    eng.set_profile(p100)
    r0 = eng.diag()["reqtab_runs"]
    out.append(_schedule(eng, *q["table"], "k_batch_top_commit"))
    assert eng.diag()["reqtab_runs"] > r0
    rows, _ = eng.sweep_loaded([p100, weights], max_lanes=2)
    out.append(rows.tolist())
    out.append(_framework_cycle(eng, q["table"][1]))
    out.append(_schedule(eng, *q["stab"], "k_batch_top"))
    out.append(_schedule(eng, *q["tbatch"], "k_tb_filter"))
    eng.set_profile(adapt)
    out.append(_schedule(eng, *q["adapt"], "k_adapt_top"))
    out.append(_preemption(eng, _bound(n)))
    mp = _match_problem()
    counts = np.zeros((mp.n_classes, mp.n_nodes), np.int32)
    out.append([eng.match_terms(mp.struct(), mp.n_words, counts).tolist(), counts.tolist()])
    return out


# ---- the cases (each in a child process: torch first) ------------------------------------------------------------
def _create_use_destroy() -> list:
    want, free = None, []
    for cycle in range(4):
        got = []
        for n in SIZES:
            eng = Engine(0)
            try:
                got.append(_use(eng, n))
            finally:
                eng.close()
        free.append(_free())
        print(f"create/use/destroy cycle {cycle + 1}: free {free[-1]}", flush=True)
        want = got if want is None else want
        assert got == want, f"cycle {cycle + 1} computed something else"
    return [[free[0] - f for f in free[1:]]]


def _round(eng, n: int) -> list:
    b = _bound(n)
    out = _preemption(eng, b)
    eng.set_profile(_profiles()[0])
    eng.load_pods(rf.queue(300))
    chosen, _ = eng.schedule_loaded(0, 300)
    return out + [chosen.tolist()]


def _replace_in_place() -> list:
    eng = Engine(0)
    try:
        want, free = {}, []
        for r in range(6):
            n = SIZES[r % 2]
            got = _round(eng, n)
            free.append(_free())
            print(f"replace round {r + 1} ({n} nodes): free {free[-1]}", flush=True)
            assert got == want.setdefault(n, got), f"round {r + 1} computed something else"
        return [[free[1] - f for f in free[2:]]]
    finally:
        eng.close()


def _each_list_set_again() -> list:
    b = _bound(SIZES[1])
    t = b.table
    eng = Engine(0)
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(b.table)                                     # the three lists, once
        want = _dry_runs(eng, b)
        setters = {"adds": lambda: eng.set_bound_pod_adds(t.adds_off, t.adds),
                   "budgets": lambda: eng.set_bound_pod_pdbs(t.pdb_allowed, t.pdb_off, t.pdb_ids),
                   "volumes": lambda: eng.set_bound_pod_volumes(t.vol_off, t.vol_uses)}
        falls = []
        for name, again in setters.items():
            again()                                                     # the second set
            free = [_free()]
            for _ in range(10):
                again()
                free.append(_free())
            falls.append([free[0] - f for f in free[1:]])
            print(f"{name} set again: free {free}", flush=True)
            assert _dry_runs(eng, b) == want, name
        return falls
    finally:
        eng.close()


CASES = {f.__name__: f for f in (_create_use_destroy, _replace_in_place, _each_list_set_again)}


def _child(case: str, conn) -> None:
    try:
        import torch
        torch.cuda.init()                          # before the engine library is loaded
        conn.send(("ok", CASES[case]()))
    except BaseException:                          # noqa: B902 (the parent reports it)
        conn.send(("failed", traceback.format_exc()))
    finally:
        conn.close()


def _falls(case: str) -> list:
    """The case in a child process; per comparison, how far free memory fell below its baseline."""
    ctx = mp.get_context("spawn")
    recv, send = ctx.Pipe(duplex=False)
    p = ctx.Process(target=_child, args=(case, send))
    p.start()
    send.close()                                   # the child's end alone is open: its death ends recv()
    try:
        status, payload = recv.recv()
    except EOFError:
        status, payload = "failed", "the child process ended without an answer"
    p.join(60)
    assert status == "ok", payload
    assert p.exitcode == 0
    print(f"{case} falls: {payload}")
    return payload


def test_create_use_destroy():
    """Free memory after cycles 2, 3 and 4 against cycle 1."""
    (falls,) = _falls("_create_use_destroy")
    assert max(falls) <= MARGIN_CYCLES, falls


def test_replace_in_place():
    """One handle, the 64-node and the 96-node cluster in turn six times: free
    memory after rounds 3 to 6 against round 2 (both sizes seen by then)."""
    (falls,) = _falls("_replace_in_place")
    assert max(falls) <= MARGIN_REPLACE, falls


def test_each_list_set_again():
    """Adds, budgets, volumes: each set ten more times after its second set."""
    for falls in _falls("_each_list_set_again"):
        assert max(falls) <= MARGIN_LISTS, falls
