"""ksim_preempt_many_dom: the batched dry run with the rows that read domain
tables batched too (csrc/ksim_preempt.hip: k_preempt_many_dom fills every such
row's own tables, totals and flag, k_preempt_many_mins its minima,
k_preempt_many_dom_nodes runs the row forms on the (node, row) grid).

Every answer is compared with the CPU reference of tests/preemptmanydomcases.py
(checked on the CPU by tests/test_preempt_many_dom_cases.py) and, on the same
handle, with a loop of Engine.preempt(..., full=True) and with the old call.
Every test also asserts that the node state, the class counts, the attached
counts and nextStartNodeIndex are what they were and that the call repeated
gives the same answers; the single dry runs and a per-pod cycle afterwards
show that the handle's own tables and flags were left alone.

Shapes: 1 node; 255 / 256 / 257 nodes with the deciding node at the block edge
(the full form); a hostname table of 255 / 256 / 257 / 300 values; a zone key
of 128 and 129 value ids (either side of the LDS staging); 1, 2, 63, 64, 65
and 130 domain rows per call."""
import ctypes

import numpy as np
import pytest

import preemptfullcases as fc
import preemptmanydomcases as dc
from ksim import abi
from ksim.engine import Engine, KsimError

pytestmark = pytest.mark.gpu
CANARY = -77


def _engine(b) -> Engine:
    eng = Engine(0)
    eng.set_profile(b.prof)
    eng.set_cluster(b.cluster)
    eng.set_bound_pods(b.table)
    return eng


@pytest.fixture(scope="module")
def engines():
    """One handle per scene, a few kept open."""
    held = {}

    def get(name):
        if name not in held:
            if len(held) >= 3:
                held.pop(next(iter(held))).close()
            held[name] = _engine(dc.scenes()[name].built())
        return held[name]

    yield get
    for e in held.values():
        e.close()


def _state(eng):
    st = eng.node_state()
    out = [st[k].copy() for k in sorted(st)] + [eng.class_count().copy(), np.array([eng.next_start])]
    if getattr(eng, "n_vol_families", 0):
        out.append(eng.volume_attached().copy())
    return out


def _many(eng, s, rows=None, **kw):
    """One call through ksim_preempt_many_dom, that it left no trace, and that it repeats."""
    rows = s.rows if rows is None else rows
    b = s.built()
    idx, prio = [p for p, _ in rows], [q for _, q in rows]
    before = _state(eng)
    got = eng.preempt_many(b.enc, idx, prio, with_pdb=True, domains=True, **kw)
    after = _state(eng)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    if "outs" not in kw:
        assert eng.preempt_many(b.enc, idx, prio, with_pdb=True, domains=True) == got
    return got


def _loop(eng, s, rows=None):
    b = s.built()
    return [eng.preempt(b.enc, pod, prio, full=True, with_pdb=True) for pod, prio in (s.rows if rows is None else rows)]


# ---- every scene: the reference, the loop of single calls, the old call, the counters ---------------
@pytest.mark.parametrize("name", dc.scene_ids())
def test_equals_the_reference_the_loop_and_the_old_call(engines, name):
    s = dc.scenes()[name]
    eng = engines(name)
    b = s.built()
    forms = [s.form(pod) for pod, _ in s.rows]
    n_dom = sum(f >= 2 for f in forms)
    d0 = eng.diag()
    got = _many(eng, s)                                              # (two calls: the repeat)
    d1 = eng.diag()
    print(name, got[:4])
    assert got == s.reference()
    assert d1["preempt_many_dom"] - d0["preempt_many_dom"] == 2 * n_dom
    assert d1["preempt_many_rows"] - d0["preempt_many_rows"] == 2 * (len(forms) - n_dom)
    assert d1["preempt_many_single"] == d0["preempt_many_single"]
    assert got == _loop(eng, s)                                      # the handle's own tables and flags still serve
    old = eng.preempt_many(b.enc, [p for p, _ in s.rows], [q for _, q in s.rows], with_pdb=True)
    d2 = eng.diag()
    assert old == got
    assert d2["preempt_many_single"] - d1["preempt_many_single"] == n_dom and d2["preempt_many_dom"] == d1["preempt_many_dom"]
    assert _many(eng, s) == got                                      # after the single calls used the handle's own arrays


@pytest.mark.parametrize("name", ["selectors_differ", "honor_beside_ignore", "affinity_only_here"])
def test_a_per_pod_cycle_afterwards_sees_the_handles_own_tables_untouched(name):
    s = dc.scenes()[name]
    b = s.built()
    eng, fresh = _engine(b), _engine(b)
    try:
        assert _many(eng, s) == s.reference()
        for pod in sorted({p for p, _ in s.rows}):
            got, clean = eng.eval_pod(b.enc, pod), fresh.eval_pod(b.enc, pod)
            assert got["status"] == clean["status"] and got["chosen"] == clean["chosen"]
            for k in ("fail_plugin", "fail_detail"):
                assert np.array_equal(got[k], clean[k]), (pod, k)
            if got["chosen"] >= 0:                                   # the cycle bound its pod on both handles
                break
    finally:
        eng.close()
        fresh.close()


def test_two_priorities_on_one_node_in_both_orders(engines):
    """Rows of different priority whose candidate is the same node with
    different victims, the low row before and after the high one."""
    s = dc.scenes()["two_priorities"]
    eng = engines("two_priorities")
    hi, lo = (0, 1000), (1, 15)
    want_hi, want_lo = s.answer(*hi), s.answer(*lo)
    assert want_hi[0] == want_lo[0] >= 0 and want_hi[1] == [0, 1] and want_lo[1] == [1]
    assert _many(eng, s, [hi, lo]) == [want_hi, want_lo]
    assert _many(eng, s, [lo, hi]) == [want_lo, want_hi]
    assert _many(eng, s, [lo, hi, lo, lo, hi]) == [want_lo, want_hi, want_lo, want_lo, want_hi]
    nobody = (0, 15)
    assert _many(eng, s, [nobody, hi]) == [s.answer(*nobody), want_hi] and s.answer(*nobody)[:2] == (-1, [])


def test_unsorted_indices_that_name_a_pod_twice(engines):
    s = dc.scenes()["routes"]
    eng = engines("routes")
    rows = [(10, 1000), (9, 25), (0, 1000), (8, 1000), (10, 1000), (11, 9), (2, 25), (8, 1000), (9, 25), (3, 1000)]
    got = _many(eng, s, rows)
    assert got == [s.answer(*r) for r in rows] == _loop(eng, s, rows)
    assert got[0] == got[4] and got[3] == got[7] and got[1] == got[8]


# ---- the victims step on a domain row -----------------------------------------------------------------
def test_victims_cap_on_a_domain_row(engines):
    """victims_cap 0, one short, exact and one more: n_victims is the true
    count, the list is the head of the full list, nothing is written at or
    past the cap."""
    s = dc.scenes()["host_spread_300"]
    eng = engines("host_spread_300")
    full = s.answer(0, 1000)
    assert full[0] == 299 and full[1] == [300, 301]
    caps = [0, 1, 2, 3]
    outs = []
    for cap in caps:
        o = abi.PreemptOut(8)
        o.victims[:] = CANARY
        o.c.victims_cap = cap
        outs.append(o)
    got = _many(eng, s, [(0, 1000)] * len(caps), outs=outs)
    for cap, o, g in zip(caps, outs, got):
        assert (o.c.nominated, o.c.n_victims, o.c.n_potential, o.c.n_candidates, o.c.n_pdb_violations) == \
            (full[0], 2) + full[2:]
        k = min(cap, 2)
        assert list(o.victims[:k]) == full[1][:k] and g[1] == full[1][:k]
        assert (o.victims[k:] == CANARY).all()
    o = abi.PreemptOut(1)                                            # a row without a victims array at all
    o.c.victims, o.c.victims_cap = None, 5
    assert _many(eng, s, [(0, 1000)], outs=[o])[0][2:] == full[2:] and o.c.n_victims == 2


# ---- every route in one call, budgets set, cleared and set again ---------------------------------------
def test_every_route_with_budgets_set_and_cleared():
    plain, guarded = dc.scenes()["routes"], dc.scenes()["routes_guarded"]
    b = guarded.built()
    eng = _engine(b)
    try:
        n_dom = sum(guarded.form(pod) >= 2 for pod, _ in guarded.rows)
        for s in (guarded, plain, guarded):
            if s is plain:
                eng.set_bound_pod_pdbs([], [0], [])
            else:
                eng.set_bound_pod_pdbs(b.table.pdb_allowed, b.table.pdb_off, b.table.pdb_ids)
            d0 = eng.diag()
            got = _many(eng, s)
            d1 = eng.diag()
            assert got == s.reference() == _loop(eng, s)
            assert d1["preempt_many_dom"] - d0["preempt_many_dom"] == 2 * n_dom
            assert d1["preempt_many_rows"] - d0["preempt_many_rows"] == 2 * (len(s.rows) - n_dom)
            assert d1["preempt_many_single"] == d0["preempt_many_single"]
        assert plain.reference() != guarded.reference()
    finally:
        eng.close()


# ---- refusals: host checks, before anything runs ---------------------------------------------------------
def _refused(eng, enc, idx, prio, code, *words, raw=None):
    """The call is refused with ``code``, the message carries ``words``, and no out was written."""
    outs = [abi.PreemptOut(4) for _ in idx]
    for o in outs:
        o.victims[:] = CANARY
        o.c.nominated, o.c.n_victims, o.c.n_potential, o.c.n_candidates, o.c.n_pdb_violations = (CANARY,) * 5
    with pytest.raises(KsimError) as e:
        if raw is not None:
            eng._chk(raw())
        else:
            eng.preempt_many(enc, idx, prio, outs=outs, domains=True)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    for o in outs:
        assert (o.c.nominated, o.c.n_victims, o.c.n_potential, o.c.n_candidates, o.c.n_pdb_violations) == (CANARY,) * 5
        assert (o.victims == CANARY).all()


def test_refusals_write_no_row_and_a_valid_call_follows():
    s = dc.scenes()["routes"]
    b = s.built()
    eng = _engine(b)
    try:
        want = s.reference()
        ps = b.enc.pod_set()
        i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        outs = (abi._PreemptOutC * 2)()
        L, h = eng.L, eng.h
        _refused(eng, b.enc, [], [], abi.E_INVALID, raw=lambda: L.ksim_preempt_many_dom(h, ctypes.byref(ps), -1, None, None, None))
        for args in ((None, i32([0]), i32([1]), outs), (ctypes.byref(ps), None, i32([1]), outs),
                     (ctypes.byref(ps), i32([0]), None, outs), (ctypes.byref(ps), i32([0]), i32([1]), None)):
            _refused(eng, b.enc, [], [], abi.E_INVALID, raw=lambda a=args: L.ksim_preempt_many_dom(h, a[0], 1, *a[1:]))
        _refused(eng, b.enc, [8, 9, b.enc.n_pods], [1000] * 3, abi.E_INVALID, "ksim_preempt_many_dom row 2")
        _refused(eng, b.enc, [8, -1, 10], [1000] * 3, abi.E_INVALID, "row 1")
        assert eng.preempt_many(b.enc, [], [], domains=True) == []
        assert _many(eng, s) == want                                   # a valid call right after
        # a PreFilterResult row among domain rows
        flags = b.enc.pods["flags"].copy()
        b.enc.pods["flags"][9] |= abi.POD_NODE_NAMES
        try:
            _refused(eng, b.enc, [8, 10, 9], [1000] * 3, abi.E_UNSUPPORTED, "row 2", "PreFilterResult")
        finally:
            b.enc.pods["flags"][:] = flags
        assert _many(eng, s) == want
        # missing tables: the class adds for a port row and for a domain row, the holdings for a volume row
        for adds, holdings, idx, row, call in ((False, True, [0, 0, 1, 8], 2, "ksim_set_bound_pod_adds"),
                                               (False, True, [0, 0, 8, 1], 2, "ksim_set_bound_pod_adds"),
                                               (False, True, [0, 9, 8], 1, "ksim_set_bound_pod_adds"),
                                               (True, False, [0, 8, 10, 2], 2, "ksim_set_bound_pod_volumes")):
            eng.set_bound_pods(fc.build(s.sc, adds=adds, holdings=holdings).table)
            _refused(eng, b.enc, idx, [1000] * len(idx), abi.E_INVALID, f"row {row}", call)
            assert eng.preempt_many(b.enc, [0, 0], [1000, 9], with_pdb=True, domains=True) == [s.answer(0, 1000),
                                                                                               s.answer(0, 9)]
        eng.set_bound_pods(b.table)
        assert _many(eng, s) == want
    finally:
        eng.close()
    eng = Engine(0)                                                    # no bound table at all
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        _refused(eng, b.enc, [8], [1000], abi.E_INVALID, "row 0", "ksim_set_bound_pods")
    finally:
        eng.close()


def test_network_bandwidth_profiles_and_shard_handles_are_refused():
    import test_netbw
    from ksim import gen, profile
    from ksim.encode import encode_cluster, encode_pods
    nodes, bound, pending = gen.netbw_objects(n_nodes=20, n_pods=4, node_errors=False, pod_errors=False)
    sp = test_netbw.nb_profile(100, filt=True, score=False)
    cluster, _ = encode_cluster(nodes, bound, nb_args=sp.network_bandwidth)
    enc = encode_pods(cluster, pending)
    eng = Engine(0)
    try:
        eng.set_profile(profile.compile_profile(sp))
        eng.set_cluster(cluster)
        eng.set_bound_pods(abi.BoundPods([0], [1], [100], np.zeros((1, abi.PREEMPT_REQ), np.int64)))
        _refused(eng, enc, [0, 1], [1000, 35], abi.E_UNSUPPORTED, "row 0", "NetworkBandwidth")
    finally:
        eng.close()
    s = dc.scenes()["selectors_differ"]
    b = s.built()
    eng = Engine(0)
    try:
        eng.set_shard(0, b.cluster.n_nodes)
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(b.table)
        _refused(eng, b.enc, [0, 1], [1000, 35], abi.E_UNSUPPORTED, "row 0", "unsharded")
    finally:
        eng.close()
