"""ksim_preempt_many: many preemptors against one snapshot in a few launches
(csrc/ksim_preempt.hip: k_preempt_many_nodes, one thread per (node, row) on the
row's own result and flag slabs; k_preempt_pick, one block per row;
k_preempt_many_victims, one wave per row).

Every answer is compared with the CPU reference of tests/preemptmanycases.py
(checked on the CPU by tests/test_preempt_many_cases.py) and, on the same
handle, with a loop of Engine.preempt(..., full=True), the call the contract
names.  Every test also asserts that the node state, the class counts, the
attached counts and nextStartNodeIndex are what they were, and that the call
repeated gives the same answers (nothing is left behind in the slabs).

Shapes: 1 node; 255 / 256 / 257 nodes with the victim-bearing node at the block
edge; 1,025 and 2,049 nodes with the ``want`` cut inside a pick chunk; 0, 1, 2,
63, 64, 65 and 130 rows per call (three launch groups, the last partial); 63,
64 and 65 victims on the nominated node with every victims_cap that matters."""
import numpy as np
import pytest

import preemptmanycases as mc
from ksim import abi
from ksim.engine import Engine, KsimError

pytestmark = pytest.mark.gpu


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
            held[name] = _engine(mc.scenes()[name].build())
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
    """One batched call, that it left no trace, and that it repeats."""
    rows = s.rows if rows is None else rows
    b = s.build()
    idx, prio = [p for p, _ in rows], [q for _, q in rows]
    before = _state(eng)
    got = eng.preempt_many(b.enc, idx, prio, with_pdb=True, **kw)
    after = _state(eng)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    if "outs" not in kw:
        assert eng.preempt_many(b.enc, idx, prio, with_pdb=True) == got
    return got


def _loop(eng, s, rows=None):
    b = s.build()
    return [eng.preempt(b.enc, pod, prio, full=True, with_pdb=True) for pod, prio in (s.rows if rows is None else rows)]


# ---- every scene: the reference, the loop of single calls, the counters ---------------------------
@pytest.mark.parametrize("name", mc.scene_ids())
def test_equals_the_reference_and_the_loop_of_single_calls(engines, name):
    s = mc.scenes()[name]
    eng = engines(name)
    d0 = eng.diag()
    got = _many(eng, s)                                              # (two calls: the repeat)
    d1 = eng.diag()
    print(name, got[:4])
    assert got == s.reference()
    assert got == _loop(eng, s)
    assert _many(eng, s) == got                                      # after the single calls used the handle's own arrays
    forms = [s.form(pod) for pod, _ in s.rows]
    assert d1["preempt_many_rows"] - d0["preempt_many_rows"] == 2 * sum(f != 2 for f in forms)
    assert d1["preempt_many_single"] - d0["preempt_many_single"] == 2 * sum(f == 2 for f in forms)


def test_two_priorities_on_one_node_in_both_orders(engines):
    """The shared-flag race: rows of different priority whose candidate is the
    same node with different victims, the low row before and after the high one."""
    s = mc.scenes()["race"]
    eng = engines("race")
    hi, lo = (0, 1000), (1, 35)
    want_hi, want_lo = s.answer(*hi).result, s.answer(*lo).result
    assert want_hi[0] == want_lo[0] == 2 and want_hi[1] != want_lo[1]
    assert _many(eng, s, [hi, lo]) == [want_hi, want_lo]
    assert _many(eng, s, [lo, hi]) == [want_lo, want_hi]
    assert _many(eng, s, [lo, hi, lo, lo, hi]) == [want_lo, want_hi, want_lo, want_lo, want_hi]
    nobody, everybody = (3, 10), (4, 2000)
    assert _many(eng, s, [nobody, everybody]) == [s.answer(*nobody).result, s.answer(*everybody).result]
    assert s.answer(*nobody).result[:2] == (-1, [])


def test_unsorted_indices_that_name_a_pod_twice(engines):
    s = mc.scenes()["race"]
    eng = engines("race")
    rows = [(4, 2000), (1, 35), (0, 1000), (1, 35), (2, 45), (0, 1000), (3, 10)]
    got = _many(eng, s, rows)
    assert got == [s.answer(*r).result for r in rows] == _loop(eng, s, rows)
    assert got[1] == got[3] and got[2] == got[5]


# ---- the victims step ---------------------------------------------------------------------------------
CANARY = -77


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("v", [63, 64, 65])
def test_victims_cap(engines, v, guarded):
    """victims_cap 0, 1, exact, one short and one more: n_victims is the true
    count, the list is the head of the full list (the violating victims first
    under the budget), and nothing is written at or past the cap."""
    name = f"victims_{v}" + ("_guarded" if guarded else "")
    s = mc.scenes()[name]
    eng = engines(name)
    b = s.build()
    full = s.answer(0, 1000).result
    assert full[0] == 0 and len(full[1]) == v and (full[4] > 0) == guarded
    caps = [0, 1, v, v - 1, v + 1, 64]
    outs = []
    for cap in caps:
        o = abi.PreemptOut(v + 8)
        o.victims[:] = CANARY
        o.c.victims_cap = cap
        outs.append(o)
    got = _many(eng, s, [(0, 1000)] * len(caps), outs=outs)
    for cap, o, g in zip(caps, outs, got):
        assert (o.c.nominated, o.c.n_victims, o.c.n_potential, o.c.n_candidates, o.c.n_pdb_violations) == \
            (full[0], v) + full[2:]
        k = min(cap, v)
        assert list(o.victims[:k]) == full[1][:k] and g[1] == full[1][:k]
        assert (o.victims[k:] == CANARY).all()
    # a row without a victims array at all
    o = abi.PreemptOut(1)
    o.c.victims, o.c.victims_cap = None, 5
    assert _many(eng, s, [(0, 1000)], outs=[o])[0][2:] == full[2:] and o.c.n_victims == v


# ---- every route in one call, budgets set and cleared ------------------------------------------------
def test_every_route_with_budgets_set_and_cleared():
    plain, guarded = mc.scenes()["mixed"], mc.scenes()["mixed_guarded"]
    b = guarded.build()
    eng = _engine(b)
    try:
        n_batched = sum(guarded.form(pod) != 2 for pod, _ in guarded.rows)
        for s in (guarded, plain, guarded):
            if s is plain:
                eng.set_bound_pod_pdbs([], [0], [])
            else:
                eng.set_bound_pod_pdbs(b.table.pdb_allowed, b.table.pdb_off, b.table.pdb_ids)
            d0 = eng.diag()
            got = _many(eng, s)
            d1 = eng.diag()
            assert got == s.reference() == _loop(eng, s)
            assert d1["preempt_many_rows"] - d0["preempt_many_rows"] == 2 * n_batched
            assert d1["preempt_many_single"] - d0["preempt_many_single"] == 2 * (len(s.rows) - n_batched)
        assert plain.reference() != guarded.reference()
    finally:
        eng.close()


# ---- refusals: host checks, before anything runs ---------------------------------------------------------
def _refused(eng, enc, idx, prio, code, *words, n=None, raw=None):
    """The call is refused with ``code``, the message carries ``words``, and no out was written."""
    outs = [abi.PreemptOut(4) for _ in idx]
    for o in outs:
        o.victims[:] = CANARY
        o.c.nominated, o.c.n_victims, o.c.n_potential, o.c.n_candidates, o.c.n_pdb_violations = (CANARY,) * 5
    with pytest.raises(KsimError) as e:
        if raw is not None:
            eng._chk(raw())
        else:
            eng.preempt_many(enc, idx, prio, outs=outs)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    for o in outs:
        assert (o.c.nominated, o.c.n_victims, o.c.n_potential, o.c.n_candidates, o.c.n_pdb_violations) == (CANARY,) * 5
        assert (o.victims == CANARY).all()


def test_refusals_write_no_row_and_a_valid_call_follows():
    import ctypes
    s = mc.scenes()["mixed"]
    b = s.build()
    eng = _engine(b)
    try:
        want = s.reference()
        idx, prio = [p for p, _ in s.rows], [q for _, q in s.rows]
        ps = b.enc.pod_set()
        i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        outs = (abi._PreemptOutC * 2)()
        L, h = eng.L, eng.h
        # invalid arguments
        _refused(eng, b.enc, [], [], abi.E_INVALID, raw=lambda: L.ksim_preempt_many(h, ctypes.byref(ps), -1, None, None, None))
        for args in ((None, i32([0]), i32([1]), outs), (ctypes.byref(ps), None, i32([1]), outs),
                     (ctypes.byref(ps), i32([0]), None, outs), (ctypes.byref(ps), i32([0]), i32([1]), None)):
            _refused(eng, b.enc, [], [], abi.E_INVALID, raw=lambda a=args: L.ksim_preempt_many(h, a[0], 1, *a[1:]))
        _refused(eng, b.enc, [0, 1, b.enc.n_pods], [1000] * 3, abi.E_INVALID, "row 2")
        _refused(eng, b.enc, [0, -1, 2], [1000] * 3, abi.E_INVALID, "row 1")
        assert eng.preempt_many(b.enc, [], []) == []
        assert _many(eng, s) == want                                   # a valid call right after
        # a PreFilterResult row
        flags = b.enc.pods["flags"].copy()
        b.enc.pods["flags"][2] |= abi.POD_NODE_NAMES
        try:
            _refused(eng, b.enc, [0, 1, 2], [1000] * 3, abi.E_UNSUPPORTED, "row 2", "PreFilterResult")
        finally:
            b.enc.pods["flags"][:] = flags
        assert _many(eng, s) == want
        # missing tables: the adds for a port row, the holdings for a volume row
        import preemptfullcases as fc
        sc = mc.mixed()
        for adds, holdings, row, call in ((False, True, 1, "ksim_set_bound_pod_adds"),
                                          (True, False, 2, "ksim_set_bound_pod_volumes")):
            eng.set_bound_pods(fc.build(sc, adds=adds, holdings=holdings).table)
            _refused(eng, b.enc, [0, 0, 1, 2], [1000] * 4, abi.E_INVALID, f"row {row + 1}", call)
            assert eng.preempt_many(b.enc, [0, 0], [1000, 9], with_pdb=True) == [s.answer(0, 1000).result,
                                                                                 s.answer(0, 9).result]
        eng.set_bound_pods(b.table)
        assert _many(eng, s) == want
    finally:
        eng.close()
    # no bound table at all; NetworkBandwidth in the filter list
    eng = Engine(0)
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        _refused(eng, b.enc, [0], [1000], abi.E_INVALID, "row 0", "ksim_set_bound_pods")
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
    s = mc.scenes()["race"]
    b = s.build()
    eng = Engine(0)
    try:
        eng.set_shard(0, b.cluster.n_nodes)
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(b.table)
        _refused(eng, b.enc, [0, 1], [1000, 35], abi.E_UNSUPPORTED, "row 0", "unsharded")
    finally:
        eng.close()
