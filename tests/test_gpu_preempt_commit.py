"""ksim_preempt_commit on the device (csrc/ksim_preempt.hip: k_commit_evict, one
wave per victim; k_commit_sums / k_commit_carry / k_commit_scatter, the stable
compaction of the bound table and the lists on its rows over tiles of
ksim.preemption.COMMIT_TILE positions; k_commit_off).

The reference is the rebuild form on a second engine with the same cluster,
profile and pods: ``forget`` of every victim, ``ksim.preemption.bound_table``
over the survivors, ``set_bound_pods`` with its three setters.  After every
commit the node state, the class counts, the attached volumes and nb_alloc are
equal word for word, the state's change is the model's
(tests/preemptcommitcases.py), and every pending pod of the scene gets the same
answer from ``preempt_many`` (both forms) and from the full single entry, the
reference's victims mapped through the survivor map.  The plain scene is also
compared with the CPU oracle's rebuild form.

Shapes: 1, 63, 64 and 65 rows; one scan tile less two, less one, exactly and
plus one row (positions 0 .. n are scanned, so n = tile - 1 fills a tile), two
tiles; victims at the table's first and last rows, a node emptied between two
others, the whole table, empty nodes around the victims' nodes, several nodes
in one call, two commits in a row."""
import ctypes

import numpy as np
import pytest

import preemptcommitcases as cc
from ksim import abi
from ksim.engine import Engine, KsimError
from ksim.preemption import commit_args

pytestmark = pytest.mark.gpu


def _engine(b, table=None) -> Engine:
    eng = Engine(0)
    eng.set_profile(b.prof)
    eng.set_cluster(b.cluster)
    eng.set_bound_pods(b.table if table is None else table)
    return eng


def _state(eng) -> dict:
    out = {k: v.copy() for k, v in eng.node_state().items()}
    out["class_count"] = eng.class_count().copy()
    out["nb_alloc"] = eng.nb_alloc().copy()
    out["next_start"] = np.array([eng.next_start])
    nf = getattr(eng, "n_vol_families", 0)                             # (the getter needs a volume table)
    out["attached"] = eng.volume_attached().copy() if nf else np.zeros((0, eng.n_nodes), np.int32)
    return out


def _same(x: dict, y: dict) -> None:
    assert sorted(x) == sorted(y)
    for k in x:
        np.testing.assert_array_equal(x[k], y[k], err_msg=k)


def _answers(eng, b, alive=None, single=True) -> list:
    """Every pending pod's dry run: the batched call (which must agree with its
    domain form and with the full single entry).  ``alive``: the survivor map
    of a rebuilt table (its row k is the scene's row alive[k])."""
    idx = list(range(b.n_pending))
    prio = [p.priority for p in b.sc.pending]
    got = eng.preempt_many(b.enc, idx, prio, with_pdb=True)
    assert eng.preempt_many(b.enc, idx, prio, with_pdb=True, domains=True) == got
    if single:
        assert [eng.preempt(b.enc, i, q, full=True, with_pdb=True) for i, q in zip(idx, prio)] == got
    if alive is not None:
        got = [(g[0], [alive[v] for v in g[1]]) + tuple(g[2:]) for g in got]
    return got


def _model_delta(m0: dict, m1: dict, s0: dict, s1: dict, n_nodes: int) -> None:
    """The state moved as the model's snapshot did."""
    for v in range(n_nodes):
        a, z = m0["node"][v], m1["node"][v]
        for col, key in (("req_cpu", "cpu"), ("nz_cpu", "nz_cpu"), ("nz_mem", "nz_mem"), ("num_pods", "num_pods")):
            assert int(s0[col][v]) - int(s1[col][v]) == a[key] - z[key], (col, v)
        assert int(s0["nb_alloc"][v]) - int(s1["nb_alloc"][v]) == a["nb"] - z["nb"]
    moved = {k: m0["cnt"].get(k, 0) - m1["cnt"].get(k, 0) for k in set(m0["cnt"]) | set(m1["cnt"])}
    d = s0["class_count"].astype(np.int64) - s1["class_count"]
    for c, v in zip(*np.nonzero(d)):
        assert moved.get((int(c), int(v)), 0) == d[c, v], ("class", c, v)
    assert all(d[c, v] == x for (c, v), x in moved.items())
    moved = {k: m0["att"].get(k, 0) - m1["att"].get(k, 0) for k in set(m0["att"]) | set(m1["att"])}
    d = s0["attached"].astype(np.int64) - s1["attached"]
    assert {(int(f), int(v)): int(d[f, v]) for f, v in zip(*np.nonzero(d))} == {k: x for k, x in moved.items() if x}


def _commit_and_rebuild(eng, ref, b, rows, alive):
    """One commit on ``eng`` and its rebuild form on ``ref``; the survivors."""
    eng.preempt_commit(b.enc, rows, [b.record(r) for r in rows])
    for r in rows:
        ref.forget(b.enc, b.record(r), int(b.table.node[r]))
    alive = [i for i in alive if i not in set(rows)]
    ref.set_bound_pods(cc.survivors_table(b, alive))
    return alive


# ---- every scene against the rebuild form and the model -----------------------------------------------------
@pytest.mark.parametrize("name", cc.scene_ids())
def test_equals_the_rebuild_form_and_the_model(name):
    b = cc.build(name)
    eng, ref = _engine(b), _engine(b)
    try:
        m = cc.model_of(b)
        alive = list(range(b.table.n))
        before = _answers(eng, b)
        assert before == _answers(ref, b)
        for step in b.sc.steps:
            rows = b.rows_of(step)
            s0, m0 = _state(eng), m.snapshot()
            alive = _commit_and_rebuild(eng, ref, b, rows, alive)
            m.commit(rows)
            s1 = _state(eng)
            _same(s1, _state(ref))
            _model_delta(m0, m.snapshot(), s0, s1, b.cluster.n_nodes)
            got = _answers(eng, b)
            want = _answers(ref, b, alive)
            print(name, len(rows), "rows out;", [(g[0], len(g[1])) + tuple(g[2:]) for g in got])
            assert got == want
            gone = set(range(b.table.n)) - set(alive)
            assert not any(set(g[1]) & gone for g in got)              # an evicted row is never a victim again
            _same(_state(eng), s1)                                     # the dry runs left no trace
        assert before != got or not any(g[1] for g in before)          # the commits changed some answer
    finally:
        eng.close()
        ref.close()


def test_against_the_oracles_rebuild_form():
    """Requests alone: the oracle's forget and dry run over the survivors."""
    from oracle.oracle import Oracle
    b = cc.build("plain")
    eng = _engine(b)
    try:
        ora = Oracle(b.cluster, b.prof)
        alive = list(range(b.table.n))
        for step in b.sc.steps:
            rows = b.rows_of(step)
            eng.preempt_commit(b.enc, rows, [b.record(r) for r in rows])
            for r in rows:
                ora.forget(b.enc, b.record(r), int(b.table.node[r]))
            alive = [i for i in alive if i not in set(rows)]
            es, os_ = eng.node_state(), ora.node_state()
            for k in es:
                np.testing.assert_array_equal(es[k], os_[k], err_msg=k)
            np.testing.assert_array_equal(eng.class_count(), ora.class_count())
            np.testing.assert_array_equal(eng.nb_alloc(), ora.nb_alloc())
            t = cc.survivors_table(b, alive)
            for i, p in enumerate(b.sc.pending):
                want = ora.preempt(b.enc, i, p.priority, t)
                want = (want[0], [alive[v] for v in want[1]]) + tuple(want[2:])
                assert eng.preempt(b.enc, i, p.priority) == want, (i, want)
    finally:
        eng.close()


# ---- the chain ----------------------------------------------------------------------------------------------
def test_the_chain_sees_the_evictions():
    """A preempts and is nominated, its victim is committed, B's dry run sees
    both; then B's victim, then C.  Hand-derived in preemptcommitcases.chain and
    checked against the object-level reference on the CPU."""
    b = cc.build("chain")
    eng, ref = _engine(b), _engine(b)
    try:
        n0, n1 = b.pos["n0"], b.pos["n1"]
        row = b.sc.order
        A, B, C = 0, 1, 2
        prio = [p.priority for p in b.sc.pending]
        row_pod = {r: b.record(r) for r in range(b.table.n)}
        alive = list(range(b.table.n))

        def full(e, i, groups=None):
            return e.preempt(b.enc, i, prio[i], groups=groups, full=True, with_pdb=True)

        what_if = full(eng, B)
        assert what_if[:2] == (n0, [row["a0"]])
        got = full(eng, A)
        assert got[:2] == (n0, [row["a0"]])
        rows, idx = commit_args(got, row_pod)
        eng.preempt_commit(b.enc, rows, idx)
        for r in rows:
            ref.forget(b.enc, b.record(int(r)), int(b.table.node[r]))
        alive = [i for i in alive if i not in set(rows.tolist())]
        ref.set_bound_pods(cc.survivors_table(b, alive))
        _same(_state(eng), _state(ref))
        groups = [(n0, [A])]
        got = full(eng, B, groups)
        print("B what-if", what_if, "in the chain", got)
        assert got[:2] == (n0, [row["a1"]]) and got != what_if          # the chain saw the eviction
        want = full(ref, B, groups)
        assert got == (want[0], [alive[v] for v in want[1]]) + tuple(want[2:])
        assert got[4] == 0                                              # a1's budget allows one disruption
        rows, idx = commit_args(got, row_pod)
        eng.preempt_commit(b.enc, rows, idx)
        for r in rows:
            ref.forget(b.enc, b.record(int(r)), int(b.table.node[r]))
        alive = [i for i in alive if i not in set(rows.tolist())]
        ref.set_bound_pods(cc.survivors_table(b, alive))
        _same(_state(eng), _state(ref))
        groups = [(n0, [A, B])]
        got = full(eng, C, groups)
        assert got[:2] == (n1, [row["c0"]])
        want = full(ref, C, groups)
        assert got == (want[0], [alive[v] for v in want[1]]) + tuple(want[2:])
        assert eng.node_state()["num_pods"][n0] == 0
    finally:
        eng.close()
        ref.close()


# ---- the setters after a commit -----------------------------------------------------------------------------
def test_the_setters_take_the_original_rows_after_a_commit():
    """Each list is set again from the CSR over all the rows set_bound_pods was
    given (the evicted rows' entries are passed over), cleared and set; then a
    second commit moves the lists the setters uploaded."""
    b = cc.build("seam_65")
    t = b.table
    eng, ref = _engine(b), _engine(b)
    try:
        alive = _commit_and_rebuild(eng, ref, b, b.rows_of(b.sc.steps[0]), list(range(t.n)))
        want = _answers(ref, b, alive)
        assert _answers(eng, b) == want
        eng.set_bound_pod_adds(t.adds_off, t.adds)
        assert _answers(eng, b) == want
        eng.set_bound_pod_pdbs(t.pdb_allowed, t.pdb_off, t.pdb_ids)
        assert _answers(eng, b) == want
        # a list that differs on the survivors: every row under the budget
        eng.set_bound_pod_pdbs(t.pdb_allowed, np.arange(t.n + 1, dtype=np.int32), np.zeros(t.n, np.int32))
        ref.set_bound_pod_pdbs(t.pdb_allowed, np.arange(len(alive) + 1, dtype=np.int32), np.zeros(len(alive), np.int32))
        guarded = _answers(ref, b, alive)
        assert _answers(eng, b) == guarded and guarded != want
        eng.set_bound_pod_pdbs([], [0], [])                             # cleared: only the adds are left
        ref.set_bound_pod_pdbs([], [0], [])
        assert _answers(eng, b) == _answers(ref, b, alive)
        with pytest.raises(KsimError):                                  # an evicted row's entries are still validated
            bad = t.adds.copy()
            bad[t.adds_off[b.rows_of(b.sc.steps[0])[0]]:, 0] = 10 ** 6
            eng.set_bound_pod_adds(t.adds_off, bad)
        eng.set_bound_pod_adds(t.adds_off, t.adds)
        eng.set_bound_pod_pdbs(t.pdb_allowed, t.pdb_off, t.pdb_ids)
        alive = _commit_and_rebuild(eng, ref, b, b.rows_of(b.sc.steps[1]), alive)
        _same(_state(eng), _state(ref))
        assert _answers(eng, b) == _answers(ref, b, alive)
    finally:
        eng.close()
        ref.close()


# ---- refusals: host checks, before anything runs ---------------------------------------------------------------
def _refused(eng, code, *words, call):
    with pytest.raises(KsimError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_change_nothing():
    b = cc.build("only_adds")
    enc, t = b.enc, b.table
    eng = _engine(b)
    try:
        rec = b.record
        eng.preempt_commit(enc, [2], [rec(2)])
        state, answers = _state(eng), _answers(eng, b)
        L, h, ps = eng.L, eng.h, enc.pod_set()
        i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        raw = lambda *a: (lambda: eng._chk(L.ksim_preempt_commit(h, *a)))                    # noqa: E731
        commit = lambda rows, idx: (lambda: eng.preempt_commit(enc, rows, idx))             # noqa: E731
        cases = [
            (abi.E_INVALID, ("negative",), raw(ctypes.byref(ps), -1, None, None)),
            (abi.E_INVALID, ("null",), raw(None, 1, i32([0]), i32([rec(0)]))),
            (abi.E_INVALID, ("null",), raw(ctypes.byref(ps), 1, None, i32([rec(0)]))),
            (abi.E_INVALID, ("null",), raw(ctypes.byref(ps), 1, i32([0]), None)),
            (abi.E_INVALID, ("entry 1", "outside the bound-pod table"), commit([0, t.n], [rec(0), rec(1)])),
            (abi.E_INVALID, ("entry 0", "outside the bound-pod table"), commit([-1], [rec(0)])),
            (abi.E_INVALID, ("entry 1", "already evicted"), commit([0, 2], [rec(0), rec(2)])),
            (abi.E_INVALID, ("entry 2", "named twice"), commit([0, 1, 0], [rec(0), rec(1), rec(0)])),
            (abi.E_INVALID, ("entry 1", "outside the pod set"), commit([0, 1], [rec(0), enc.n_pods])),
            (abi.E_INVALID, ("entry 0", "outside the pod set"), commit([0], [-1])),
            (abi.E_INVALID, ("entry 1", "requests differ"), commit([0, 1], [rec(0), 0])),
        ]
        for code, words, call in cases:
            _refused(eng, code, *words, call=call)
            _same(_state(eng), state)
            assert _answers(eng, b, single=False) == answers
        # a record the per-pod calls refuse, and one whose requests were changed
        for field, value, words in (("node_name", 10 ** 6, ("entry 1", "node_name")),
                                    ("req_mem", 12345, ("entry 1", "requests differ")),
                                    ("scalar_req", 7, ("entry 1", "requests differ"))):
            keep = enc.pods[field][rec(1)].copy()
            enc.pods[field][rec(1)] = value
            try:
                _refused(eng, abi.E_INVALID, *words, call=commit([0, 1], [rec(0), rec(1)]))
            finally:
                enc.pods[field][rec(1)] = keep
            _same(_state(eng), state)
        assert _answers(eng, b) == answers
        eng.preempt_commit(enc, [], [])                                  # n == 0
        _same(_state(eng), state)
        eng.preempt_commit(enc, [0, 1], [rec(0), rec(1)])                # a valid call right after
        assert eng.node_state()["num_pods"].sum() == t.n - 3
    finally:
        eng.close()
    eng = Engine(0)                                                      # no bound table
    try:
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.preempt_commit(enc, [], [])
        _refused(eng, abi.E_INVALID, "ksim_set_bound_pods", call=lambda: eng.preempt_commit(enc, [0], [b.record(0)]))
    finally:
        eng.close()
    eng = Engine(0)                                                      # a shard handle
    try:
        eng.set_shard(0, b.cluster.n_nodes)
        eng.set_profile(b.prof)
        eng.set_cluster(b.cluster)
        eng.set_bound_pods(t)
        _refused(eng, abi.E_UNSUPPORTED, "unsharded", call=lambda: eng.preempt_commit(enc, [0], [b.record(0)]))
    finally:
        eng.close()
