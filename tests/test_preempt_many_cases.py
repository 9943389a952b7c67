"""The scenes of tests/preemptmanycases.py, on the CPU: the references of a
row agree with each other, the scenes tell the call's model from its wrong
readings, and the library carries the new entry points
(tests/test_gpu_preempt_many.py runs the engine on the same scenes)."""
import dataclasses
import os
import re

import pytest

import preemptcases as pc
import preemptfullref
import preemptmanycases as mc
from ksim import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = [n for n, s in mc.scenes().items() if s.case is not None]
OBJECT = [n for n, s in mc.scenes().items() if s.case is None]


# ---- the references of one row ----------------------------------------------------------------------
@pytest.mark.parametrize("name", FIT)
def test_fit_rows_equal_the_restated_criteria(name):
    """fit_dry_run (the model's reference, budgets and flags included) against
    preemptcases.criteria, row by row, wherever no budget is set."""
    s = mc.scenes()[name]
    for (pod, prio), got in zip(s.rows, s.reference()):
        if s.budgets:
            plain = mc.fit_dry_run(s.case, (prio, s.preemptors[pod][1])).result
            assert sorted(got[1]) == sorted(plain[1]) and got[:1] + got[2:4] == plain[:1] + plain[2:4]   # one candidate
            continue
        want = pc.criteria(dataclasses.replace(s.case, preemptor=(prio, s.preemptors[pod][1]))).result
        assert got == want + (0,), (pod, prio)


@pytest.mark.parametrize("name", ["race", "victims_65", "edge_257_256"])
def test_fit_rows_equal_the_oracle_and_the_object_reference(name):
    from oracle.oracle import Oracle
    s = mc.scenes()[name]
    b = s.build()
    ora = Oracle(b.cluster, b.prof)
    nodes, bound, start, order, _ = pc.objects(s.case)
    for (pod, prio), got in dict(zip(s.rows, s.reference())).items():      # each distinct row once
        assert ora.preempt(b.enc, pod, prio, b.table) == got[:4]
        p = pc.preemptor_pod((prio, s.preemptors[pod][1]))
        obj = preemptfullref.dry_run(nodes, [], [], bound, start, order, p, prio, s.case.args)
        assert preemptfullref.as_indices(obj, b.cluster.node_names, order) == got[:4]


def test_the_guarded_victims_lead_the_list():
    """One budget that allows nothing over every third row: those victims come
    first, each in importance order, and the plain list is importance order."""
    s = mc.scenes()["victims_65_guarded"]
    node, victims, _, _, nviol = s.reference()[0]
    assert node == 0 and len(victims) == 65 and nviol == 22
    assert all(v % 3 == 0 for v in victims[:22]) and all(v % 3 for v in victims[22:])
    csr = s.csr(0)
    assert victims[:22] == [i for i in csr if i % 3 == 0] and victims[22:] == [i for i in csr if i % 3]
    assert mc.scenes()["victims_65"].reference()[0][1] == csr


@pytest.mark.parametrize("name", OBJECT)
def test_the_object_scene_takes_every_route(name):
    s = mc.scenes()[name]
    ref = s.reference()
    assert {s.form(pod) for pod, _ in s.rows} == {0, 1, 2}
    forms = [s.form(pod) for pod, _ in s.rows]
    assert forms != sorted(forms)                                    # interleaved
    assert all(r[0] >= 0 for r, (pod, prio) in zip(ref, s.rows) if prio == 1000), ref
    by_pod = {pod: r for r, (pod, prio) in zip(ref, s.rows) if prio == 1000}
    if not s.budgets:
        assert by_pod[0][0] == 2 and by_pod[4][0] in (0, 3)          # the pinned volume keeps its row off n2
    assert len({repr(r) for r in ref}) >= 5
    if s.budgets:
        assert any(r[4] > 0 for r in ref) and ref != mc.scenes()["mixed"].reference()


def test_the_compiled_preemptors_carry_the_uses_the_routes_need():
    from ksim import abi
    b = mc.scenes()["mixed"].build()

    def kinds(i):
        p = b.enc.pods[i]
        return {int(k) for k in b.enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]}
    assert kinds(0) == set() and kinds(1) == {abi.USE_NODE_PORT} and kinds(2) == {abi.USE_VOLUME}
    assert kinds(3) == {abi.USE_NODE_PORT, abi.USE_VOLUME} and int(b.enc.pods[4]["vb_count"]) > 0
    assert kinds(5) == {abi.USE_PTS_SOFT} and kinds(7) == {abi.USE_IMAGE}
    assert kinds(6) and not kinds(6) & {abi.USE_IPA_AFFINITY, abi.USE_IPA_ANTI, abi.USE_PTS_HARD, abi.USE_NODE_PORT}
    assert abi.USE_IPA_ANTI in kinds(8) and abi.USE_PTS_HARD in kinds(9)


# ---- the scenes against the wrong readings ------------------------------------------------------------
@pytest.mark.parametrize("fault", mc.FAULTS)
def test_every_wrong_reading_changes_a_row_of_a_scene_aimed_at_it(fault):
    aimed = [s for s in mc.scenes().values() if fault in s.aims]
    assert aimed, fault
    for s in aimed:
        ref = s.reference()
        got = mc.call_model(s.rows, s.answer, s.form, s.csr, fault)
        assert len(got) == len(ref) and got != ref, (s.name, fault)


def test_the_race_scenes_put_two_priorities_on_one_node():
    """Both orders: two rows of different priority nominate node 2 with
    different victims, and the later row's flags would replace the earlier's."""
    for name in ("race", "race_reversed", "two_rows"):
        ref = mc.scenes()[name].reference()
        on2 = {tuple(r[1]) for r in ref if r[0] == 2}
        assert len(on2) == 2, name
    a, b = mc.scenes()["two_rows"].reference()
    x, y = mc.call_model(*_args("two_rows"), "shared_flags")
    assert (x, y) == ((a[0], b[1]) + a[2:], b)                        # the later, high row's flags replaced the low row's
    assert mc.scenes()["nobody_beside_everybody"].reference()[0][:2] == (-1, [])


def _args(name):
    s = mc.scenes()[name]
    return s.rows, s.answer, s.form, s.csr


def test_the_row_counts_and_the_node_counts_asked_for_are_there():
    sc = mc.scenes()
    assert sorted(len(s.rows) for s in sc.values() if s.name.startswith(("rows_", "no_", "one_", "two_"))) == \
        [0, 1, 2, 63, 64, 65, 130]
    assert {s.n_nodes for s in sc.values()} >= {1, 255, 256, 257, 1025, 2049}
    for n in (1025, 2049):
        c = sc[f"cut_{n}"].case
        assert pc.inside_a_chunk(n, c.want)
    assert sc["edge_257_255"].reference()[0][0] == 255 and sc["edge_257_256"].reference()[0][0] == 256
    assert sc["edge_256_255"].reference()[0][0] == 255 and sc["edge_255_254"].reference()[0][0] == 254


# ---- the ABI --------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_batched_call():
    """Fails on a library without ksim_preempt_many."""
    src = open(os.path.join(ROOT, "include", "ksim_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ksim_preempt_many\s*\(", src) and re.search(r"\bint32_t\s+ksim_preempt_many_rows\s*\(", src)
    assert re.search(r"#define\s+KSIM_PREEMPT_MANY_ROWS\s+64\b", src)
    L = engine.lib()
    assert hasattr(L, "ksim_preempt_many") and hasattr(L, "ksim_preempt_many_rows")
    assert {"ksim_preempt_many", "ksim_preempt_many_rows"} <= set(engine.EXPORTS)
    assert L.ksim_abi_version() == 12


def test_rows_per_group_is_bounded_monotone_and_64_on_every_scene():
    L = engine.lib()
    sizes = [0, 1, 255, 4096, 100_000, 1_000_000, 8_388_608, 2 ** 31 - 1]
    last_n = None
    for n in sizes:
        row = [L.ksim_preempt_many_rows(n, b) for b in sizes]
        assert all(1 <= r <= mc.MAX_ROWS for r in row)
        assert row == sorted(row, reverse=True)                      # non-increasing in n_bound
        assert row == [mc.many_rows(n, b) for b in sizes]
        if last_n is not None:
            assert all(a >= b for a, b in zip(last_n, row))          # ... and in n_nodes
        last_n = row
    assert L.ksim_preempt_many_rows(-5, -5) == mc.MAX_ROWS
    assert L.ksim_preempt_many_rows(2 ** 31 - 1, 2 ** 31 - 1) == 1
    # the stated bound: rows x (32 n + n_bound) <= 256 MiB whenever more than one row is taken
    for n, b in ((100_000, 1_000_000), (1_000_000, 50_000_000), (4096, 0)):
        r = L.ksim_preempt_many_rows(n, b)
        assert r == 1 or r * (32 * n + b) <= mc.SLAB_BYTES
    assert L.ksim_preempt_many_rows(100_000, 1_000_000) >= 63
    for s in mc.scenes().values():
        assert s.n_nodes < 4096 and L.ksim_preempt_many_rows(s.n_nodes, s.n_bound) == mc.MAX_ROWS == mc.many_rows(
            s.n_nodes, s.n_bound)
