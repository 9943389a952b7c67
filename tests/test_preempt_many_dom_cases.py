"""The scenes of tests/preemptmanydomcases.py, on the CPU: the restated dry run
over an explicit PreFilter state agrees with the reference row by row, every
wrong reading of the call's model changes a row of every scene aimed at it,
and the library carries the new entry points (tests/test_gpu_preempt_many_dom.py
runs the engine on the same scenes)."""
import os
import re

import pytest

import preemptmanydomcases as dc
from ksim import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restated dry run against the reference --------------------------------------------------------
@pytest.mark.parametrize("name", dc.scene_ids())
def test_the_restated_dry_run_equals_the_reference(name):
    s = dc.scenes()[name]
    seen = 0
    for pod, prio in dict.fromkeys(s.rows):                              # each distinct row once
        p = s.sc.pending[pod]
        if s.form(pod) < 2 or not dc.simple(p) or s.budgets:
            continue
        seen += 1
        assert dc.dry_run(s.sc, p, prio, dc.prefilter(s.sc, p), s.built().nodes) == s.answer(pod, prio), (pod, prio)
    assert seen or name.startswith(("routes", "block_edge")), name
    assert s.model() == s.reference()


def _named(s):
    """The scene's reference with node names: [(node name or None, victims), ...]."""
    names = s.built().cluster.node_names
    return [(names[r[0]] if r[0] >= 0 else None, r[1]) for r in s.reference()]


def test_the_scenes_say_what_their_docstrings_say():
    sc = dc.scenes()
    assert _named(sc["selectors_differ"]) == [("n0000", [0, 1]), ("n0002", [2, 3]), (None, []), (None, [])]
    assert _named(sc["affinity_only_here"]) == [("n0002", [4]), ("n0000", [1])]
    s = sc["minima_differ"]
    st = [dc.prefilter(s.sc, p) for p in s.sc.pending]
    assert st[0].minima[0][0] == st[0].minima[0][2] == 1                 # tied
    assert st[1].minima[0] == (4, "r1", dc.NONE_LEFT)                    # the only domain
    assert _named(s) == [("n0000", [0]), ("n0002", [3])]
    s = sc["honor_beside_ignore"]
    assert _named(s) == [(None, []), ("n0001", [3]), ("n0001", [3])]
    honor, ignore, hosts = (dc.prefilter(s.sc, p) for p in s.sc.pending)
    assert honor.tables[0]["za"] == [3, 2] and ignore.tables[0]["za"] == [5, 3]
    assert hosts.tables[0]["n0000"] == [0, 0] and hosts.minima[0][0] == 1   # a pair without a mark
    assert dc.minima_of(hosts.tables[0], marks=False)[0] == 0


def test_the_routes_scene_interleaves_five_routes():
    for name in ("routes", "routes_guarded"):
        s = dc.scenes()[name]
        forms = [s.form(pod) for pod, _ in s.rows]
        assert set(forms) == {0, 1, 2, 3} and forms != sorted(forms)
        b = s.built()
        ports = {pod for pod, _ in s.rows if int(b.enc.pods[pod]["use_count"]) and s.form(pod) == 0 and
                 any(c.ports for c in s.sc.pending[pod].containers)}
        assert ports                                                     # ports and free: two routes of form 0
        ref = s.reference()
        assert len({repr(r) for r in ref}) >= 6
        assert all(r[0] >= 0 for r, (pod, prio) in zip(ref, s.rows) if prio == 1000), ref
    assert any(r[4] > 0 for r in dc.scenes()["routes_guarded"].reference())
    assert dc.scenes()["routes_guarded"].reference() != dc.scenes()["routes"].reference()


def test_the_row_counts_and_the_shapes_asked_for_are_there():
    sc = dc.scenes()
    assert sorted(len(s.rows) for s in sc.values() if s.name.startswith("rows_")) == [1, 2, 63, 64, 65, 130]
    assert {len(s.sc.nodes) for s in sc.values()} >= {1, 127, 128, 255, 256, 257, 300}
    assert all(len(s.sc.nodes) <= 2049 for s in sc.values())
    rows = sc["rows_130"].rows
    assert all(rows[64 + k][0] != rows[k][0] for k in range(64))         # another selector at the same place
    for n in (255, 256, 257):
        assert sc[f"block_edge_{n}"].form(0) == 3
        assert sc[f"block_edge_{n}"].reference()[0][0] == n - 1          # the deciding node is the last one
        assert sc[f"host_spread_{n}"].reference()[0][:2] == (n - 1, [n, n + 1])
    for s in sc.values():
        b = s.built()
        assert dc.dom_rows(b.cluster.n_nodes, len(s.sc.bound), b.cluster.n_nodes + 2) == dc.MAX_ROWS


# ---- the scenes against the wrong readings ------------------------------------------------------------
@pytest.mark.parametrize("fault", dc.FAULTS)
def test_every_wrong_reading_changes_a_row_of_a_scene_aimed_at_it(fault):
    aimed = [s for s in dc.scenes().values() if fault in s.aims]
    assert aimed, fault
    for s in aimed:
        ref, got = s.reference(), s.model(fault)
        assert len(got) == len(ref) and got != ref, (s.name, fault)


def test_the_stale_sum_flips_a_skew_verdict():
    """Row 64 + k on a slab that still holds row k's sums: both zones count 2
    for it, no node fails the skew, and the answer is 'nothing to do'."""
    s = dc.scenes()["rows_65"]
    ref, got = s.reference(), s.model("tables_not_zeroed")
    assert got[:64] == ref[:64] and ref[64][0] >= 0 and got[64][0] == -1
    s = dc.scenes()["rows_130"]
    ref, got = s.reference(), s.model("tables_not_zeroed")
    assert all(a != b for a, b in zip(ref[64:], got[64:]))


# ---- the ABI --------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_domain_call():
    """Fails on a library without ksim_preempt_many_dom."""
    src = open(os.path.join(ROOT, "include", "ksim_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ksim_preempt_many_dom\s*\(", src)
    assert re.search(r"\bint32_t\s+ksim_preempt_many_dom_rows\s*\(", src)
    L = engine.lib()
    assert hasattr(L, "ksim_preempt_many_dom") and hasattr(L, "ksim_preempt_many_dom_rows")
    assert {"ksim_preempt_many_dom", "ksim_preempt_many_dom_rows"} <= set(engine.EXPORTS)
    assert L.ksim_abi_version() == 12
    go = open(os.path.join(ROOT, "integration", "go", "engine", "engine.go")).read()
    assert "C.ksim_preempt_many_dom(" in go and "func (e *Engine) PreemptManyDom(" in go


def test_domain_rows_per_group_against_the_restatement():
    sizes = [-7, 0, 1, 255, 4096, 10_000, 10_001, 100_000, 1_000_000, 8_388_608, 2 ** 31 - 1]
    for n in sizes:
        for b in sizes:
            row = [engine.preempt_many_dom_rows(n, b, v) for v in sizes]
            assert row == [dc.dom_rows(n, b, v) for v in sizes], (n, b)
            assert all(1 <= r <= dc.MAX_ROWS for r in row)
            assert row[1:] == sorted(row[1:], reverse=True)              # non-increasing in n_values
            assert all(r <= max(1, engine.lib().ksim_preempt_many_rows(n, b)) for r in row)
            for r, v in zip(row, sizes):                                 # the stated bound
                assert r == 1 or r * (32 * max(n, 0) + max(b, 0) + 8 * 16 * max(v, 0)) <= dc.SLAB_BYTES
    assert engine.preempt_many_dom_rows(10_000, 100_000, 10_001) == 64   # config 3's shape
    assert engine.preempt_many_dom_rows(-5, -5, -5) == dc.MAX_ROWS
    assert engine.preempt_many_dom_rows(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == 1
    assert engine.preempt_many_dom_rows(100_000, 1_000_000, 100_001) == 15
