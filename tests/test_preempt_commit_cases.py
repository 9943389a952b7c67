"""The scenes of tests/preemptcommitcases.py on the CPU: the model scenes tell
every wrong reading of ksim_preempt_commit (FLAWS) from the model, the model's
hand-derived facts hold, the engine scenes compile and their model after every
step is the table ksim.preemption.bound_table builds from the survivors, and
the chain scene's answers are the object-level reference's
(tests/preemptfullref.py).  The engine runs them in
tests/test_gpu_preempt_commit.py."""
import os
import re

import numpy as np
import pytest

import preemptcommitcases as cc
import preemptfullref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the wrong readings ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flaw", cc.FLAWS)
def test_every_wrong_reading_changes_some_scene(flaw):
    told = [s.name for s in cc.model_scenes().values() if s.result(flaw) != s.result()]
    print(flaw, told)
    assert told
    for s in cc.model_scenes().values():
        if flaw in s.tells:
            assert s.name in told, (flaw, s.name)


def test_every_scene_names_what_it_tells():
    named = {f for s in cc.model_scenes().values() for f in s.tells}
    assert named == set(cc.FLAWS)
    for s in cc.model_scenes().values():
        assert set(s.tells) <= set(cc.FLAWS)


# ---- hand-derived facts of the model --------------------------------------------------------------------
def test_the_middle_node_becomes_empty_between_two_others():
    s = cc.model_scenes()["middle_of_three_nodes"]
    snap, view, probes = s.result()[0]
    assert [len(v) for v in view] == [2, 0, 2]
    assert view[0] == [(0, 10, 100, 100, ((0, 1), (1, 2)), (0,), ()), (1, 5, 100, 100, (), (), ())]
    assert view[2] == [(4, 8, 100, 100, (), (1,), ()), (5, 6, 100, 100, ((1, 1),), (0,), ())]
    assert probes == [[0, 1], [], [4, 5], [5]]
    assert snap["node"][1] == dict(cpu=0, nz_cpu=0, nz_mem=0, num_pods=0, nb=0)
    assert snap["cnt"] == {(0, 0): 1, (1, 0): 2, (1, 2): 1}


def test_two_victims_that_are_the_only_holders_detach_once():
    s = cc.model_scenes()["only_two_holders"]
    m = cc.Model(s.n_nodes, s.rows)
    assert m.att == {(0, 0): 3, (1, 0): 1} and m.cnt == {(7, 0): 2, (8, 0): 2}
    m.commit([0, 1])
    assert m.att[(0, 0)] == 2 and m.cnt[(7, 0)] == 0          # by exactly one
    m.commit([3])
    assert m.att[(1, 0)] == 1 and m.cnt[(8, 0)] == 1          # one of two holders: no change
    m.commit([2])
    assert m.att[(0, 0)] == 0                                 # the classless count of two
    assert [r[0] for r in m.view()[0]] == [4]


def test_row_numbers_keep_their_meaning_and_refusals_change_nothing():
    s = cc.model_scenes()["two_commits"]
    r = s.result()
    assert [x[0] for x in r[0][1][0]] == [0, 2, 3, 4, 5] and r[0][2] == [[0, 2, 3, 4, 5]]
    assert [x[0] for x in r[1][1][0]] == [2, 3, 5] and r[1][2] == [[2, 3, 5]]
    assert r[2][:3] == ("refused", 0, "row already evicted") and r[2][3:] == r[1][:2]
    m = cc.Model(s.n_nodes, s.rows)
    for bad, why in (([6], "outside"), ([-1], "outside"), ([2, 3, 2], "twice")):
        before = (m.snapshot(), m.view())
        with pytest.raises(cc.Refused, match=why) as e:
            m.commit(bad)
        assert e.value.entry == len(bad) - 1 and (m.snapshot(), m.view()) == before
    with pytest.raises(cc.Refused, match="requests differ"):
        m.commit([2, 3], cpus=[100, 101])


# ---- the engine scenes ------------------------------------------------------------------------------------
def _view_of_table(t, n_nodes, alive):
    """cc.Model.view()'s form of a bound table over the rows ``alive``."""
    rows = []
    for k in range(t.n):
        adds = tuple((int(c), int(x)) for c, x in t.adds[t.adds_off[k]:t.adds_off[k + 1]])
        pids = () if t.pdb_off is None else tuple(int(x) for x in t.pdb_ids[t.pdb_off[k]:t.pdb_off[k + 1]])
        vols = () if t.vol_off is None else tuple((int(u["cls"]), int(u["col"]), int(u["arg"]))
                                                 for u in t.vol_uses[t.vol_off[k]:t.vol_off[k + 1]])
        rows.append(cc.Row(int(t.node[k]), int(t.priority[k]), int(t.start_time[k]), int(t.req[k, 0]), adds, pids, vols))
    view = cc.Model(n_nodes, rows).view()
    return [[(alive[r[0]],) + r[1:] for r in node] for node in view]


@pytest.mark.parametrize("name", cc.scene_ids())
def test_the_model_after_every_step_is_the_table_built_from_the_survivors(name):
    b = cc.build(name)
    m = cc.model_of(b)
    alive = list(range(b.table.n))
    assert m.view() == _view_of_table(b.table, b.cluster.n_nodes, alive)
    assert b.sc.steps
    for step in b.sc.steps:
        rows = b.rows_of(step)
        m.commit(rows, cpus=[int(b.enc.pods[b.record(r)]["req_cpu"]) for r in rows])
        alive = [i for i in alive if i not in set(rows)]
        assert m.view() == _view_of_table(cc.survivors_table(b, alive), b.cluster.n_nodes, alive)
        assert sum(v["num_pods"] for v in m.snapshot()["node"]) == len(alive)


def test_the_seams_and_the_edges_are_in_the_scenes():
    from ksim import preemption
    src = open(os.path.join(ROOT, "kube-scheduler-simulator_amd", "csrc", "ksim_internal.h")).read()
    tile = int(re.search(r"constexpr int kCommitTile = (\d+);", src).group(1))
    assert tile == preemption.COMMIT_TILE == cc.TILE
    sizes = sorted(len(s.bound) for s in cc.scenes().values() if s.name.startswith("seam_"))
    # positions 0 .. n are scanned: n = tile - 1 fills one tile, n = tile starts the second
    assert sizes == [1, 63, 64, 65, tile - 2, tile - 1, tile, tile + 1, 2 * tile]
    b = cc.build("seam_65")
    m = cc.model_of(b)
    first = b.rows_of(b.sc.steps[0])
    assert m.table[0] in first and m.table[-1] in first            # the table's first and last rows
    view = m.view()
    assert [len(v) for v in view].count(0) == 2                    # empty nodes beside the victims' nodes
    lens = sorted({len(r[4]) for v in view for r in v})
    assert lens[0] == 0 and lens[-1] >= 3                           # rows without entries beside rows with many
    m.commit(first)
    m.commit(b.rows_of(b.sc.steps[1]))
    assert len(m.view()[b.pos["n3"]]) == 0 and m.view()[b.pos["n1"]] and m.view()[b.pos["n4"]]
    bv = cc.build("volumes")
    assert bv.table.vol_off is not None and bv.table.pdb_off is None
    bo = cc.build("only_adds")
    assert bo.table.vol_off is None and bo.table.pdb_off is None and bo.table.adds_off is not None


def test_the_volume_scene_detaches_once():
    b = cc.build("volumes")
    m = cc.model_of(b)
    n0, n1 = b.pos["n0"], b.pos["n1"]
    assert (m.att[(0, n0)], m.att[(0, n1)]) == (5, 4)              # {s, t, p, q, r} and {u, w, y, z}
    m.commit(b.rows_of(b.sc.steps[0]))
    assert (m.att[(0, n0)], m.att[(0, n1)]) == (4, 3)              # s and u detach once each; t stays (b3 holds it)
    m.commit(b.rows_of(b.sc.steps[1]))
    assert m.att[(0, n0)] == 2                                     # b4's two volumes


# ---- the chain ---------------------------------------------------------------------------------------------
def _dry(sc, bound, pod, nominated=None):
    got = ref.dry_run(sc.nodes, sc.pvs, sc.pvcs, bound, sc.start, sc.order, pod, pod.priority, sc.args,
                      nominated, None, sc.filter_order, pdbs=sc.budgets)
    return got[0], got[1]


def test_the_chain_by_the_object_level_reference():
    sc = cc.chain()
    A, B, C = sc.pending
    left = list(sc.bound)
    assert _dry(sc, left, A) == ("n0", ["a0"])
    assert _dry(sc, left, B) == ("n0", ["a0"])                     # the what-if answer
    assert _dry(sc, left, B, {"n0": [A]}) == ("n0", ["a1", "a0"])  # a nomination without the eviction
    left = [p for p in left if p.name != "a0"]
    assert _dry(sc, left, B, {"n0": [A]}) == ("n0", ["a1"])        # the chain's
    left = [p for p in left if p.name != "a1"]
    assert _dry(sc, left, C, {"n0": [A, B]}) == ("n1", ["c0"])


# ---- the helper and the names --------------------------------------------------------------------------------
def test_commit_args():
    from ksim.preemption import commit_args
    rows, idx = commit_args((3, [7, 2], 4, 1), {2: 12, 7: 17})
    assert rows.dtype == idx.dtype == np.int32 and list(rows) == [7, 2] and list(idx) == [17, 12]
    rows, idx = commit_args((-1, [], 0, 0), [])
    assert rows.size == idx.size == 0


def test_the_call_is_declared_everywhere():
    """Fails on a tree without ksim_preempt_commit."""
    from ksim import engine
    hdr = open(os.path.join(ROOT, "include", "ksim_engine.h")).read()
    assert re.search(r"\bint\s+ksim_preempt_commit\s*\(", hdr)
    assert int(re.search(r"#define KSIM_ABI_VERSION (\d+)", hdr).group(1)) == 12
    assert "ksim_preempt_commit" in engine.EXPORTS and hasattr(engine.Engine, "preempt_commit")
    go = open(os.path.join(ROOT, "integration", "go", "engine", "engine.go")).read()
    assert "C.ksim_preempt_commit(" in go and "func (e *Engine) PreemptCommit(" in go
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ksim_preempt_commit" in open(os.path.join(ROOT, doc)).read(), doc
