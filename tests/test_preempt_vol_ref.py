"""The reference of the volume dry run (tests/preemptvolref.py), on the CPU.

1. On every use-free case of tests/preemptcases.py it equals
   tests/preemptobjref.py dry_run: the limit plugins and the wider
   potential-node rule change nothing there.
2. Every hand-derived result of tests/preemptvolcases.py holds, with and
   without the scene's nominated group.
3. Every faulty reading (preemptvolref.FLAWS) changes the 4-tuple of the scenes
   meant to tell it, and ``sums_32bit`` that of the array scene.
4. The numpy restatement of the device's incremental rule over the compiled
   tables (tests/preemptvolmodel.py) equals the reference on every scene, with
   and without groups: the compile (``VolumeLimits.bound_uses``,
   ``bound_table(..., vol_limits=)``) and the reaches-0 rule, before any GPU run.
5. The compile itself: the holdings agree with ``attached`` and the class
   counts, and the library exports the two calls."""
import functools

import numpy as np
import pytest

import preemptcases as pc
import preemptobjref
import preemptvolcases as cases
import preemptvolmodel as model
import preemptvolref as ref
from ksim import abi
from ksim.model import Container, Pod


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_reference_equals_objref_on_use_free_cases(name, grouped):
    case = pc.all_cases()[name]
    prio = case.preemptor[0]
    nodes, bound, start, order, pod = pc.objects(case)
    nom = Pod("nominated", priority=prio + 1, containers=[Container({"cpu": "700m"})])
    nominated = {nodes[min(1, case.n_nodes - 1)].name: [nom]} if grouped else None
    want = preemptobjref.dry_run(nodes, bound, start, order, pod, prio, case.args, nominated)
    assert ref.dry_run(nodes, [], [], bound, start, order, pod, prio, case.args, nominated) == want


@functools.lru_cache(maxsize=None)
def _built(name):
    return model.build(cases.scenes()[name])


@functools.lru_cache(maxsize=None)
def _result(name: str, flaw=None, grouped=True):
    s = cases.scenes()[name]
    nodes = _built(name).nodes                           # the cluster's node order is the scan order
    return ref.dry_run(nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], cases.PRIO, s.args,
                       s.nominated_pods() if grouped else None, flaw=flaw, filter_order=s.filter_order)


def _as_tuple(expect):
    return (expect[0], list(expect[1]), expect[2], expect[3])


@pytest.mark.parametrize("name", cases.scene_ids())
def test_scene_reference(name):
    s = cases.scenes()[name]
    assert s.expect_result is not None
    assert _result(name) == _as_tuple(s.expect_result)
    if s.nominated:
        assert s.expect_plain is not None
        assert _result(name, None, False) == _as_tuple(s.expect_plain)
    else:
        assert _result(name, None, False) == _result(name)


def test_scene_sizes():
    sizes = sorted(len(s.nodes) for s in cases.scenes().values())
    assert sizes[-2:] == [257, 300] and all(1 <= n <= 8 for n in sizes[:-2])


def test_every_flaw_is_told_by_the_scenes_meant_for_it():
    meant = {}
    for name, s in cases.scenes().items():
        for flaw in s.tells:
            meant.setdefault(flaw, []).append(name)
    assert set(meant) == set(ref.FLAWS)
    for flaw, names in meant.items():
        for name in names:
            assert _result(name, flaw) != _result(name), (flaw, name)


# ---- the device rule, restated over the compiled tables ---------------------------------------------
def _indices(name, result):
    b = _built(name)
    return preemptobjref.as_indices(result, b.cluster.node_names, b.sc.order)


@pytest.mark.parametrize("name", cases.scene_ids())
def test_device_rule_equals_the_reference(name):
    b = _built(name)
    assert model.device_rule(b) == _indices(name, _result(name))
    assert model.device_rule(b, grouped=False) == _indices(name, _result(name, None, False))


def test_sums_past_2_31():
    """No object scene holds 2^31 volumes: the scene's compiled tables are
    patched, the 64-bit rule gives the hand-derived result and 32-bit sums
    lose the node (attached + arg wraps below the limit)."""
    sc = cases.past_2_31()
    b = model.build(sc)
    assert model.device_rule(b) == (-1, [], 0, 0)         # unpatched: 1 + 1 <= 39, nothing is potential
    model.patch_past_2_31(b)
    assert cases.PAST_ATTACHED + cases.PAST_ARG > 2 ** 31 > cases.PAST_LIMIT
    assert model.device_rule(b) == (0, [0], 1, 1) == preemptobjref.as_indices(
        _as_tuple(sc.expect_result), b.cluster.node_names, sc.order)
    assert model.device_rule(b, wrap32=True) == (-1, [], 0, 0)


# ---- the compile ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.scene_ids())
def test_holdings_agree_with_the_tables(name):
    """attached[f][n] = the rows' classless counts plus the classes with a
    holder; class_count[cls][n] = the rows naming cls (what the header asks of
    ksim_set_bound_pod_volumes' caller)."""
    b = _built(name)
    t, vl, c = b.table, b.vl, b.cluster
    assert t.vol_off.size == t.n + 1 and (t.vol_uses["kind"] == abi.USE_VOLUME).all()
    att = np.zeros_like(vl.attached)
    cnt = np.zeros_like(c.class_count)
    for j in range(t.n):
        n = int(t.node[j])
        row = t.vol_uses[t.vol_off[j]:t.vol_off[j + 1]]
        assert len({int(u["cls"]) for u in row if int(u["cls"]) >= 0}) == sum(int(u["cls"]) >= 0 for u in row)
        for u in row:
            if int(u["cls"]) < 0:
                att[int(u["col"]), n] += int(u["arg"])
            else:
                assert int(u["arg"]) == 1
                if cnt[int(u["cls"]), n] == 0:
                    att[int(u["col"]), n] += 1
                cnt[int(u["cls"]), n] += 1
    assert np.array_equal(att, vl.attached)
    vol_classes = sorted(c.topo.vol_ids)
    assert np.array_equal(cnt[vol_classes], c.class_count[vol_classes])


def test_reordered_carries_the_bound_uses():
    b = _built("two_victims_share")
    assert b.vl.bound_uses and b.vl.reordered(list(reversed(b.vl.node_names))).bound_uses is b.vl.bound_uses


def test_the_library_exports_the_calls():
    from ksim import engine
    assert {"ksim_set_bound_pod_volumes", "ksim_preempt_volumes"} <= set(engine.EXPORTS)
    lib = engine.lib()
    assert lib.ksim_preempt_volumes is not None and lib.ksim_set_bound_pod_volumes is not None
    assert lib.ksim_abi_version() == 12
