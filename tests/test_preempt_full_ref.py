"""The reference of the full dry run (tests/preemptfullref.py), on the CPU.

1. On the volume-only scenes of tests/preemptvolcases.py it equals
   tests/preemptvolref.py, on the spread-only scenes of
   tests/preemptspreadcases.py tests/preemptspreadref.py, and on the
   affinity-only scenes of tests/preemptaffcases.py tests/preemptobjref.py:
   knowing the PVs and asking the limit plugins changes nothing where there
   is nothing to know or to ask.
2. Every hand-derived result of tests/preemptfullcases.py holds, with and
   without the scene's nominated group.
3. Every wrong reading (preemptfullref.FLAWS) changes the 4-tuple of the scenes
   that name it in ``tells``; the readings in EQUAL change none.
4. The compiled preemptors carry the use kinds and volume groups the scenes
   are there for, no class add names a volume class, the library exports
   ksim_preempt_full, the header declares it and Engine.preempt takes ``full``."""
import functools
import inspect
import os
import re

import pytest

import preemptaffcases as ac
import preemptfullcases as cases
import preemptfullref as ref
import preemptobjref
import preemptspreadcases as sc_mod
import preemptspreadref
import preemptvolcases as vc
import preemptvolref
from ksim import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the older references ------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", [n for n in vc.scene_ids() if n != "three_hundred_shared"])
def test_equals_the_volume_reference_on_volume_only_scenes(name, grouped):
    s = vc.scenes()[name]
    nominated = s.nominated_pods() if grouped else None
    a = (s.nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], vc.PRIO, s.args, nominated)
    assert ref.dry_run(*a, filter_order=s.filter_order) == preemptvolref.dry_run(*a, filter_order=s.filter_order)


@pytest.mark.parametrize("name", [n for n in sc_mod.scene_ids() if n != "three_hundred_hosts"])
def test_equals_the_spread_reference_on_spread_only_scenes(name):
    s = sc_mod.scenes()[name]
    order = sc_mod.filter_order(s)
    for nominated in (s.nominated_pods(), None):
        want = preemptspreadref.dry_run(s.nodes, s.bound, s.start, s.order, s.pods[0], sc_mod.PRIO, s.args, nominated,
                                        filter_order=order)
        assert ref.dry_run(s.nodes, [], [], s.bound, s.start, s.order, s.pods[0], sc_mod.PRIO, s.args, nominated,
                           filter_order=order) == want


@pytest.mark.parametrize("name", ac.scene_ids())
def test_equals_objref_on_affinity_only_scenes(name):
    s = ac.scenes()[name]
    want = preemptobjref.dry_run(s.nodes, s.bound, s.start, s.order, s.pods[0], ac.PRIO, s.args, s.nominated_pods())
    assert ref.dry_run(s.nodes, [], [], s.bound, s.start, s.order, s.pods[0], ac.PRIO, s.args,
                       s.nominated_pods()) == want


# ---- 2. the combined scenes ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _result(name: str, flaw=None, grouped=True):
    s = cases.scenes()[name]
    return ref.dry_run(s.nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], cases.PRIO, s.args,
                       s.nominated_pods() if grouped else None, flaw=flaw, filter_order=s.filter_order,
                       classes=s.classes)


def _as_tuple(expect):
    return (expect[0], list(expect[1]), expect[2], expect[3])


HAND_DERIVED = [n for n in cases.scene_ids() if cases.scenes()[n].expect_result is not None]


def test_at_least_six_combined_scenes_are_hand_derived():
    small = [n for n in HAND_DERIVED if n not in cases.WIDE]
    assert len(small) >= 6 and {"statefulset_replica", "shared_volume_and_zone", "pv_excludes_best"} <= set(small)


@pytest.mark.parametrize("name", HAND_DERIVED)
def test_scene_reference(name):
    s = cases.scenes()[name]
    assert _result(name) == _as_tuple(s.expect_result)
    if s.nominated:
        assert s.expect_plain is not None
        plain = _result(name, None, False)
        assert plain == _as_tuple(s.expect_plain) and plain != _result(name)


# ---- 3. the wrong readings -----------------------------------------------------------------------------
SMALL = [n for n in cases.scene_ids() if n not in cases.WIDE]


@pytest.mark.parametrize("flaw", ref.FLAWS)
def test_scenes_discriminate(flaw):
    named = [n for n in SMALL if flaw in cases.scenes()[n].tells]
    assert named, f"no scene names the reading {flaw}"
    for n in named:
        assert _result(n, flaw) != _result(n), (flaw, n)


@pytest.mark.parametrize("flaw", ref.EQUAL)
def test_equal_readings_change_nothing(flaw):
    for n in SMALL:
        assert _result(n, flaw) == _result(n), (flaw, n)
        if cases.scenes()[n].nominated:
            assert _result(n, flaw, False) == _result(n, None, False), (flaw, n)


def test_every_tell_is_a_known_reading():
    for n in cases.scene_ids():
        assert set(cases.scenes()[n].tells) <= set(ref.FLAWS), n


# ---- 4. the compile and the interface --------------------------------------------------------------------
def _kinds(b, i=0):
    p = b.enc.pods[i]
    return [int(k) for k in b.enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]]


@pytest.mark.parametrize("name", SMALL)
def test_compiled_preemptor(name):
    b = cases.build(cases.scenes()[name])
    kinds = _kinds(b)
    assert abi.USE_VOLUME in kinds
    assert {abi.USE_PTS_HARD, abi.USE_IPA_ANTI, abi.USE_IPA_AFFINITY} & set(kinds)
    p = b.enc.pods[0]
    assert (int(p["vb_count"]) > 0) == (name.startswith("pv_") and not name.startswith("pv_zone"))
    assert (int(p["vz_count"]) > 0) == name.startswith("pv_zone")
    if name.startswith("every_slot"):
        assert len(kinds) == abi.MAX_USES
        assert {abi.USE_NODE_PORT, abi.USE_VOLUME, abi.USE_IPA_ANTI, abi.USE_IPA_AFFINITY, abi.USE_PTS_HARD} <= set(kinds)
        fams = {int(c) for c, k in zip(b.enc.uses["col"][:len(kinds)], kinds) if k == abi.USE_VOLUME}
        assert len(fams) == 2
    if name == "eight_families":
        assert kinds.count(abi.USE_VOLUME) == 8 == b.cluster.vol_limits.limit.shape[0]
    # the two CSRs are disjoint: no class add of a row names a shared volume's class
    held = {int(c) for c in b.table.vol_uses["cls"] if int(c) >= 0}
    added = {int(c) for c in b.table.adds.reshape(-1, 2)[:, 0]} if len(b.table.adds) else set()
    assert not held & added


def test_the_library_exports_the_call_and_the_header_declares_it():
    from ksim import engine
    assert "ksim_preempt_full" in engine.EXPORTS
    assert hasattr(engine.lib(), "ksim_preempt_full")
    with open(os.path.join(ROOT, "include", "ksim_engine.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+ksim_preempt_full\s*\(\s*ksim_handle\s*\*", header)


def test_engine_preempt_takes_full():
    from ksim.engine import Engine
    from ksim.fwplugins import EnginePlugins
    from ksim.wrapped import compat_cycle
    for fn in (Engine.preempt, EnginePlugins.post_filter, compat_cycle):
        p = inspect.signature(fn).parameters
        assert "full" in p and p["full"].default is False, fn
