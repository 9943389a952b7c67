"""The reference of the spread dry run (tests/preemptspreadref.py), on the CPU.

1. On every use-free case of tests/preemptcases.py and every scene of
   tests/preemptaffcases.py (no DoNotSchedule constraint anywhere) it equals
   tests/preemptobjref.py dry_run: the added potential-node rule changes
   nothing there.
2. Every hand-derived ``expect`` of tests/preemptspreadcases.py holds, with and
   without the scene's nominated groups, and the incremental form the faulty
   readings are built on equals the recomputation.
3. Every faulty reading (preemptspreadref.FLAWS) changes the 4-tuple of at
   least one scene.
4. The compiled preemptors carry USE_PTS_HARD, bound_table(..., full_adds=True)
   lists the selector class on the matching rows, and the library exports the
   new call."""
import functools

import pytest

import preemptaffcases as ac
import preemptcases as pc
import preemptobjref
import preemptspreadcases as sc_mod
import preemptspreadref as ref
from ksim import abi
from ksim.encode import encode_cluster, encode_pods
from ksim.model import Container, Pod
from ksim.preemption import bound_table


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_reference_equals_objref_on_use_free_cases(name, grouped):
    case = pc.all_cases()[name]
    prio = case.preemptor[0]
    nodes, bound, start, order, pod = pc.objects(case)
    nom = Pod("nominated", priority=prio + 1, containers=[Container({"cpu": "700m"})])
    nominated = {nodes[min(1, case.n_nodes - 1)].name: [nom]} if grouped else None
    want = preemptobjref.dry_run(nodes, bound, start, order, pod, prio, case.args, nominated)
    assert ref.dry_run(nodes, bound, start, order, pod, prio, case.args, nominated) == want
    if not grouped:
        assert preemptobjref.as_indices(want, [n.name for n in nodes], order)[0] == case.winner


@pytest.mark.parametrize("name", ac.scene_ids())
def test_reference_equals_objref_on_affinity_scenes(name):
    s = ac.scenes()[name]
    a = (s.nodes, s.bound, s.start, s.order, s.pods[0], ac.PRIO, s.args, s.nominated_pods())
    assert ref.dry_run(*a) == preemptobjref.dry_run(*a)


@functools.lru_cache(maxsize=None)
def _result(name: str, flaw, grouped=True):
    s = sc_mod.scenes()[name]
    return ref.dry_run(s.nodes, s.bound, s.start, s.order, s.pods[0], s.pods[0].priority, s.args,
                       s.nominated_pods() if grouped else None, flaw=flaw, filter_order=sc_mod.filter_order(s))


def _as_tuple(expect):
    return (expect[0], list(expect[1]), expect[2], expect[3])


@pytest.mark.parametrize("name", sc_mod.scene_ids())
def test_scene_reference(name):
    """The reference gives what the scene was derived to give, and moving the
    pairs by each pod of the node equals recomputing them."""
    s = sc_mod.scenes()[name]
    assert s.expect is not None
    assert _result(name, None) == _as_tuple(s.expect)
    assert _result(name, "none") == _result(name, None)
    if s.nominated:
        assert s.expect_plain is not None
        assert _result(name, None, False) == _as_tuple(s.expect_plain)
        assert _result(name, "none", False) == _result(name, None, False)


@pytest.mark.parametrize("flaw", ref.FLAWS)
def test_scenes_discriminate(flaw):
    differs = [name for name in sc_mod.scene_ids() if _result(name, flaw) != _result(name, None)]
    assert differs, f"no scene tells the reference from the reading {flaw}"


def test_flaws_hit_the_scenes_meant_for_them():
    """Which scene catches which reading (at least these)."""
    meant = {"stale_domains": ["headline", "zone_and_hostname", "three_hundred_hosts"],
             "stale_min": ["group_lifts_own_domain", "only_domain"],
             "ineligible_moves": ["tainted_node_moves_nothing", "unselected_node_moves_nothing"],
             "missing_label_potential": ["zone_and_hostname"],
             "no_pts_in_reprieve": ["headline", "spread_anti_and_port"],
             "no_self_match": ["headline"],
             "other_namespace_counts": ["other_namespace"],
             "group_ignored": ["group_lifts_own_domain"]}
    assert set(meant) == set(ref.FLAWS)
    for flaw, names in meant.items():
        for name in names:
            assert _result(name, flaw) != _result(name, None), (flaw, name)


def test_removals_alone_do_not_tell_a_stale_minimum():
    """own' <= own under removals, so min(own', others) and the status pass's
    minimum give the same verdicts: only the scenes with a group differ."""
    for name in sc_mod.scene_ids():
        assert _result(name, "stale_min", False) == _result(name, None, False), name


def test_scene_pods_compile_to_hard_uses_and_full_adds_list_the_class():
    for s in sc_mod.scenes().values():
        cluster, _ = encode_cluster(s.nodes, s.bound)
        enc = encode_pods(cluster, s.pods)
        p = enc.pods[0]
        uses = enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
        kinds = {int(k) for k in uses["kind"]}
        assert {getattr(abi, "USE_" + k) for k in s.kinds} <= kinds, s.name
        full = bound_table(cluster, s.bound, s.start, cluster.topo, full_adds=True)
        ns = s.pods[0].namespace
        for u, c in zip([x for x in uses if int(x["kind"]) == abi.USE_PTS_HARD],
                        [c for c in s.pods[0].topology_spread if c.when_unsatisfiable == "DoNotSchedule"]):
            cls = int(u["cls"])
            assert cls >= 0
            for i, q in enumerate(s.bound):
                row = dict(map(tuple, full.adds[full.adds_off[i]:full.adds_off[i + 1]].tolist()))
                counts = q.namespace == ns and c.label_selector.matches(q.labels)
                assert row.get(cls, 0) == (1 if counts else 0), (s.name, q.name)


def test_the_library_exports_the_call():
    from ksim import engine
    assert "ksim_preempt_spread" in engine.EXPORTS
    lib = engine.lib()
    assert lib.ksim_preempt_spread is not None and lib.ksim_abi_version() == 12
