"""The optional budget table of tests/preemptvolref.py and tests/preemptfullref.py
(``pdbs``: filterPodsWithPDBViolation's split and the violating-first reprieve
order), on the CPU:

1. without budgets both return what they returned: the 4-tuple, and with an
   empty budget list the same result with no violation;
2. on the small scenes of tests/preemptpdbcases.py (no volumes anywhere) both
   equal tests/preemptpdbref.py, grouped and not;
3. on the two mixed-budget scenes (a reprieved row between violating and
   non-violating rows on shared volumes) both give the hand-derived results."""
import pytest

import preemptfullcases as fc
import preemptfullref
import preemptpdbcases as pp
import preemptvolcases as vc
import preemptvolref

VOL_SMALL = ["ebs_slot", "two_victims_share", "two_families_and_a_third", "group_holds_volumes", "port_and_volume"]
FULL_SMALL = ["statefulset_replica", "shared_volume_and_zone", "pv_excludes_best", "group_holds_and_counts", "one_node_anti"]


def _vol(s, **kw):
    return preemptvolref.dry_run(s.nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], vc.PRIO, s.args,
                                 s.nominated_pods(), filter_order=s.filter_order, **kw)


def _full(s, **kw):
    return preemptfullref.dry_run(s.nodes, s.pvs, s.pvcs, s.bound, s.start, s.order, s.pods[0], fc.PRIO, s.args,
                                  s.nominated_pods(), filter_order=s.filter_order, classes=getattr(s, "classes", ()),
                                  **kw)


@pytest.mark.parametrize("name", VOL_SMALL)
def test_volume_reference_without_budgets_is_unchanged(name):
    s = vc.scenes()[name]
    assert _vol(s) == s.expect_result
    assert _vol(s, pdbs=[]) == s.expect_result + (0,)


@pytest.mark.parametrize("name", FULL_SMALL)
def test_full_reference_without_budgets_is_unchanged(name):
    s = fc.scenes()[name]
    assert _full(s) == s.expect_result
    assert _full(s, pdbs=[]) == s.expect_result + (0,)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pp.small_ids())
def test_both_equal_the_pdb_reference_on_its_scenes(name, grouped):
    want = pp.reference(name, grouped)
    sc = pp.scenes()[name].grouped() if grouped else pp.scenes()[name]
    head = (sc.nodes, [], [], sc.bound, sc.start, sc.order, sc.pods[0], pp.PRIO, sc.args, sc.nominated_pods())
    assert preemptfullref.dry_run(*head, pdbs=sc.pdbs) == want
    if not sc.pods[0].pod_anti_affinity_required:            # the volume reference takes no affinity terms
        assert preemptvolref.dry_run(*head, pdbs=sc.pdbs) == want


@pytest.mark.parametrize("scene,run", [(vc.mixed_budget, _vol), (vc.mixed_budget, _full), (fc.mixed_budget, _full)],
                         ids=["volume", "volume_by_full", "full"])
def test_mixed_budget_scenes(scene, run):
    s = scene()
    assert run(s) == s.expect_result
    assert run(s, pdbs=[]) == s.expect_result + (0,)
    got = run(s, pdbs=s.budgets)
    assert got == s.expect_budgets
    assert got[4] == 1 and got[1] != s.expect_result[1]      # a violating victim, and the budget changed the list
