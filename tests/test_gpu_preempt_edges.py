"""ksim_preempt (csrc/ksim_preempt.hip) on the hand-made clusters of
tests/preemptcases.py: one case per level of better()'s cascade, the ``want``
cut of k_preempt_pick either side of the best candidate at N = 1, 1,023,
1,024, 1,025, 2,049 and 3,000 (cuts at a thread boundary and strictly inside a
thread's chunk), and two preemptors in sequence on one table.  The engine's
full 4-tuple (nominated node, victim list, potential nodes, candidates) must
equal the C oracle's; tests/test_preemption.py pins the oracle against the
plain-Python criteria() and shows which level decides each case."""
import pytest

import preemptcases as pc
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """One handle per cluster (the cut cases of one N share a cluster)."""
    from ksim.engine import Engine
    held = {}

    def get(cluster, prof):
        key = id(cluster)
        if key not in held:
            if len(held) >= 4:                           # keep few handles open
                held.pop(next(iter(held)))[0].close()
            e = Engine(0)
            e.set_profile(prof)
            e.set_cluster(cluster)
            held[key] = (e, cluster)
        else:
            held[key][0].set_profile(prof)
        return held[key][0]

    yield get
    for e, _ in held.values():
        e.close()


def _both(engines, case):
    cluster, table, enc, prof = pc.encoded(case)
    eng = engines(cluster, prof)
    eng.set_bound_pods(table)
    got = eng.preempt(enc, 0, case.preemptor[0])
    want = Oracle(cluster, prof).preempt(enc, 0, case.preemptor[0], table)
    return got, want


@pytest.mark.parametrize("name", pc.cascade_ids())
def test_cascade_case_vs_oracle(engines, name):
    case = pc.all_cases()[name]
    got, want = _both(engines, case)
    assert got == want
    assert got[0] == case.winner


@pytest.mark.parametrize("name", pc.geometry_ids())
def test_cut_case_vs_oracle(engines, name):
    case = pc.all_cases()[name]
    got, want = _both(engines, case)
    assert got == want
    assert got[0] == case.winner and got[2:] == (case.n_nodes, case.want)


def test_two_preemptors_in_sequence_on_one_handle(engines):
    """A high-priority preemptor, then a low-priority one on the same table
    and handle: the second victim list carries no flags of the first."""
    case = pc.SEQUENCE
    cluster, table, _, prof = pc.encoded(case)
    eng = engines(cluster, prof)
    eng.set_bound_pods(table)
    ora = Oracle(cluster, prof)
    results = []
    for p in pc.SEQUENCE_PREEMPTORS:
        _, _, enc, _ = pc.encoded(case, p)
        got = eng.preempt(enc, 0, p[0])
        assert got == ora.preempt(enc, 0, p[0], table)
        results.append(got)
    assert results[0][0] == results[1][0] == 2
    assert len(results[0][1]) == 4 and results[1][1] == [3, 2]
