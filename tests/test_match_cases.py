"""The case table of tests/matchcases.py can tell a wrong ksim_match_terms
from a right one: every case is non-degenerate by the reference alone, and
each of ten faulty restatements of the reference (stand-ins for kernel
faults; numpy only) is told apart from it by a named case.  The device side is
tests/test_gpu_match_edges.py."""
import numpy as np
import pytest

import matchcases as mc


@pytest.fixture(scope="module")
def refs():
    return {name: mc.reference(p) for name, p in mc.cases().items()}


def test_case_table_covers_the_sizes():
    t = mc.cases()
    assert {p.n_sigs for p in t.values()} >= set(mc.SIG_SIZES)
    assert {p.n_feat for p in t.values()} >= set(mc.FEAT_SIZES) | {mc.MAX_FEAT}
    assert {p.n_reqs for p in t.values()} >= set(mc.REQ_SIZES) | {mc.MAX_REQS}
    assert {p.n_matchers for p in t.values()} >= set(mc.MATCHER_SIZES)
    assert {p.n_classes for p in t.values()} >= set(mc.CLASS_SIZES)
    assert t["classes_no_pods"].n_pods == 0 and t["classes_no_pods"].n_classes > 0
    assert t["one_node"].n_nodes == 1 and t["one_node"].n_pods > 0
    hot = t["hot_node_5000"]
    assert hot.n_pods == 5000 and set(hot.pod_node.tolist()) == {3}
    assert t["reqs_0"].n_matchers > 0 and all(not m for m in t["reqs_0"].matchers)
    big = t["reqs_4096"]
    assert big.n_sigs == 16 and {r >> 4 for m in big.matchers for r in m} == set(range(256))
    assert any(4095 in m for m in big.matchers)
    assert t["feat_65536"].n_sigs == 17 and t["feat_65536"].n_reqs == 16
    assert t[mc.SMALLEST].n_sigs == 1


@pytest.mark.parametrize("name", mc.case_ids())
def test_case_is_well_formed(name):
    """What ksim_match_terms validates, so a refusal on the device is never
    the case's fault: offsets from 0 and non-decreasing, ids in range."""
    p = mc.cases()[name]
    for off, val, rows, bound in ((p.sig_off, p.sig_feat, p.n_sigs, p.n_feat),
                                  (p.req_off, p.req_feat, p.n_reqs, p.n_feat),
                                  (p.m_off, p.m_req, p.n_matchers, p.n_reqs)):
        assert off.size == rows + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == val.size
        assert val.size == 0 or (val.min() >= 0 and val.max() < bound)
    assert p.n_reqs <= mc.MAX_REQS and p.n_feat <= mc.MAX_FEAT
    assert p.n_classes == 0 or (p.class_matcher.min() >= 0 and p.class_matcher.max() < p.n_matchers)
    assert p.n_pods == 0 or (0 <= p.pod_sig.min() and p.pod_sig.max() < p.n_sigs and
                             0 <= p.pod_node.min() and p.pod_node.max() < p.n_nodes)


@pytest.mark.parametrize("name", mc.case_ids())
def test_case_is_not_degenerate(name, refs):
    p = mc.cases()[name]
    bits, counts = refs[name]
    assert bits.shape == (p.n_sigs, p.n_matchers) and counts.shape == (p.n_classes, p.n_nodes)
    if p.n_matchers >= 1 and p.n_sigs >= 1:
        for w in range(p.n_words):
            assert bits[:, 32 * w:32 * w + 32].any(), f"matcher word {w} has no set bit in any row"
    if p.n_sigs >= 2 and p.n_matchers >= 1:
        assert bits.any()
        # with no requirement every matcher is empty and matches everything:
        # a clear bit cannot exist there
        assert p.n_reqs == 0 or not bits.all()
    if p.n_classes > 0 and p.n_pods > 0:
        assert counts.sum() > 0
        assert counts[-1].sum() > 0, "the last class (last word, last 256-chunk) counts nothing"
    if p.n_feat >= 1 and name.startswith(("feat_", "sigs_", "reqs_", "matchers_", "classes_")) and name != "reqs_4096":
        held, named = {f for r in p.sigs for f in r}, {f for r in p.reqs for f in r}
        assert {0, p.n_feat - 1} <= held
        assert p.n_reqs == 0 or {0, p.n_feat - 1} <= named


def test_random_content_mix():
    """About 30 % negative requirements, matchers of 0-4 requirements, empty
    requirements of both signs, empty matchers."""
    t = mc.cases()
    neg = np.concatenate([p.neg for n, p in t.items() if n.startswith(("sigs_", "feat_", "matchers_"))])
    assert 0.2 < neg.mean() < 0.4
    p = t["matchers_129"]
    assert {len(m) for m in p.matchers} == {0, 1, 2, 3, 4}
    empty = [(len(r) == 0, int(g)) for r, g in zip(p.reqs, p.neg)]
    assert (True, 0) in empty and (True, 1) in empty
    assert len({c for c in p.class_matcher.tolist() if p.class_matcher.tolist().count(c) > 1}) >= 1


@pytest.mark.parametrize("k", mc.ACC_OVERLAPS)
def test_accumulator_cases_have_the_stated_overlap(k, refs):
    p = mc.cases()[f"acc_{k}"]
    assert mc.overlap(p, 0, 0) == k and mc.overlap(p, 0, 1) == k
    assert p.neg.tolist()[:2] == [0, 1]
    assert mc.overlap(p, 1, 0) == 0 and mc.overlap(p, 2, 0) == 1
    assert int(mc.hits(p)[0, 0]) == k
    bits, _ = refs[f"acc_{k}"]
    assert bits[0, 0] and not bits[0, 1] and not bits[1, 0] and bits[1, 1]


@pytest.mark.parametrize("k", mc.ONE_FEATURE_AT)
def test_one_feature_cases_share_exactly_that_feature(k, refs):
    p = mc.cases()[f"one_feature_at_{k}"]
    fp = max(64, (p.n_feat + 63) // 64 * 64)
    assert mc.ONE_FEATURE_AT[-1] == fp - 1
    assert set(p.sigs[0]) & set(p.reqs[0]) == {k} and set(p.sigs[0]) & set(p.reqs[1]) == {k}
    bits, _ = refs[f"one_feature_at_{k}"]
    assert bits[0, 0] and not bits[0, 1]


def test_duplicate_cases_have_duplicates():
    t = mc.cases()
    p = t["duplicate_features"]
    assert any(len(r) != len(set(r)) for r in p.sigs) and any(len(r) != len(set(r)) for r in p.reqs)
    assert int(mc.hits(p).max()) == 1                    # sets: a repeated id is one feature
    assert any(len(m) != len(set(m)) for m in t["duplicate_requirement"].matchers)


def test_pack_bits_is_the_inverse_of_unpack_bits():
    from ksim.termmatch import unpack_bits
    bits, _ = mc.reference(mc.cases()["matchers_97"])
    w = mc.pack_bits(bits)
    assert w.shape == (bits.shape[0], 4)
    np.testing.assert_array_equal(unpack_bits(w, 97), bits)
    assert not (w[:, 3] >> 1).any()                      # padding bits above matcher 96


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("mutant", list(mc.MUTANTS))
def test_mutant_is_caught_by_its_named_case(mutant, refs):
    """Each faulty restatement differs from the reference on the case
    CAUGHT_BY names (and the full list of catching cases is printed)."""
    catching = [name for name, p in mc.cases().items() if _differs(mc.reference(p, mutant), refs[name])]
    print(f"{mutant} ({mc.MUTANTS[mutant]}): caught by {catching}")
    assert mc.CAUGHT_BY[mutant] in catching


def test_every_mutant_has_a_named_case():
    assert set(mc.CAUGHT_BY) == set(mc.MUTANTS) and len(mc.MUTANTS) == 10
    assert set(mc.CAUGHT_BY.values()) <= set(mc.cases())


def test_reference_agrees_with_the_compiled_matcher_checker():
    """The raw-array reference and tests/test_termmatch.py's NumpyMatcher give
    the same answer on a compiled problem (one restatement, two input forms)."""
    from test_termmatch import NumpyMatcher, _exists_problem
    mp, _, _ = _exists_problem(40)
    rows = lambda off, val: [val[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    p = mc.Problem("compiled", len(mp.feat), rows(mp.sig_off, mp.sig_feat), rows(mp.req_off, mp.req_feat), mp.neg,
                   rows(mp.m_off, mp.m_req), mp.pod_sig, mp.pod_node, mp.n_nodes, mp.class_matcher)
    bits, counts = mc.reference(p)
    hit, cn = NumpyMatcher().match(mp)
    np.testing.assert_array_equal(bits[mp.sig_row], hit)
    np.testing.assert_array_equal(counts, cn)
