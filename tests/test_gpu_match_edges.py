"""ksim_match_terms (csrc/ksim_match.hip) at the edges of its tiles, called
through the C ABI on raw arrays (tests/matchcases.py): every size one side
and the other of the 16-row block, the 16-column requirement tile, the 64-wide
feature step, the 64-matcher ballot and the 256-class block; the accumulator
width; the API limits; the refusals.  The reference is the numpy int64
restatement of the header's formulas, and the results are compared exactly.
tests/test_match_cases.py shows on the CPU that these cases tell a faulty
restatement from the right one."""
import ctypes

import numpy as np
import pytest

import matchcases as mc
from ksim import abi
from ksim.termmatch import unpack_bits

pytestmark = pytest.mark.gpu

GUARD = 64                                   # sentinel words after each output buffer
BITS_FILL = 0xFFFFFFFF
COUNTS_FILL = 0x7F7F7F7F
SENTINEL_U = 0xA5C3F00D
SENTINEL_I = 0x5EEDBEEF


@pytest.fixture(scope="module")
def engine():
    """A bare handle: neither cluster nor profile set (ksim_match_terms needs neither)."""
    from ksim.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    return {}


def _ref(refs, name):
    if name not in refs:
        refs[name] = mc.reference(mc.cases()[name])
    return refs[name]


def call(eng, p, struct=None, with_counts=True):
    """-> (rc, bits words [n_sigs][n_words], counts [n_classes][n_nodes], guards intact).
    The buffers are pre-filled so that a word the call does not write shows."""
    nb, nc = p.n_sigs * p.n_words, p.n_classes * p.n_nodes
    bits = np.full(nb + GUARD, BITS_FILL, np.uint32)
    bits[nb:] = SENTINEL_U
    counts = np.full(nc + GUARD, COUNTS_FILL, np.int32)
    counts[nc:] = SENTINEL_I
    s = p.struct() if struct is None else struct
    rc = eng.L.ksim_match_terms(eng.h, ctypes.byref(s), bits.ctypes.data,
                                counts.ctypes.data if (with_counts and p.n_classes > 0) else None)
    intact = bool((bits[nb:] == SENTINEL_U).all() and (counts[nc:] == SENTINEL_I).all())
    return rc, bits[:nb].reshape(p.n_sigs, p.n_words), counts[:nc].reshape(p.n_classes, p.n_nodes), intact


def check(eng, p, ref):
    rbits, rcounts = ref
    rc, words, counts, intact = call(eng, p)
    assert rc == 0, eng.L.ksim_last_error(eng.h).decode()
    assert intact, "words past the end of an output buffer were written"
    np.testing.assert_array_equal(unpack_bits(words, p.n_matchers), rbits)
    # the padding bits above n_matchers in each row's last word are 0 (whole
    # words are read by the Go binding), so the packed words are equal too
    if p.n_sigs and p.n_matchers % 32:
        assert not (words[:, -1] >> np.uint32(p.n_matchers % 32)).any(), "padding bits set"
    np.testing.assert_array_equal(words, mc.pack_bits(rbits))
    np.testing.assert_array_equal(counts.astype(np.int64), rcounts)


@pytest.mark.parametrize("name", mc.case_ids())
def test_match_case_vs_reference(engine, refs, name):
    check(engine, mc.cases()[name], _ref(refs, name))


def test_small_case_after_large_case_on_one_handle(refs):
    """No state survives a call: the largest case, then the smallest, on a
    fresh handle with neither cluster nor profile."""
    from ksim.engine import Engine
    e = Engine(0)
    try:
        for name in (mc.LARGEST, mc.SMALLEST, "feat_65536", mc.SMALLEST, "classes_513", "matchers_1"):
            check(e, mc.cases()[name], _ref(refs, name))
    finally:
        e.close()


@pytest.mark.parametrize("which", ["reqs", "feat"])
def test_one_past_a_limit_is_unsupported(engine, which):
    p = mc.over_limit_problem(which)
    assert (p.n_reqs, p.n_feat)[which == "feat"] == (mc.MAX_REQS, mc.MAX_FEAT)[which == "feat"] + 1
    rc, words, _, intact = call(engine, p)
    assert rc == abi.E_UNSUPPORTED
    assert intact and (words == BITS_FILL).all()


def test_no_signatures_zero_fills_counts(engine):
    p = mc.Problem("no_sigs", 4, [], [[0], [3]], [0, 1], [[0], [1], []], n_nodes=5, class_matcher=[0, 2, 1])
    rc, _, counts, intact = call(engine, p)
    assert rc == 0 and intact
    assert counts.shape == (3, 5) and not counts.any()


def _base():
    return mc.Problem("refusal_base", 6, [[0, 1], [5]], [[0], [5], []], [0, 1, 0], [[0], [1, 2], []],
                      pod_sig=[0, 1, 1], pod_node=[0, 1, 2], n_nodes=3, class_matcher=[0, 2])


def _with(arr_name, index, value):
    """A copy of the base problem with one array element replaced."""
    p = _base()
    a = getattr(p, arr_name)
    a[index] = value
    return p, p.struct(), True


def _sized(field, value):
    p = _base()
    s = p.struct()
    setattr(s, field, value)
    return p, s, True


def _no_counts():
    p = _base()
    return p, p.struct(), False


REFUSALS = {
    "negative_n_sigs": lambda: _sized("n_sigs", -1),
    "negative_n_feat": lambda: _sized("n_feat", -1),
    "negative_n_reqs": lambda: _sized("n_reqs", -1),
    "negative_n_matchers": lambda: _sized("n_matchers", -1),
    "negative_n_pods": lambda: _sized("n_pods", -1),
    "negative_n_nodes": lambda: _sized("n_nodes", -1),
    "negative_n_classes": lambda: _sized("n_classes", -1),
    "counts_null_with_classes": _no_counts,
    "sig_off0_nonzero": lambda: _with("sig_off", 0, 1),
    "req_off0_nonzero": lambda: _with("req_off", 0, 1),
    "m_off0_nonzero": lambda: _with("m_off", 0, 1),
    "sig_feat_equals_n_feat": lambda: _with("sig_feat", 2, 6),
    "req_feat_equals_n_feat": lambda: _with("req_feat", 1, 6),
    "m_req_equals_n_reqs": lambda: _with("m_req", 0, 3),
    "class_matcher_equals_n_matchers": lambda: _with("class_matcher", 1, 3),
    "pod_sig_equals_n_sigs": lambda: _with("pod_sig", 2, 2),
    "pod_node_equals_n_nodes": lambda: _with("pod_node", 0, 3),
}


def test_refusals_then_a_valid_call(engine, refs):
    null_bits = np.zeros(8, np.uint32)
    p = _base()
    s = p.struct()
    assert engine.L.ksim_match_terms(engine.h, None, null_bits.ctypes.data, None) == abi.E_INVALID
    assert engine.L.ksim_match_terms(engine.h, ctypes.byref(s), None, None) == abi.E_INVALID
    for name, make in REFUSALS.items():
        q, st, with_counts = make()
        rc, words, counts, intact = call(engine, q, st, with_counts)
        assert rc == abi.E_INVALID, name
        assert intact and (words == BITS_FILL).all() and (counts == COUNTS_FILL).all(), name
    # a decreasing offset inside each CSR (the last offset kept, so only the
    # order is wrong)
    for arr, idx, val in (("sig_off", 1, 4), ("req_off", 1, 3), ("m_off", 1, 4)):
        q = _base()
        getattr(q, arr)[idx] = val
        off = getattr(q, arr)
        assert off[0] == 0 and (np.diff(off) < 0).any()
        rc, words, counts, intact = call(engine, q)
        assert rc == abi.E_INVALID, arr
        assert intact and (words == BITS_FILL).all() and (counts == COUNTS_FILL).all(), arr
    # the handle is unharmed
    check(engine, p, mc.reference(p))
    check(engine, mc.cases()["matchers_65"], _ref(refs, "matchers_65"))
