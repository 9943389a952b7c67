"""Raw ``ksim_match_problem`` inputs at the edges of csrc/ksim_match.hip, and
the reference they are checked against (tests/test_match_cases.py on the CPU,
tests/test_gpu_match_edges.py on the device).

The problems are numpy CSR arrays handed straight to the C ABI: nothing here
goes through ksim.termmatch.MatchProblem, whose compiler de-duplicates
requirements and signature rows and so never lets a test choose n_sigs,
n_feat, n_reqs, n_matchers or n_classes.  ``reference`` is a dense restatement
in numpy int64 of the three formulas of include/ksim_engine.h
(hits / match / counts); ``MUTANTS`` are the same restatement with one fault
each, standing in for kernel faults on the CPU only.

The kernel's geometry the sizes are chosen against: 16 signatures per block,
16 requirement columns per tile with 4 waves striding the tiles, 64 features
per MFMA step (fp = features padded to 64, floor 64; rp = requirements padded
to 16, floor 16), 64 matchers per ballot (two 32-bit words), 256 classes per
class block (32 per word)."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ksim import abi

MAX_REQS = 4096
MAX_FEAT = 65536


def _csr(rows: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(rows) + 1, np.int32)
    if len(rows):
        off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.fromiter((x for r in rows for x in r), np.int32, int(off[-1]))
    return off, flat


def _p(a: Optional[np.ndarray]):
    return a.ctypes.data if a is not None and a.size else None


class Problem:
    """One ksim_match_problem: the numpy arrays (kept alive here) and the struct."""

    def __init__(self, name: str, n_feat: int, sigs, reqs, neg, matchers, pod_sig=(), pod_node=(), n_nodes=0,
                 class_matcher=()):
        self.name = name
        self.n_feat = int(n_feat)
        self.sigs = [list(map(int, r)) for r in sigs]
        self.reqs = [list(map(int, r)) for r in reqs]
        self.matchers = [list(map(int, r)) for r in matchers]
        self.sig_off, self.sig_feat = _csr(self.sigs)
        self.req_off, self.req_feat = _csr(self.reqs)
        self.neg = np.ascontiguousarray(neg, np.uint8).reshape(-1)
        self.m_off, self.m_req = _csr(self.matchers)
        self.pod_sig = np.ascontiguousarray(pod_sig, np.int32).reshape(-1)
        self.pod_node = np.ascontiguousarray(pod_node, np.int32).reshape(-1)
        self.class_matcher = np.ascontiguousarray(class_matcher, np.int32).reshape(-1)
        self.n_nodes = int(n_nodes)
        assert len(self.reqs) == self.neg.size and self.pod_sig.size == self.pod_node.size

    n_sigs = property(lambda self: len(self.sigs))
    n_reqs = property(lambda self: len(self.reqs))
    n_matchers = property(lambda self: len(self.matchers))
    n_pods = property(lambda self: int(self.pod_sig.size))
    n_classes = property(lambda self: int(self.class_matcher.size))
    n_words = property(lambda self: (len(self.matchers) + 31) // 32)

    def struct(self) -> abi.MatchProblem:
        """The C struct over this object's arrays (always non-NULL offset
        arrays; empty value arrays are NULL, as ksim.termmatch passes them)."""
        s = abi.MatchProblem()
        s.n_sigs, s.n_feat, s.n_reqs, s.n_matchers = self.n_sigs, self.n_feat, self.n_reqs, self.n_matchers
        s.sig_feat_off, s.sig_feat = self.sig_off.ctypes.data, _p(self.sig_feat)
        s.req_feat_off, s.req_feat = self.req_off.ctypes.data, _p(self.req_feat)
        s.req_neg, s.m_req_off, s.m_req = _p(self.neg), self.m_off.ctypes.data, _p(self.m_req)
        s.n_pods, s.n_nodes, s.n_classes = self.n_pods, self.n_nodes, self.n_classes
        s.pod_sig, s.pod_node, s.class_matcher = _p(self.pod_sig), _p(self.pod_node), _p(self.class_matcher)
        return s


# ---- the reference and its mutants ------------------------------------------------
MUTANTS = {
    "int8_accumulator": "hits accumulated modulo 256 as int8",
    "odd_words_dropped": "matcher words with an odd index dropped",
    "neg_ignored": "the negative flag ignored",
    "first_64_reqs": "only the first 64 requirements evaluated",
    "first_64_feats": "only the first 64 features evaluated",
    "rows_mod_16": "rows past the first 16 treated as row s % 16",
    "classes_below_256": "only classes < 256 counted",
    "last_class_word_cleared": "the last class word cleared",
    "empty_matches_nothing": "an empty matcher matches nothing",
    "pair_counted_once": "each (signature, node) pair counted once, not once per pod",
}


def hits(p: Problem) -> np.ndarray:
    """hits[s][r] = |features(s) & features(r)| as int64 (feature SETS: an id
    listed twice in a CSR row is one feature)."""
    nf = max(p.n_feat, 1)
    a = np.zeros((p.n_sigs, nf), np.int64)
    for s, f in enumerate(p.sigs):
        a[s, f] = 1
    b = np.zeros((nf, p.n_reqs), np.int64)
    for r, f in enumerate(p.reqs):
        b[f, r] = 1
    return a @ b


def reference(p: Problem, mutant: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(bits bool [n_sigs][n_matchers], counts int64 [n_classes][n_nodes]) by
    the formulas of include/ksim_engine.h; ``mutant`` names one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    h = hits(p)
    if mutant == "first_64_feats":
        q = Problem(p.name, p.n_feat, [[f for f in r if f < 64] for r in p.sigs], p.reqs, p.neg, p.matchers)
        h = hits(q)
    if mutant == "int8_accumulator":
        h = h.astype(np.int8).astype(np.int64)
    neg = p.neg.astype(bool)[None, :]
    sat = (h > 0) if mutant == "neg_ignored" else ((h > 0) != neg)
    if mutant == "first_64_reqs":
        sat[:, 64:] = True                               # never looked at: cannot fail a matcher
    bits = np.ones((p.n_sigs, p.n_matchers), bool)
    for m, reqs in enumerate(p.matchers):
        for r in reqs:
            bits[:, m] &= sat[:, r]
        if mutant == "empty_matches_nothing" and not reqs:
            bits[:, m] = False
    if mutant == "odd_words_dropped":
        bits[:, (np.arange(p.n_matchers) >> 5) & 1 == 1] = False
    if mutant == "rows_mod_16":
        bits = bits[np.arange(p.n_sigs) % 16]
    counts = np.zeros((p.n_classes, p.n_nodes), np.int64)
    for c, m in enumerate(p.class_matcher):
        on = bits[p.pod_sig, m] if p.n_pods else np.zeros(0, bool)
        if mutant == "pair_counted_once":
            for s, node in set(zip(p.pod_sig[on].tolist(), p.pod_node[on].tolist())):
                counts[c, node] += 1
        else:
            np.add.at(counts[c], p.pod_node[on], 1)
    if mutant == "classes_below_256":
        counts[256:] = 0
    if mutant == "last_class_word_cleared" and p.n_classes:
        counts[(p.n_classes - 1) // 32 * 32:] = 0
    return bits, counts


def overlap(p: Problem, s: int, r: int) -> int:
    return len(set(p.sigs[s]) & set(p.reqs[r]))


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """bool [rows][n] -> u32 [rows][ceil(n / 32)], padding bits 0."""
    rows, n = bits.shape
    w = (n + 31) // 32
    pad = np.zeros((rows, w * 32), np.uint8)
    pad[:, :n] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u4").reshape(rows, w) if w else np.zeros((rows, 0), np.uint32)


# ---- seeded-random content ---------------------------------------------------------
def _draw_feats(rng, n_feat: int, k: int) -> List[int]:
    """k feature ids: mostly from a few hot features so requirements and
    signatures meet often enough, the rest uniform over the vocabulary."""
    if n_feat == 0 or k == 0:
        return []
    hot = min(n_feat, 8)
    out = [int(rng.integers(hot)) if rng.random() < 0.7 else int(rng.integers(n_feat)) for _ in range(k)]
    return sorted(set(out))


def random_problem(name: str, seed: int, n_sigs=20, n_feat=40, n_reqs=24, n_matchers=40, n_classes=12, n_pods=200,
                   n_nodes=7, pod_node=None, all_words=True) -> Problem:
    """Seeded-random content: about 30 % negative requirements, matchers of 0-4
    requirements, a few requirements naming no feature (positive: never
    satisfied; negative: always), a few empty matchers (match everything).
    For n_feat >= 1 the feature ids 0 and n_feat - 1 are each named by a
    requirement and held by a signature.  ``all_words``: every matcher word
    gets a set bit in some row, and (with a requirement to fail) some bit of
    the matrix is clear."""
    rng = np.random.default_rng(seed)
    sigs = [_draw_feats(rng, n_feat, int(rng.integers(0, 7))) for _ in range(n_sigs)]
    reqs = [_draw_feats(rng, n_feat, int(rng.integers(1, 4))) for _ in range(n_reqs)]
    neg = (rng.random(n_reqs) < 0.3).astype(np.uint8)
    if n_reqs >= 6:                                      # requirements naming no feature, both signs
        a, b = 2, n_reqs - 3
        reqs[a], neg[a] = [], 0
        reqs[b], neg[b] = [], 1
    if n_feat >= 1:
        if n_reqs >= 1:
            reqs[0] = sorted(set(reqs[0]) | {0})
            reqs[-1] = sorted(set(reqs[-1]) | {n_feat - 1})
        if n_sigs >= 1:
            sigs[0] = sorted(set(sigs[0]) | {0})
            sigs[-1] = sorted(set(sigs[-1]) | {n_feat - 1})
    matchers = []
    for m in range(n_matchers):
        k = int(rng.integers(0, 5)) if n_reqs else 0
        matchers.append([int(x) for x in rng.integers(0, max(n_reqs, 1), k)])
    for m in range(5, n_matchers, 29):                   # a few with no requirement at all
        matchers[m] = []
    if n_reqs and n_matchers:                            # the edge requirements are in use
        matchers[0] = [0]
        matchers[-1] = sorted(set(matchers[-1]) | {n_reqs - 1})
    cm = rng.integers(0, max(n_matchers, 1), n_classes).astype(np.int32) if n_matchers else np.zeros(0, np.int32)
    if cm.size >= 2:
        cm[1] = cm[0]                                    # classes sharing one matcher
    np_ = n_pods if (n_sigs and n_nodes and cm.size) else 0
    ps = rng.integers(0, max(n_sigs, 1), np_).astype(np.int32)
    pn = rng.integers(0, max(n_nodes, 1), np_).astype(np.int32) if pod_node is None else np.full(np_, pod_node, np.int32)
    p = Problem(name, n_feat, sigs, reqs, neg, matchers, ps, pn, n_nodes, cm)
    if not (all_words and n_sigs and n_matchers):
        return p
    # non-degeneracy fix-ups, decided by the reference alone
    bits, _ = reference(p)
    changed = False
    for w in range(p.n_words):
        if not bits[:, 32 * w:32 * w + 32].any():
            matchers[min(32 * w + 7, n_matchers - 1)] = []
            changed = True
    if n_reqs and bits.all():
        reqs[0], neg[0] = [], 0                          # a positive requirement naming no feature: never
        if n_feat >= 1:
            reqs[-1] = sorted(set(reqs[-1]) | {0})       # feature 0 stays named
        matchers[0] = [0]
        changed = True
    if changed:
        p = Problem(name, n_feat, sigs, reqs, neg, matchers, ps, pn, n_nodes, cm)
        bits, _ = reference(p)
    if cm.size and np_:                                  # the last class (its word, its 256-chunk) counts something
        live = np.flatnonzero(bits[ps].any(axis=0))
        if live.size and not bits[ps, cm[-1]].any():
            cm[-1] = live[-1]
            p = Problem(name, n_feat, sigs, reqs, neg, matchers, ps, pn, n_nodes, cm)
    return p


# ---- hand-made cases ---------------------------------------------------------------
ACC_OVERLAPS = (127, 128, 255, 256, 300)


def accumulator_problem(k: int) -> Problem:
    """Signature 0 shares exactly ``k`` features with requirement 0 (positive)
    and with requirement 1 (negative); an 8-bit accumulator reads 128 as -128,
    255 as -1 and 256 as 0.  Signature 1 shares none, signature 2 one."""
    n_feat = k + 24
    shared = list(range(k))
    rest = list(range(k, k + 10))                        # named by the requirements, not held by signature 0
    sigs = [shared + [k + 20], [k + 21, k + 23], [k + 3, k + 22], shared[:k // 2]]
    reqs = [shared + rest, shared + rest, [k + 23]]
    neg = [0, 1, 0]
    matchers = [[0], [1], [0, 2], []]
    ps = np.arange(40) % 4
    pn = np.arange(40) % 3
    return Problem(f"acc_{k}", n_feat, sigs, reqs, neg, matchers, ps, pn, 3, [0, 1, 2, 3, 1])


ONE_FEATURE_AT = (0, 15, 16, 63, 64, 127)                # 127 = fp - 1 at n_feat = 128


def one_feature_problem(k: int) -> Problem:
    """n_feat = 128 (fp = 128, two MFMA steps): signature 0 and requirements
    0 (positive) / 1 (negative) share exactly feature ``k``: one byte of one
    lane's 16-byte slice decides the row."""
    n_feat = 128
    others = [f for f in range(n_feat) if f != k]
    sigs = [[k] + others[0:40:2], others[1:41:2], [], others[60:70]]
    reqs = [[k] + others[1:41:2][:8], [k] + others[1:41:2][:8], [others[61]]]
    neg = [0, 1, 0]
    matchers = [[0], [1], [2], [0, 1]]
    ps = np.arange(24) % 4
    pn = np.arange(24) % 2
    return Problem(f"one_feature_at_{k}", n_feat, sigs, reqs, neg, matchers, ps, pn, 2, [0, 1, 2])


def reqs_4096_problem() -> Problem:
    """n_reqs = 4096, 16 signatures: requirement r is positive over feature
    r % 48 (negative for r % 5 == 0); matcher i < 256 needs requirement
    16 i + i % 16, so every one of the 256 LDS ``sat`` words of a row is read,
    and the last matchers need requirement 4095."""
    n_feat, n_reqs, n_sigs = 48, MAX_REQS, 16
    rng = np.random.default_rng(4096)
    sigs = [sorted(set(int(x) for x in rng.integers(0, n_feat, 20))) for _ in range(n_sigs)]
    sigs[0] = sorted(set(sigs[0]) | {0})
    sigs[-1] = sorted(set(sigs[-1]) | {n_feat - 1})
    reqs = [[r % n_feat] for r in range(n_reqs)]
    neg = [1 if r % 5 == 0 else 0 for r in range(n_reqs)]
    matchers = [[16 * i + i % 16] for i in range(256)]
    matchers += [[4095], [4095, 0], [4094, 4095, 17], []]
    matchers += [[int(x) for x in rng.integers(0, n_reqs, 3)] for _ in range(40)]
    ps = rng.integers(0, n_sigs, 300)
    pn = rng.integers(0, 5, 300)
    return Problem("reqs_4096", n_feat, sigs, reqs, neg, matchers, ps, pn, 5, rng.integers(0, len(matchers), 20))


def feat_65536_problem() -> Problem:
    """n_feat = 65536 (1,024 MFMA steps), 17 signatures (a second block with one
    live row), 16 requirements; features 0 and 65535 are live."""
    p = random_problem("feat_65536", 65536, n_sigs=17, n_feat=MAX_FEAT, n_reqs=16, n_matchers=20)
    assert 0 in p.sigs[0] and MAX_FEAT - 1 in p.sigs[-1] and 0 in p.reqs[0] and MAX_FEAT - 1 in p.reqs[-1]
    return p


def over_limit_problem(which: str) -> Problem:
    """One past a limit, otherwise valid: KSIM_E_UNSUPPORTED."""
    if which == "reqs":
        return Problem("reqs_4097", 4, [[0]], [[r % 4] for r in range(MAX_REQS + 1)], [0] * (MAX_REQS + 1), [[MAX_REQS]])
    return Problem("feat_65537", MAX_FEAT + 1, [[MAX_FEAT]], [[MAX_FEAT]], [0], [[0]])


def duplicate_feature_problem() -> Problem:
    """Feature ids listed more than once within a CSR row (signatures and
    requirements): sets, not multisets."""
    sigs = [[3, 3, 3, 5], [5, 5], [7, 1, 7], []]
    reqs = [[3, 3], [5, 5, 5, 9], [7, 7], [1, 1]]
    neg = [0, 1, 0, 1]
    matchers = [[0], [1], [2, 3], [0, 1], []]
    return Problem("duplicate_features", 10, sigs, reqs, neg, matchers, np.arange(12) % 4, np.arange(12) % 2, 2,
                   [0, 1, 2, 3, 4])


def duplicate_requirement_problem() -> Problem:
    """The same requirement listed twice in one matcher."""
    sigs = [[0, 1], [1], [2], []]
    reqs = [[0], [1], [2]]
    neg = [0, 0, 1]
    matchers = [[0, 0], [1, 2, 1], [2, 2, 2, 2], [0, 1, 0, 1]]
    return Problem("duplicate_requirement", 3, sigs, reqs, neg, matchers, np.arange(12) % 4, np.arange(12) % 3, 3,
                   [0, 1, 2, 3])


SIG_SIZES = (1, 15, 16, 17, 33)
FEAT_SIZES = (0, 1, 63, 64, 65, 129)
REQ_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 81)
MATCHER_SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97, 129)
CLASS_SIZES = (0, 1, 31, 32, 33, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Problem]:
    """The case table: id -> Problem (built once, never modified)."""
    out: List[Problem] = []
    seed = 1000
    for n in SIG_SIZES:
        out.append(random_problem(f"sigs_{n}", seed + n, n_sigs=n))
    for n in FEAT_SIZES:
        out.append(random_problem(f"feat_{n}", seed + 100 + n, n_feat=n))
    for n in REQ_SIZES:
        # more requirements per matcher would not reach the high tiles more
        # often; more matchers do
        out.append(random_problem(f"reqs_{n}", seed + 200 + n, n_reqs=n, n_matchers=max(40, 2 * n)))
    for n in MATCHER_SIZES:
        out.append(random_problem(f"matchers_{n}", seed + 300 + n, n_matchers=n, n_classes=12 if n else 0))
    for n in CLASS_SIZES:
        out.append(random_problem(f"classes_{n}", seed + 400 + n, n_classes=n, n_sigs=20, n_pods=300))
    out.append(random_problem("classes_no_pods", seed + 500, n_classes=40, n_pods=0))
    out.append(random_problem("one_node", seed + 501, n_nodes=1))
    out.append(random_problem("hot_node_5000", seed + 502, n_sigs=6, n_nodes=4, n_pods=5000, pod_node=3, n_classes=40))
    out.extend(accumulator_problem(k) for k in ACC_OVERLAPS)
    out.extend(one_feature_problem(k) for k in ONE_FEATURE_AT)
    out.append(reqs_4096_problem())
    out.append(feat_65536_problem())
    out.append(duplicate_feature_problem())
    out.append(duplicate_requirement_problem())
    table = {p.name: p for p in out}
    assert len(table) == len(out)
    return table


def case_ids() -> List[str]:
    return list(cases())


SMALLEST = "sigs_1"
LARGEST = "reqs_4096"

# the case each mutant is caught by (tests/test_match_cases.py asserts it)
CAUGHT_BY = {
    "int8_accumulator": "acc_128",
    "odd_words_dropped": "matchers_33",
    "neg_ignored": "acc_127",
    "first_64_reqs": "reqs_65",
    "first_64_feats": "one_feature_at_64",
    "rows_mod_16": "sigs_17",
    "classes_below_256": "classes_257",
    "last_class_word_cleared": "classes_33",
    "empty_matches_nothing": "reqs_0",
    "pair_counted_once": "hot_node_5000",
}
