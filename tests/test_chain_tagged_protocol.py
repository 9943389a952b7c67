"""A model check of the batch chain's tagged one-barrier round (ksim_chain.h
chain_block).  tests/test_chain_protocol.py models the protocol before it
(two barriers and two resets per round).

Round r has parity r & 1 and tag r + 1.  A pod registers (tag << 9) | (511 -
pod) in hold[r & 1] by an atomic max, one barrier B(r) follows, and after it
every thread reads its entries' holders (blocked only by a word of this
round's tag and a lower pod; an older word is empty) and, in the same wait,
the previous round's flag first[(r & 1) ^ 1]: no tag of round r - 1 in it
means round r - 1 was a fixpoint and the wave leaves.  Otherwise the wave
reports its first changed pod into first[r & 1], tagged, and registers for
round r + 1.  Nothing is ever reset.  At the cap the last pass is the barrier
and the flag read alone.

The model runs whole rounds: 6 pods, 2 per wave, 3 waves; a wave's segment
between two barriers runs atomically, and after each barrier the segments run
in a chosen wave order.  It is vectorised over the inputs (numpy, one row per
list assignment), because the exhaustive T = 2 set is large: every ordered
pair of distinct nodes out of 4 for each pod, with pod 0's list fixed to
(0, 1) -- node ids are only slot names to the chain, so every other
assignment is a relabelling of one of these 12^5.
"""
import itertools

import numpy as np
import pytest

PODS, WAVES, PER_WAVE = 6, 3, 2
KBP = PODS                     # the model's kBatchPods: "no pod"
NO_CAP = 8                     # never binds: pod i is exact after round i, so 6 pods leave by pass 7
ORDERS = list(itertools.permutations(range(WAVES)))


# ---- inputs -------------------------------------------------------------------
def _pad(lists, t):
    """lists: [n][PODS] tuples of node ids -> (nodes [n, PODS, t] with -1 padding, cnt [n, PODS])."""
    n = len(lists)
    nodes = np.full((n, PODS, t), -1, np.int64)
    cnt = np.zeros((n, PODS), np.int64)
    for x, inst in enumerate(lists):
        for p, lst in enumerate(inst):
            nodes[x, p, :len(lst)] = lst
            cnt[x, p] = len(lst)
    return nodes, cnt


def t2_inputs():
    pairs = np.array(list(itertools.permutations(range(4), 2)), np.int64)       # 12 lists
    idx = np.array(list(itertools.product(range(len(pairs)), repeat=PODS - 1)), np.int64)
    idx = np.concatenate([np.zeros((len(idx), 1), np.int64), idx], axis=1)        # pod 0: (0, 1)
    nodes = pairs[idx]                                                            # [n, PODS, 2]
    cnt = np.full(nodes.shape[:2], 2, np.int64)
    return nodes, cnt


T3_LISTS = [
    # a dependency chain of length 5: pod i moves off node i - 1 in round i - 1
    [(0, 6, 7), (0, 1, 6), (1, 2, 6), (2, 3, 6), (3, 4, 6), (4, 5, 6)],
    # every list alike: pods 3.. run out
    [(0, 1, 2)] * 6,
    # guesses that move forth and back
    [(0, 1, 2), (0, 1, 2), (1, 0, 3), (3, 1, 0), (2, 3, 4), (4, 2, 3)],
    # short lists, one of them exhausted at pod 1
    [(0,), (0,), (0, 1), (1, 0, 2), (2,), (2, 1, 3)],
    # empty lists among full ones
    [(), (5, 4, 3), (), (5, 4, 3), (5, 4, 3), (5, 4, 3)],
    [(7, 0, 1), (7, 0, 1), (0, 7, 1), (1, 0, 7), (1, 2, 7), (2, 1, 0)],
]
# per input: complete[pod]; an incomplete exhausted list inside the prefix cuts the chain
T3_COMPLETE = [
    [True] * 6,
    [True, True, True, True, False, True],     # pod 4 exhausted and incomplete: the cut
    [True] * 6,
    [True, False, True, True, True, True],     # pod 1 exhausted and incomplete
    [False, True, False, True, True, False],   # an empty incomplete list at pod 0
    [True, True, True, False, True, True],
]


# ---- references -----------------------------------------------------------------
def greedy(nodes, cnt):
    """Sequential greedy: pod i takes its first entry that no earlier pod took."""
    n, _, t = nodes.shape
    taken = np.zeros((n, nodes.max() + 2), bool)
    rows = np.arange(n)
    a = np.full((n, PODS), -1, np.int64)
    for p in range(PODS):
        for e in reversed(range(t)):
            free = (e < cnt[:, p]) & ~taken[rows, nodes[:, p, e]]
            a[:, p] = np.where(free, e, a[:, p])
        got = a[:, p] >= 0
        taken[rows[got], nodes[rows[got], p, a[got, p]]] = True
    return a


def jacobi(nodes, cnt, cap):
    """The plain relaxation: every round all pods register, a fresh table per
    round; leave after the first round in which no pod changed, or after cap
    rounds.  Returns (guesses, first of the last round run, rounds run)."""
    n, _, t = nodes.shape
    slots = nodes.max() + 2
    rows = np.arange(n)
    a = np.where(cnt > 0, 0, -1)
    first = np.full(n, KBP, np.int64)
    rounds = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    for r in range(cap):
        hold = np.full((n, slots), KBP, np.int64)
        for p in range(PODS):
            reg = live & (a[:, p] >= 0)
            s = nodes[rows, p, np.maximum(a[:, p], 0)]
            hold[rows[reg], s[reg]] = np.minimum(hold[rows[reg], s[reg]], p)
        na = np.full((n, PODS), -1, np.int64)
        for p in range(PODS):
            for e in reversed(range(t)):
                ok = (e < cnt[:, p]) & (hold[rows, nodes[:, p, e]] >= p)
                na[:, p] = np.where(ok, e, na[:, p])
        chg = na != a
        f = np.where(chg.any(axis=1), chg.argmax(axis=1), KBP)
        first = np.where(live, f, first)
        a = np.where(live[:, None], na, a)
        rounds = np.where(live, r + 1, rounds)
        live = live & (f != KBP)
        if not live.any():
            break
    return a, first, rounds


def prefix(a, first, complete):
    """chain_block's epilogue: nchain = min(first exhausted incomplete pod below first, first, nb)."""
    idx = np.arange(PODS)[None, :]
    cut = (idx < first[:, None]) & (a < 0) & ~complete
    s_cut = np.where(cut.any(axis=1), cut.argmax(axis=1), KBP)
    return np.minimum(np.minimum(s_cut, first), PODS)


# ---- the model --------------------------------------------------------------------
def run(nodes, cnt, order, cap=NO_CAP, variant="tagged"):
    """variant: "tagged" (the protocol), or a mutant: "onetable" (one table for
    both parities), "untagged" (bare pod values in the tables and the flags,
    512 - pod with 0 = empty, never reset), "sameround" (the flag read in the
    round that wrote it, no barrier between).
    Returns (guesses, first per wave, exit pass per wave)."""
    n, _, t = nodes.shape
    slots = int(nodes.max()) + 2                      # the last slot of a row: the padding's
    rows = np.arange(n, dtype=np.int64) * slots
    # flat table index of every list entry, and whether the entry exists
    at = [[rows + np.where(nodes[:, p, e] < 0, slots - 1, nodes[:, p, e]) for e in range(t)] for p in range(PODS)]
    has = [[e < cnt[:, p] for e in range(t)] for p in range(PODS)]
    hold = np.zeros((2, n * slots), np.int32)         # tag 0: the setup clear
    flag = np.zeros((2, n), np.int32)
    a = [np.where(cnt[:, p] > 0, 0, -1).astype(np.int32) for p in range(PODS)]
    live = [np.ones(n, bool) for _ in range(WAVES)]
    exit_pass = np.full((n, WAVES), -1, np.int32)
    first_out = np.full((n, WAVES), KBP, np.int32)
    tab = (lambda par: 0) if variant == "onetable" else (lambda par: par)
    untagged = variant == "untagged"

    def word(r, p):
        return 512 - p if untagged else ((r + 1) << 9) | (511 - p)

    def register(w, r):
        if r >= cap:
            return
        h = hold[tab(r & 1)]
        for p in range(w * PER_WAVE, (w + 1) * PER_WAVE):
            for e in range(t):
                x = at[p][e][live[w] & (a[p] == e)]
                h[x] = np.maximum(h[x], word(r, p))

    def leave(w, r, fl, tag_round):
        changed = fl > 0 if untagged else fl >= ((tag_round + 1) << 9)
        out = live[w] & (~changed | (r == cap))
        first_out[:, w] = np.where(out, np.where(changed, 512 - fl if untagged else 511 - (fl & 511), KBP),
                                   first_out[:, w])
        exit_pass[:, w] = np.where(out, r, exit_pass[:, w])
        live[w] = live[w] & ~out

    def segment(w, r):
        """Wave w between B(r) and B(r + 1)."""
        par = r & 1
        fl = flag[par ^ 1].copy()                      # in the same wait as the table reads
        h = hold[tab(par)]
        na = []
        for p in range(w * PER_WAVE, (w + 1) * PER_WAVE):
            x = np.full(n, -1, np.int32)
            for e in reversed(range(t)):
                x = np.where(has[p][e] & (h[at[p][e]] <= word(r, p)), e, x)
            na.append(x)
        if variant != "sameround" and r >= 1:
            leave(w, r, fl, r - 1)
        if r < cap:
            pod = np.full(n, KBP, np.int32)            # the wave's first changed pod
            for q, p in reversed(list(enumerate(range(w * PER_WAVE, (w + 1) * PER_WAVE)))):
                pod = np.where(na[q] != a[p], p, pod)
                a[p] = np.where(live[w], na[q], a[p])
            rep = live[w] & (pod != KBP)
            flag[par] = np.where(rep, np.maximum(flag[par], word(r, pod)), flag[par])
        if variant == "sameround":
            leave(w, r + 1, flag[par].copy(), r)
        register(w, r + 1)

    for w in order:                                    # kernel start .. B(0)
        register(w, 0)
    r = 0
    while any(m.any() for m in live):
        for w in order:
            segment(w, r)
        r += 1
        assert r <= cap + 1
    return np.stack(a, axis=1), first_out, exit_pass


_REF = {}


def reference(nodes, cnt, cap):
    """The references of one input set, computed once and shared (read only)."""
    key = (id(nodes), cap)
    if key not in _REF:
        _REF[key] = jacobi(nodes, cnt, cap) + (greedy(nodes, cnt),)
    return _REF[key]


def agrees(nodes, cnt, complete, order, cap, variant="tagged"):
    """Per input: every wave leaves in the same pass, one pass after the
    reference's last round; first is the reference's; the guesses below the
    prefix are the sequential greedy's (all of them at a fixpoint)."""
    a, first, ex = run(nodes, cnt, order, cap, variant)
    ra, rfirst, rrounds, g = reference(nodes, cnt, cap)
    ok = (ex == ex[:, :1]).all(axis=1) & (first == first[:, :1]).all(axis=1)
    ok &= (ex[:, 0] == rrounds) & (first[:, 0] == rfirst) & (a == ra).all(axis=1)
    nchain = prefix(a, first[:, 0], complete)
    ok &= nchain == prefix(ra, rfirst, complete)
    below = np.arange(PODS)[None, :] < nchain[:, None]
    ok &= ((a == g) | ~below).all(axis=1)
    ok &= ((rfirst != KBP) | (ra == g).all(axis=1))   # the reference itself: a fixpoint is the greedy
    return ok


@pytest.fixture(scope="module")
def t2():
    nodes, cnt = t2_inputs()
    # the loop does not read `complete`: pods 1, 2 and 5 incomplete exercises the cut
    complete = np.ones(cnt.shape, bool)
    complete[:, [1, 2, 5]] = False
    return nodes, cnt, complete


@pytest.fixture(scope="module")
def t3():
    nodes, cnt = _pad(T3_LISTS, 3)
    return nodes, cnt, np.array(T3_COMPLETE, bool)


def test_references_see_the_chain_and_the_cut(t3):
    nodes, cnt, complete = t3
    a, first, rounds = jacobi(nodes, cnt, NO_CAP)
    assert rounds[0] == 6 and first[0] == KBP          # five dependent moves, then the fixpoint round
    assert rounds.max() < NO_CAP
    assert (a == greedy(nodes, cnt)).all()
    assert prefix(a, first, complete).tolist()[:5] == [6, 4, 6, 1, 0]
    a2, first2, rounds2 = jacobi(nodes, cnt, 2)
    assert rounds2[0] == 2 and first2[0] == 2          # cut short: pods 0 and 1 exact


@pytest.mark.parametrize("cap", [NO_CAP, 2, 3])
@pytest.mark.parametrize("order", ORDERS)
def test_tagged_protocol_t3(t3, order, cap):
    assert agrees(*t3, order, cap).all()


@pytest.mark.parametrize("cap", [NO_CAP, 2, 3])
@pytest.mark.parametrize("order", ORDERS)
def test_tagged_protocol_every_t2_assignment(t2, order, cap):
    ok = agrees(*t2, order, cap)
    assert ok.all(), (t2[0][~ok][0].tolist(), order, cap)


@pytest.mark.parametrize("variant", ["onetable", "untagged", "sameround"])
def test_mutants_fail(t2, t3, variant):
    """Each mutant breaks under at least one wave order (else the model proves nothing)."""
    failed = [(order, t) for order in ORDERS for t, inp in (("t3", t3), ("t2", t2))
              if t == "t3" or order == ORDERS[0] or order == ORDERS[-1]
              if not agrees(*inp, order, NO_CAP, variant).all()]
    assert failed, variant
