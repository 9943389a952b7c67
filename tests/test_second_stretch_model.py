"""The deferred-commit batch's commit rule with the second stretch, as a small
reference over an abstract key function (no GPU, no engine).

A batch starts from snapshot S.  Every pod takes its top-T list under S; the
chain gives pod j the first entry of its list that no earlier pod guessed
(g_j, key G_j); M_j is the maximum over k < j of key_j(S[g_k] + pod k).  The
first cut i* is the first j with M_j > G_j: pods below it commit on their
guesses, i* on n* = node(M_i*) = g_k*.  The stretch then goes on: pod j > i*
keeps its guess while max(M_j, D_j, F_j) <= G_j, with D_j = key_j(S[n*] + pod k*
+ pod i*) and F_j = key_j(S[f]), f = g_i* (which holds nobody); the batch ends
before the first j where that fails (i2), and the next batch starts there.

The rule must place every pod where pod-by-pod greedy placement does, on every
scene; three mutants of it (no F, the stale single-pod key for D, i2 committed
on its guess too) must each fail somewhere; and the scene set must reach every
way a stretch can end.  The key is deliberately not monotone in a node's load
(a balance term), as BalancedAllocation is not: a stale pair key may lie on
either side of the true one."""
import numpy as np
import pytest

T = 8
MIX = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def _hash(a, b):
    x = ((a + 1) * MIX ^ (b + 0x1234567) * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 31
    x = (x * 0x94D049BB133111EB) & MASK
    return (x >> 40) & 0xFFFF


class Scene:
    def __init__(self, seed):
        r = np.random.default_rng(seed)
        self.n = int(r.integers(8, 65))
        self.p = int(r.integers(40, 301))
        self.alloc = np.stack([r.choice([8, 16, 32], self.n), r.choice([16, 32, 64], self.n)], 1).astype(np.int64)
        self.used0 = (self.alloc * r.uniform(0, 0.5, (self.n, 2))).astype(np.int64)
        self.req = np.stack([r.integers(0, 5, self.p), r.integers(0, 9, self.p)], 1).astype(np.int64)
        self.cap = r.integers(3, 12, self.n)           # pods per node
        self.cnt0 = np.zeros(self.n, np.int64)

    def key(self, j, node, used, cnt):
        """Pod j's key on a node with the given load: 0 infeasible, else unique per node."""
        a, q = self.alloc[node], self.req[j]
        if cnt >= self.cap[node] or np.any(used + q > a):
            return 0
        fc, fm = (used[0] + q[0]) / a[0], (used[1] + q[1]) / a[1]
        least = int((1 - fc) * 50 + (1 - fm) * 50) // 2
        bal = int((1 - abs(fc - fm) / 2) * 100)
        return ((least + bal) << 24) | (_hash(j, node) << 8) | (255 - node)


def node_of(k):
    return 255 - (k & 0xFF)


def greedy(sc):
    used, cnt = sc.used0.copy(), sc.cnt0.copy()
    out = []
    for j in range(sc.p):
        ks = [sc.key(j, n, used[n], cnt[n]) for n in range(sc.n)]
        best = max(ks)
        if best == 0:
            out.append(-1)
            continue
        n = node_of(best)
        used[n] += sc.req[j]
        cnt[n] += 1
        out.append(n)
    return out


def batched(sc, B, mutant=None, events=None):
    """Placements by the batch rule.  mutant: None, "noF", "staleD", "commit_i2".
    events: a dict of counters of the ways the batches ended."""
    used, cnt = sc.used0.copy(), sc.cnt0.copy()
    out = [None] * sc.p
    cur, batches = 0, 0

    def ev(name):
        if events is not None:
            events[name] = events.get(name, 0) + 1

    def bind(j, n):
        out[j] = n
        if n >= 0:
            used[n] += sc.req[j]
            cnt[n] += 1

    while cur < sc.p:
        batches += 1
        nb = min(B, sc.p - cur)
        S_used, S_cnt = used.copy(), cnt.copy()

        def skey(j, n, extra=()):                      # pod cur + j on node n at S plus the pods in extra
            u, c = S_used[n].copy(), S_cnt[n]
            for k in extra:
                u += sc.req[cur + k]
                c += 1
            return sc.key(cur + j, n, u, c)

        # lists, chain
        g, taken, nchain = [], set(), nb
        for j in range(nb):
            ks = sorted((k for k in (skey(j, n) for n in range(sc.n)) if k), reverse=True)
            complete = len(ks) <= T
            mine = next((k for k in ks[:T] if node_of(k) not in taken), 0)
            if mine == 0 and not complete:
                nchain = j
                break
            g.append(mine)
            if mine:
                taken.add(node_of(mine))
        assert nchain >= 1
        M = [max([skey(j, node_of(g[k]), (k,)) for k in range(j) if g[k]], default=0) for j in range(nchain)]
        istar = next((j for j in range(nchain) if M[j] > g[j]), nchain)
        for j in range(min(istar, nchain)):
            bind(cur + j, node_of(g[j]) if g[j] else -1)
        committed = nchain
        if istar < nchain:
            nstar = node_of(M[istar])
            kstar = next(k for k in range(istar) if g[k] and node_of(g[k]) == nstar)
            bind(cur + istar, nstar)
            f = node_of(g[istar]) if g[istar] else -1
            committed = istar + 1
            if istar == nchain - 1:
                ev("no_stretch")
            i2 = nchain
            for j in range(istar + 1, nchain):
                D = skey(j, nstar, (kstar,) if mutant == "staleD" else (kstar, istar))
                F = skey(j, f) if f >= 0 and mutant != "noF" else 0
                if max(M[j], D, F) > g[j]:
                    i2 = j
                    sole = [x for x, v in (("M", M[j]), ("D", D), ("F", F)) if v > g[j]]
                    if len(sole) == 1:
                        ev("ended_by_" + sole[0])
                    if j == istar + 1:
                        ev("zero_length")
                    break
            else:
                if istar + 1 < nchain:
                    ev("ran_to_nchain")
            for j in range(istar + 1, i2):
                bind(cur + j, node_of(g[j]) if g[j] else -1)
                if not g[j]:
                    ev("unschedulable_inside")
            committed = i2
            if mutant == "commit_i2" and i2 < nchain:
                bind(cur + i2, node_of(g[i2]) if g[i2] else -1)
                committed = i2 + 1
        cur += committed
    return out, batches


SEEDS = range(12)
BS = (256, 24)                                          # one batch holds most scenes; several batches chain
_SCENES, _RUNS = {}, {}


def _scene(seed):
    if seed not in _SCENES:
        sc = Scene(seed)
        _SCENES[seed] = (sc, greedy(sc))
    return _SCENES[seed]


def _run(seed, B):
    """The rule's placements and end events on a scene, computed once."""
    if (seed, B) not in _RUNS:
        events = {}
        got, _ = batched(_scene(seed)[0], B, events=events)
        _RUNS[(seed, B)] = (got, events)
    return _RUNS[(seed, B)]


@pytest.mark.parametrize("B", BS)
def test_rule_equals_greedy(B):
    for seed in SEEDS:
        assert _run(seed, B)[0] == _scene(seed)[1], (seed, B)


@pytest.mark.parametrize("mutant", ["noF", "staleD", "commit_i2"])
def test_mutants_fail(mutant):
    for seed in SEEDS:
        for B in BS:
            if batched(_scene(seed)[0], B, mutant)[0] != _scene(seed)[1]:
                print(mutant, "differs from greedy on scene", seed, "B", B)
                return
    pytest.fail(f"mutant {mutant} placed every scene as greedy does")


def test_scene_set_reaches_every_end():
    events = {}
    for seed in SEEDS:
        for B in BS:
            for k, v in _run(seed, B)[1].items():
                events[k] = events.get(k, 0) + v
    print(events)
    for name in ("ended_by_M", "ended_by_D", "ended_by_F", "ran_to_nchain", "no_stretch", "zero_length"):
        assert events.get(name, 0) > 0, (name, events)
