"""The image scenes of tests/imagecases.py on the CPU: the C oracle runs every
scene, the image classes take the scores the scenes claim, every pod that must
be an image pod is one, and each wrong reading of imagecases.FAULTS, run
through the same oracle, moves a placement of some scene (so a batch path that
read the image part that way would fail tests/test_gpu_image_batch.py)."""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle

import imagecases as ic

PCTS = (100, 0)


def _schedule(cluster, pods, prof, first=0, count=None, ora=None):
    o = ora or Oracle(cluster.copy_state(), prof)
    chosen, _ = o.schedule(pods, first, count)
    if ora is None:
        o.close()
    return chosen.copy()


@functools.lru_cache(maxsize=None)
def _right(name, pct):
    s = ic.scene(name)
    return _schedule(*s.encoded, s.compiled(pct))


@pytest.mark.parametrize("name", ic.SCENES)
def test_scene_takes_its_scores(name):
    """The image rows hold finished scores in 0..100, each claimed value on
    some node, and the queue's pods are image pods (one use, of kind image)
    where the scene pins a route."""
    s = ic.scene(name)
    cluster, pods = s.encoded
    rows = ic.image_rows(cluster)
    assert rows, name
    vals = set()
    for r in rows:
        row = cluster.class_count[r]
        assert row.min() >= 0 and row.max() <= 100, (name, r)
        vals |= set(int(v) for v in row)
    for v in s.scores:
        assert v in vals, (name, v, sorted(vals))
    img = ic.image_pods(pods)
    if s.route is not None:
        assert img.all(), name
    else:
        assert img.any() and not img.all(), name
    assert (_right(name, 100) >= 0).all(), name          # every pod is placed


def test_score_values_exact():
    """0, 1, 63, 64, 99 and 100 through the 23 MB floor and the 1000 MB x
    containers ceiling, by the formula and in the encoded rows."""
    assert ic.image_score(ic.MIN_T) == 0 and ic.image_score(ic.MIN_T - 1) == 0
    assert ic.image_score(ic.MAX_T) == 100 and ic.image_score(ic.MAX_T + 1) == 100
    assert ic.image_score(2 * ic.MAX_T - 1, 2) == 99 and ic.image_score(3 * ic.MAX_T, 3) == 100
    for sc in (1, 63, 64, 99, 100):
        for k in (1, 2, 3):
            size = ic.size_for(sc, 2, 12, k)
            assert ic.image_score(int(float(size) * (2.0 / 12.0)), k) == sc
            assert ic.image_score(int(float(size - 1) * (2.0 / 12.0)), k) == sc - 1
    cluster, pods = ic.scene("score_values").encoded
    by_names = {key[1]: cid for key, cid in cluster.topo.ids.items() if key[0] == "image"}
    want = {("reg.io/one:v1",): {0, 1}, ("reg.io/lo:v1",): {0, 63}, ("reg.io/hi:v1",): {0, 64},
            ("reg.io/most:v1",): {0, 99}, ("reg.io/full:v1",): {0, 100}}
    for names, vals in want.items():
        assert set(int(v) for v in cluster.class_count[by_names[names]]) == vals, names
    # two containers: the same sums against the 2000 MB ceiling
    pair = cluster.class_count[by_names[("reg.io/pa:latest", "reg.io/pb:latest")]]
    assert int(pair[10]) == 99 and int(pair[11]) == 64 and int(pair[:10].max()) == 0
    # an unlisted image beside a listed one adds nothing, and counts as a container
    half = cluster.class_count[by_names[("reg.io/pa:latest", "reg.io/nowhere:latest")]]
    assert int(half[10]) == 99 and int(half.sum()) == 99
    three = cluster.class_count[by_names[("reg.io/nowhere:latest", "reg.io/full:v1", "other.io/nowhere:latest")]]
    assert 0 < int(three[8]) < 100 and int(three[8]) == ic.image_score(
        int(float(ic.size_for(100, 2, 12)) * (2.0 / 12.0)), 3)


def test_ties_are_broken_by_the_hash():
    """Equal image scores on equal nodes: the first pods do not all land on
    node 0, and the image term changes nothing there."""
    s = ic.scene("ties")
    a = _right("ties", 100)
    assert len(set(int(x) for x in a[:9])) > 3
    b = _schedule(*s.encoded, s.compiled(100, ic.make_profile(None)))
    np.testing.assert_array_equal(a, b)


def test_preference_moves_off_the_full_holders():
    """fills_up: the first pods take the four holders, later ones leave them."""
    s = ic.scene("fills_up")
    a = _right("fills_up", 100)
    hold = {3, 50, 77, 139}
    assert set(int(x) for x in a[:4]) == hold
    assert any(int(x) not in hold for x in a[:ic.BATCH_PODS])      # within the first batch
    assert len(a) > ic.BATCH_PODS


@pytest.mark.parametrize("fault", list(ic.FAULTS))
def test_wrong_reading_moves_a_placement(fault):
    moved = []
    for name in ic.SCENES:
        s = ic.scene(name)
        for pct in PCTS:
            cluster, pods, prof = ic.FAULTS[fault](s, pct)
            if not np.array_equal(_schedule(cluster, pods, prof), _right(name, pct)):
                moved.append((name, pct))
    assert moved, fault
    # both modes tell it
    assert {p for _, p in moved} == set(PCTS), (fault, moved)


def _delta_run(s, pct, second_cluster):
    """Half the queue on the first snapshot, the node delta, the other half."""
    c0, p0 = s.encoded
    c1, p1 = s.encoded_after
    half = len(s.queue) // 2
    prof = s.compiled(pct)
    ora = Oracle(c0.copy_state(), prof)
    a = _schedule(c0, p0, prof, 0, half, ora)
    st = ora.node_state()
    c = second_cluster.copy_state()
    old_pos = ic.old_positions(c0, c1)
    ora.upsert_nodes(c, old_pos)
    b = _schedule(c, p1, prof, half, len(s.queue) - half, ora)
    ora.close()
    del st
    return np.concatenate([a, b])


def test_stale_rows_after_a_delta_move_a_placement():
    s = ic.scene("delta")
    c0, _ = s.encoded
    c1, _ = s.encoded_after
    r = ic.image_rows(c1)
    assert r == ic.image_rows(c0)
    assert set(int(v) for v in c0.class_count[r[0]]) == {0, 30}
    assert set(int(v) for v in c1.class_count[r[0]]) == {0, 81}
    for pct in PCTS:
        right = _delta_run(s, pct, c1)
        stale = _delta_run(s, pct, ic.stale_after_delta(s))
        assert not np.array_equal(right, stale), pct
        assert (right[len(s.queue) // 2:] >= c0.n_nodes).any()      # the new holders are used


def test_key_bound_scenes():
    """The sums the two bound scenes are named for."""
    lo, hi = ic.scene("bound_below").compiled(100), ic.scene("bound_above").compiled(100)

    def il_weight(p):
        from ksim import abi
        for k in range(p.n_score):
            if p.score[k] == abi.PL_IMAGE_LOCALITY:
                return int(p.score_weight[k])
        raise AssertionError("ImageLocality is not scored")
    assert 100 * (2 + il_weight(lo)) == ic.KEY_TOTAL_LIMIT - 76 < ic.KEY_TOTAL_LIMIT
    assert 100 * (2 + il_weight(hi)) == ic.KEY_TOTAL_LIMIT + 24


def test_scenes_stay_small():
    for name in ic.SCENES:
        s = ic.scene(name)
        assert len(s.queue) <= 300 and len(s.nodes) <= 140, name
