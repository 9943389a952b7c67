"""The enqueue rule of the deferred-commit runs' host loop
(ksim_feed_more_batches: host arithmetic, no device).  With `left` pods behind
the last commit the host has seen and `pending` enqueued batches that start at
or after it, ceil(left / B) - pending more batches may be enqueued: a batch
commits at most B pods, so none of them can start past the end.  The loop's
fallback (a flush and a state read) has pending = 0."""
import pytest

from ksim import engine

B = 256


def more(left, pending):
    return engine.lib().ksim_feed_more_batches(left, pending)


def test_export_listed_and_present():
    assert "ksim_feed_more_batches" in engine.EXPORTS
    assert hasattr(engine.lib(), "ksim_feed_more_batches")


@pytest.mark.parametrize("left,want", [(0, 0), (-5, 0), (1, 1), (B - 1, 1), (B, 1), (B + 1, 2), (4 * B, 4),
                                       (4 * B + 1, 5), (16 * B, 16), (16 * B + 1, 17), (50000, 196),
                                       (2**31 - 1, 2**23)])
def test_nothing_pending(left, want):
    assert more(left, 0) == want


@pytest.mark.parametrize("left,pending,want", [(B, 1, 0), (B + 1, 1, 1), (B + 1, 2, 0), (B + 1, 3, 0),
                                               (16 * B, 16, 0), (16 * B + 1, 16, 1), (16 * B, 20, 0),
                                               (50000, 190, 6), (1, 1, 0), (0, 3, 0)])
def test_pending_batches_count_against_the_bound(left, pending, want):
    assert more(left, pending) == want


def test_never_past_the_end():
    """Whatever the pending batches commit (1..B pods each; the last one may
    commit fewer only by ending the run), a batch the rule allows starts
    before the end: the worst case is every earlier batch committing B."""
    for left in list(range(1, 3 * B + 2)) + [16 * B - 1, 16 * B, 16 * B + 1]:
        for pending in range(0, 20):
            n = more(left, pending)
            assert n >= 0
            if n:
                # the last allowed batch starts after pending + n - 1 full batches at the latest
                assert (pending + n - 1) * B < left, (left, pending, n)
            # and one more could start at or past the end
            assert (pending + n) * B >= left, (left, pending, n)
