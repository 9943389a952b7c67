"""bench.py --dump-outputs: the files dump_outputs() writes (names, dtypes, the
64 MB cap with its seeded sample), on a stand-in engine: no GPU."""
import glob
import os
import types

import numpy as np

import bench


class FakeEngine:
    def __init__(self, n_nodes, chosen):
        self.n_nodes, self.chosen, self.next_start, self.resets = n_nodes, chosen, 7, 0

    def node_state(self):
        return {"req_cpu": np.arange(self.n_nodes, dtype=np.int64) << 33,
                "num_pods": np.arange(self.n_nodes, dtype=np.int32)}

    def reset_cluster(self):
        self.resets += 1

    def schedule_loaded(self, first, count):
        assert (first, count, self.resets) == (0, self.chosen.size, 1)   # one more pass, from the reset snapshot
        return self.chosen, None


def _stats():
    return types.SimpleNamespace(pods=5, scheduled=4, unschedulable=1, evals=1 << 40, batches=2, truncations=0,
                                 perpod_cycles=3)


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def test_dump_outputs_files(tmp_path):
    chosen = np.array([3, -1, 0, 2, 2], np.int32)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, FakeEngine(4, chosen), _stats(), 5, 2, False, 0)
    got = _load(d)
    assert sorted(got) == ["next_start", "node_num_pods", "node_req_cpu", "placements", "stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["stats"].tolist() == [5, 4, 1, float(1 << 40), 2, 0, 3]
    assert got["placements"].tolist() == chosen.tolist()
    assert got["node_req_cpu"].tolist() == [0, 1 << 33, 2 << 33, 3 << 33]
    assert got["next_start"].tolist() == [7]


def test_dump_outputs_other_ranks_write_nothing(tmp_path):
    d = str(tmp_path / "out")
    eng = FakeEngine(4, np.zeros(5, np.int32))
    bench.dump_outputs(d, eng, _stats(), 5, 2, True, 1)
    assert eng.resets == 1 and not os.path.exists(d)         # joined the pass, wrote no file


def test_dump_outputs_cap_and_sample(tmp_path):
    n = 9_000_000                                            # 72 MB as float64: past the cap
    chosen = (np.arange(n, dtype=np.int64) % 4999).astype(np.int32)
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        bench.dump_outputs(d, FakeEngine(4, chosen), _stats(), n, 2, False, 0)
        assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(d, "*.npy"))) <= 64 * 1000 * 1000
        runs.append(_load(d))
    a, b = runs
    idx = a["placements_index"].astype(np.int64)
    assert idx.size == a["placements"].size > 1_000_000 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["placements"], chosen[idx])
    assert np.array_equal(idx, b["placements_index"].astype(np.int64))   # the same sample every run
    assert a["node_req_cpu"].size == 4                       # the small arrays stay whole
