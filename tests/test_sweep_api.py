"""The packed policy sweep's interface without a GPU: the export, the ABI
number on every side of the boundary, and sweep.run_sweep's choice between the
packed call and the serial loop (on a stand-in engine)."""
import os
import re

import numpy as np
import pytest

from ksim import abi, engine, sweep

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_export_listed_and_present():
    assert "ksim_sweep_loaded" in engine.EXPORTS
    assert hasattr(engine.lib(), "ksim_sweep_loaded")
    assert hasattr(engine.Engine, "sweep_loaded")


def test_abi_12_everywhere():
    header = open(os.path.join(ROOT, "include", "ksim_engine.h")).read()
    assert int(re.search(r"#define KSIM_ABI_VERSION (\d+)", header).group(1)) == 12
    assert abi.ABI_VERSION == 12 and engine.lib().ksim_abi_version() == 12
    go = open(os.path.join(ROOT, "integration", "go", "engine", "engine.go")).read()
    assert re.search(r"const ABIVersion = 12\b", go) and "C.ksim_sweep_loaded(" in go
    # the header documents the call's limits; the binding's default is "library default"
    assert int(re.search(r"#define KSIM_SWEEP_MAX_LANES (\d+)", header).group(1)) == 64
    assert 1 <= int(re.search(r"#define KSIM_SWEEP_DEFAULT_LANES (\d+)", header).group(1)) <= 64


class _Pods:
    n_pods = 5


class _FakeEngine:
    """Records the calls; sweep_loaded answers with the given error code or rows."""

    def __init__(self, code):
        self.code, self.calls, self._profile, self.cur = code, [], "own", "own"

    def load_pods(self, pods):
        self.calls.append("load")

    def sweep_loaded(self, profiles, first, count, max_lanes):
        self.calls.append(("sweep", first, count, max_lanes))
        if self.code:
            raise engine.KsimError(self.code, "refused")
        return np.arange(len(profiles) * count, dtype=np.int32).reshape(len(profiles), count), ["st"] * len(profiles)

    def set_profile(self, p):
        self.cur = p
        self.calls.append(("profile", p))

    def reset_cluster(self):
        self.calls.append("reset")

    def schedule_loaded(self, first, count):
        self.calls.append(("run", self.cur))
        return np.full(count, int(self.cur), np.int32), f"st{self.cur}"


def test_run_sweep_packed():
    e = _FakeEngine(0)
    rows, stats, packed = sweep.run_sweep(e, _Pods(), [1, 2, 3], max_lanes=7)
    assert packed is True and rows.shape == (3, 5) and len(stats) == 3
    assert e.calls == ["load", ("sweep", 0, 5, 7)]


def test_run_sweep_serial_on_unsupported_only():
    e = _FakeEngine(abi.E_UNSUPPORTED)
    rows, stats, packed = sweep.run_sweep(e, _Pods(), [1, 2])
    assert packed is False and stats == ["st1", "st2"]
    np.testing.assert_array_equal(rows, np.array([[1] * 5, [2] * 5], np.int32))
    per_vector = lambda p: [("profile", p), "load", "reset", ("run", p)]
    assert e.calls == ["load", ("sweep", 0, 5, 0)] + per_vector(1) + per_vector(2) + [("profile", "own"), "load", "reset"]
    assert e.cur == "own"
    # any other error is the caller's to see
    e = _FakeEngine(abi.E_INVALID)
    with pytest.raises(engine.KsimError):
        sweep.run_sweep(e, _Pods(), [1, 2])
    assert e.calls == ["load", ("sweep", 0, 5, 0)]
