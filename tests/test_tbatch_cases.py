"""The topology batch edge scenes of tests/tbatchcases.py on the CPU: the C
oracle and the object-level restatement (oracle/objref.py) agree on every
scene cycle by cycle, every scene reaches each edge its ``reaches`` names
(proved from the oracle's cycle outputs, before any GPU time is spent), a
scene's twin without the edge is placed differently, and the geometry
constants the scenes are cut to are the ones the kernels are built with."""
import os
import re

import pytest

import tbatchcases as tc
from test_topology import run_both

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kube-scheduler-simulator_amd", "csrc")


def test_geometry_constants():
    """kTbPods, kTopT, kVarDom, kTbMaxBlocks and kFuseMinValues as
    csrc/ksim_internal.h and csrc/ksim_device.h define them: a changed
    constant fails here instead of moving the scenes off their edges."""
    text = ""
    for f in ("ksim_internal.h", "ksim_device.h"):
        with open(os.path.join(CSRC, f)) as fh:
            text += fh.read()
    for name, want in tc.CONSTANTS.items():
        m = re.findall(r"constexpr\s+u?int(?:32_t)?\s+" + name + r"\s*=\s*(\w+)\s*;", text)
        assert len(m) == 1, (name, m)
        value = m[0]
        if not value.isdigit():                    # kTopT = KSIM_TOP_T: the macro's default
            d = re.findall(r"#ifndef\s+" + value + r"\s*\n\s*#define\s+" + value + r"\s+(\d+)", text)
            assert len(d) == 1, (name, value, d)
            value = d[0]
        assert int(value) == want, (name, value, want)
    assert tc.MAX_NODES == 16384


@pytest.mark.parametrize("name", [n for n in tc.SCENES if tc.scene(n).objref])
def test_oracle_equals_objref(name):
    """Every filter outcome and message, raw and normalized score, total and
    placement, at percentageOfNodesToScore 100 (the topology batches' mode).
    The 16,384- and 16,385-node forms of block_edges are the 257-node form
    with more small nodes; the object-level restatement is left to the three
    small forms."""
    s = tc.scene(name)
    _, _, _, chosen = run_both(s.nodes, s.bound, s.queue, pct=100)
    assert chosen == tc.trace(name).names()


@pytest.mark.parametrize("name", list(tc.SCENES))
def test_scene_reaches_its_edges(name):
    s = tc.scene(name)
    t = tc.trace(name)
    assert s.reaches, name
    for edge, claim in s.reaches.items():
        assert claim(t), f"{name} does not reach: {edge} (n_feasible {t.nf}, chosen {t.names()})"


@pytest.mark.parametrize("name", [n for n in tc.SCENES if tc.scene(n).twin])
def test_twin_is_placed_differently(name):
    s = tc.scene(name)
    assert tc.trace(name).names() != tc.trace(s.twin).names(), (name, s.twin)


def test_every_edge_is_named():
    """Each edge of the list maps to a scene that claims it under that name."""
    for edge, (name, claim) in tc.EDGES.items():
        assert claim in tc.scene(name).reaches, (edge, name, claim)


def test_scenes_stay_small():
    for name in tc.SCENES:
        s = tc.scene(name)
        assert len(s.queue) <= 100 and len(s.bound) <= 40, name
