"""What makes tests/test_gpu_fast_edges.py mean something, checked on the CPU:

  - tests/fastref.py with no fault equals the C oracle on every scene of
    tests/fastcases.py under every profile: per cycle the scored nodes, their
    raw NodeResourcesFit and NodeResourcesBalancedAllocation scores and the
    Fit verdict of every node, then the placements and the final node state;
  - every wrong reading of fastref.FAULTS changes the placements of at least
    one scene (the test prints which);
  - every scene has the property its name claims."""
import functools

import numpy as np
import pytest

from ksim import abi
from oracle.oracle import Oracle

import fastcases
import fastref

PROFILES = fastcases.DEFAULT_SHAPE + fastcases.OTHER_SHAPES
FAULT_PROFILES = fastcases.DEFAULT_SHAPE + ("res21",)
FIT_SLOT = "NodeResourcesFit"
BA_SLOT = "NodeResourcesBalancedAllocation"


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    s = fastcases.scene(name)
    chosen, cols, next_start, _ = fastref.schedule(s.cluster, s.pods, fastcases.compiled(kind), prev=s.prev,
                                                   seq0=s.seq0)
    chosen.setflags(write=False)
    return chosen, cols, next_start


def _slot(prof, plugin):
    return [k for k in range(prof.n_score) if abi.PLUGINS[prof.score[k]] == plugin][0]


@pytest.mark.parametrize("kind", PROFILES)
@pytest.mark.parametrize("name", list(fastcases.SCENES))
def test_reference_equals_oracle(name, kind):
    s = fastcases.scene(name)
    prof = fastcases.compiled(kind)
    chosen, cols, next_start, cycles = fastref.schedule(s.cluster, s.pods, prof, prev=s.prev, seq0=s.seq0,
                                                        trace=True)
    ora = Oracle(s.cluster.copy_state(), prof)
    ora.set_pod_seq(s.seq0)
    fit, ba = _slot(prof, FIT_SLOT), _slot(prof, BA_SLOT)
    fit_id = abi.PLUGIN_ID[FIT_SLOT]
    n_scored = 0
    for j, (scored, ok, la, bal) in enumerate(cycles):
        o = ora.cycle(s.pods, j)
        tag = f"{name} {kind} pod {j}"
        assert o["chosen"] == chosen[j], tag
        np.testing.assert_array_equal(o["fail_plugin"] == abi.PASSED, ok, err_msg=tag)
        assert set(o["fail_plugin"][~ok].tolist()) <= {fit_id}, tag
        np.testing.assert_array_equal(np.nonzero(o["scored"])[0], np.sort(scored), err_msg=tag)
        np.testing.assert_array_equal(o["raw"][fit][scored], la[scored], err_msg=tag)
        np.testing.assert_array_equal(o["raw"][ba][scored], bal[scored], err_msg=tag)
        n_scored += scored.size
    assert n_scored > s.cluster.n_nodes * s.pods.n_pods // 4, "the scene scores too few nodes to pin anything"
    assert ora.next_start == next_start
    for k, v in ora.node_state().items():
        np.testing.assert_array_equal(v, cols[k], err_msg=f"{name} {kind} {k}")
    # ... and the batch entry point the GPU tests compare with
    ora = Oracle(s.cluster.copy_state(), prof)
    ora.set_pod_seq(s.seq0)
    ochosen, _ = ora.schedule(s.pods, nthreads=4)
    np.testing.assert_array_equal(ochosen, chosen, err_msg=f"{name} {kind}")
    np.testing.assert_array_equal(_reference(name, kind)[0], chosen)


def test_every_fault_moves_a_placement():
    caught = {}
    for fault in fastref.FAULTS:
        hits = []
        for name in fastcases.SCENES:
            s = fastcases.scene(name)
            if fault == "stale_reciprocal" and s.prev is None:
                continue                              # no allocatable moved: the reading changes nothing
            for kind in FAULT_PROFILES:
                got = fastref.schedule(s.cluster, s.pods, fastcases.compiled(kind), fault=fault, prev=s.prev,
                                      seq0=s.seq0)[0]
                moved = int((got != _reference(name, kind)[0]).sum())
                if moved:                             # the scene's first profile that tells, and how many picks
                    hits.append(f"{name}/{kind}:{moved}")
                    break
        caught[fault] = hits
        print(f"{fault:28s} {' '.join(hits) if hits else 'NOT CAUGHT'}")
    missed = [f for f, h in caught.items() if not h]
    assert not missed, f"no scene's placements tell these readings from the reference: {missed}"


@pytest.mark.parametrize("name", list(fastcases.SCENES))
def test_scene_has_the_property_it_claims(name):
    s = fastcases.scene(name)
    print(name, s.claims)
    assert s.claims and all(v > 0 for v in s.claims.values()), s.claims
    assert fastcases.is_narrow(s.cluster)


def test_larger_forms_stay_narrow():
    s = fastcases.scene("quotient_boundary")
    c = fastcases.tiled(s)
    assert c.n_nodes >= 8193 and c.n_nodes % s.cluster.n_nodes == 0
    np.testing.assert_array_equal(c.alloc_mem[-16:], s.cluster.alloc_mem)
    q = fastcases.with_zone_selector(fastcases.repeated(s.pods, 700))
    assert q.n_pods == 700 and int((q.pods["sel_count"] == 1).sum()) == 234
