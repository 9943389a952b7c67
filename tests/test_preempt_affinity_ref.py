"""The reference of the affinity dry run (tests/preemptobjref.py), on the CPU.

1. Agreement on what already exists: on every use-free case of
   tests/preemptcases.py, without and with a nominated group, it equals
   oracle/objref.py ObjScheduler.preempt (node and victims) and the C oracle
   (the whole 4-tuple).
2. The scenes of tests/preemptaffcases.py discriminate: each faulty variant of
   the dry run (preemptobjref.FLAWS) differs from the reference on at least one
   scene, and the incremental form the variants are built on equals the
   recomputation on every scene."""
import functools

import numpy as np
import pytest

import preemptaffcases as ac
import preemptcases as pc
import preemptobjref
from ksim import abi, profile
from ksim.encode import encode_pods
from ksim.model import Container, Pod
from oracle.objref import ObjScheduler
from oracle.oracle import Oracle


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_reference_equals_objref_and_oracle_on_use_free_cases(name, grouped):
    case = pc.all_cases()[name]
    prio = case.preemptor[0]
    nodes, bound, start, order, pod = pc.objects(case)
    names = [n.name for n in nodes]
    nom = Pod("nominated", priority=prio + 1, containers=[Container({"cpu": "700m"})])
    at = min(1, case.n_nodes - 1)
    nominated = {names[at]: [nom]} if grouped else None
    got = preemptobjref.dry_run(nodes, bound, start, order, pod, prio, case.args, nominated)
    ref = ObjScheduler(nodes, bound, pct=100, seed=0, preemption=profile.PreemptionArgs(*case.args))
    assert got[:2] == ref.preempt(pod, prio, start, order, nominated=nominated)
    cluster, table, _, prof = pc.encoded(case)
    assert list(cluster.node_names) == names
    enc = encode_pods(cluster, [pod, nom])
    want = Oracle(cluster, prof).preempt(enc, 0, prio, table, [(at, [1])] if grouped else None)
    assert preemptobjref.as_indices(got, names, order) == want
    if not grouped:
        assert want[0] == case.winner


@functools.lru_cache(maxsize=None)
def _result(name: str, flaw):
    sc = ac.scenes()[name]
    return preemptobjref.dry_run(sc.nodes, sc.bound, sc.start, sc.order, sc.pods[0], sc.pods[0].priority, sc.args,
                                 sc.nominated_pods(), flaw=flaw)


@pytest.mark.parametrize("name", ac.scene_ids())
def test_scene_reference(name):
    """The reference gives what the scene was built for, and moving the maps
    by each pod's own contribution equals recomputing them."""
    sc = ac.scenes()[name]
    right = _result(name, None)
    if sc.expect is not None:
        assert right == (sc.expect[0], list(sc.expect[1]), sc.expect[2], sc.expect[3])
    assert _result(name, "none") == right


@pytest.mark.parametrize("flaw", preemptobjref.FLAWS)
def test_scenes_discriminate(flaw):
    differs = [name for name in ac.scene_ids() if _result(name, flaw) != _result(name, None)]
    assert differs, f"no scene tells the reference from the variant {flaw}"


def test_flaws_hit_the_scenes_meant_for_them():
    """Which scene catches which variant (at least these)."""
    meant = {"stale_domains": ["headline", "existing_anti", "affinity"],
             "node_local_only": ["headline", "host_and_zone"],
             "multiplicity_one": ["existing_anti_twice"],
             "stale_emptiness": ["first_pod"],
             "no_ipa_in_reprieve": ["fit_and_anti"],
             "affinity_potential": ["affinity"]}
    assert set(meant) == set(preemptobjref.FLAWS)
    for flaw, names in meant.items():
        for name in names:
            assert _result(name, flaw) != _result(name, None), (flaw, name)


def test_bound_table_full_adds_carries_every_class():
    """ksim.preemption.bound_table(..., full_adds=True): each row's adds are
    topo.adds of its pod (selector classes and carried terms with their
    multiplicity); the default stays the port holdings."""
    from ksim.encode import encode_cluster
    from ksim.preemption import bound_table
    sc = ac.scenes()["existing_anti_twice"]
    cluster, _ = encode_cluster(sc.nodes, sc.bound)
    encode_pods(cluster, sc.pods)
    topo = cluster.topo
    full = bound_table(cluster, sc.bound, sc.start, topo, full_adds=True)
    rows = [list(map(tuple, full.adds[full.adds_off[i]:full.adds_off[i + 1]].tolist())) for i in range(full.n)]
    assert rows == [topo.adds(p) for p in sc.bound]
    assert rows[0] and rows[0][0][1] == 2                     # the term carried twice counts 2
    ports = bound_table(cluster, sc.bound, sc.start, topo)
    assert ports.adds.shape[0] == 0 and ports.adds_off.tolist() == [0] * (full.n + 1)
    for k in ("node", "priority", "start_time", "req"):
        np.testing.assert_array_equal(getattr(ports, k), getattr(full, k))


def test_scene_pods_compile_to_the_kinds_they_are_for():
    """Every scene's preemptor carries its use kinds once compiled (the GPU
    tests assert the same on the set they run)."""
    from ksim.encode import encode_cluster
    for sc in ac.scenes().values():
        cluster, _ = encode_cluster(sc.nodes, sc.bound)
        enc = encode_pods(cluster, sc.pods)
        p = enc.pods[0]
        kinds = {int(k) for k in enc.uses["kind"][int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]}
        assert {getattr(abi, "USE_" + k) for k in sc.kinds} <= kinds, sc.name
        if sc.name == "sixteen_uses":
            assert int(p["use_count"]) == abi.MAX_USES
        if sc.name == "host_and_zone":
            u = enc.uses[int(p["use_first"]):int(p["use_first"]) + int(p["use_count"])]
            assert (np.asarray(u["cls"]) == -1).any()
