"""DefaultPreemption for pods with uses, the parts that need no GPU: the
numpy restatement tests/preemptref.py equals the frozen C oracle on every
use-free case of tests/preemptcases.py (so it can stand in for the oracle
where the oracle refuses, tests/test_gpu_preempt_uses.py); the engine exports
ksim_set_bound_pod_adds; ksim.preemption.bound_table carries the bound pods'
host-port holdings when it is given the cluster's TopologyIndex."""
import numpy as np
import pytest

import preemptcases as pc
import preemptref
from ksim import abi, engine
from ksim.encode import encode_cluster, encode_pods
from ksim.model import Container, ContainerPort, Node, Pod
from ksim.preemption import bound_table
from oracle.oracle import Oracle


@pytest.mark.parametrize("name", pc.cascade_ids() + pc.geometry_ids())
def test_helper_equals_oracle_on_use_free_preemptors(name):
    case = pc.all_cases()[name]
    cluster, table, enc, prof = pc.encoded(case)
    ora = Oracle(cluster, prof)
    fail = Oracle(cluster, prof).cycle(enc, 0)["fail_plugin"]    # its own handle: a cycle binds a pod that fits
    req, ports = preemptref.pod_inputs(enc, 0)
    assert ports == []
    fit, port = preemptref.filter_positions(prof)
    got = preemptref.dry_run(fail, preemptref.columns(cluster), table, case.preemptor[0], req, ports, fit, port,
                             *case.args)
    assert got == ora.preempt(enc, 0, case.preemptor[0], table)


def test_export_listed_and_present():
    assert "ksim_set_bound_pod_adds" in engine.EXPORTS
    assert hasattr(engine.lib(), "ksim_set_bound_pod_adds")
    assert hasattr(engine.Engine, "set_bound_pod_adds")


def _port_pod(name, ports, node="", priority=0):
    return Pod(name, node_name=node, priority=priority,
               containers=[Container({"cpu": "100m"}, [ContainerPort(*p) for p in ports])])


def test_bound_table_carries_port_adds_with_topo():
    nodes = [Node(name=f"n{i}", labels={"kubernetes.io/hostname": f"n{i}"},
                  allocatable={"cpu": "4", "memory": "8Gi", "pods": "110"}) for i in range(3)]
    bound = [_port_pod("wild", [(80, "TCP", "")], node="n0"),               # 0.0.0.0:80
             _port_pod("specific", [(80, "TCP", "10.0.0.1")], node="n1"),   # 10.0.0.1:80
             _port_pod("plain", [], node="n2"),
             _port_pod("other", [(443, "TCP", "")], node="n2")]             # a port nobody asks about
    start = {p.name: i for i, p in enumerate(bound)}
    cluster, _ = encode_cluster(nodes, bound)
    # the preemptor's check registers ("*", TCP, 80) for its 0.0.0.0 port, and
    # ("0.0.0.0", TCP, 8080) + ("10.0.0.9", TCP, 8080) for its specific-ip one
    encode_pods(cluster, [_port_pod("preemptor", [(80, "TCP", ""), (8080, "TCP", "10.0.0.9")])])
    topo = cluster.topo
    star = topo.ids[("port", "*", "TCP", 80)]
    plain = bound_table(cluster, bound, start)
    assert plain.adds_off is None and plain.adds is None
    table = bound_table(cluster, bound, start, topo)
    assert table.n == 4 and table.adds_off.tolist()[0] == 0 and table.adds_off.size == 5
    rows = [dict(map(tuple, table.adds[table.adds_off[i]:table.adds_off[i + 1]].tolist())) for i in range(4)]
    assert rows == [topo.port_adds(p) for p in bound]
    assert rows[0] == {star: 1} and rows[1] == {star: 1}        # both hold TCP 80 on some ip
    assert rows[2] == {} and rows[3] == {}                      # no registered class counts port 443
    # the three-argument form is what it was
    for k in ("node", "priority", "start_time", "req"):
        np.testing.assert_array_equal(getattr(plain, k), getattr(table, k))
    # a later preemptor on a specific ip registers the exact-triple classes; a
    # table built afterwards carries them too
    encode_pods(cluster, [_port_pod("p2", [(80, "TCP", "10.0.0.1")])])
    exact = topo.ids[("port", "10.0.0.1", "TCP", 80)]
    wild = topo.ids[("port", "0.0.0.0", "TCP", 80)]
    t2 = bound_table(cluster, bound, start, topo)
    rows = [dict(map(tuple, t2.adds[t2.adds_off[i]:t2.adds_off[i + 1]].tolist())) for i in range(4)]
    assert rows[0] == {star: 1, wild: 1} and rows[1] == {star: 1, exact: 1}
    assert abi.BoundPods(t2.node, t2.priority, t2.start_time, t2.req).adds is None
