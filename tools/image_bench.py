#!/usr/bin/env python3
"""Device-path time of a queue in which every pod names a container image:
config 2's shape (5,000 bare nodes x 50,000 bare pods, gen.config2), every node
listing three of 64 images (1 to 8 GB, each on about 1 node in 21), every pod
naming one of them, so every pod carries one KSIM_USE_IMAGE use and
ImageLocality scores 2 to 36 on the holders and 0 elsewhere.

A step is bench.py's: Engine.reset_cluster, then schedule_loaded over the whole
queue; the figure is host wall time per step, under percentageOfNodesToScore
100 (P100) and 0 (ADAPT, K < N), a fresh handle each.  --imageless: the same
nodes and pods without the uses (config 2 itself), for the cost of the image
part over the FAST keys.

Prints one JSON line.  To compare two builds on one machine run it once per
library (KSIM_LIB_VARIANT=<tag> loads libksim_engine_<tag>.so,
tools/build_ref_flavor.sh).

    python tools/image_bench.py [--nodes 5000] [--pods 50000] [--steps 10] [--warmup 2] [--imageless]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "kube-scheduler-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from ksim import abi, engine, gen, profile  # noqa: E402
from ksim.encode import EncodedPods  # noqa: E402
from ksim.model import Container, Pod  # noqa: E402

N_IMAGES = 64
MB = 1024 * 1024


def build(n_nodes: int, n_pods: int, images: bool):
    cluster, pods = gen.config2(n_nodes=n_nodes, n_pods=n_pods)
    if not images:
        return cluster, pods, {}
    node = np.arange(n_nodes)
    cls = np.zeros(N_IMAGES, np.int32)
    for k in range(N_IMAGES):
        mask = (node % N_IMAGES == k) | ((node * 7 + 3) % N_IMAGES == k) | ((node * 13 + 5) % N_IMAGES == k)
        cluster.topo.images[f"registry.example/app-{k}:v1"] = ((1024 + 112 * k) * MB, mask)
    for k in range(N_IMAGES):                     # the class of a one-container pod naming image k
        cls[k] = cluster.topo.image_class(Pod(f"img-{k}", containers=[Container(image=f"registry.example/app-{k}:v1")]))
    cluster.refresh_classes()
    rows = cluster.class_count[cls]
    uses = np.zeros(N_IMAGES, abi.TOPO_USE_DTYPE)
    uses["cls"] = cls
    uses["col"] = abi.COL_NONE
    uses["kind"] = abi.USE_IMAGE
    p = pods.pods.copy()
    p["use_first"] = (np.arange(n_pods) * 31) % N_IMAGES
    p["use_count"] = 1
    q = EncodedPods(p, pods.exprs, pods.terms, pods.names, uses, pods.adds, pods.nn)
    return cluster, q, dict(images=N_IMAGES, holders_per_image=int((rows > 0).sum(axis=1).min()),
                            score_min=int(rows[rows > 0].min()), score_max=int(rows.max()))


def measure(cluster, pods, pct: int, steps: int, warmup: int) -> dict:
    import torch
    eng = engine.Engine(0)
    eng.set_profile(profile.compile_profile(profile.SchedulerProfile(percentage_of_nodes_to_score=pct)))
    eng.set_cluster(cluster)
    eng.load_pods(pods)
    st = None
    for _ in range(warmup):
        eng.reset_cluster()
        _, st = eng.schedule_loaded(0, pods.n_pods, want_chosen=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.reset_cluster()
        _, st = eng.schedule_loaded(0, pods.n_pods, want_chosen=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = dict(ms_per_step=dt / steps * 1e3, batches=int(st.batches), perpod_cycles=int(st.perpod_cycles),
               scheduled=int(st.scheduled), evals=int(st.evals))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--imageless", action="store_true", help="the same nodes and pods without image uses")
    args = ap.parse_args()
    cluster, pods, info = build(args.nodes, args.pods, not args.imageless)
    res = dict(bench="image_batch" if not args.imageless else "image_batch_imageless",
               library=os.path.basename(engine.LIB_PATH), nodes=args.nodes, pods=args.pods, steps=args.steps,
               warmup=args.warmup, **info)
    res["p100"] = measure(cluster, pods, 100, args.steps, args.warmup)
    res["adapt"] = measure(cluster, pods, 0, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
