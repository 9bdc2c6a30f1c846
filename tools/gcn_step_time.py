"""Milliseconds per sampling step of the GCN denoiser (architecture="gcn") next to the transformer's, on the two Batches
DESIGN 3h quotes: 64 dense 144-piece puzzles and 32 Exphander 900-piece puzzles at d = 539 (the scripted 60 %).

Each configuration runs the captured DDIM loop (da_sample_loop, hipGraph, bf16 unless --precision fp32) once as warm-up
(it records the graph), then `--reps` replays of a `--steps`-step loop between two device events; the line reports
the mean per step.  Synthetic seeded weights / inputs (oracle/weights.py, tests/golden/gcn_cases.py).  One JSON line per
(configuration, arch).   Run:  python tools/gcn_step_time.py [--steps 20] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from diffassemble_amd import DenoiserEngine, Schedule, _lib  # noqa: E402
from oracle import diffusion as ODF  # noqa: E402
from oracle import weights as W  # noqa: E402
import gcn_cases as GC  # noqa: E402


def step_ms(eng, plan, feats, x0, steps, reps, dev):
    sch = Schedule(ODF.make_schedule(steps), dev)
    kw = dict(ratio=1, mean_type=_lib.MEAN_START_X, keep_trajectory=False, use_graph=True)
    eng.sample_loop(plan, sch, x0, feats, **kw)            # warm-up: stages the features, records the graph
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        eng.sample_loop(plan, sch, x0, feats, restage=False, **kw)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / (reps * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = {"gcn": GC.make_gcn_state(100, 4, 4, 1152, 128, "2d", 0),
           "transformer": W.make_denoiser_state(100, 4, 4, arch="transformer", virt_nodes=0, seed=0)}
    rng = np.random.default_rng(0)
    configs = [("dense_64x144", 64, 144, None), ("expander_32x900_d539", 32, 900, 539)]
    for name, G, n, d in configs:
        x0, feats = W.make_inputs(G * n, 4, 1088, 0)
        x0, feats = x0.to(dev), feats.to(dev)
        if d is None:
            ei, batch = W.collate([W.dense_edge_index(n, True)] * G, [n] * G)
            ei, batch = ei.to(dev), batch.to(dev)
        else:
            perms = torch.from_numpy(np.stack([rng.permutation(n) for _ in range(G)]).astype(np.int64)).to(dev)
        for arch, sd in sds.items():
            eng = DenoiserEngine(sd, variant="2d", arch=arch, precision=args.precision, device=dev)
            plan = eng.plan(ei, batch) if d is None else eng.plan_expander(perms, d)
            ms = step_ms(eng, plan, feats, x0, args.steps, args.reps, dev)
            print(json.dumps(dict(config=name, arch=arch, precision=args.precision, graphs=G, pieces=n, degree=d,
                                  plan="dense" if plan.dense else ("band" if arch == "gcn" and plan.band_degree else
                                                                   ("hybrid" if plan.hybrid else "csr")),
                                  ms_per_step=round(ms, 4), steps=args.steps, reps=args.reps)), flush=True)
            del eng, plan
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
