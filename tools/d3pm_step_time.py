"""Milliseconds per sampling step of the DISCRETE position diffusion (DA_VARIANT_DISCRETE, da_sample_loop_idx) next to the continuous
2D DDPM loop's (da_sample_loop_ex) for the same Batch, measured in the same process: 64 complete 144-piece puzzles (K = 144), bf16.

The continuous step is the yardstick: the two loops share the denoiser body; the discrete one swaps the pose MLP for the embedding
lookup (k_embed_idx_time_rot without its addend rows) and the pose head + DDPM update for the tail kernel (k_d3pm_tail: K-wide head, softmax, posterior, Gumbel
term from the in-kernel generator, argmax).  Each loop runs once as warm-up (it records the hipGraph), then ``--reps`` replays of a
``--steps / --ratio``-iteration loop between two device events; a line reports the mean per iteration.  Synthetic seeded weights /
inputs (oracle/weights.py, tests/golden/discrete_cases.py).  One JSON line per loop, then their difference.
Run:  python tools/d3pm_step_time.py [--steps 100] [--ratio 5] [--reps 10] [--guided]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from diffassemble_amd import DenoiserEngine, Schedule  # noqa: E402
from oracle import diffusion as ODF  # noqa: E402
from oracle import weights as W  # noqa: E402
import discrete_cases as DC  # noqa: E402


def timed_ms(run, reps, iters, dev):
    run(True)                                              # warm-up: stages the features, records the graph
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run(False)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / (reps * iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ratio", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--pieces", type=int, default=144)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--guided", action="store_true", help="classifier-free guidance (w = 0.5) in both loops")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, n, K = args.graphs, args.pieces, args.pieces
    iters = (args.steps + args.ratio - 1) // args.ratio
    sch = Schedule(ODF.make_schedule(args.steps), dev)
    x0, feats = W.make_inputs(G * n, 2, 1088, 0)
    x0, feats = x0.to(dev), feats.to(dev)
    idx0 = torch.randint(0, K, (G * n,), generator=torch.Generator().manual_seed(0)).to(dev)
    ei, batch = W.collate([W.dense_edge_index(n, True)] * G, [n] * G)
    ei, batch = ei.to(dev), batch.to(dev)
    cfg_w = 0.5 if args.guided else None
    common = dict(precision=args.precision, graphs=G, pieces=n, K=K, steps=args.steps, ratio=args.ratio, iterations=iters,
                  reps=args.reps, guided=bool(args.guided))
    res = {}

    eng = DenoiserEngine(W.make_denoiser_state(args.steps, 2, 2, seed=0), variant="2d", arch="transformer", precision=args.precision,
                         device=dev)
    plan = eng.plan(ei, batch)
    kw = dict(ratio=args.ratio, keep_trajectory=False, use_graph=True, cfg_w=cfg_w, sampler="DDPM")
    res["continuous"] = timed_ms(lambda first: eng.sample_loop(plan, sch, x0, feats, restage=first, **kw), args.reps, iters, dev)
    print(json.dumps(dict(loop="continuous_2d_ddpm", ms_per_step=round(res["continuous"], 4),
                          **common)), flush=True)
    del eng, plan
    torch.cuda.empty_cache()

    eng = DenoiserEngine(DC.make_discrete_state(K, args.steps, seed=0), variant="discrete", arch="transformer", precision=args.precision,
                         device=dev)
    plan = eng.plan(ei, batch)
    res["discrete"] = timed_ms(lambda first: eng.sample_loop_idx(plan, sch, idx0, feats, ratio=args.ratio, keep_traj=False, use_graph=True,
                                                                 cfg_w=cfg_w, restage=first), args.reps, iters, dev)
    print(json.dumps(dict(loop="discrete_d3pm", folds=int(eng.flags) & 3, ms_per_step=round(res["discrete"], 4), **common)), flush=True)
    print(json.dumps(dict(discrete_minus_continuous_ms=round(res["discrete"] - res["continuous"], 4),
                          ratio=round(res["discrete"] / res["continuous"], 3))), flush=True)


if __name__ == "__main__":
    main()
