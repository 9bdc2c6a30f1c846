"""Milliseconds per sampling step of the discrete position + ROTATION diffusion (DA_VARIANT_DISCRETE_ROT, da_sample_loop_rot) next to
the position model's loop (da_sample_loop_idx) for the same Batch, measured in one process: 64 complete 144-piece puzzles (K = 144),
bf16, 20-iteration loops.

Three loops:
  (a) the position loop at its default folds (mlp.2 composed into its consumers + folded last layer);
  (b) the position loop created with disable_folds = 2: the generic last layer, which is the one the rotation variant runs (the folded
      last-layer attention exists for 32 value channels only and the stacked head of the rotation variant has 64);
  (c) the rotation loop (cold diffusion, so that both posteriors and both draws run every step).
(c) - (b) is what the second head, the two-process tail and the addend-row select cost; (b) - (a) is what the missing 64-wide fold
costs.  Each loop runs once as warm-up (it records the hipGraph), then ``--reps`` replays between two device events; a line reports the
mean per iteration.  Synthetic seeded weights / inputs (tests/golden/discrete_cases.py, discrete_rot_cases.py).
Run:  python tools/d3pm_rot_step_time.py [--steps 100] [--ratio 5] [--reps 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from diffassemble_amd import DenoiserEngine, Schedule, _lib  # noqa: E402
from oracle import diffusion as ODF  # noqa: E402
from oracle import weights as W  # noqa: E402
import discrete_cases as DC  # noqa: E402
import discrete_rot_cases as RC  # noqa: E402


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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, n, K = args.graphs, args.pieces, args.pieces
    N = G * n
    iters = (args.steps + args.ratio - 1) // args.ratio
    sch = Schedule(ODF.make_schedule(args.steps), dev)
    gen = torch.Generator().manual_seed(0)
    idx0, rot0 = torch.randint(0, K, (N,), generator=gen).to(dev), torch.randint(0, 4, (N,), generator=gen).to(dev)
    feats4 = RC.feature_images(N, 1).to(dev)
    ei, batch = W.collate([W.dense_edge_index(n, True)] * G, [n] * G)
    ei, batch = ei.to(dev), batch.to(dev)
    common = dict(precision=args.precision, graphs=G, pieces=n, K=K, steps=args.steps, ratio=args.ratio, iterations=iters, reps=args.reps)
    res = {}

    def position(folds_off):
        old = _lib.set_config(disable_folds=folds_off)          # a denoiser keeps the folds it was created with
        try:
            eng = DenoiserEngine(DC.make_discrete_state(K, args.steps, seed=0), variant="discrete", arch="transformer",
                                 precision=args.precision, device=dev)
        finally:
            _lib.set_config(disable_folds=old.disable_folds)
        plan = eng.plan(ei, batch)
        ms = timed_ms(lambda first: eng.sample_loop_idx(plan, sch, idx0, feats4[0], ratio=args.ratio, keep_traj=False, use_graph=True,
                                                        restage=first), args.reps, iters, dev)
        return ms, int(eng.flags) & 3

    for name, off in (("a_position_default_folds", 0), ("b_position_generic_last_layer", 2)):
        res[name[0]], folds = position(off)
        print(json.dumps(dict(loop=name, folds=folds, ms_per_step=round(res[name[0]], 4), **common)), flush=True)
        torch.cuda.empty_cache()

    eng = DenoiserEngine(RC.make_rot_state(K, args.steps, seed=0), variant="discrete_rot", arch="transformer", precision=args.precision,
                         device=dev)
    plan = eng.plan(ei, batch)
    res["c"] = timed_ms(lambda first: eng.sample_loop_rot(plan, sch, idx0, rot0, feats4, ratio=args.ratio, keep_traj=False, use_graph=True,
                                                          cold=True, restage=first), args.reps, iters, dev)
    print(json.dumps(dict(loop="c_rotation", folds=int(eng.flags) & 3, ms_per_step=round(res["c"], 4), **common)), flush=True)
    print(json.dumps(dict(c_minus_b_ms=round(res["c"] - res["b"], 4), b_minus_a_ms=round(res["b"] - res["a"], 4),
                          c_over_a=round(res["c"] / res["a"], 3))), flush=True)


if __name__ == "__main__":
    main()
