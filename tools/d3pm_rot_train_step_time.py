"""Milliseconds per phase of one TRAINING step of the discrete position + rotation model -- noising (da_d3pm_q_sample_rot: both
processes, one launch), denoiser forward (da_train_forward_rot), both losses + both logit gradients (da_d3pm_rot_loss), denoiser
backward (da_train_backward_rot), optimizer (da_adafactor_step) -- next to the discrete position model's phases (da_d3pm_q_sample,
da_train_forward_idx, da_d3pm_loss, da_train_backward_idx, da_adafactor_step) for the same Batch in the same process: the shape of
tools/d3pm_train_step_time.py, 64 complete 144-piece puzzles (K = 144), both mma_precision modes.

The position model is the yardstick: the two share everything up to the head; the rotation model widens the head's first layer from
32 to 64 rows (one product each way), adds a [4, 32] second layer, and evaluates a four-class row per piece beside the K-wide one.
Every phase is timed on its own between two device events (``--reps`` repetitions after one warm-up step, the median reported), so
the sum leaves out what a pipelined step overlaps; ``step`` is the whole step timed as one.  ``--only-rotation`` adds the rotation
model's step without the position half (no position noising, no K-wide loss row, no final_mlp.2 products).  Synthetic seeded weights /
inputs.  One JSON line per model and mode.
Run:  python tools/d3pm_rot_train_step_time.py [--graphs 64] [--pieces 144] [--reps 20] [--loss hybrid] [--only-rotation]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from diffassemble_amd.engine import Schedule, d3pm_loss, d3pm_q_sample, d3pm_q_sample_rot, d3pm_rot_loss  # noqa: E402
from diffassemble_amd.graph_plan import build_plan  # noqa: E402
from diffassemble_amd.model.backbones import Eff_GAT_Discrete, Eff_GAT_Discrete_ROT  # noqa: E402
from diffassemble_amd.train import FusedAdafactor  # noqa: E402
from oracle import diffusion as ODF  # noqa: E402
from oracle import weights as W  # noqa: E402
import discrete_cases as DC  # noqa: E402
import discrete_rot_cases as RC  # noqa: E402
from d3pm_train_step_time import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--pieces", type=int, default=144)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loss", default="hybrid", choices=("vb", "cross_entropy", "hybrid"))
    ap.add_argument("--only-rotation", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, n, K, steps = args.graphs, args.pieces, args.pieces, args.steps
    N = G * n
    sch = Schedule(ODF.make_schedule(steps), dev)
    feats = W.make_inputs(N, 2, 1088, 0)[1].to(dev)
    gen = torch.Generator().manual_seed(0)
    idx0 = torch.cat([torch.randperm(K, generator=gen) for _ in range(G)]).to(dev)
    rot0 = torch.randint(0, 4, (N,), generator=gen).to(dev)
    ei, batch = W.collate([W.dense_edge_index(n, True)] * G, [n] * G)
    ei, batch = ei.to(dev), batch.to(dev)
    t = torch.randint(0, steps, (G,), generator=gen).to(dev)[batch]
    seed = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    print(json.dumps(dict(graphs=G, pieces=n, K=K, steps=steps, reps=args.reps, loss=args.loss)), flush=True)

    for precision in ("fp32", "bf16"):
        # ---- discrete position model (the yardstick)
        m = Eff_GAT_Discrete(steps=steps, input_channels=K, output_channels=K)
        m.load_state_dict(DC.make_discrete_state(K, steps, seed=0), strict=False)
        m = m.to(dev).train()
        te = m.train_engine(dev)
        te.precision = precision
        plan = build_plan(ei, batch, 0).with_source_csr()
        opt = FusedAdafactor(m.parameters(), te)
        sd = {}

        def d_noise():
            sd["x_t"] = d3pm_q_sample(sch, idx0, t, K, seed=seed)

        def d_fwd():
            sd["logits"] = te.forward(plan, sd["x_t"], t, feats)

        def d_loss():
            _, sd["d"], _ = d3pm_loss(sch, sd["logits"], idx0, sd["x_t"], t, args.loss, 0.01)

        def d_bwd():
            te.backward(plan, sd["x_t"], t, sd["d"])

        phases = dict(noising=d_noise, forward=d_fwd, loss=d_loss, backward=d_bwd, optimizer=opt.step)
        measure("discrete", precision, phases, args.reps, dev)
        del m, te, opt, plan, sd
        torch.cuda.empty_cache()

        # ---- discrete position + rotation model
        for only_rot in ((False, True) if args.only_rotation else (False,)):
            m = Eff_GAT_Discrete_ROT(steps=steps, input_channels=K, output_channels=K)
            m.load_state_dict(RC.make_rot_state(K, steps, seed=0), strict=False)
            m = m.to(dev).train()
            te = m.train_engine(dev)
            te.precision = precision
            plan = build_plan(ei, batch, 0).with_source_csr()
            opt = FusedAdafactor(m.parameters(), te)
            sr = {}

            def r_noise():
                x_t, sr["rot_t"] = d3pm_q_sample_rot(sch, idx0, rot0, t, K, seed=seed, want_x=not only_rot)
                sr["x_t"] = idx0 if only_rot else x_t

            def r_fwd():
                sr["logits"], sr["rot_logits"] = te.forward(plan, sr["x_t"], t, feats)

            def r_loss():
                _, sr["d"], sr["d_rot"], _ = d3pm_rot_loss(sch, None if only_rot else sr["logits"], sr["rot_logits"], idx0, sr["x_t"], rot0,
                                                           sr["rot_t"], t, args.loss, 0.01)

            def r_bwd():
                te.backward(plan, sr["x_t"], t, sr["d"], d_out_rot=sr["d_rot"])

            name = "discrete_rot_only_rotation" if only_rot else "discrete_rot"
            phases = dict(noising=r_noise, forward=r_fwd, loss=r_loss, backward=r_bwd, optimizer=opt.step)
            measure(name, precision, phases, args.reps, dev)
            del m, te, opt, plan, sr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
