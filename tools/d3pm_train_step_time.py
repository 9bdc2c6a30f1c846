"""Milliseconds per phase of one TRAINING step of the discrete position model -- noising (da_d3pm_q_sample), denoiser forward
(da_train_forward_idx), loss + its gradient (da_d3pm_loss), denoiser backward (da_train_backward_idx), optimizer (da_adafactor_step)
-- next to the continuous 2D training step's phases (da_q_sample, da_train_forward_ex, da_loss_grad, da_train_backward_stage,
da_adafactor_step) for the same Batch in the same process: 64 complete 144-piece puzzles (K = 144), both mma_precision modes.

The continuous step is the yardstick: the two share the denoiser body, the flat buffers and the optimizer; the discrete one swaps the
pose MLP for the embedding lookup and its one-owner-per-row gradient, the pose head for the K-wide logits head and its [K, 32]
weight gradient, and the elementwise noising / Huber loss for the K-wide per-piece kernels.  Every phase is timed on its own between
two device events (``--reps`` repetitions after one warm-up step, the median reported), so the sum leaves out what a pipelined step
overlaps; ``step`` is the whole step timed as one.  Synthetic seeded weights / inputs (oracle/weights.py,
tests/golden/discrete_cases.py).  One JSON line per model and mode.
Run:  python tools/d3pm_train_step_time.py [--graphs 64] [--pieces 144] [--reps 20] [--loss hybrid]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from diffassemble_amd import _lib  # noqa: E402
from diffassemble_amd.engine import Schedule, d3pm_loss, d3pm_q_sample  # noqa: E402
from diffassemble_amd.graph_plan import build_plan  # noqa: E402
from diffassemble_amd.model.backbones import Eff_GAT, Eff_GAT_Discrete  # noqa: E402
from diffassemble_amd.train import FusedAdafactor  # noqa: E402
from oracle import diffusion as ODF  # noqa: E402
from oracle import weights as W  # noqa: E402
import discrete_cases as DC  # noqa: E402


def median_ms(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def measure(model, precision, phases, reps, dev):
    """phases: ordered {name: callable}; each is timed alone (the ones before it have run), then the whole sequence as ``step``."""
    res = {}

    def whole():
        for fn in phases.values():
            fn()

    whole()                                        # warm-up: workspaces, plans, gradient views
    for name, fn in phases.items():
        res[name] = round(median_ms(fn, reps, dev), 4)
    res["sum"] = round(sum(res.values()), 4)
    res["step"] = round(median_ms(whole, reps, dev), 4)
    print(json.dumps(dict(model=model, mma_precision=precision, ms=res)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--pieces", type=int, default=144)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loss", default="hybrid", choices=("vb", "cross_entropy", "hybrid"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, n, K, steps = args.graphs, args.pieces, args.pieces, args.steps
    N = G * n
    sch_cpu = ODF.make_schedule(steps)
    sch = Schedule(sch_cpu, dev)
    x0, feats = W.make_inputs(N, 2, 1088, 0)
    x0, feats = x0.to(dev), feats.to(dev)
    gen = torch.Generator().manual_seed(0)
    idx0 = torch.cat([torch.randperm(K, generator=gen) for _ in range(G)]).to(dev)
    ei, batch = W.collate([W.dense_edge_index(n, True)] * G, [n] * G)
    ei, batch = ei.to(dev), batch.to(dev)
    t = torch.randint(0, steps, (G,), generator=gen).to(dev)[batch]
    seed = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    print(json.dumps(dict(graphs=G, pieces=n, K=K, steps=steps, reps=args.reps, loss=args.loss)), flush=True)

    for precision in ("fp32", "bf16"):
        # ---- continuous 2D (the yardstick)
        m = Eff_GAT(steps=steps, visual_pretrained=False)
        m.load_state_dict(W.make_denoiser_state(steps, 2, 2, seed=0), strict=False)
        m = m.to(dev).train()
        te = m.train_engine(dev)
        te.precision = precision
        plan = build_plan(ei, batch, 0).with_source_csr()
        opt = FusedAdafactor(m.parameters(), te)
        sac, somac = sch_cpu["sqrt_alphas_cumprod"].to(dev), sch_cpu["sqrt_one_minus_alphas_cumprod"].to(dev)
        st = {}

        def c_noise():
            st["noise"] = torch.randn_like(x0)
            st["x"] = sac[t, None] * x0 + somac[t, None] * st["noise"]

        def c_fwd():
            st["out"] = te.forward(plan, st["x"], t, feats)

        def c_loss():
            loss = torch.empty((), dtype=torch.float32, device=dev)
            d = torch.empty_like(st["out"])
            _lib.check(_lib.lib().da_loss_grad(2, st["out"].numel(), _lib.ptr(st["noise"]), _lib.ptr(st["out"]), _lib.ptr(loss), _lib.ptr(d),
                                               _lib.stream_ptr(dev)))
            st["d"] = d

        def c_bwd():
            te.backward(plan, st["x"], t, st["d"])

        measure("continuous_2d", precision, dict(noising=c_noise, forward=c_fwd, loss=c_loss, backward=c_bwd, optimizer=opt.step),
                args.reps, dev)
        del m, te, opt, plan, st
        torch.cuda.empty_cache()

        # ---- discrete
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

        measure("discrete", precision, dict(noising=d_noise, forward=d_fwd, loss=d_loss, backward=d_bwd, optimizer=opt.step), args.reps, dev)
        del m, te, opt, plan, sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
