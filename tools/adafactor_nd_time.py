#!/usr/bin/env python3
"""A/B timing of the optimizer step of the real training configuration (bench.py --config 5 --pixels: the denoiser plus the trainable
resnet18equiv piece encoder), protocol of tools/ab_config.py: ONE process, the two settings as INTERLEAVED pairs A B B A ..., every
timing after a warm-up and ended by a device synchronise.

    A  HybridAdafactor(..., fused_rest=True)    da_adafactor_step + da_adafactor_nd_step: two library calls, eight launches
    B  HybridAdafactor(..., fused_rest=False)   da_adafactor_step + transformers' Adafactor (torch eager) for the encoder

    python tools/adafactor_nd_time.py [--pairs 12] [--reps 20]

No forward / backward: the module's real parameter list with seeded random gradients (the denoiser's in the training engine's flat
gradient buffer, the encoder's as plain .grad tensors).  Both optimizers update the same parameters; the values are irrelevant here
(parity: tests/test_gpu_adafactor_nd.py).  Prints both medians, the median paired difference and the launch count of A; run it under
`rocprofv3 --kernel-trace --stats -- python tools/adafactor_nd_time.py --pairs 2` for the per-kernel times."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from diffassemble_amd import _lib  # noqa: E402
from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType  # noqa: E402
from diffassemble_amd.train import HybridAdafactor  # noqa: E402

LAUNCHES_PER_CALL = {"da_adafactor_step": 4, "da_adafactor_nd_step": 4}       # da_optim.hip / da_optim_nd.hip


class CountingLib:
    """Counts the optimizer's library calls (a thin wrapper around the ctypes handle)."""

    def __init__(self, counts):
        self.counts = counts

    def __getattr__(self, name):
        fn = getattr(_lib.lib(), name)
        if name not in LAUNCHES_PER_CALL:
            return fn

        def call(*a):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*a)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    m = GNN_Diffusion(steps=100, sampling="DDIM", rotation=True, visual_pretrained=False, model_mean_type=ModelMeanType.EPSILON,
                      backbone="resnet18equiv", freeze_backbone=False).to(dev).train()
    te = m.model.train_engine(dev)
    opts = {"A": HybridAdafactor(m.parameters(), te, fused_rest=True), "B": HybridAdafactor(m.parameters(), te, fused_rest=False)}
    gen = torch.Generator(device=dev).manual_seed(5)
    te.flat_grad.copy_(torch.randn(te.flat_grad.shape, generator=gen, device=dev) * 0.01)
    for p, gv in zip(te.params, te.grad_views):
        p.grad = gv
    rest = [p for g in opts["A"].rest.param_groups for p in g["params"]]
    for p in rest:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 0.01
    n_rest = sum(p.numel() for p in rest)
    print(f"denoiser: {sum(p.numel() for p in te.params)} values in {len(te.params)} tensors (flat buffer); "
          f"encoder: {n_rest} values in {len(rest)} tensors (by pointer)", flush=True)

    def timed(tag, reps):
        opt = opts[tag]
        opt.step()                                            # warm-up (tables uploaded, transformers' state allocated)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    for tag in opts:
        timed(tag, 3)
    counts = {}
    opts["A"].fused.lib = opts["A"].rest.lib = CountingLib(counts)
    opts["A"].step()
    torch.cuda.synchronize()
    opts["A"].fused.lib = opts["A"].rest.lib = _lib.lib()
    ta, tb = [], []
    for i in range(a.pairs):
        for tag in (("A", "B") if i % 2 == 0 else ("B", "A")):
            (ta if tag == "A" else tb).append(timed(tag, a.reps))
    d = [y - x for x, y in zip(ta, tb)]
    launches = sum(LAUNCHES_PER_CALL[k] * v for k, v in counts.items())
    print(f"A (fused_rest=True)  median {statistics.median(ta):.4f} ms/step   library calls per step {counts} (counted) x 4 kernels per call in the source = {launches} launches (traced count: the rocprofv3 run)")
    print(f"B (fused_rest=False) median {statistics.median(tb):.4f} ms/step   (da_adafactor_step + torch eager)")
    print(f"median(B - A) {statistics.median(d):+.4f} ms, A faster in {sum(x > 0 for x in d)} of {len(d)} pairs; "
          f"A range {min(ta):.4f} .. {max(ta):.4f}, B range {min(tb):.4f} .. {max(tb):.4f}")


if __name__ == "__main__":
    main()
