"""Milliseconds of the PointNet fragment encoder (backbone="pointnet") on its own: the eval forward at --eval-parts x --points
(default 640 x 1000: one sampling Batch of 32 objects of 20 fragments) and the train-mode forward, backward and both at
--train-parts x --points (default 160 x 1000).  Device events on the one stream around each call, `--warmup` calls first, then
the median and the spread (min .. max) over `--reps` calls.  Seeded random weights and clouds.  One JSON line per measurement,
with the arithmetic floor of the forward next to it: 65 920 FLOP per point at the fp32 matrix rate (155 TFLOP/s).
Run:  python tools/pointnet_step_time.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

FLOP_PER_POINT = 2 * (3 * 64 + 64 * 64 + 64 * 64 + 64 * 128 + 128 * 128)
FP32_MATRIX_FLOPS = 155e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval-parts", type=int, default=640)
    ap.add_argument("--train-parts", type=int, default=160)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from diffassemble_amd.model.backbones.pointnet import PointNet
    assert torch.cuda.is_available(), "pointnet_step_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet(128).to(dev)
    with torch.no_grad():
        for l in range(1, 6):
            bn = getattr(net, f"bn{l}")
            bn.running_mean.normal_(0, 0.3)
            bn.running_var.uniform_(0.25, 1.75)

    def report(what, parts, med, lo, hi, flop_factor):
        floor = parts * args.points * FLOP_PER_POINT * flop_factor / FP32_MATRIX_FLOPS * 1e3
        print(json.dumps(dict(what=what, parts=parts, points=args.points, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                              matrix_floor_ms=round(floor, 4), reps=args.reps, warmup=args.warmup)), flush=True)

    pts = 0.5 * torch.randn(args.eval_parts, args.points, 3, device=dev)
    net.eval()
    eng = net.engine()
    out = torch.empty(args.eval_parts, 128, device=dev)
    report("eval_forward", args.eval_parts, *timed(lambda: eng.forward(pts, out=out), args.reps, args.warmup), 1)

    pts = 0.5 * torch.randn(args.train_parts, args.points, 3, device=dev)
    w = torch.randn(args.train_parts, 128, device=dev)
    net.train()
    with torch.no_grad():
        report("train_forward", args.train_parts, *timed(lambda: net(pts), args.reps, args.warmup), 1)

    def both():
        net.zero_grad(set_to_none=True)
        net(pts).backward(w)

    med, lo, hi = timed(both, args.reps, args.warmup)
    report("train_forward_backward", args.train_parts, med, lo, hi, 3)       # backward: dX and dW products, twice the forward's


if __name__ == "__main__":
    main()
