"""Milliseconds of the PointNet++ fragment encoder (backbone="pointnet_plus") on its own: the eval forward at --parts x --points
(default 640 x 1000: one sampling Batch of 32 objects of 20 fragments) and each of its stages alone -- farthest point sampling
and ball query of both levels, the three grouped stacks, the head -- on the workspace a full call left
(da_pointnet_plus_stages).  Device events on the one stream around each call, `--warmup` calls first, then the median and the
spread (min .. max) over `--reps` calls.  Generated weights (tests/golden/pointnet_plus_refs.py) and 0.3 randn clouds.  One JSON
line per measurement; the matrix stages carry their arithmetic floor at the fp32 matrix rate (155 TFLOP/s).
Run:  python tools/pointnet_plus_step_time.py [--reps 10] [--warmup 3]      (tools/pointnet_step_time.py: the plain PointNet)
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

FP32_MATRIX_FLOPS = 155e12
# multiply-adds per fragment: rows x the three layers of the level
MAC = {"sa1": 512 * 32 * (6 * 64 + 64 * 64 + 64 * 128), "sa2": 128 * 64 * (131 * 128 + 128 * 128 + 128 * 256),
       "sa3": 128 * (259 * 256 + 256 * 512 + 512 * 1024), "head": 1024 * 512 + 512 * 256}


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
    ap.add_argument("--parts", type=int, default=640)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import pointnet_plus_refs as R
    from diffassemble_amd.pointnet_plus_encoder import STAGES, PointNetPlusEngine
    assert torch.cuda.is_available(), "pointnet_plus_step_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    eng = PointNetPlusEngine(R.state(), device=dev)
    torch.manual_seed(0)
    pts = (0.3 * torch.randn(args.parts, args.points, 3)).half().float().to(dev)
    start = (torch.randint(0, args.points, (args.parts,)).to(dev, torch.int32), torch.randint(0, 512, (args.parts,)).to(dev, torch.int32))
    out = torch.empty(args.parts, 256, device=dev)

    def report(what, med, lo, hi, mac):
        line = dict(what=what, parts=args.parts, points=args.points, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if mac:
            floor = 2 * mac * args.parts / FP32_MATRIX_FLOPS * 1e3
            line.update(matrix_floor_ms=round(floor, 4), share_of_floor=round(floor / med, 4))
        print(json.dumps(dict(line, reps=args.reps, warmup=args.warmup)), flush=True)

    report("eval_forward", *timed(lambda: eng.forward(pts, start, out=out), args.reps, args.warmup), sum(MAC.values()))
    for name, bit in STAGES.items():
        report(name, *timed(lambda: eng.run_stages(pts, start, out, bit), args.reps, args.warmup), MAC.get(name))
    matrix = sum(STAGES[k] for k in ("sa1", "sa2", "sa3", "head"))
    report("matrix_stages", *timed(lambda: eng.run_stages(pts, start, out, matrix), args.reps, args.warmup), sum(MAC.values()))


if __name__ == "__main__":
    main()
