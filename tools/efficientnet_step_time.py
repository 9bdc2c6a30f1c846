"""Milliseconds of the EfficientNet-B0 piece encoder (model="efficientnet_b0", use_hip_encoder=True) on its own: the eval forward at
9 216 crops (64 x 12 x 12) and 57 600 crops (64 x 30 x 30; --crops overrides), each of its stages alone -- stem, the eleven blocks,
the output rows -- on the workspace a full call left (da_effnet_forward_taps with a stage set), and the launch alone (host time of
the call's enqueue, no synchronisation inside).  Device events on the one stream around each call, `--warmup` calls first, then the
median and the spread (min .. max) over `--reps` calls.  Generated weights and crops (tests/golden/efficientnet_refs.py).  One JSON
line per measurement, with two derived floors: the arithmetic at the fp32 matrix rate (2 FLOP per multiply-add, 155 TFLOP/s) and
the activation traffic of the chosen fusion (every map written once and read once per consumer) at the device-copy rate DESIGN 3q
measured past the Infinity Cache (0.291 ms for 708 MB read + 708 MB written = 4.87 TB/s).
Run:  python tools/efficientnet_step_time.py [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

FP32_MATRIX_FLOPS = 155e12
COPY_BYTES_PER_S = 4.87e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), float(np.median(host))


def stage_costs(E):
    """{stage: (multiply-adds, bytes read + written)} per crop, in the kernels' padded NHWC layout."""
    p = E.p16
    out = {"stem": (27 * 32 * 256, 4 * (3 * 1024 + 256 * 32))}
    for name, cin, mid, cout, k, s, r, h, skip in E.BLOCKS:
        ho, first = h // s, name == "blocks.0.0"
        mac = (0 if first else cin * mid * h * h) + k * k * mid * ho * ho + 2 * mid * r + mid * cout * ho * ho
        words = 0 if first else p(cin) * h * h + p(mid) * h * h                 # expansion: read x, write e
        words += p(mid) * h * h + p(mid) * ho * ho + p(mid)                     # depthwise: read, write d and the gate
        words += p(mid) * ho * ho + p(mid) + p(cout) * ho * ho * (2 if skip else 1)      # projection: read d, gate (, x), write
        out[name] = (mac, 4 * words)
    out["out"] = (0, 4 * 2 * 1088)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, nargs="*", default=[9216, 57600])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import efficientnet_refs as R
    from diffassemble_amd import efficientnet_encoder as E
    assert torch.cuda.is_available(), "efficientnet_step_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    eng = E.EfficientNetEngine(R.state(), device=dev)
    costs = stage_costs(E)
    base = torch.from_numpy(R.make_crops(256, 3)).to(dev)
    for n in args.crops:
        x = base.repeat((n + 255) // 256, 1, 1, 1)[:n].contiguous()
        out = torch.empty(n, E.OUT_DIM, device=dev)

        def report(what, med, lo, hi, host, mac, nbytes):
            line = dict(what=what, crops=n, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), launch_host_ms=round(host, 4))
            if mac:
                line.update(matrix_floor_ms=round(2 * mac * n / FP32_MATRIX_FLOPS * 1e3, 4))
            if nbytes:
                line.update(traffic_floor_ms=round(nbytes * n / COPY_BYTES_PER_S * 1e3, 4), gbytes=round(nbytes * n / 1e9, 3))
            print(json.dumps(dict(line, reps=args.reps, warmup=args.warmup, chunk=eng.chunk)), flush=True)

        total = tuple(sum(c[i] for c in costs.values()) for i in range(2))
        report("eval_forward", *timed(lambda: eng.forward(x, out=out), args.reps, args.warmup), *total)
        for name, bit in E.STAGES.items():
            report(name, *timed(lambda: eng.run_stages(x, bit, out=out), args.reps, args.warmup), *costs[name])


if __name__ == "__main__":
    main()
