"""Timing of the 2D renderer (diffassemble_amd/render2d.py, csrc/da_render2d.hip): the frames of a sampling loop's trajectory,
64 puzzles of 12x12 x 10 steps and 8 puzzles of 30x30 x 10 steps, with rotations, crops and poses already on the device.  The
trajectory runs from every piece near the origin with noise (heavy overlap) to the solved puzzle.

Arms, each after 5 warm-ups, median of the repetitions:
  batch_frames   the whole call on device tensors, host clock between two device synchronisations: the copy of the (cos, sin)
                 columns, the coefficients made on the host, their upload, ONE ``da_render2d`` launch
  da_render2d    the launch alone, everything prepared, device events around it
  _loop_frame    the per-piece host route on host copies (what ``batch_frames`` does for CPU tensors), timed on
                 ``--host-frames`` frames spread over the trajectory (it is far too slow for all of them)
The device frames must equal the host route's on those frames first.  ms per frame = time / frames; GB/s = frame bytes / time.
One JSON line per shape.

    python tests/tools/render2d_bench.py [--reps 30] [--shapes 64x12x12x10 8x30x30x10] [--host-frames 4]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffassemble_amd import _lib, render2d  # noqa: E402

WARMUP = 5


def make_batch(G, rows, cols, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = rows * cols
    x, y = torch.linspace(-1, 1, cols), torch.linspace(-1, 1, rows)
    solved = torch.stack(torch.meshgrid(x, y, indexing="xy"), -1).reshape(-1, 2).repeat(G, 1)
    steps = []
    for k in range(K):
        w = k / max(K - 1, 1)                                       # 0: noise about the origin, 1: solved
        pos = w * solved + (1 - w) * 0.4 * torch.randn(G * n, 2, generator=g)
        a = (1 - w) * math.pi * (2 * torch.rand(G * n, generator=g) - 1)
        steps.append(torch.cat((pos, a.cos()[:, None], a.sin()[:, None]), 1))
    patches = torch.randint(0, 256, (G * n, 3, 32, 32), generator=g).float() / 255
    return patches, torch.stack(steps), [[rows, cols]] * G, torch.arange(G).repeat_interleave(n)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def host_timed(fn, reps, sync=True):
    ms = []
    for rep in range(WARMUP + reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if rep >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def event_timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for rep in range(WARMUP + reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        if rep >= WARMUP:
            ms.append(ev[0].elapsed_time(ev[1]))
    return stats(ms)


def launch_alone(patches, poses, dims, dev, reps):
    """da_render2d through the C ABI with the tables and the coefficients prepared (equal puzzles, all pieces present)."""
    K, N, G = poses.shape[0], poses.shape[1], len(dims)
    rows, cols = dims[0]
    n, size = rows * cols, 4 * 32 * rows * 32 * cols
    coef = torch.from_numpy(render2d.rotation_coefficients(render2d.piece_angles(poses[..., 2:4]).numpy())).to(dev)
    table = np.zeros((G, 8), dtype=np.int32)
    for g in range(G):
        table[g, :4] = (g * n, n, rows, cols)
        table[g, 4:6] = np.array(render2d._scales(rows, cols), dtype=np.float32).view(np.int32)
        table[g, 6:8] = np.array([g * size], dtype=np.int64).view(np.int32)
    table = torch.from_numpy(table).to(dev)
    out = torch.empty(K * G * size, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)

    def launch():
        _lib.check(_lib.lib().da_render2d(K, G, N, n, _lib.ptr(patches), _lib.ptr(poses), poses.stride(1), poses.stride(0), _lib.ptr(coef),
                                          _lib.ptr(table), G * size, _lib.ptr(out), st))

    return event_timed(launch, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x12x12x10", "8x30x30x10"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-frames", type=int, default=4)
    a = ap.parse_args()
    assert a.reps >= 20, "median of at least 20 repetitions"
    assert torch.cuda.is_available(), "render2d_bench needs the GPU"
    dev = torch.device("cuda:0")
    for shape in a.shapes:
        G, rows, cols, K = (int(v) for v in shape.split("x"))
        patches, poses, dims, batch = make_batch(G, rows, cols, K)
        n, frames = rows * cols, K * G
        frame_bytes = 4 * 32 * rows * 32 * cols
        d_patches, d_poses, d_batch = patches.to(dev), poses.to(dev), batch.to(dev)
        got = render2d.batch_frames(d_patches, d_poses, dims, batch=d_batch)
        # the host route on a few frames spread over the trajectory: one puzzle of one step each
        picks = [(int(round(i * (K - 1) / max(a.host_frames - 1, 1))), (7 * i) % G) for i in range(a.host_frames)]

        def host_route():
            return [render2d.batch_frames(patches[g * n:(g + 1) * n], poses[k, g * n:(g + 1) * n], [dims[g]])[0][0] for k, g in picks]

        for (k, g), want in zip(picks, host_route()):
            assert torch.equal(got[k][g].cpu(), want), (shape, k, g)
        del got
        res = {"puzzles": G, "rows": rows, "cols": cols, "steps": K, "frames": frames, "frame_bytes": frame_bytes, "warmup": WARMUP,
               "reps": a.reps, "host_frames": len(picks),
               "batch_frames": host_timed(lambda: render2d.batch_frames(d_patches, d_poses, dims, batch=d_batch), a.reps),
               "da_render2d": launch_alone(d_patches, d_poses, dims, dev, a.reps),
               "_loop_frame": host_timed(host_route, 5, sync=False)}
        for arm, count in (("batch_frames", frames), ("da_render2d", frames), ("_loop_frame", len(picks))):
            res[arm]["ms_per_frame"] = round(res[arm]["median_ms"] / count, 5)
            res[arm]["GB_per_s"] = round(frame_bytes * count / (res[arm]["median_ms"] * 1e-3) / 1e9, 3)
        res["host_over_batch_frames"] = round(res["_loop_frame"]["ms_per_frame"] / res["batch_frames"]["ms_per_frame"], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
