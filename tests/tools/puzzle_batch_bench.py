"""Timing of the Batch builder (diffassemble_amd/puzzle_batch.py, csrc/da_puzzle_batch.hip): 64 puzzles of 12 x 12 and 64 of
30 x 30 cut from noise pictures that already lie on the device, with rotation, ``views`` 1 and 4 (``all_equivariant``),
``edges=None``.

Arms, each after 5 warm-ups, median of the repetitions:
  make_batch       the whole call on device pictures, host clock between two device synchronisations: the draws and the tables
                   made on the host, their one upload, ONE ``da_puzzle_batch`` launch
  da_puzzle_batch  the launch alone, everything prepared, device events around it
  copy             ``Tensor.copy_`` of as many bytes as the launch writes into ``patches``, device to device, same process: the
                   kernel is a store stream (it reads a twelfth, or a forty-eighth, of what it writes), and this is its yardstick
  _loop_batch      the per-piece host route (what ``make_batch`` does for CPU pictures, and what the reference's datasets do),
                   timed on ``--host-puzzles`` puzzles of the shape and scaled to the Batch
The device Batch must equal the host route's on those puzzles first.  GB/s = bytes written to ``patches`` / time (the copy
arm moves as many again on the read side).  One JSON line per (shape, views).

    python tests/tools/puzzle_batch_bench.py [--reps 30] [--shapes 64x12x12 64x30x30] [--host-puzzles 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from diffassemble_amd import _lib, make_batch  # noqa: E402
from diffassemble_amd import puzzle_batch as P  # noqa: E402

WARMUP = 5


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def host_timed(fn, reps, warmup=WARMUP, sync=True):
    ms = []
    for rep in range(warmup + reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if rep >= warmup:
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


def launch_alone(flat, dims, turns, views, dev, reps):
    """da_puzzle_batch through the C ABI with the tables prepared (all pieces present)."""
    keeps = [list(range(r * c)) for r, c in dims]
    host, where, N, _, n_lin = P._tables(dims, turns, keeps, list(range(len(dims))), False)
    small = torch.from_numpy(host).to(dev)

    def part(name):
        a, b, dtype, shape = where[name]
        return small[a:b].view(P._TORCH_OF[dtype]).view(shape)

    patches = torch.empty((N, views, 3, 32, 32), device=dev)
    x = torch.empty((N, 4), device=dev)
    rot = torch.empty((N, 2), dtype=torch.long, device=dev)
    ri, idx, bv = (torch.empty(N, dtype=torch.long, device=dev) for _ in range(3))
    st = _lib.stream_ptr(dev)
    args = (len(dims), N, _lib.ptr(flat), flat.numel(), _lib.ptr(part("puzzles")), _lib.ptr(part("pieces")), _lib.ptr(part("lin")), n_lin,
            _lib.ptr(part("unit")), 0, views, 4, _lib.ptr(patches), _lib.ptr(x), _lib.ptr(rot), _lib.ptr(ri), _lib.ptr(idx), _lib.ptr(bv), st)
    res = event_timed(lambda: _lib.check(_lib.lib().da_puzzle_batch(*args)), reps)
    src = torch.empty_like(patches)
    return res, event_timed(lambda: patches.copy_(src), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x12x12", "64x30x30"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-puzzles", type=int, default=2)
    a = ap.parse_args()
    assert a.reps >= 20, "median of at least 20 repetitions"
    assert torch.cuda.is_available(), "puzzle_batch_bench needs the GPU"
    dev = torch.device("cuda:0")
    for shape in a.shapes:
        G, rows, cols = (int(v) for v in shape.split("x"))
        n, dims = rows * cols, [(rows, cols)] * G
        gen = torch.Generator().manual_seed(0)
        imgs = torch.randint(0, 256, (G, 32 * rows, 32 * cols, 3), generator=gen, dtype=torch.uint8)
        rot_index = torch.randint(0, 4, (G * n,), generator=gen)
        d_imgs = imgs.to(dev)
        hp = min(a.host_puzzles, G)
        for views in (1, 4):
            kw = dict(rotation=True, all_equivariant=views == 4, edges=None)
            got = make_batch(d_imgs, (rows, cols), rot_index=rot_index, **kw)
            want = make_batch(imgs[:hp], (rows, cols), rot_index=rot_index[:hp * n], **kw)
            for name in ("x", "patches", "indexes", "rot", "rot_index", "batch"):
                assert torch.equal(getattr(got, name)[:hp * n].cpu(), getattr(want, name)), (shape, views, name)
            del got, want
            out_bytes = G * n * views * 3 * 32 * 32 * 4
            kernel, copy = launch_alone(d_imgs.reshape(-1), dims, rot_index.reshape(G, n).tolist(), views, dev, a.reps)
            res = {"puzzles": G, "rows": rows, "cols": cols, "views": views, "pieces": G * n, "patch_bytes": out_bytes, "warmup": WARMUP,
                   "reps": a.reps, "host_puzzles": hp,
                   "make_batch": host_timed(lambda: make_batch(d_imgs, (rows, cols), rot_index=rot_index, **kw), a.reps),
                   "da_puzzle_batch": kernel, "copy": copy,
                   "_loop_batch": host_timed(lambda: make_batch(imgs[:hp], (rows, cols), rot_index=rot_index[:hp * n], **kw), 3, warmup=1,
                                             sync=False)}
            for arm in ("make_batch", "da_puzzle_batch", "copy"):
                res[arm]["GB_per_s"] = round(out_bytes / (res[arm]["median_ms"] * 1e-3) / 1e9, 1)
            res["_loop_batch"]["batch_ms"] = round(res["_loop_batch"]["median_ms"] * G / hp, 1)       # scaled from hp puzzles to the Batch
            res["kernel_over_copy"] = round(kernel["median_ms"] / copy["median_ms"], 3)
            res["host_over_make_batch"] = round(res["_loop_batch"]["batch_ms"] / res["make_batch"]["median_ms"], 1)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
