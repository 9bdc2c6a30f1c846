"""Timing of the 2D validation_step's scoring (diffassemble_amd/score2d.py, csrc/da_score2d.hip) on Batches of G puzzles, with the
sampled poses and the ground truth already on the device: 64 x 12x12 and 32 x 30x30, ``rotation`` off and on, complete and with
10 % of every puzzle's pieces removed (the missing-pieces experiment).

Two arms per setting, each timed on the host clock between two device synchronisations (5 warm-ups, median of 30):
  parent_loop     what ``_eval_step`` did before: ``int(batch.max())``, ``patches_dim.tolist()``, then the per-puzzle loop, which
                  stays in the tree as ``score2d._loop_scores`` -- two batched ``greedy_assign`` launches for a complete Batch,
                  two per puzzle otherwise, and per puzzle ``torch.where``, two sorts, the comparison, ``bool(all)`` (the metric
                  updates, which cost the parent further device reads, are left out)
  batch_scores    one ``da_score2d`` call between the two host copies (sizes before, flags after)
Both arms must agree on every flag first.  Next to them, with device events around the launches alone: ``da_score2d`` against
ONE and TWO ``da_greedy_assign`` launches of the same Batch (the kernel runs both assignments under one set of barriers: how
close to one launch's time does it stay?).  One Batch is in flight at a time.  One JSON line per setting.

    python tests/tools/score2d_bench.py [--reps 30] [--shapes 64x12x12 32x30x30]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from diffassemble_amd import _lib, score2d  # noqa: E402

WARMUP = 5


def make_batch(G, rows, cols, missing, rotation, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = rows * cols
    n = m - int(round(missing * m))
    grid = score2d._grid(rows, cols, "cpu")
    step = 2.0 / (max(rows, cols) - 1)
    gts, preds = [], []
    for _ in range(G):
        gt = grid[torch.randperm(m, generator=g)[:n]]
        pred = gt + 0.3 * step * torch.randn(n, 2, generator=g)
        if rotation:
            a = torch.randint(0, 4, (n,), generator=g).float() * (math.pi / 2)
            b = a + 0.6 * torch.randn(n, generator=g)
            gt = torch.cat((gt, torch.stack((a.cos(), a.sin()), 1)), 1)
            pred = torch.cat((pred, torch.stack((b.cos(), b.sin()), 1)), 1)
        gts.append(gt)
        preds.append(pred)
    batch = torch.arange(G).repeat_interleave(n)
    dims = torch.tensor([[rows, cols]] * G)
    return torch.cat(preds).to(dev), torch.cat(gts).to(dev), dims.to(dev), batch.to(dev), n


def parent_loop(pred, gt, patches_dim, batch, rotation):
    """The scoring of ``_eval_step`` before ``batch_scores``, on device tensors."""
    G = int(batch.max()) + 1
    dims = patches_dim.tolist()
    assert len(dims) == G
    return score2d._loop_scores(pred, gt, dims, batch, rotation)


def host_timed(fn, reps):
    ms = []
    for rep in range(WARMUP + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def launches_alone(pred, gt, rows, cols, G, n, rotation, dev, reps):
    """da_score2d, and one / two da_greedy_assign launches, through the C ABI with everything prepared."""
    lib = _lib.lib()
    m, N = rows * cols, pred.shape[0]
    grid = score2d._grid(rows, cols, dev).repeat(G, 1).contiguous()
    ptr_n = (torch.arange(G + 1, dtype=torch.int32) * n).to(dev)
    ptr_m = (torch.arange(G + 1, dtype=torch.int32) * m).to(dev)
    ok = torch.empty(N, dtype=torch.uint8, device=dev)
    per = torch.empty(G, 4, dtype=torch.int32, device=dev)
    out = torch.zeros(2, N, 3, dtype=torch.int64, device=dev)
    st, ld = _lib.stream_ptr(dev), pred.shape[1]

    def fused():
        _lib.check(lib.da_score2d(G, _lib.ptr(pred), ld, _lib.ptr(gt), ld, _lib.ptr(grid), 2, _lib.ptr(ptr_n), _lib.ptr(ptr_m), n, m,
                                  int(rotation), None, None, _lib.ptr(ok), _lib.ptr(per), st))

    def greedy(k):
        for pos, o in ((gt, out[0]), (pred, out[1]))[:k]:
            _lib.check(lib.da_greedy_assign(G, _lib.ptr(pos), ld, _lib.ptr(grid), 2, _lib.ptr(ptr_n), _lib.ptr(ptr_m), n, m, _lib.ptr(o), st))

    return {"da_score2d": event_timed(fused, reps), "da_greedy_assign_x1": event_timed(lambda: greedy(1), reps),
            "da_greedy_assign_x2": event_timed(lambda: greedy(2), reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x12x12", "32x30x30"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20, "median of at least 20 repetitions"
    assert torch.cuda.is_available(), "score2d_bench needs the GPU: there is no CPU timing"
    dev = torch.device("cuda:0")
    for shape in a.shapes:
        G, rows, cols = (int(v) for v in shape.split("x"))
        for missing in (0.0, 0.1):
            for rotation in (False, True):
                pred, gt, dims, batch, n = make_batch(G, rows, cols, missing, rotation, dev)
                flags, verdicts, _, _ = parent_loop(pred, gt, dims, batch, rotation)
                piece_ok, correct = score2d.batch_scores(pred, gt, dims, batch=batch, rotation=rotation)
                assert torch.equal(torch.cat(flags).bool().cpu(), piece_ok) and verdicts == correct.tolist(), (shape, missing, rotation)
                res = {"puzzles": G, "rows": rows, "cols": cols, "pieces_per_puzzle": n, "rotation": rotation, "warmup": WARMUP,
                       "reps": a.reps, "piece_acc": round(float(piece_ok.float().mean()), 4), "puzzles_correct": int(correct.sum()),
                       "parent_loop": host_timed(lambda: parent_loop(pred, gt, dims, batch, rotation), a.reps),
                       "batch_scores": host_timed(lambda: score2d.batch_scores(pred, gt, dims, batch=batch, rotation=rotation), a.reps)}
                res["parent_over_batch_scores"] = round(res["parent_loop"]["median_ms"] / res["batch_scores"]["median_ms"], 2)
                res["launches_alone"] = launches_alone(pred, gt, rows, cols, G, n, rotation, dev, a.reps)
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
