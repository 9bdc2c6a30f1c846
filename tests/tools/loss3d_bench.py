"""Timing of the 3D assembly losses (diffassemble_amd/losses3d.py, csrc/da_loss3d.hip) at the training step's size: 32 shapes
x 20 parts x N points, (a) every shape full and (b) 2 .. 20 valid parts per shape.

Arms, alternated inside every repetition, each timed with device events around the call:
  new_fwd       assembly_losses forward (prep + search both ways + reduction)
  new_fwd_bwd   the same + backward to the predicted poses
  base_search   what the library offered before for the same search: pcd_encoder.nearest_sq on the two assembled shapes
                [n_batch, n_parts N, 3], already posed and filled with 1e3 (no gradient, so forward only)
  base_total    base_search + the torch ops that pose the fragments and build the filled shapes
Per arm: median, min .. max and the inter-quartile range over --reps repetitions after --warmup.  The search's pair count
(both directions, valid queries x valid candidates) over the median gives pairs / s; with the inner loop's 7.25 VALU
instructions per pair (24 + 2 min + 3 select per 4 pairs, read off the ISA) that is a share of the chip's fp32 VALU issue
rate, 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 7.86e13 lane-operations / s (unpacked, nominal clock).  One JSON line per case.

    python tests/tools/loss3d_bench.py [--reps 30] [--warmup 5] [--points 1000] [--shapes 32]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from diffassemble_amd import losses3d  # noqa: E402
from diffassemble_amd.pcd_encoder import nearest_sq  # noqa: E402

VALU_PER_PAIR = 7.25
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9


def rotate(q, v):
    """q (0, v) conj(q) without normalisation, [P, 4] x [P, N, 3]."""
    w, u = q[:, None, :1], q[:, None, 1:].expand(-1, v.shape[1], -1)
    uv = torch.cross(u, v, dim=-1)
    return (w * w - (u * u).sum(-1, keepdim=True)) * v + 2.0 * (u * v).sum(-1, keepdim=True) * u + 2.0 * w * uv


def make_case(n_batch, n_parts, N, counts, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    valids = torch.zeros(n_batch, n_parts, dtype=torch.bool)
    for b, c in enumerate(counts):
        valids[b, :c] = True
    P = int(valids.sum())
    pts = torch.rand(P, N, 3, generator=g) - 0.5
    gt_q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1)
    gt_t = torch.randn(P, 3, generator=g)
    pr_q = torch.nn.functional.normalize(gt_q + 0.2 * torch.randn(P, 4, generator=g), dim=-1)
    pr_t = gt_t + 0.2 * torch.randn(P, 3, generator=g)
    return tuple(t.to(dev) for t in (torch.cat((pr_q, pr_t), 1), torch.cat((gt_q, gt_t), 1), pts, valids))


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "iqr_ms": round(q[2] - q[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--shapes", type=int, default=32)
    ap.add_argument("--parts", type=int, default=20)
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 repetitions"
    assert torch.cuda.is_available(), "loss3d_bench needs the GPU: there is no CPU timing"
    dev = torch.device("cuda:0")
    B, S, N = a.shapes, a.parts, a.points
    ragged = [2 + (b * (S - 2)) // max(B - 1, 1) for b in range(B)]
    for name, counts in (("full", [S] * B), ("ragged_2_to_%d" % S, ragged)):
        pred, gt, pts, valids = make_case(B, S, N, counts, dev)
        pred_leaf = pred.clone().requires_grad_(True)
        mask = valids.reshape(B, S)

        def materialise():
            s1 = torch.full((B, S, N, 3), 1e3, device=dev)
            s2 = torch.full((B, S, N, 3), 1e3, device=dev)
            s1[mask] = rotate(pred[:, :4], pts) + pred[:, None, 4:]
            s2[mask] = rotate(gt[:, :4], pts) + gt[:, None, 4:]
            return s1.flatten(1, 2), s2.flatten(1, 2)

        shapes = materialise()

        def new_fwd():
            with torch.no_grad():
                return losses3d.assembly_losses(pred, gt, pts, B, valids, n_parts=S)

        def new_fwd_bwd():
            l = losses3d.assembly_losses(pred_leaf, gt, pts, B, valids, n_parts=S)
            return torch.autograd.grad(l["trans_loss"] + l["transform_pt_cd_loss"] + l["rot_loss"], pred_leaf)

        arms = {"new_fwd": new_fwd, "new_fwd_bwd": new_fwd_bwd, "base_search": lambda: nearest_sq(*shapes),
                "base_total": lambda: nearest_sq(*materialise())}
        # same results first (section 6 of the measuring guide): the Chamfer term from the baseline's distances
        d_ab, d_ba = nearest_sq(*shapes)
        vpt = mask.float().unsqueeze(2).repeat(1, 1, N).view(B, -1)
        base_cd = ((d_ab * vpt).mean(1) + (d_ba * vpt).mean(1)).mean() * 10.0
        new_cd = new_fwd()["transform_pt_cd_loss"]
        assert torch.allclose(new_cd, base_cd, rtol=1e-4, atol=0), (name, float(new_cd), float(base_cd))     # the two arms compute the same thing
        times = {k: [] for k in arms}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rep in range(a.warmup + a.reps):
            for k, fn in arms.items():
                ev[0].record()
                fn()
                ev[1].record()
                ev[1].synchronize()
                if rep >= a.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
        pairs = 2 * sum((c * N) ** 2 for c in counts)
        res = {"case": name, "n_batch": B, "n_parts": S, "n_points": N, "pieces": int(sum(counts)), "reps": a.reps, "pairs": pairs,
               "transform_pt_cd_loss": {"new": float(new_cd), "baseline": float(base_cd)}}
        for k in arms:
            res[k] = stats(times[k])
        fwd = res["new_fwd"]["median_ms"] * 1e-3
        res["new_fwd_pairs_per_s"] = pairs / fwd
        res["new_fwd_valu_share"] = round(pairs * VALU_PER_PAIR / fwd / PEAK_LANE_OPS, 4)
        res["speedup_vs_base_search"] = round(res["base_search"]["median_ms"] / res["new_fwd"]["median_ms"], 3)
        res["beats_base_search_by_more_than_its_spread"] = bool(
            res["new_fwd"]["max_ms"] < res["base_search"]["min_ms"] and
            res["base_search"]["median_ms"] - res["new_fwd"]["median_ms"] > res["base_search"]["max_ms"] - res["base_search"]["min_ms"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
