"""Timing of the 3D validation_step's scoring (diffassemble_amd/metrics3d.py, csrc/da_metrics3d.hip) on Batches of G objects x 20
parts x 1000 points, G in {8, 32, 256}, with the poses and the clouds already on the device.

Two lines per shape, each timed with device events around the scoring alone (3 warm-ups, mean of 10):
  parent_loop     what validation_step did before: per object ``torch.where(batch == i)`` (a host round trip), then
                  ``trans_metrics`` / ``rot_metrics`` / ``calc_part_acc`` on the object's rows (kept here as a local function built
                  from the public functions; the MeanMetric updates, which cost the parent another device read each, are left out)
  batch_metrics   one ``da_metrics3d`` call for the Batch, ``ptr`` from ``batch`` by bincount + cumsum, and the [G, 4] copy to the host
Both arms must agree first (rmse / geodesic to 1e-4, part_acc to one fp32 ulp).  Next to them: the 30-step sampling loop of the same
Batch (the 3D module with random weights, DDIM T = 300 / ratio 10, ``pcd_feats`` given), and the per-part kernel alone against
its arithmetic floor: P x 2 N^2 squared distances, 3 sub + 1 mul + 2 fma + 1/2 min3 per pair = 3.5 issue slots with the six
arithmetic operations packed two to a slot (6.5 unpacked), at 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 7.86e13 lane-slots / s.
One JSON line per shape.

    python tests/tools/metrics3d_bench.py [--objects 8 32 256] [--points 1000] [--no-loop]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from diffassemble_amd import _lib, metrics3d  # noqa: E402

PEAK_LANE_SLOTS = 256 * 4 * 32 * 2.4e9
SLOTS_PACKED, SLOTS_UNPACKED = 3.5, 6.5
WARMUP, REPS = 3, 10


def make_batch(G, parts, N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = G * parts
    pcds = (torch.rand(P, N, 3, generator=g) - 0.5)
    gt = torch.cat((torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1), 0.5 * torch.randn(P, 3, generator=g)), 1)
    pred = gt + 0.1 * torch.rand(P, 1, generator=g) * torch.randn(P, 7, generator=g)
    pred[:, :4] = torch.nn.functional.normalize(pred[:, :4], dim=-1)
    batch = torch.arange(G).repeat_interleave(parts)
    return pcds.to(dev), pred.to(dev), gt.to(dev), batch.to(dev)


def parent_loop(pcds, pred, gt, batch):
    """The scoring loop of the 3D ``_eval_step`` before ``batch_metrics``; returns [G, 4] on the host."""
    rows = []
    for i in range(int(batch.max()) + 1):
        idx = torch.where(batch == i)[0]
        gt_pos, pred_pos = gt[idx], pred[idx]
        pred_r, pred_t, gt_r, gt_t = pred_pos[:, :4], pred_pos[:, 4:7], gt_pos[:, :4], gt_pos[:, 4:]
        rows.append(torch.stack((metrics3d.trans_metrics(pred_t, gt_t), metrics3d.rot_metrics(pred_r, gt_r, "rmse"),
                                 metrics3d.rot_metrics(pred_r, gt_r, "geodesic"),
                                 metrics3d.calc_part_acc(pcds[idx], pred_t, gt_t, pred_r, gt_r))))
    return torch.stack(rows).cpu()


def batched(pcds, pred, gt, batch):
    return metrics3d.batch_metrics(pcds, pred, gt, batch=batch).cpu()


def timed(fn, warmup=WARMUP, reps=REPS):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for rep in range(warmup + reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        if rep >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {"mean_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def sampling_loop(G, parts, dev):
    """p_sample_loop of the 3D module on the same Batch: 30 denoising steps, dense graph per object, fragment features given."""
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    torch.manual_seed(0)
    m = GNN_Diffusion(steps=300, sampling="DDIM", inference_ratio=10, model_mean_type=ModelMeanType.START_X, backbone="vn_dgcnn",
                      architecture="transformer").to(dev).eval()
    P = G * parts
    batch = torch.arange(G, device=dev).repeat_interleave(parts)
    i = torch.arange(parts, device=dev)
    local = torch.stack(torch.meshgrid(i, i, indexing="ij")).reshape(2, -1)
    edge_index = (local[:, None, :] + parts * torch.arange(G, device=dev)[None, :, None]).reshape(2, -1)
    feats = torch.randn(P, 768, device=dev)
    with torch.no_grad():
        res = timed(lambda: m.p_sample_loop((P, 7), None, edge_index, batch, pcd_feats=feats))
    res["precision"] = getattr(m.model, "precision", "?")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, nargs="+", default=[8, 32, 256])
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--no-loop", action="store_true", help="skip the sampling loop's time")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metrics3d_bench needs the GPU: there is no CPU timing"
    dev = torch.device("cuda:0")
    for G in a.objects:
        pcds, pred, gt, batch = make_batch(G, a.parts, a.points, dev)
        P, N = pred.shape[0], a.points
        old, new = parent_loop(pcds, pred, gt, batch), batched(pcds, pred, gt, batch)
        assert torch.allclose(new[:, :3], old[:, :3], rtol=1e-4, atol=1e-6), (G, float((new[:, :3] - old[:, :3]).abs().max()))
        # part_acc to one fp32 ulp: the kernel divides count / parts (the host route's value), torch's device division by a scalar multiplies by the reciprocal
        assert float((new[:, 3] - old[:, 3]).abs().max()) < 1e-6, (G, new[:, 3].tolist(), old[:, 3].tolist())
        res = {"objects": G, "parts": a.parts, "points": N, "warmup": WARMUP, "reps": REPS,
               "part_acc_mean": round(float(new[:, 3].mean()), 4),
               "parent_loop": timed(lambda: parent_loop(pcds, pred, gt, batch)),
               "batch_metrics": timed(lambda: batched(pcds, pred, gt, batch))}
        res["parent_over_batched"] = round(res["parent_loop"]["mean_ms"] / res["batch_metrics"]["mean_ms"], 2)
        # the library call alone (no ptr construction, no copy): the per-part kernel dominates it
        ptr = torch.arange(G + 1, device=dev, dtype=torch.int32) * a.parts
        pp, po = torch.empty(P, 4, device=dev), torch.empty(G, 4, device=dev)
        call = lambda: _lib.check(_lib.lib().da_metrics3d(P, N, G, _lib.ptr(pred), 7, _lib.ptr(gt), 7, _lib.ptr(pcds), _lib.ptr(ptr),  # noqa: E731
                                                          0.01, _lib.ptr(pp), _lib.ptr(po), _lib.stream_ptr(dev)))
        res["da_metrics3d"] = timed(call)
        pairs = P * 2 * N * N
        res["pairs"] = pairs
        res["floor_packed_ms"] = round(pairs * SLOTS_PACKED / PEAK_LANE_SLOTS * 1e3, 4)
        res["floor_unpacked_ms"] = round(pairs * SLOTS_UNPACKED / PEAK_LANE_SLOTS * 1e3, 4)
        res["kernel_over_packed_floor"] = round(res["da_metrics3d"]["mean_ms"] / res["floor_packed_ms"], 2)
        if not a.no_loop:
            res["sampling_loop_30_steps"] = sampling_loop(G, a.parts, dev)
            res["scoring_over_sampling_loop"] = {k: round(res[k]["mean_ms"] / res["sampling_loop_30_steps"]["mean_ms"], 3)
                                                 for k in ("parent_loop", "batch_metrics")}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
