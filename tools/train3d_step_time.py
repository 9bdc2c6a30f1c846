"""Milliseconds per training step of the 3D model at the reference's shape (train_3d.py: 32 shapes, max_num_part = 20, 1000
points per fragment, START_X, loss_type="all"; --backbone vn_dgcnn (the default, D = 832) or pointnet (D = 192)), in the exact-fp32 and the bf16-operand mode, split into noising,
encoder forward, denoiser forward, loss, loss backward + denoiser backward, encoder backward and optimizer.

Every shape holds 20 fragments (640 pieces).  The phases run as the step runs them (GNN_Diffusion.q_sample_se3 ->
Eff_GAT_3d.pcd_features_train -> forward_with_feats -> pose_losses -> backward -> configure_optimizers().step()), each between two
device events on the one stream; the backward is cut at d_feats (the encoder's features are a leaf whose gradient is then fed
into the encoder's own backward), so the two backward phases add up to what ``loss.backward()`` does in one piece.  `--warmup`
whole steps first, then the mean over `--reps` steps and the spread (min .. max) of the step total.  Synthetic seeded weights /
inputs (oracle/weights.py, tests/golden/train3d_cases.py).  One JSON line per (arch, precision).
``--use-6dof``: the 13-channel model of train_3d.py --use_6dof_rot (nine Gaussian channels, da_rot6d_to_pose in front of the loss;
its launch and its backward are counted in the ``loss`` and ``loss_denoiser_bwd`` phases).
Run:  python tools/train3d_step_time.py [--arch transformer] [--backbone pointnet] [--reps 10] [--warmup 3] [--frozen] [--use-6dof]
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

from oracle import weights as W  # noqa: E402
import train3d_cases as T3  # noqa: E402

PHASES = ("noising", "encoder_fwd", "denoiser_fwd", "loss", "loss_denoiser_bwd", "encoder_bwd", "optimizer")


def make_state(arch, D, steps=600, seed=0, use_6dof=False):
    """T3.make_state at the denoiser width of the chosen backbone (832 with vn_dgcnn, 192 with pointnet); ``use_6dof``: with the two
    tensors the mode widens (pos_mlp.0.weight [16, 13], mlp_t.2 [9, 256] / [9])."""
    import gcn_cases as GC
    if arch == "gcn":
        sd = GC.make_gcn_state(steps, 7, None, D, T3.HIDDEN, "3d", seed)
    else:
        sd = W.make_denoiser_state(steps, 7, None, D=D, hidden=T3.HIDDEN, variant="3d", arch=arch, virt_nodes=T3.VIRT, seed=seed)
    if use_6dof:
        g = torch.Generator().manual_seed(seed + 913)
        sd = dict(sd)
        sd["pos_mlp.0.weight"] = (torch.rand(16, 13, generator=g) * 2 - 1) / 13 ** 0.5
        sd["mlp_t.2.weight"] = (torch.rand(9, 256, generator=g) * 2 - 1) / 16
        sd["mlp_t.2.bias"] = (torch.rand(9, generator=g) * 2 - 1) / 16
    return sd


def one_step(m, opt, b, frozen, dev):
    """One training step with an event after every phase -> the list of len(PHASES) + 1 events."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
    ev[0].record()
    x_noisy = m.q_sample_se3(b["x"], b["t"])
    ev[1].record()
    if frozen:
        feats = m.model.pcd_features(b["pts"])
        leaf = feats
    else:
        feats = m.model.pcd_backbone(b["pts"])
        leaf = feats.detach().requires_grad_(True)
    ev[2].record()
    pred, _ = m.forward_with_feats(x_noisy, b["t"], b["edge_index"], pcd_feats=leaf, batch=b["batch"])
    ev[3].record()
    if m.use_6dof:
        from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import Rot6dToPoseFn
        pred = Rot6dToPoseFn.apply(pred)
    losses = m.pose_losses(pred, b["x"], b["pts"], b["n_batch"], b["valids"])
    loss = sum(losses.values())
    ev[4].record()
    loss.backward()
    ev[5].record()
    if not frozen:
        feats.backward(leaf.grad)
    ev[6].record()
    opt.step()
    opt.zero_grad()
    ev[7].record()
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="transformer,exophormer,gcn")
    ap.add_argument("--shapes", type=int, default=32)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--backbone", default="vn_dgcnn", choices=("vn_dgcnn", "pointnet"))
    ap.add_argument("--frozen", action="store_true", help="freeze_backbone=True: no encoder backward, FusedAdafactor alone")
    ap.add_argument("--use-6dof", action="store_true", help="the 13-channel model (train_3d.py --use_6dof_rot)")
    args = ap.parse_args()
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    assert torch.cuda.is_available(), "train3d_step_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    G, n = args.shapes, args.parts
    P = G * n
    edge_index, batch = W.collate([W.dense_edge_index(n, True)] * G, [n] * G)
    rng = np.random.default_rng(0)
    b = dict(x=T3.poses(P, 0).to(dev), pts=W.make_point_clouds(P, args.points, 0).to(dev), edge_index=edge_index.to(dev), batch=batch.to(dev),
             valids=T3.valids_of([n] * G, n).to(dev), n_batch=G, t=torch.from_numpy(rng.integers(0, 600, size=G))[batch].to(dev))
    for arch in args.arch.split(","):
        for precision in ("fp32", "bf16"):
            m = GNN_Diffusion(steps=600, sampling="DDIM", model_mean_type=ModelMeanType.START_X, backbone=args.backbone, architecture=arch,
                              max_num_part=n, loss_type="all", freeze_backbone=args.frozen, use_6dof=args.use_6dof)
            m.model.load_state_dict(make_state(arch, m.model.gnn_feat_dim, use_6dof=args.use_6dof), strict=False)
            m = m.to(dev).train()
            m.model.train_engine(dev).precision = precision
            opt = m.configure_optimizers()
            for _ in range(args.warmup):
                one_step(m, opt, b, args.frozen, dev)
            torch.cuda.synchronize(dev)
            runs = [one_step(m, opt, b, args.frozen, dev) for _ in range(args.reps)]
            torch.cuda.synchronize(dev)
            ms = np.array([[ev[i].elapsed_time(ev[i + 1]) for i in range(len(PHASES))] for ev in runs])
            total = ms.sum(1)
            print(json.dumps(dict(arch=arch, backbone=args.backbone, use_6dof=args.use_6dof, precision=precision, shapes=G, parts=n, points=args.points, pieces=P, frozen_encoder=args.frozen,
                                  optimizer=type(opt).__name__, **{f"{k}_ms": round(float(v), 3) for k, v in zip(PHASES, ms.mean(0))},
                                  step_ms=round(float(total.mean()), 3), step_ms_min=round(float(total.min()), 3),
                                  step_ms_max=round(float(total.max()), 3), reps=args.reps, warmup=args.warmup)), flush=True)
            del m, opt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
