"""Writes tests/golden/pointnet_v1.npz from the reference's own PointNet (puzzle_diff/model/backbones/pointnet.py:8-43).  Build
container only: it needs the reference tree (REFERENCE_ROOT, default /root/reference); the file it loads imports only numpy
and torch.  No reference program text goes into the repository, only these arrays:

  keys                  the state-dict keys of PointNet(128), in order
  sd/<key>              the state dict: seeded init, BatchNorm parameters re-drawn so that nothing is trivial (running mean
                        0.3 randn, running var in [0.25, 1.75], |gamma| in [0.5, 1.5] with about a quarter negative, beta 0.3 randn)
  case/<P>x<N>/points   0.5 randn, rounded to fp16 (stored as fp16: exact in fp32)
  case/<P>x<N>/w        the loss weights [P, 128]: loss = sum(out * w)
  case/<P>x<N>/eval_out, train_out, run_mean/<l>, run_var/<l>, grad/<key>     the reference's fp32 results (train: one forward +
                        backward from the state dict above)
  case/<P>x<N>/dev/...  for each of those, max |fp32 - fp64| / max |fp64| of the reference module itself (fp64: module.double())

To stay under 500 KB, grad/<key> of a tensor with more than 1024 entries holds the flat gradient's entries [::GRAD_STRIDE]; the
recorded deviation is of the whole tensor.  (1, 1) is eval only: BatchNorm refuses one value per channel in train()."""
import importlib.util
import os
import sys

import numpy as np
import torch

CASES = [(1, 1), (1, 20), (2, 63), (3, 65), (5, 257), (20, 1000)]
GRAD_STRIDE = 8
HERE = os.path.dirname(os.path.abspath(__file__))


def grad_sample(g):
    g = np.asarray(g).reshape(-1)
    return g[::GRAD_STRIDE] if g.size > 1024 else g


def load_reference():
    root = os.environ.get("REFERENCE_ROOT", "/root/reference")
    spec = importlib.util.spec_from_file_location("ref_pointnet", os.path.join(root, "puzzle_diff", "model", "backbones", "pointnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PointNet


def rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def main():
    PointNet = load_reference()
    torch.manual_seed(20240)
    net = PointNet(128)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for l in range(1, 6):
            bn = getattr(net, f"bn{l}")
            c = bn.weight.numel()
            bn.running_mean.copy_(0.3 * torch.randn(c, generator=g))
            bn.running_var.copy_(0.25 + 1.5 * torch.rand(c, generator=g))
            sign = torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
            bn.weight.copy_(sign * (0.5 + torch.rand(c, generator=g)))
            bn.bias.copy_(0.3 * torch.randn(c, generator=g))
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    out = {"keys": np.array(list(sd0))}
    for k, v in sd0.items():
        out[f"sd/{k}"] = v.numpy()
    for ci, (P, N) in enumerate(CASES):
        gc = torch.Generator().manual_seed(100 + ci)
        pts = (0.5 * torch.randn(P, N, 3, generator=gc)).half()
        w = torch.randn(P, 128, generator=gc)
        pre = f"case/{P}x{N}/"
        out[pre + "points"], out[pre + "w"] = pts.numpy(), w.numpy()
        res = {}
        for dt in (torch.float32, torch.float64):
            m = PointNet(128)
            m.load_state_dict(sd0)
            m = m.to(dt)
            r = {}
            m.eval()
            with torch.no_grad():
                r["eval_out"] = m(pts.to(dt)).clone()
            if P * N > 1:
                m.train()
                o = m(pts.to(dt))
                (o * w.to(dt)).sum().backward()
                r["train_out"] = o.detach().clone()
                for l in range(1, 6):
                    bn = getattr(m, f"bn{l}")
                    r[f"run_mean/{l}"], r[f"run_var/{l}"] = bn.running_mean.clone(), bn.running_var.clone()
                for k, p in m.named_parameters():
                    r[f"grad/{k}"] = p.grad.clone()
            res[dt] = r
        for k, v in res[torch.float32].items():
            out[pre + k] = grad_sample(v.numpy()) if k.startswith("grad/") else v.numpy()
            out[pre + "dev/" + k] = np.float64(rel(v, res[torch.float64][k]))
    path = os.path.join(HERE, "pointnet_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
