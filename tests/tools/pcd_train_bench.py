"""Timing of the 3D piece encoder in train() mode: forward + backward of VN_DGCNN(128) through the HIP path at 20 x 1000,
160 x 1000 (the Breaking Bad script's step: 8 objects of up to 20 fragments) and 640 x 1000 points, beside the eval forward
on the same clouds and beside a torch autograd restatement (written from the maths, point-major, fp32, the same batch
statistics) at 160 x 1000 on the same GPU.  One line per measurement.

    python tests/tools/pcd_train_bench.py [--reps R] [--shapes 20,160,640] [--no-torch]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from oracle import weights as W  # noqa: E402
from diffassemble_amd.model.backbones.vnn.vn_dgcnn import VN_DGCNN  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden"))
from pcd_train_torch import torch_encoder  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="20,160,640")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = VN_DGCNN(128)
    net.load_state_dict(W.make_vn_dgcnn_state(128, 1))
    net = net.to(dev)
    for P in (int(s) for s in a.shapes.split(",")):
        pts = W.make_point_clouds(P, 1000, 2).to(dev)
        G = torch.randn(P, 768, device=dev)

        def train_step():
            net.zero_grad(set_to_none=True)
            p = pts.clone().requires_grad_(True)
            (net(p) * G).sum().backward()

        net.train()
        t_train = timed(train_step, a.reps)
        net.eval()
        with torch.no_grad():
            t_eval = timed(lambda: net(pts), a.reps)
        print(f"pcd train P={P} N=1000: forward+backward {t_train:.2f} ms, eval forward {t_eval:.2f} ms "
              f"(ratio {t_train / t_eval:.2f})", flush=True)
        if P == 160 and not a.no_torch:
            net.train()

            def torch_step():
                net.zero_grad(set_to_none=True)
                p = pts.clone().requires_grad_(True)
                (torch_encoder(net, p) * G).sum().backward()

            print(f"torch restatement P={P} N=1000: forward+backward {timed(torch_step, a.reps):.2f} ms", flush=True)


if __name__ == "__main__":
    main()
