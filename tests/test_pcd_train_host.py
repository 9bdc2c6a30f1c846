"""CPU checks of the train-mode 3D piece encoder's test infrastructure: the fixture of the reference's train() run
(tests/golden/pcd_train_v1.npz) and the fp64 torch restatement beside cases.py (tests/golden/pcd_train_torch.py) that
tests/tools/pcd_train_bench.py times, pinned to each other."""
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
import pcd_train_torch as PT

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcd_train_v1.npz"))
CASES = sorted({k.split("/")[1] for k in GOLD.files})


class _Params(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.p = {k: torch.nn.Parameter(v.double()) for k, v in sd.items() if v.is_floating_point() and "running" not in k}

    def named_parameters(self):
        return iter(self.p.items())


def test_fixture_layout():
    assert len(CASES) >= 5
    for c in CASES:
        k = f"pcd_train/{c}"
        for key in ("out", "grad/points", "grad/conv1.map_to_feat.weight", "grad/conv6.batchnorm.bn.bias",
                    "bn/VnInv.vn2.batchnorm.bn.running_var", "bn/conv1.batchnorm.bn.num_batches_tracked"):
            assert f"{k}/{key}" in GOLD.files, (c, key)
        none = set(str(x) for x in GOLD[f"{k}/none"])
        assert "VnInv.vn1.map_to_feat.weight" in none and "VnInv.vn_lin.weight" in none
        assert ("linear0.weight" in none) == ("inv" not in c)


@pytest.mark.parametrize("name", [c for c in CASES if "two_forwards" not in c])
def test_torch_restatement_matches_reference(name):
    k = f"pcd_train/{name}"
    wseed, seed, gseed = (int(v) for v in GOLD[f"{k}/seeds"])
    P, N = (int(t[1:]) for t in name.split("_")[:2])
    inv = "inv" in name
    feat = GOLD[f"{k}/out"].shape[1] // (2 if inv else 6)
    net = _Params(W.make_vn_dgcnn_state(feat, wseed))
    pts = W.make_point_clouds(P, N, seed).double().requires_grad_(True)
    G = torch.from_numpy(np.random.default_rng(gseed).standard_normal((P, GOLD[f"{k}/out"].shape[1])))
    out = PT.torch_encoder(net, pts, inv=inv)
    (out * G).sum().backward()

    def rel(a, key):
        b = torch.from_numpy(np.asarray(GOLD[f"{k}/{key}"])).double()
        return float((a.detach() - b).abs().max() / b.abs().max())

    assert rel(out, "out") < 1e-6
    assert rel(pts.grad, "grad/points") < 1e-5
    for n in ("conv1.map_to_feat.weight", "conv4.map_to_dir.weight", "conv6.map_to_feat.weight", "conv3.batchnorm.bn.weight"):
        assert rel(net.p[n].grad, f"grad/{n}") < 1e-5, n
