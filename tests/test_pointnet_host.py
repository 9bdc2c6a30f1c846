"""Host tests of the PointNet fragment encoder (backbone="pointnet"): the fp64 contract of tests/golden/pointnet_refs.py against
the reference's own module (tests/golden/pointnet_v1.npz: its fp32 results and how far they lie from its own fp64 run) and
against torch autograd, the module surface, the C header.  The HIP kernels: tests/test_gpu_pointnet.py."""
import os
import re

import numpy as np
import pytest
import torch

import pointnet_refs as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "pointnet_v1.npz"))
CASES = [(1, 1), (1, 20), (2, 63), (3, 65), (5, 257), (20, 1000)]
GRAD_STRIDE = 8                                                   # make_pointnet_golden.py: grads of > 1024 entries are stored [::8]


def state(dtype=torch.float64):
    return {k: torch.from_numpy(GOLD[f"sd/{k}"]).to(dtype if GOLD[f"sd/{k}"].dtype.kind == "f" else torch.int64) for k in GOLD["keys"]}


def case(P, N, dtype=torch.float64):
    pre = f"case/{P}x{N}/"
    return pre, torch.from_numpy(GOLD[pre + "points"].astype(np.float32)).to(dtype), torch.from_numpy(GOLD[pre + "w"]).to(dtype)


def rel(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


def sample(g):
    g = g.reshape(-1)
    return g[::GRAD_STRIDE] if g.numel() > 1024 else g


def test_fixture_has_every_case_and_stays_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointnet_v1.npz")) < 500 * 1024
    for P, N in CASES:
        assert GOLD[f"case/{P}x{N}/points"].shape == (P, N, 3) and GOLD[f"case/{P}x{N}/eval_out"].shape == (P, 128)
    assert "case/1x1/train_out" not in GOLD.files                  # eval only


@pytest.mark.parametrize("P,N", CASES)
def test_contract_reproduces_the_reference(P, N):
    """|contract(fp64) - reference(fp32)| <= 4 x the reference's own fp32-versus-fp64 deviation + 1e-12, for every tensor."""
    sd = state()
    pre, pts, w = case(P, N)

    def hold(name, got):
        e, bound = rel(got, GOLD[pre + name]), 4 * float(GOLD[pre + "dev/" + name]) + 1e-12
        assert e <= bound, (name, e, bound)

    hold("eval_out", R.eval_forward(sd, pts))
    if P * N == 1:
        return
    f = R.train_forward(sd, pts)
    hold("train_out", f.out)
    for l in range(1, 6):
        hold(f"run_mean/{l}", f.run_mean[l - 1])
        hold(f"run_var/{l}", f.run_var[l - 1])
    grads = R.backward(sd, pts, f, w)
    for k in R.param_keys():
        e = float((sample(grads[k]) - torch.from_numpy(GOLD[pre + "grad/" + k]).double()).abs().max() / grads[k].abs().max())
        assert e <= 4 * float(GOLD[pre + "dev/grad/" + k]) + 1e-12, (k, e)


@pytest.mark.parametrize("P,N", [(1, 20), (3, 65), (5, 257)])
def test_contract_backward_is_autograd_of_its_forward(P, N):
    sd = state()
    for k in R.param_keys():
        sd[k].requires_grad_(True)
    pre, pts, w = case(P, N)
    f = R.train_forward(sd, pts)
    auto = torch.autograd.grad((f.out * w).sum(), [sd[k] for k in R.param_keys()])
    with torch.no_grad():
        grads = R.backward(sd, pts, f, w)
    for k, a in zip(R.param_keys(), auto):
        assert rel(grads[k], a) <= 1e-12, (k, rel(grads[k], a))


def test_contract_ties_go_to_the_lowest_index():
    z = torch.tensor([[[1.0, 5.0], [3.0, 5.0], [3.0, 2.0]]])      # [1, 3, 2]
    assert R.first_argmax(z).tolist() == [[1, 0]]
    assert R.top2_gap(z).tolist() == [[0.0, 0.0]]


def test_module_state_dict_matches_the_reference():
    from diffassemble_amd.model.backbones.pointnet import PointNet
    net = PointNet(128)
    sd = net.state_dict()
    assert list(sd) == list(GOLD["keys"])
    assert all(tuple(sd[k].shape) == GOLD[f"sd/{k}"].shape for k in sd)
    net.load_state_dict(state(torch.float32), strict=True)
    assert torch.equal(net.conv5.weight, torch.from_numpy(GOLD["sd/conv5.weight"]))
    with pytest.raises(NotImplementedError):
        PointNet(128, global_feat=False)


def test_eff_gat_3d_builds_the_pointnet_backbone():
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.model.backbones.pointnet import PointNet
    m = Eff_GAT_3d(steps=10, backbone="pointnet")
    assert isinstance(m.pcd_backbone, PointNet) and m.gnn_feat_dim == 192
    assert isinstance(Eff_GAT_3d(steps=10).pcd_backbone, PointNet)         # its own default
    for name in ("pointnet_inv", "pointnet_plus"):
        other = Eff_GAT_3d(steps=10, backbone=name)
        assert other.pcd_backbone is None
        with pytest.raises(NotImplementedError, match="pass pcd_feats"):
            other.pcd_features(torch.zeros(2, 20, 3))


def test_gnn_diffusion_3d_takes_the_backbone():
    from diffassemble_amd.model.backbones.pointnet import PointNet
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion
    m = GNN_Diffusion(steps=20, sampling="DDIM", backbone="pointnet", max_num_part=6)
    assert isinstance(m.model.pcd_backbone, PointNet)
    assert sum(1 for k in m.state_dict() if k.startswith("model.pcd_backbone.")) == len(GOLD["keys"])


def test_off_device_calls_raise():
    from diffassemble_amd import _lib
    from diffassemble_amd.model.backbones.pointnet import PointNet
    from diffassemble_amd.pointnet_encoder import PointNetEngine
    net = PointNet(128)
    with pytest.raises(_lib.DaError):
        PointNetEngine(net.state_dict(), device="cpu")
    with pytest.raises(_lib.DaError):
        net.eval()(torch.zeros(2, 20, 3))
    with pytest.raises(_lib.DaError):
        net.train()(torch.zeros(2, 20, 3))


def test_header_declares_the_functions_and_keeps_the_abi():
    from diffassemble_amd import _lib
    text = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define\s+DA_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19
    for fn in ("da_pointnet_workspace_bytes", "da_pointnet_forward", "da_pointnet_train_state_bytes", "da_pointnet_train_workspace_bytes",
               "da_pointnet_train_forward", "da_pointnet_train_backward"):
        assert re.search(r"\b" + fn + r"\s*\(", text), fn
        assert fn in _lib.PROTOTYPES, fn
    assert os.path.exists(os.path.join(ROOT, "diffassemble_amd", "csrc", "da_pointnet.hip"))
