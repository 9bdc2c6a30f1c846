"""Host tests of the PointNet++ fragment encoder (backbone="pointnet_plus"): the fixture tests/golden/pointnet_plus_v1.npz (the
reference's own indices, starts and fp32 outputs), the weight and cloud generators and the contract of
tests/golden/pointnet_plus_refs.py against it, the module surface, the C header.  The HIP kernels: tests/test_gpu_pointnet_plus.py.

(1, 1) is a case without reference results: the reference cannot run fewer points than sa1's 32 samples (the fixture records
that); the selection rule defines its groups, and the contract and the kernels are held on it."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import pointnet_plus_refs as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "tests", "golden", "pointnet_plus_v1.npz")
GOLD = np.load(PATH)
CASES = [(1, 1), (1, 64), (2, 513), (3, 1000), (2, 2048), (20, 1000)]
REF_CASES = [c for c in CASES if f"case/{c[0]}x{c[1]}/eval_out" in GOLD.files]
FACTOR, FLOOR = 16, 1e-5


def cloud(P, N):
    return R.make_cloud(P, N, int(GOLD[f"case/{P}x{N}/cloud_seed"]))


@functools.lru_cache(maxsize=None)
def selection(P, N):
    pre = f"case/{P}x{N}/"
    return R.select(cloud(P, N), GOLD[pre + "start1"], GOLD[pre + "start2"])


def test_fixture_has_every_case_and_stays_small():
    assert os.path.getsize(PATH) < 500 * 1024
    assert R.CASES == CASES and REF_CASES == CASES[1:]
    assert bool(GOLD["case/1x1/reference_refuses"])
    for P, N in CASES:
        pre = f"case/{P}x{N}/"
        assert GOLD[pre + "start1"].shape == (P,) and GOLD[pre + "start2"].shape == (P,)
        assert R.digest(cloud(P, N)) == str(GOLD[pre + "cloud_sha"])
    for P, N in REF_CASES:
        assert GOLD[f"case/{P}x{N}/eval_out"].shape == (P, 256)
        nz = float((GOLD[f"case/{P}x{N}/eval_out"] != 0).mean())
        assert 0.2 <= nz <= 0.8, nz


def test_regenerated_weights_hash_to_the_stored_digests():
    w = R.make_weights(int(GOLD["weight_seed"]))
    assert list(w) == list(GOLD["keys"])
    assert sum(v.size for k, v in w.items() if v.dtype.kind == "f" and "running" not in k) == 1_465_600       # the 1.47 M parameters
    for k, v in w.items():
        assert v.shape == tuple(GOLD[f"shapes/{k}"]), k
        assert R.digest(v) == str(GOLD[f"sha/{k}"]), k


@pytest.mark.parametrize("P,N", REF_CASES)
def test_contract_indices_are_the_references(P, N):
    pre, sel = f"case/{P}x{N}/", selection(P, N)
    for k, v in sel.items():
        if P <= 3:
            assert np.array_equal(v, GOLD[pre + k].astype(np.int64)), k
        else:
            assert R.digest(v.astype(np.int32)) == str(GOLD[pre + k + "_sha"]), k
    if N == 1000:                                  # both branches of the ball query occur
        members = np.stack([(~(R.d2(cloud(P, N)[p][sel["fps1"][p]][:, None, :], cloud(P, N)[p][None]) > np.float32(R.R1 ** 2))).sum(1)
                            for p in range(P)])
        assert (members > R.K1).any() and (members == 1).any()


@pytest.mark.parametrize("P,N", REF_CASES)
def test_contract_reproduces_the_reference(P, N):
    """|contract(fp64) - reference(fp32)| / max |reference| <= max(16 x the reference's own fp32-versus-fp64 deviation, 1e-5)."""
    out = R.eval_forward(R.state(torch.float64), torch.from_numpy(cloud(P, N)).double(), selection(P, N))
    ref = torch.from_numpy(GOLD[f"case/{P}x{N}/eval_out"]).double()
    e = float((out - ref).abs().max() / ref.abs().max())
    bound = max(FACTOR * float(GOLD[f"case/{P}x{N}/dev/eval_out"]), FLOOR)
    print(f"pointnet_plus contract vs reference {P}x{N}: {e:.3e} (bound {bound:.3e})")
    assert e <= bound, (e, bound)


def test_contract_on_one_point():
    """N = 1: every pick and every group member is point 0, and the output is finite."""
    sel = selection(1, 1)
    assert not sel["fps1"].any() and not sel["grp1"].any() and sel["grp2"].shape == (1, 128, 64)
    assert sel["fps2"][0, 0] == GOLD["case/1x1/start2"][0] and not sel["fps2"][0, 1:].any()      # all distances 0: index 0
    out = R.eval_forward(R.state(torch.float64), torch.from_numpy(cloud(1, 1)).double(), sel)
    assert out.shape == (1, 256) and bool(torch.isfinite(out).all())


def test_selection_rule_ties_and_the_radius_edge():
    pts = cloud(1, 64)
    twice = np.concatenate([pts, pts], 1)
    idx = R.fps(twice, 128, [70])
    assert idx[0, 0] == 70 and (idx[0, 1:64] < 64).all() and not idx[0, 65:].any()              # ties to the lowest index, then index 0
    lo, hi = np.float16(0.2), np.nextafter(np.float16(0.2), np.float16(1))
    assert float(lo) < 0.2 < float(hi)                                                            # the two fp16 values next to 0.2
    line = np.array([[[0, 0, 0], [float(lo), 0, 0], [-float(hi), 0, 0]]], np.float32)
    assert R.ball_query(line, [[0]], 0.2, 4).tolist() == [[[0, 1, 0, 0]]]


@pytest.mark.parametrize("P,N", CASES)
def test_module_draws_the_references_starts(P, N):
    from diffassemble_amd.model.backbones.pointnet import PointNetPlus
    torch.manual_seed(int(GOLD[f"case/{P}x{N}/seed"]))
    s1, s2 = PointNetPlus.draw_fps_start(P, N)
    assert s1.device.type == "cpu" and np.array_equal(s1.numpy(), GOLD[f"case/{P}x{N}/start1"])
    assert np.array_equal(s2.numpy(), GOLD[f"case/{P}x{N}/start2"])


def test_eff_gat_3d_builds_the_pointnet_plus_backbone():
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.model.backbones.pointnet import PointNetPlus
    m = Eff_GAT_3d(10, backbone="pointnet_plus")
    # the inference-only encoder has its own slot; `pcd_backbone` is the encoder the training step differentiates: none here
    assert m.gnn_feat_dim == 320 and isinstance(m.pcd_encoder, PointNetPlus) and m.pcd_backbone is None
    sd = m.pcd_encoder.state_dict()
    assert list(sd) == list(GOLD["keys"])
    assert all(tuple(sd[k].shape) == tuple(GOLD[f"shapes/{k}"]) for k in sd)
    m.pcd_encoder.load_state_dict(R.state(), strict=True)
    assert torch.equal(m.pcd_encoder.sa3.mlp_convs[2].weight, R.state()["sa3.mlp_convs.2.weight"])
    # the model's own checkpoint holds the encoder under the reference's name and loads back with strict=True
    full = m.state_dict()
    assert [k[len("pcd_backbone."):] for k in full if k.startswith("pcd_backbone.")] == list(GOLD["keys"])
    assert not any(k.startswith("pcd_encoder") for k in full) and not any(k.startswith("pcd_encoder") for k in full._metadata)
    other = Eff_GAT_3d(10, backbone="pointnet_plus")
    other.load_state_dict(full, strict=True)
    assert torch.equal(other.pcd_encoder.fc2.weight, m.pcd_encoder.fc2.weight) and torch.equal(other.mlp_t[0].weight, m.mlp_t[0].weight)
    missing, unexpected = other.load_state_dict({k: v for k, v in full.items() if not k.startswith("pcd_backbone.")}, strict=False)
    # (a plain dict carries no version metadata: BatchNorm then fills num_batches_tracked in itself and does not report it)
    assert not unexpected and missing == ["pcd_backbone." + k for k in GOLD["keys"] if not k.endswith("num_batches_tracked")]
    for name in ("pointnet_inv",):                    # ("vnn" has no denoiser width: 2168 is no multiple of 64)
        other = Eff_GAT_3d(10, backbone=name)
        assert other.pcd_backbone is None
        with pytest.raises(NotImplementedError, match="'pointnet_inv' and 'vnn' have none: pass pcd_feats"):
            other.pcd_features(torch.zeros(2, 20, 3))


def test_gnn_diffusion_3d_takes_the_backbone():
    from diffassemble_amd.model.backbones.pointnet import PointNetPlus
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion
    m = GNN_Diffusion(steps=20, sampling="DDIM", backbone="pointnet_plus", max_num_part=6)
    assert isinstance(m.model.pcd_encoder, PointNetPlus)
    assert sum(1 for k in m.state_dict() if k.startswith("model.pcd_backbone.")) == len(GOLD["keys"])


def test_refusals_on_the_host():
    from diffassemble_amd import _lib
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.model.backbones.pointnet import PointNetPlus
    from diffassemble_amd.pointnet_plus_encoder import PointNetPlusEngine
    with pytest.raises(NotImplementedError, match="normal_channel"):
        PointNetPlus(normal_channel=True)
    net = PointNetPlus()
    with pytest.raises(NotImplementedError, match=r"follow-up.*inference needs \.eval\(\)"):
        net.train()(torch.zeros(2, 20, 3))
    m = Eff_GAT_3d(10, backbone="pointnet_plus").train()
    for call in (m.pcd_features, m.pcd_features_train):
        with pytest.raises(NotImplementedError, match=r"follow-up.*inference needs \.eval\(\)"):
            call(torch.zeros(2, 20, 3))
    with pytest.raises(_lib.DaError):
        PointNetPlusEngine(net.state_dict(), device="cpu")
    with pytest.raises(_lib.DaError):
        net.eval()(torch.zeros(2, 20, 3))


def test_header_declares_the_functions_and_keeps_the_abi():
    from diffassemble_amd import _lib
    text = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define\s+DA_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19            # additive
    for fn in ("da_pnp_fps", "da_pnp_ball_query", "da_pointnet_plus_workspace_bytes", "da_pointnet_plus_forward", "da_pointnet_plus_stages",
               "da_pointnet_plus_workspace_offsets"):
        assert re.search(r"\b" + fn + r"\s*\(", text), fn
        assert fn in _lib.PROTOTYPES, fn
    assert os.path.exists(os.path.join(ROOT, "diffassemble_amd", "csrc", "da_pointnet_plus.hip"))
