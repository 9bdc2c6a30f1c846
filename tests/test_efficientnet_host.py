"""Host tests of the EfficientNet-B0 piece encoder (no GPU): the module's keys against the contract of
tests/golden/efficientnet_refs.py, the host packing of diffassemble_amd.efficientnet_encoder against the unfolded NCHW chain, the
conditioning of the generated weights, the opt-in wiring (use_hip_encoder) and the refusals."""
import os
import re

import numpy as np
import pytest
import torch

import efficientnet_refs as R

RTOL32 = 1e-4                                        # the GPU parity bound of tests/test_gpu_efficientnet.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "efficientnet_v1.npz"))


def rel(a, ref):
    a, ref = torch.as_tensor(a).detach().double(), torch.as_tensor(ref).detach().double()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


@pytest.fixture(scope="module")
def module():
    from diffassemble_amd.model.backbones.efficientnet import EfficientNetB0Features
    torch.manual_seed(0)
    return EfficientNetB0Features()


@pytest.fixture(scope="module")
def sd64():
    return R.state(torch.float64)


@pytest.fixture(scope="module")
def crops():
    return torch.from_numpy(R.make_crops(6, 1))


@pytest.fixture(scope="module")
def ref64(sd64, crops):
    return R.forward(sd64, crops)


def test_the_generators_give_the_recorded_fixture():
    sd = R.make_weights()
    assert [str(k) for k in GOLD["keys"]] == list(sd) and int(GOLD["weight_seed"]) == R.WEIGHT_SEED
    assert [tuple(int(v) for v in s.split("x") if v) for s in GOLD["shapes"]] == [tuple(v.shape) for v in sd.values()]
    assert str(GOLD["weights_sha256"]) == R.digest(sd.values())
    assert str(GOLD["crops_sha256"]) == R.digest([R.make_crops(6, 1)])
    c = R.make_crops(6, 1)
    assert c.dtype == np.float32 and np.array_equal(np.rint(c * 255) / np.float32(255), c)
    assert not c[5].any() and (c[4] == 1).all() and c[3].sum() == 3 and (c[3][:, 0, 31] == 1).all()


def test_module_keys_order_and_shapes(module):
    got = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    assert got == R.key_shapes()
    shapes = dict(got)
    assert sum(p.numel() for p in module.parameters()) == 3595388
    assert sum(p.numel() for k, p in module.named_parameters() if not k.startswith(("blocks.5.", "blocks.6."))) == 851808
    assert shapes["blocks.0.0.se.conv_reduce.weight"] == (8, 32, 1, 1)
    assert shapes["blocks.1.0.se.conv_reduce.weight"] == (4, 96, 1, 1)
    assert shapes["blocks.2.0.conv_dw.weight"] == (144, 1, 5, 5)
    assert shapes["blocks.4.2.conv_pwl.weight"] == (112, 672, 1, 1)
    assert shapes["blocks.6.0.bn3.running_var"] == (320,)
    for k in ("blocks.0.0.conv_pw.weight", "blocks.0.0.bn2.weight", "blocks.1.0.conv_pwl.weight", "blocks.1.0.bn3.bias"):
        assert k in shapes
    assert "blocks.0.0.conv_pwl.weight" not in shapes and "blocks.0.0.bn3.weight" not in shapes


def test_module_initialisation(module):
    sd = module.state_dict()
    for k, v in sd.items():
        if k.endswith("running_var") or (".bn" in "." + k and k.endswith(".weight")):
            assert bool((v == 1).all()), k
        elif k.endswith(("running_mean", ".bias")):
            assert bool((v == 0).all()), k
    w = sd["blocks.4.2.conv_pwl.weight"]                                 # fan_out = 1 * 1 * 112
    assert abs(float(w.std()) / (2.0 / 112) ** 0.5 - 1) < 0.05
    w = sd["blocks.2.0.conv_dw.weight"]                                  # fan_out = 5 * 5 * 144 / 144
    assert abs(float(w.std()) / (2.0 / 25) ** 0.5 - 1) < 0.05


def test_one_crop_costs_5_11_million_multiply_adds():
    from diffassemble_amd import efficientnet_encoder as E
    macs = 27 * 32 * 256
    for p, cin, mid, cout, k, s, r, h, skip in E.BLOCKS:
        ho = h // s
        macs += (0 if p == "blocks.0.0" else cin * mid * h * h) + k * k * mid * ho * ho + 2 * mid * r + mid * cout * ho * ho
    assert round(macs / 1e6, 2) == 5.11, macs
    assert [(p, cin, mid, cout, k, s, r) for p, cin, mid, cout, k, s, r, h, skip in E.BLOCKS] == \
        [(p, cin, mid, cout, k, s, r) for p, cin, mid, cout, k, s, r, ds in R.live_blocks()]
    assert [b[0] for b in E.BLOCKS].index(R.MAP2) == E.MAP2 and [b[0] for b in E.BLOCKS].index(R.MAP3) == E.MAP3


def test_turn_source_is_a_clockwise_quarter_turn():
    from diffassemble_amd import efficientnet_encoder as E
    x = torch.arange(2 * 3 * 32 * 32, dtype=torch.float32).view(2, 3, 32, 32)
    for r in range(4):
        si, sj = E.turn_source(r)
        assert torch.equal(x[:, :, si, sj], torch.rot90(x, -r, (2, 3))), r
    with pytest.raises(ValueError):
        E.turn_source(4)


@pytest.mark.parametrize("turns", [0, 1, 2, 3])
def test_packing_equals_the_unfolded_chain(turns, sd64, crops, ref64):
    """Fold, K padding, flatten order and quarter-turn index map: the packed weights through the NHWC evaluator against the
    contract, both fp64."""
    from diffassemble_amd import efficientnet_encoder as E
    packed = E.pack(sd64)
    taps, rows = R.forward_packed(packed, E.BLOCKS, E.turn_source, crops, turns)
    ref_taps, ref_row = ref64 if turns == 0 else R.forward(sd64, crops, turns)
    assert len(taps) == len(ref_taps) == 11
    for b, (a, ref) in enumerate(zip(taps, ref_taps)):
        assert a.shape == ref.shape == (6, *E.tap_shape(b)) and rel(a, ref) < 1e-12, (b, rel(a, ref))
    row = torch.cat([rows[E.MAP2], rows[E.MAP3]], -1)
    assert row.shape == (6, E.OUT_DIM) and rel(row, ref_row) < 1e-12
    for f in ("exp_w", "prj_w", "dw_w", "se_rw", "se_ew"):             # every width the kernels stride by is a multiple of 16
        assert all(t is None or t.shape[-1] % 16 == 0 for t in packed[f]), f
    assert all(t.shape[0] % 16 == 0 for t in packed["prj_w"]) and packed["exp_w"][0] is None


def test_the_contract_is_well_conditioned(sd64, crops, ref64):
    """The contract in fp32 on the CPU against itself in fp64: under a quarter of the GPU bound at every tap and the row, so the
    GPU bound measures the kernels and not the weights."""
    taps32, row32 = R.forward(R.state(torch.float32), crops)
    for b, (a, ref) in enumerate(zip(taps32 + [row32], ref64[0] + [ref64[1]])):
        print(f"fp32 contract vs fp64, tap {b}: {rel(a, ref):.3e}")
        assert rel(a, ref) < RTOL32 / 4, (b, rel(a, ref))
        assert float(ref.abs().max()) > 1.0 and float(ref.std()) > 0.1, b        # nothing died on the way


# ------------------------------------------------------------------------------------------------------ wiring
def _models(**kw):
    from diffassemble_amd.model.backbones import Eff_GAT, Eff_GAT_Discrete, Eff_GAT_Discrete_ROT
    return [Eff_GAT(steps=10, visual_pretrained=False, **kw), Eff_GAT_Discrete(10, 36, 36, **kw), Eff_GAT_Discrete_ROT(10, 36, 36, **kw)]


def _diffusions(**kw):
    from diffassemble_amd.model import spatial_diffusion as SD, spatial_diffusion_discrete as SDD, spatial_diffusion_discrete_rot as SDR
    return [SD.GNN_Diffusion(steps=10, visual_pretrained=False, **kw), SDD.GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=10, **kw),
            SDR.GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=10, **kw)]


def _timm_absent():
    try:
        import timm  # noqa: F401
        return False
    except Exception:  # noqa: BLE001
        return True


def test_default_construction_is_unchanged():
    for m in _models() + [d.model for d in _diffusions()]:
        assert m.use_hip_encoder is False
        if _timm_absent():
            assert m.visual_backbone is None
            with pytest.raises(NotImplementedError, match="patch_feats"):
                m.visual_features(torch.zeros(2, 3, 32, 32))
    assert all(d.use_hip_encoder is False for d in _diffusions())


def test_use_hip_encoder_builds_the_module_everywhere():
    from diffassemble_amd.model.backbones import Eff_GAT
    from diffassemble_amd.model.backbones.efficientnet import EfficientNetB0Features
    for m in _models(use_hip_encoder=True) + [d.model for d in _diffusions(use_hip_encoder=True)]:
        assert isinstance(m.visual_backbone, EfficientNetB0Features) and m.use_hip_encoder is True
        assert m.combined_features_dim == 1088 + 64
    from diffassemble_amd.model.backbones.resnet_equivariant import ResNet
    assert isinstance(Eff_GAT(steps=10, model="resnet18equiv", use_hip_encoder=True).visual_backbone, ResNet)
    for model in ("resnet18", "resnet50"):
        with pytest.raises(NotImplementedError, match="use_hip_encoder"):
            Eff_GAT(steps=10, model=model, use_hip_encoder=True)


def test_state_dict_round_trips_strictly():
    enc = R.state(torch.float32)
    for m in _models(use_hip_encoder=True):
        sd = m.state_dict()
        assert [k[len("visual_backbone."):] for k in sd if k.startswith("visual_backbone.")] == list(enc)
        sd.update({"visual_backbone." + k: v for k, v in enc.items()})
        m.load_state_dict(sd, strict=True)
        assert torch.equal(m.visual_backbone.blocks[6][0].bn3.running_var, enc["blocks.6.0.bn3.running_var"])
        other = type(m)(10, 36, 36, use_hip_encoder=True) if type(m).__name__ != "Eff_GAT" else type(m)(steps=10, use_hip_encoder=True)
        other.load_state_dict(m.state_dict(), strict=True)
        assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), m.state_dict().values()))


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals(module):
    from diffassemble_amd import _lib
    from diffassemble_amd.efficientnet_encoder import EfficientNetEngine
    with pytest.raises(_lib.DaError, match="ROCm device"):
        EfficientNetEngine(R.state(), device="cpu")
    module.train()
    try:
        with pytest.raises(NotImplementedError, match="frozen_eval_stats = True"):
            module.patch_features(torch.zeros(1, 3, 32, 32))
    finally:
        module.eval()
    with pytest.raises(NotImplementedError, match="patch_features"):
        module(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_lib.DaError):                                     # eval mode on the CPU: the engine refuses, nothing falls back
        module.patch_features(torch.zeros(1, 3, 32, 32))


def test_header_declares_the_entries_and_keeps_the_abi():
    text = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define DA_ABI_VERSION 19\b", text)
    for name in ("da_effnet_workspace_bytes", "da_effnet_forward", "da_effnet_forward_taps", "da_effnet_constant"):
        assert re.search(r"\b%s\(" % name, text), name
    assert "typedef struct da_effnet_weights" in text
    from diffassemble_amd import _lib
    for name in ("da_effnet_workspace_bytes", "da_effnet_forward", "da_effnet_forward_taps", "da_effnet_constant"):
        assert name in _lib.PROTOTYPES
    fields = re.search(r"typedef struct da_effnet_weights \{(.*?)\} da_effnet_weights;", text, re.S).group(1)
    assert re.findall(r"const float \*(\w+)", fields) == [f for f, _ in _lib.DaEffnetWeights._fields_]
