"""GPU tests of the EfficientNet-B0 piece encoder (model="efficientnet_b0" with use_hip_encoder=True; da_efficientnet.hip through
diffassemble_amd.efficientnet_encoder and model/backbones/efficientnet.py) against the fp64 contract of
tests/golden/efficientnet_refs.py on its generated weights and crops (tests/test_efficientnet_host.py holds the contract's
conditioning and the host packing).

Parity: max |out - contract| <= 1e-4 max |contract| (RTOL32, the project's fp32 parity bound) at each of the eleven block taps and at
the output row; every figure is printed (pytest -s).  Quarter turns, batch invariance, reproducibility and the routes through the
models: bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import efficientnet_refs as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
RTOL32 = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    from diffassemble_amd.efficientnet_encoder import EfficientNetEngine
    return EfficientNetEngine(R.state(torch.float32), device=dev)


def rel(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


@functools.lru_cache(maxsize=None)
def sd64():
    return R.state(torch.float64)


@functools.lru_cache(maxsize=None)
def crops(n, seed=1):
    return torch.from_numpy(R.make_crops(n, seed))


@functools.lru_cache(maxsize=None)
def contract(n, rows=None):
    """The fp64 contract of ``crops(n)`` (of its rows ``rows`` only), computed once and left unchanged."""
    x = crops(n) if rows is None else crops(n)[list(rows)]
    return R.forward(sd64(), x)


def shape_cases(eng):
    """N = 1, 3, one more than the crops of a 1x1 convolution's row tile at the 2 x 2 stage, one more than a chunk."""
    return [1, 3, eng.pw_rows // 4 + 1, eng.chunk + 1]


# ------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["one", "three", "row-tile+1", "chunk+1"])
def test_parity_against_the_fp64_contract(which, eng, dev):
    n = shape_cases(eng)[which]
    assert eng.pw_rows % 4 == 0 and eng.chunk >= 1 and n >= 1
    rows = None if n <= eng.chunk else (0, eng.chunk - 1, eng.chunk)      # across the chunk seam: its two sides and the first row
    ref_taps, ref_row = contract(n, rows)
    taps, out = eng.forward_blocks(crops(n).to(dev))
    assert out.shape == (n, 1088) and out.dtype == torch.float32 and len(taps) == 11
    pick = (lambda t: t) if rows is None else (lambda t: t[list(rows)])
    worst = 0.0
    for b, (t, ref) in enumerate(zip(taps, ref_taps)):
        assert t.shape[1:] == ref.shape[1:] and t.shape[0] == n
        e = rel(pick(t), ref)
        print(f"N={n} block {b} tap {tuple(ref.shape[1:])}: {e:.3e}")
        worst = max(worst, e)
        assert e <= RTOL32, (b, e)
    e = rel(pick(out), ref_row)
    print(f"N={n} output row: {e:.3e} (worst tap {worst:.3e})")
    assert e <= RTOL32, e
    assert torch.equal(eng.forward(crops(n).to(dev)), out)                # the plain entry: the same bits
    # the row is [map 2 | map 3] of the taps in NCHW order
    assert torch.equal(out[:, :640], taps[4].reshape(n, -1)) and torch.equal(out[:, 640:], taps[10].reshape(n, -1))


@pytest.mark.parametrize("turns", [1, 2, 3])
def test_quarter_turns_are_bit_equal_to_turned_crops(turns, eng, dev):
    x = crops(5).to(dev)
    a = eng.forward(x, quarter_turns=turns)
    b = eng.forward(torch.rot90(x, -turns, (2, 3)))
    assert torch.equal(a, b)
    assert not torch.equal(a[0], eng.forward(x)[0])                       # (a turn changes a picture's features)
    assert rel(a, R.forward(sd64(), crops(5), turns)[1]) <= RTOL32
    with pytest.raises(ValueError):
        eng.forward(x, quarter_turns=4)


def test_batch_invariance_and_reproducibility(eng, dev):
    n = eng.pw_rows // 4 + 1
    x = crops(n).to(dev)
    out = eng.forward(x).clone()
    for i in range(n):
        assert torch.equal(eng.forward(x[i:i + 1])[0], out[i]), i
    for _ in range(7):
        assert torch.equal(eng.forward(x), out)
    big = crops(eng.chunk + 1).to(dev)                                    # a crop's row does not depend on its place or its chunk
    ob = eng.forward(big)
    assert torch.equal(eng.forward(big[eng.chunk:])[0], ob[eng.chunk]) and torch.equal(eng.forward(big[eng.chunk - 1:eng.chunk])[0], ob[eng.chunk - 1])


def test_other_shape_cases(eng, dev):
    empty = eng.forward(torch.zeros(0, 3, 32, 32, device=dev))
    assert empty.shape == (0, 1088)
    taps, out = eng.forward_blocks(torch.zeros(0, 3, 32, 32, device=dev))
    assert out.shape == (0, 1088) and [t.shape[0] for t in taps] == [0] * 11
    x = crops(3).to(dev)
    ref = eng.forward(x).clone()
    # a strided out with sentinels around it
    buf = torch.full((3, 1088 + 64), -7.0, device=dev)
    view = buf[:, 32:32 + 1088]
    assert eng.forward(x, out=view) is view
    assert torch.equal(view, ref) and bool((buf[:, :32] == -7).all()) and bool((buf[:, 32 + 1088:] == -7).all())
    # other input dtypes: uint8-derived values, fp16, fp64 (converted to fp32 as torch does)
    u8 = np.rint(R.make_crops(3, 1) * 255).astype(np.uint8)                # (divided on the host: the crops' own k / 255)
    from_u8 = torch.from_numpy(u8.astype(np.float32) / np.float32(255)).to(dev)
    assert torch.equal(from_u8, x) and torch.equal(eng.forward(from_u8), ref)
    assert torch.equal(eng.forward(x.double()), ref)
    assert torch.equal(eng.forward(x.half()), eng.forward(x.half().float()))
    with pytest.raises(Exception):
        eng.forward(x.cpu())
    assert eng.lib.da_effnet_workspace_bytes(eng.chunk) == eng.lib.da_effnet_workspace_bytes(100 * eng.chunk) > eng.lib.da_effnet_workspace_bytes(1) > 0


# ------------------------------------------------------------------------------------------------------ through the models
def _load_encoder(model, dev):
    model.visual_backbone.load_state_dict(R.state(torch.float32), strict=True)
    model.precision = "fp32"
    return model.to(dev).eval()


def test_visual_features_of_the_three_denoisers(eng, dev):
    from diffassemble_amd.model.backbones import Eff_GAT, Eff_GAT_Discrete, Eff_GAT_Discrete_ROT
    x = crops(7).to(dev)
    ref = eng.forward(x)
    torch.manual_seed(0)
    for m in (Eff_GAT(steps=10, visual_pretrained=False, use_hip_encoder=True), Eff_GAT_Discrete(10, 36, 36, use_hip_encoder=True),
              Eff_GAT_Discrete_ROT(10, 36, 36, use_hip_encoder=True)):
        m = _load_encoder(m, dev)
        f = m.visual_features(x)
        assert torch.equal(f, ref) and not f.requires_grad
    f4 = m.visual_features4(x)                                              # m: the rotation model
    assert f4.shape == (4, 7, 1088)
    for r in range(4):
        assert torch.equal(f4[r], eng.forward(torch.rot90(x, -r, (2, 3)))), r
    # all_equivariant: [N, 4, 3, 32, 32] -> the mean of the four single-view calls
    me = _load_encoder(Eff_GAT(steps=10, input_channels=4, output_channels=4, visual_pretrained=False, all_equivariant=True, use_hip_encoder=True), dev)
    views = torch.stack([torch.rot90(x, -r, (2, 3)) for r in range(4)], 1)
    got = me.visual_features(views)
    want = torch.stack([eng.forward(views[:, r]) for r in range(4)]).double().mean(0)
    print(f"all_equivariant vs the mean of four calls: {rel(got, want):.3e}")
    assert got.shape == (7, 1088) and rel(got, want) <= RTOL32


def _puzzle(dev, n=36):
    return W.dense_edge_index(n, True).to(dev), torch.zeros(n, dtype=torch.int64, device=dev)


def test_sampling_loops_from_crops_equal_the_loops_from_features(dev):
    from diffassemble_amd.model import spatial_diffusion as SD, spatial_diffusion_discrete as SDD, spatial_diffusion_discrete_rot as SDR
    ei, batch = _puzzle(dev)
    patches = crops(36).to(dev)
    torch.manual_seed(1)
    m = SD.GNN_Diffusion(steps=100, sampling="DDIM", inference_ratio=10, noise_weight=1.0, visual_pretrained=False, use_hip_encoder=True)
    m.model = _load_encoder(m.model, dev)
    m = m.to(dev).eval()
    torch.manual_seed(5)
    a, _ = m.p_sample_loop((36, 2), patches, ei, batch)
    torch.manual_seed(5)
    b, _ = m.p_sample_loop((36, 2), None, ei, batch, patch_feats=m.visual_features(patches))
    assert len(a) == len(b) == 10 and all(torch.equal(p, q) for p, q in zip(a, b)) and bool(torch.isfinite(a[-1]).all())
    for mod, rot in ((SDD, False), (SDR, True)):
        torch.manual_seed(2)
        m = mod.GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=40, inference_ratio=4, sampling="DDPM", use_hip_encoder=True)
        m.model = _load_encoder(m.model, dev)
        m = m.to(dev).eval()
        feats = m.model.visual_features4(patches) if rot else m.visual_features(patches)
        torch.manual_seed(6)
        a = m.p_sample_loop((36,), patches, ei, batch)
        torch.manual_seed(6)
        b = m.p_sample_loop((36,), None, ei, batch, patch_feats=feats)
        assert len(a) == len(b) == 10
        for p, q in zip(a, b):
            assert all(torch.equal(u, v) for u, v in zip(p, q)) if rot else torch.equal(p, q)


def _train_case(dev):
    from diffassemble_amd.model import spatial_diffusion as SD
    torch.manual_seed(3)
    m = SD.GNN_Diffusion(steps=100, sampling="DDIM", inference_ratio=10, visual_pretrained=False, freeze_backbone=True, use_hip_encoder=True)
    m.model.visual_backbone.load_state_dict(R.state(torch.float32), strict=True)
    m.model.precision = "fp32"
    m = m.to(dev).train()
    ei, bt = _puzzle(dev)
    g = torch.Generator().manual_seed(4)
    batch = SimpleNamespace(x=torch.randn(36, 2, generator=g).to(dev), patches=crops(36).to(dev), edge_index=ei, batch=bt)
    return m, batch


def test_training_step_from_crops_with_a_frozen_encoder(dev):
    m, batch = _train_case(dev)
    enc = m.model.visual_backbone
    enc.frozen_eval_stats = True
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    torch.manual_seed(9)
    loss = m.training_step(batch, 1)
    assert loss.requires_grad and bool(torch.isfinite(loss))
    loss.backward()
    assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for k, p in m.model.named_parameters() if not k.startswith("visual_backbone."))
    assert all(p.grad is None for p in enc.parameters())
    assert all(torch.equal(v, before[k]) for k, v in enc.state_dict().items())
    # the same step from precomputed features: the same draws (t, then the noise inside p_losses), the same loss bits
    m.zero_grad(set_to_none=True)
    feats = m.visual_features(batch.patches)
    assert not feats.requires_grad and torch.equal(feats, enc.engine().forward(batch.patches))
    torch.manual_seed(9)
    t = torch.randint(0, m.steps, (1,), device=dev).long()
    ref = m.p_losses(batch.x, torch.gather(t, 0, batch.batch), loss_type="huber", cond=None, edge_index=batch.edge_index, batch=batch.batch,
                     patch_feats=feats)
    assert torch.equal(ref.detach(), loss.detach())


def test_training_step_on_batch_statistics_is_refused(dev):
    m, batch = _train_case(dev)
    assert m.model.visual_backbone.frozen_eval_stats is False
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm and the backward are not built"):
        m.training_step(batch, 1)
