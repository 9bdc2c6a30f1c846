"""Host tests of the discrete position diffusion (no GPU): the closed form of the uniform transition against the reference's
matrix formula (golden_v7.npz, make_golden_v7.py), the fp64 restatements of discrete_cases.py, the module surface and the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import discrete_cases as DC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RTOL32 = 1e-4
# the closed form in fp64 against the reference's fp32 matrix products + torch.linalg.inv, measured when the fixture was generated
# (stored in it): 1.8e-4 at t = 5 (p = 0, where (1 - r) / K is 8e-5 and the fp32 inverse's absolute error shows), 2.6e-5 / 1.4e-5
# at t = 95 / 50.  Bound: 5 x the measured maximum.
POST_MEASURED = 1.8e-4
POST_BOUND = 5 * POST_MEASURED
V = DC.V7
N = sum(V["sizes"])


@pytest.fixture(scope="module")
def g7():
    return DC.load_golden7()


@pytest.fixture(scope="module")
def case():
    return DC.v7_case()


def _module(**kw):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete import GNN_Diffusion
    return GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=V["steps"], inference_ratio=V["ratio"], sampling="DDPM",
                         scheduler=SD.ModelScheduler.LINEAR, **kw)


def test_fixture_measurement_is_the_recorded_one(g7):
    assert float(g7["post/closed_form_max_abs_diff"]) <= POST_MEASURED * 1.01


@pytest.mark.parametrize("t", V["post_t"])
def test_closed_form_equals_reference_posterior(t, g7):
    ac = torch.from_numpy(g7["alphas_cumprod"])
    assert torch.equal(ac, DC.linear_alphas_cumprod(V["steps"]))
    x_t, logits = torch.from_numpy(g7[f"post/t{t}/x_t"]), torch.from_numpy(g7[f"post/t{t}/logits"])
    tt = torch.full((N,), t, dtype=torch.long)
    post = DC.posterior_logits(ac, x_t, logits, tt, tt - V["ratio"])
    err = float((post - torch.from_numpy(g7[f"post/t{t}/post"]).double()).abs().max())
    print(f"t={t}: closed form vs reference posterior, max abs diff {err:.3e} (bound {POST_BOUND:.1e})")
    assert err <= POST_BOUND


def test_module_posterior_equals_restatement(g7):
    m = _module()
    gen = torch.Generator().manual_seed(3)
    x_t = torch.randint(0, V["K"], (N,), generator=gen)
    logits = 3.0 * torch.randn(N, V["K"], generator=gen, dtype=torch.float64)
    t = torch.tensor([0, 5, 10, 50, 95, 99] * (N // 6))
    t = torch.where(t % V["ratio"] == 0, t, t - t % V["ratio"])          # multiples of the ratio: t - ratio >= 0 wherever t > 0
    got = m.q_posterior_logits(x_t, logits, t, t - V["ratio"])
    ref = DC.posterior_logits(m.alphas_cumprod, x_t, logits, t, t - V["ratio"])
    assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-5
    assert torch.equal(got[t == 0], logits[t == 0])
    probs = torch.softmax(logits, -1)
    alt = m.q_posterior_logits(x_t, probs, t, t - V["ratio"], use_x_start_logits=False)
    assert float((alt[t != 0] - ref[t != 0]).abs().max() / ref.abs().max()) <= 1e-5


@pytest.mark.parametrize("t", V["fwd_t"])
def test_restated_forward_matches_reference(t, g7, case):
    idx = torch.from_numpy(g7[f"fwd/t{t}/idx"])
    out = DC.forward_with_feats(case["sd"], idx, torch.full((N,), t, dtype=torch.long), case["edge_index"], case["feats"])
    ref = torch.from_numpy(g7[f"fwd/t{t}/logits"]).double()
    assert float((out - ref).abs().max() / ref.abs().max()) < RTOL32


def test_state_dict_layout_and_reference_checkpoint_loads(g7):
    m = _module()
    ref_keys = g7["statedict/keys"].tolist()
    shapes = dict(zip(ref_keys, g7["statedict/shapes"].tolist()))
    tables = {"Q_onestep", "Q_onestep_transpose", "overline_Q"}
    assert tables <= set(ref_keys)
    mine = {k: v for k, v in m.state_dict().items() if not k.startswith("model.visual_backbone")}
    assert sorted(mine) == sorted(set(ref_keys) - tables)
    for k, v in mine.items():
        assert str(tuple(v.shape)) == shapes[k], k
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete
    b = Eff_GAT_Discrete(steps=V["steps"], input_channels=V["K"], output_channels=V["K"])
    bk = sorted(k for k in b.state_dict() if not k.startswith("visual_backbone"))
    assert bk == sorted(k[len("model."):] for k in ref_keys if k.startswith("model."))
    assert tuple(b.pos_mlp.weight.shape) == (V["K"], 32) and tuple(b.final_mlp[2].weight.shape) == (V["K"], 32)
    # a reference checkpoint carries the three [steps, K, K] tables: it loads (strictly), the tables are dropped
    ck = {k: v.clone() for k, v in m.state_dict().items()}
    for k in tables:
        ck[k] = torch.zeros(V["steps"], V["K"], V["K"])
    ck["model.time_emb.weight"] = torch.full_like(ck["model.time_emb.weight"], 0.25)
    m.load_state_dict(ck, strict=True)
    assert float(m.model.time_emb.weight.detach()[3, 4]) == 0.25
    assert not tables & set(m.state_dict())


def test_abi_surface():
    from diffassemble_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define DA_ABI_VERSION 19\b", hdr) and _lib.ABI_VERSION == 19
    assert re.search(r"DA_VARIANT_DISCRETE = 2\b", hdr) and _lib.VARIANT_DISCRETE == 2
    for fn in ("da_denoiser_forward_idx", "da_d3pm_step", "da_d3pm_noise", "da_sample_loop_idx"):
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
        assert fn in _lib.PROTOTYPES, fn
    assert "typedef struct da_d3pm_opts" in hdr and [f[0] for f in _lib.DaD3pmOpts._fields_] == ["cfg", "cfg_w", "noise", "seed"]
    # float-pose entries on a discrete denoiser are declared to fail
    assert "every entry that takes float poses" in hdr and "REJECTS" in hdr
    src = open(os.path.join(ROOT, "diffassemble_amd", "csrc", "da_api.hip")).read()
    assert src.count("d->variant != DA_VARIANT_DISCRETE") >= 3 and "variant != DA_VARIANT_DISCRETE, \"da_ddim_step" in src


def test_cpu_construction_no_cpu_path_and_training_not_built(case):
    from diffassemble_amd import _lib
    m = _module()
    assert m.discrete is True and m.K == 36 and m.input_channels == 36 and m.output_channels == 36
    assert not any(k in dict(m.named_buffers()) for k in ("Q_onestep", "Q_onestep_transpose", "overline_Q"))
    with pytest.raises(_lib.DaError):
        m.p_sample_loop((N,), None, case["edge_index"], case["batch"], patch_feats=case["feats"])
    with pytest.raises(_lib.DaError):
        with torch.no_grad():
            m.forward_with_feats(torch.zeros(N, dtype=torch.long), torch.zeros(N, dtype=torch.long), None, case["edge_index"],
                                 case["feats"], case["batch"])
    with pytest.raises(NotImplementedError, match="discrete training is not built yet"):
        m.training_step(None, 0)
    with pytest.raises(NotImplementedError, match="discrete training is not built yet"):
        m.p_losses(torch.zeros(N, dtype=torch.long), torch.zeros(N, dtype=torch.long))
    for fn in (m.q_sample, m.vb_terms_bpd):
        with pytest.raises(NotImplementedError, match="discrete training is not built yet"):
            fn()
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete_ROT
    with pytest.raises(NotImplementedError):
        Eff_GAT_Discrete_ROT()
