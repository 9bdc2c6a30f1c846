"""Host tests of the discrete position + rotation diffusion (no GPU): the module surface and state-dict layout against the
reference's (golden_v9.npz, make_golden_v9.py), the fp64 restatements of discrete_rot_cases.py against the reference's logits and
its rotation posterior, the ABI, and what is not built."""
import os
import re

import pytest
import torch

import discrete_cases as DC
import discrete_rot_cases as RC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RTOL32 = 1e-4
# the closed form in fp64 against the reference's fp32 matrix products + torch.linalg.inv with K = 4, measured when the fixture was
# generated (stored in it): 1.8e-4, at t = 5 as for the position tables (test_discrete_host.py).  Bound: 5 x the measured maximum.
POST_MEASURED = 1.8e-4
POST_BOUND = 5 * POST_MEASURED
V = RC.V9
N = sum(V["sizes"])
TABLES = {"Q_onestep", "Q_onestep_transpose", "overline_Q", "overline_Q_rot"}


@pytest.fixture(scope="module")
def g9():
    return RC.load_golden9()


@pytest.fixture(scope="module")
def case():
    return RC.v9_case()


def _module(**kw):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete_rot import GNN_Diffusion
    return GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=V["steps"], inference_ratio=V["ratio"], sampling="DDPM",
                         scheduler=SD.ModelScheduler.LINEAR, **kw)


def test_fixture_measurements_are_the_recorded_ones(g9):
    assert float(g9["post/closed_form_max_abs_diff"]) <= POST_MEASURED * 1.01
    for name in RC.MODE_NAME.values():
        assert int(g9[f"loop/{name}/near_ties"].max()) <= RC.GAP_CAP * g9[f"loop/{name}/traj_index"].size


@pytest.mark.parametrize("t", V["post_t"])
def test_closed_form_equals_reference_rotation_posterior(t, g9):
    ac = torch.from_numpy(g9["alphas_cumprod"])
    assert torch.equal(ac, DC.linear_alphas_cumprod(V["steps"]))
    r_t, rl = torch.from_numpy(g9[f"post/t{t}/rot_t"]), torch.from_numpy(g9[f"post/t{t}/rot_logits"])
    tt = torch.full((N,), t, dtype=torch.long)
    post = DC.posterior_logits(ac, r_t, rl, tt, tt - V["ratio"])
    err = float((post - torch.from_numpy(g9[f"post/t{t}/post"]).double()).abs().max())
    print(f"t={t}: closed form vs reference rotation posterior, max abs diff {err:.3e} (bound {POST_BOUND:.1e})")
    assert err <= POST_BOUND
    m = _module()
    got = m.q_posterior_logits(r_t, rl.double(), tt, tt - V["ratio"], K=4)
    assert float((got - post).abs().max() / post.abs().max()) <= 1e-5


@pytest.mark.parametrize("t", V["fwd_t"])
def test_restated_forward_matches_reference(t, g9, case):
    idx, acc = torch.from_numpy(g9[f"fwd/t{t}/idx"]), torch.from_numpy(g9[f"fwd/t{t}/rot_acc"])
    assert len(set(acc.tolist())) == 4                                    # the recorded forward mixes all four feature images
    lo, rl = RC.forward_with_feats(case["sd"], idx, torch.full((N,), t, dtype=torch.long), case["edge_index"],
                                   RC.select_feats(case["feats4"], acc))
    for got, name in ((lo, "logits"), (rl, "rot_logits")):
        ref = torch.from_numpy(g9[f"fwd/t{t}/{name}"]).double()
        assert got.shape == ref.shape and float((got - ref).abs().max() / ref.abs().max()) < RTOL32, name


def test_restated_step_reproduces_a_recorded_iteration(g9, case):
    ac = torch.from_numpy(g9["alphas_cumprod"])
    p, it, i = "loop/cold/", 3, 80
    idx, rot, acc = (torch.from_numpy(g9[p + "in_" + k][it]) for k in ("index", "rot", "rot_acc"))
    tt = torch.full((N,), i, dtype=torch.long)
    lo, rl = RC.forward_with_feats(case["sd"], idx, tt, case["edge_index"], RC.select_feats(case["feats4"], acc))
    s = RC.rot_step(ac, idx, rot, lo, rl, tt, V["ratio"], torch.from_numpy(g9[p + "u_x"][it]), torch.from_numpy(g9[p + "u_rot"][it]))
    for got, gap, ref in (("x_prev", "gap_x", "x_prev"), ("rot_0", "gap_rot0", "rot_0"), ("rot_prev", "gap_rot", "rot_prev")):
        clear = s[gap] >= RC.GAP
        assert torch.equal(s[got][clear], torch.from_numpy(g9[p + ref][it])[clear]), got
    assert torch.equal(torch.from_numpy(g9[p + "traj_rot_acc"][it]), (acc + torch.from_numpy(g9[p + "rot_prev"][it])) % 4)


def test_state_dict_layout_and_reference_checkpoint_loads(g9):
    m = _module()
    ref_keys = g9["statedict/keys"].tolist()
    shapes = dict(zip(ref_keys, g9["statedict/shapes"].tolist()))
    assert TABLES <= set(ref_keys) and shapes["overline_Q_rot"] == str((V["steps"], 4, 4))
    mine = {k: v for k, v in m.state_dict().items() if not k.startswith("model.visual_backbone")}
    assert sorted(mine) == sorted(set(ref_keys) - TABLES)
    for k, v in mine.items():
        assert str(tuple(v.shape)) == shapes[k], k
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete_ROT
    b = Eff_GAT_Discrete_ROT(steps=V["steps"], input_channels=V["K"], output_channels=V["K"])
    bk = sorted(k for k in b.state_dict() if not k.startswith("visual_backbone"))
    assert bk == sorted(k[len("model."):] for k in ref_keys if k.startswith("model."))
    assert tuple(b.final_mlp_rot[0].weight.shape) == (32, 1152) and tuple(b.final_mlp_rot[2].weight.shape) == (4, 32)
    assert b.rotation_channels == 4 and b.variant == "discrete_rot"
    # a reference checkpoint carries the four transition tables: it loads (strictly), the tables are dropped
    ck = {k: v.clone() for k, v in m.state_dict().items()}
    for k in TABLES - {"overline_Q_rot"}:
        ck[k] = torch.zeros(V["steps"], V["K"], V["K"])
    ck["overline_Q_rot"] = torch.zeros(V["steps"], 4, 4)
    ck["model.final_mlp_rot.2.bias"] = torch.full_like(ck["model.final_mlp_rot.2.bias"], 0.25)
    m.load_state_dict(ck, strict=True)
    assert float(m.model.final_mlp_rot[2].bias.detach()[3]) == 0.25
    assert not TABLES & set(m.state_dict())


def test_module_attributes(g9):
    m = _module()
    assert (m.rot_K, m.only_rotation, m.cold_diffusion, m.losses_keys) == (4, False, False, ["rot_loss", "x_loss"])
    assert m.discrete is True and m.K == 36
    m = _module(only_rotation=True, cold_diffusion=True)
    assert (m.only_rotation, m.cold_diffusion, m.losses_keys) == (True, True, ["rot_loss"])
    assert "overline_Q_rot" not in dict(m.named_buffers())


def test_abi_surface():
    from diffassemble_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define DA_ABI_VERSION 19\b", hdr) and _lib.ABI_VERSION == 19            # additive
    assert re.search(r"DA_VARIANT_DISCRETE_ROT = 3\b", hdr) and _lib.VARIANT_DISCRETE_ROT == 3
    assert re.search(r"DA_D3PM_DRAW_SAMPLING_ROT = 2\b", hdr) and _lib.D3PM_DRAW_SAMPLING_ROT == 2
    for fn in ("da_denoiser_set_features_rot", "da_denoiser_forward_rot", "da_d3pm_rot_step", "da_sample_loop_rot"):
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
        assert fn in _lib.PROTOTYPES, fn
    assert "typedef struct da_d3pm_rot_opts" in hdr
    assert [f[0] for f in _lib.DaD3pmRotOpts._fields_] == ["cold", "reserved0", "x_fixed", "noise_x", "noise_rot", "seed"]
    src = open(os.path.join(ROOT, "diffassemble_amd", "csrc", "da_api.hip")).read()
    # float-pose entries reject the variant; the _idx entries name the rot entries
    assert src.count("d->variant != DA_VARIANT_DISCRETE_ROT") >= 5 and "da_sample_loop_idx: a discrete rot denoiser" in src
    assert "(da_sample_loop_rot)" in src and "da_denoiser_forward_rot)" in src


def test_no_cpu_path_and_training_not_built(case):
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    m = _module()
    z = torch.zeros(N, dtype=torch.long)
    with pytest.raises(_lib.DaError):
        m.p_sample_loop((N,), None, case["edge_index"], case["batch"], patch_feats=case["feats4"])
    with pytest.raises(_lib.DaError):
        with torch.no_grad():
            m.forward_with_feats(z, z, None, case["edge_index"], case["feats4"], z, case["batch"], rot_acc=z)
    with pytest.raises(_lib.DaError):
        E.d3pm_rot_step(None, z, z, torch.zeros(N, 36), torch.zeros(N, 4), 5, 5)
    with pytest.raises(NotImplementedError, match="discrete-rotation training is not built yet"):
        m.training_step(None, 0)
    with pytest.raises(NotImplementedError, match="discrete-rotation training is not built yet"):
        m.p_losses(z, z, z)
    m.model.train()
    with pytest.raises(NotImplementedError, match="discrete-rotation training is not built yet"):
        m.model.forward_with_feats(z, z, z, None, case["edge_index"], case["feats4"][0], case["batch"])
    m.model.eval()
    # without timm / kornia the module cannot encode the four rotated crops itself
    if m.model.visual_backbone is None:
        with pytest.raises(NotImplementedError, match="pass precomputed patch_feats"):
            m.p_sample_loop((N,), torch.zeros(N, 3, 32, 32), case["edge_index"], case["batch"])
    with pytest.raises(ValueError, match="x_start"):
        _module(only_rotation=True).p_sample_loop((N,), None, case["edge_index"], case["batch"], patch_feats=case["feats4"])
