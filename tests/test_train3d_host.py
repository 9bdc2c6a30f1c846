"""Host-side tests of the 3D training step (no GPU): the IGSO(3) CDF table against the reference's own columns
(golden_v6.npz), the new entry points' bindings and argument checks, the 3D flat-buffer parameter order, and the
refusals of GNN_Diffusion.p_losses."""
import ctypes as C

import numpy as np
import pytest
import torch

import train3d_cases as T3


@pytest.fixture(scope="module")
def golden6():
    return T3.load_golden6()


def test_trap_table_rows_equal_the_reference_columns_bit_for_bit(golden6):
    """Row t of igso3_trap_table = the column IsotropicGaussianSO3 builds for a piece with eps = sqrt_one_minus_alphas_cumprod[t]."""
    from diffassemble_amd.engine import igso3_trap_table
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion
    somac = torch.from_numpy(golden6["igso3/sqrt_one_minus_alphas_cumprod"])
    m = GNN_Diffusion(steps=T3.STEPS, sampling="DDIM", backbone="vn_dgcnn", max_num_part=T3.MAX_PARTS)
    assert torch.equal(m.sqrt_one_minus_alphas_cumprod, somac)          # the module's schedule is the reference's
    table = igso3_trap_table(m.sqrt_one_minus_alphas_cumprod)
    assert table.shape == (T3.STEPS, 999) and table.dtype == torch.float32 and table.is_contiguous()
    ts = golden6["igso3/t"].tolist()
    assert tuple(ts) == T3.TRAP_T
    ref = torch.from_numpy(golden6["igso3/trap"])
    assert ref.shape == (len(ts), 999)
    for i, t in enumerate(ts):
        assert torch.equal(table[t], ref[i]), t
    assert bool(torch.isfinite(table).all())
    assert bool((table[:, 1:] >= table[:, :-1]).all())
    assert bool((table[:, -1] == 1.0).all()) and bool((table >= 0).all())


def test_fixture_quaternions_are_away_from_the_sign_flip(golden6):
    """What make_golden_v6.py selected its seeds for: |w| >= 1e-3 on every x_noisy / predicted quaternion, no ground-truth rotation near pi."""
    for spec in T3.TRAIN3D:
        for key in ("x_noisy", "prediction"):
            assert float(np.abs(golden6[f"{spec['name']}/{key}"][:, 0]).min()) >= T3.W_MIN, (spec["name"], key)
        gt = T3.build_case(spec)["x_start"]
        angle = 2 * torch.acos(gt[:, 0].double().clamp(-1, 1))
        assert float((angle - np.pi).abs().min()) > 1e-3


def test_new_symbols_are_declared_and_bound_and_the_abi_stays_19():
    from diffassemble_amd import _lib
    h = _lib.lib()
    for name in ("da_head3d_backward", "da_q_sample_se3"):
        assert name in _lib.PROTOTYPES
        fn = getattr(h, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["da_q_sample_se3"][1]) == 12 and len(_lib.PROTOTYPES["da_head3d_backward"][1]) == 5
    assert h.da_abi_version() == _lib.ABI_VERSION == 19


def test_entry_points_reject_bad_arguments_before_launching():
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(4096)          # never dereferenced: every call below is refused by its argument check
    assert h.da_head3d_backward(4, None, one, one, None) != 0 and b"null" in h.da_last_error()
    assert h.da_head3d_backward(4, one, None, one, None) != 0
    assert h.da_head3d_backward(4, one, one, None, None) != 0
    assert h.da_head3d_backward(-1, one, one, one, None) != 0 and b"n < 0" in h.da_last_error()
    assert h.da_head3d_backward(0, one, one, one, None) == 0          # nothing to do
    good = [one] * 9
    for missing in range(9):
        args = list(good)
        args[missing] = None
        assert h.da_q_sample_se3(300, 4, *args, None) != 0, missing
        assert b"null" in h.da_last_error()
    assert h.da_q_sample_se3(300, -1, *good, None) != 0
    assert h.da_q_sample_se3(0, 4, *good, None) != 0
    assert h.da_q_sample_se3(300, 0, *good, None) == 0
    # the training entry points: a 3D denoiser takes c_in = 7 only
    w, g = _lib.DaWeights(), _lib.DaGraph()
    w.variant, w.arch, w.steps, w.c_in, w.c_out, w.feat_dim, w.hidden, w.heads, w.n_layers = _lib.VARIANT_3D, 0, 300, 4, 7, 768, 256, 8, 4
    g.n_nodes = g.n_real = 13
    g.n_graphs = 1
    assert h.da_train_workspace_bytes_ex(C.byref(w), C.byref(g), _lib.TRAIN_MMA_FP32) == 0 and b"c_in must be 7" in h.da_last_error()
    assert h.da_train_forward_ex(C.byref(w), C.byref(g), one, one, one, one, one, 1 << 20, _lib.TRAIN_MMA_FP32, None) != 0
    assert b"c_in must be 7" in h.da_last_error()
    assert h.da_train_backward_stage(C.byref(w), C.byref(w), C.byref(g), one, one, one, None, one, 1 << 20, _lib.TRAIN_MMA_FP32,
                                     _lib.TRAIN_BWD_ALL, None) != 0
    w.c_in, w.variant = 7, 2
    assert h.da_train_workspace_bytes_ex(C.byref(w), C.byref(g), _lib.TRAIN_MMA_FP32) == 0 and b"variant" in h.da_last_error()


@pytest.mark.parametrize("arch", ["transformer", "exophormer", "gcn"])
def test_param_order_3d_covers_every_denoiser_parameter_once(arch):
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.train import _param_order
    m = Eff_GAT_3d(steps=50, architecture=arch, backbone="vn_dgcnn", n_layers=4, virt_nodes=8)
    names, n_layers = _param_order(m)
    own = sorted(k for k, _ in m.named_parameters() if not k.startswith("pcd_backbone."))
    assert sorted(names) == own and len(set(names)) == len(names)
    assert n_layers == (2 if arch == "gcn" else 4)
    assert not any(n.startswith("final_mlp.") for n in names)
    i = names.index("mlp_t.0.weight")
    assert names[i:i + 4] == ["mlp_t.0.weight", "mlp_r.0.weight", "mlp_t.0.bias", "mlp_r.0.bias"]       # one gap-free 512-row slot
    sd = T3.make_state(arch, 50, 1)
    assert sorted(sd) == own                                          # ... and the cases' state dicts have the module's keys


def test_p_losses_refuses_what_the_reference_cannot_run():
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=20, sampling="DDIM", backbone="vn_dgcnn", max_num_part=6, model_mean_type=ModelMeanType.START_X)
    x = torch.zeros(3, 7)
    for lt in ("l1", "split"):
        with pytest.raises(NotImplementedError):
            m.p_losses(x, None, loss_type=lt)                         # before t is touched
    m = GNN_Diffusion(steps=20, sampling="DDIM", backbone="vn_dgcnn", max_num_part=6, model_mean_type=ModelMeanType.EPSILON)
    with pytest.raises(NotImplementedError, match="TypeError"):
        m.p_losses(x, None, loss_type="all")
