"""Host-side tests of the 3D model with ``use_6dof=True`` (no GPU): the constructor and its state-dict layout against the
reference's own (golden_v11.npz), the new entry points' declarations, bindings and argument checks, the closed-form backward of
``da_rot6d_to_pose`` (rot6d_refs.py, the kernel's contract) against torch autograd in fp64, what the fixture's seeds were
selected for, and the refusals the mode keeps."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rot6d_refs as R6
import train3d_6dof_cases as T6

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = {"da_head3d_backward_ex": 6, "da_q_sample_se3_6d": 12, "da_rot6d_to_pose": 5, "da_rot6d_to_pose_backward": 6}


@pytest.fixture(scope="module")
def golden11():
    return T6.load_golden11()


def module_6dof(arch="transformer", steps=T6.STEPS, **kw):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    kw.setdefault("model_mean_type", ModelMeanType.START_X)
    return GNN_Diffusion(steps=steps, sampling="DDIM", backbone="vn_dgcnn", architecture=arch, max_num_part=T6.MAX_PARTS,
                         use_6dof=True, **kw)


def test_constructor_has_the_reference_state_dict_layout(golden11):
    """GNN_Diffusion(use_6dof=True): input_channels 13, t_channels 9, and the denoiser's state dict = the reference's dump, names,
    order and shapes (pos_mlp.0.weight [16, 13], mlp_t.2 [9, 256] / [9], mlp_r.2 [3, 256])."""
    m = module_6dof()
    assert m.use_6dof and m.input_channels == 13 and m.model.input_channels == 13
    own = {k: v for k, v in m.model.state_dict().items() if not k.startswith("pcd_backbone.")}
    names = [str(k) for k in golden11["state_dict/names"]]
    shapes = [tuple(int(d) for d in s if d) for s in golden11["state_dict/shapes"]]
    assert list(own) == names
    assert [tuple(v.shape) for v in own.values()] == shapes
    assert tuple(own["pos_mlp.0.weight"].shape) == (16, 13) and tuple(own["mlp_t.2.weight"].shape) == (9, 256)
    assert tuple(own["mlp_t.2.bias"].shape) == (9,) and tuple(own["mlp_r.2.weight"].shape) == (3, 256)
    sd = T6.make_state("transformer", T6.STEPS, 1)
    assert sorted(sd) == sorted(names) and all(tuple(sd[k].shape) == s for k, s in zip(names, shapes))
    missing, unexpected = m.model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    # the 7-channel constructor is what it was
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion
    m7 = GNN_Diffusion(steps=20, sampling="DDIM", backbone="vn_dgcnn", max_num_part=6)
    assert tuple(m7.model.pos_mlp[0].weight.shape) == (16, 7) and tuple(m7.model.mlp_t[2].weight.shape) == (3, 256)


@pytest.mark.parametrize("arch", ["transformer", "exophormer", "gcn"])
def test_param_order_covers_the_13_channel_module(arch):
    from diffassemble_amd.train import _param_order
    m = module_6dof(arch, steps=50).model
    names, _ = _param_order(m)
    own = sorted(k for k, _ in m.named_parameters() if not k.startswith("pcd_backbone."))
    assert sorted(names) == own == sorted(T6.make_state(arch, 50, 1))


def test_new_entries_are_declared_and_bound_and_the_abi_stays_19():
    from diffassemble_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    h = _lib.lib()
    for name, nargs in NEW.items():
        assert f"int {name}(" in hdr, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        fn = getattr(h, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert "#define DA_ABI_VERSION 19" in hdr
    assert h.da_abi_version() == _lib.ABI_VERSION == 19
    assert len(_lib.PROTOTYPES["da_q_sample_se3"][1]) == 12 and len(_lib.PROTOTYPES["da_head3d_backward"][1]) == 5      # unchanged


def test_entry_points_reject_bad_arguments_before_launching():
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(4096)          # never dereferenced: every call below is refused by its argument check (or has nothing to do)
    assert h.da_rot6d_to_pose(4, None, 13, one, None) != 0 and b"null" in h.da_last_error()
    assert h.da_rot6d_to_pose(4, one, 13, None, None) != 0
    assert h.da_rot6d_to_pose(4, one, 12, one, None) != 0 and b"ld >= 13" in h.da_last_error()
    assert h.da_rot6d_to_pose(-1, one, 13, one, None) != 0
    assert h.da_rot6d_to_pose(0, one, 13, one, None) == 0
    for missing in range(3):
        args = [one, 13, one, one]
        args[(0, 2, 3)[missing]] = None
        assert h.da_rot6d_to_pose_backward(4, *args, None) != 0 and b"null" in h.da_last_error()
    assert h.da_rot6d_to_pose_backward(4, one, 7, one, one, None) != 0 and b"ld >= 13" in h.da_last_error()
    assert h.da_rot6d_to_pose_backward(0, one, 13, one, one, None) == 0
    assert h.da_head3d_backward_ex(4, 6, one, one, one, None) != 0 and b"neither 3 nor 9" in h.da_last_error()
    assert h.da_head3d_backward_ex(4, 9, None, one, one, None) != 0 and b"null" in h.da_last_error()
    assert h.da_head3d_backward_ex(0, 9, one, one, one, None) == 0
    good = [one] * 9
    for missing in range(9):
        args = list(good)
        args[missing] = None
        assert h.da_q_sample_se3_6d(300, 4, *args, None) != 0 and b"null" in h.da_last_error(), missing
    assert h.da_q_sample_se3_6d(0, 4, *good, None) != 0
    assert h.da_q_sample_se3_6d(300, 0, *good, None) == 0


def test_3d_variant_takes_7_or_13_channels_and_nothing_else():
    """da_denoiser_create and the training entries: c_in = 13 selects the mode, any other width but 7 is refused with a message."""
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(4096)
    w, g = _lib.DaWeights(), _lib.DaGraph()
    w.variant, w.arch, w.steps, w.c_out, w.feat_dim, w.hidden, w.heads, w.n_layers = _lib.VARIANT_3D, 0, 300, 9, 768, 256, 8, 4
    g.n_nodes = g.n_real = 13
    g.n_graphs = 1
    for c_in in (4, 8, 9, 12, 14, 16):
        w.c_in = c_in
        handle = C.c_void_p()
        assert h.da_denoiser_create(C.byref(w), _lib.PREC_F32, None, C.byref(handle)) != 0 and not handle.value
        assert b"neither 7 nor 13" in h.da_last_error(), c_in
        assert h.da_train_workspace_bytes_ex(C.byref(w), C.byref(g), _lib.TRAIN_MMA_FP32) == 0
        assert b"c_in must be 7" in h.da_last_error() and b"13" in h.da_last_error()
        assert h.da_train_forward_ex(C.byref(w), C.byref(g), one, one, one, one, one, 1 << 20, _lib.TRAIN_MMA_FP32, None) != 0
    w.variant, w.c_in = _lib.VARIANT_2D, 13          # the 2D model keeps its limit
    handle = C.c_void_p()
    assert h.da_denoiser_create(C.byref(w), _lib.PREC_F32, None, C.byref(handle)) != 0 and b"outside [1, 8]" in h.da_last_error()
    assert h.da_ddim_step(C.byref(_lib.DaSchedule()), _lib.VARIANT_3D, _lib.MEAN_START_X, 4, 9, one, one, None, 0, 1, 1, 0.0, None, one, None) != 0
    assert b"c must be 7, or 13" in h.da_last_error()


def gradient_rows(n_random=300, seed=17):
    g = torch.Generator().manual_seed(seed)
    pred = torch.cat([R6.special_rows(), torch.randn(n_random, 13, generator=g, dtype=torch.float64)])
    pred[:, :7] = torch.randn(pred.shape[0], 7, generator=g, dtype=torch.float64)
    return pred, torch.randn(pred.shape[0], 7, generator=g, dtype=torch.float64)


def test_closed_form_backward_equals_fp64_autograd():
    """rot6d_refs.rot6d_to_pose_backward (the formula the kernel implements) against torch autograd through F.normalize / cross /
    stack / matrix_to_quaternion in fp64: 300 random rows plus a1 parallel to e_x, a2 nearly parallel to a1 (sine 1e-2), |a1| = 1e-3
    and w = 1e-3 on either side of the standardisation.  1e-10 relative, per row and overall."""
    pred, g = gradient_rows()
    want, pose = R6.rot6d_to_pose_autograd(pred, g)
    got = R6.rot6d_to_pose_backward(pred, g)
    assert torch.equal(R6.rot6d_to_pose(pred), pose)
    assert float((pose[:, :4].norm(dim=1) - 1).abs().max()) < 1e-12 and float(pose[:, 0].min()) >= 0
    assert abs(float(pose[3, 0]) - 1e-3) < 1e-9 and abs(float(pose[4, 0]) - 1e-3) < 1e-9           # the two rows at the sign flip
    assert torch.equal(got[:, :4], torch.zeros_like(got[:, :4])) and torch.equal(want[:, :4], got[:, :4])
    assert torch.equal(got[:, 4:7], g[:, 4:7]) and torch.equal(want[:, 4:7], g[:, 4:7])
    row = (got - want).abs().amax(1) / want.abs().amax(1)
    print(f"closed form vs autograd: worst row {float(row.max()):.3e}, overall {float((got - want).abs().max() / want.abs().max()):.3e}")
    assert float(row.max()) < 1e-10
    assert float((got - want).abs().max() / want.abs().max()) < 1e-10


def test_closed_form_backward_is_finite_on_a_zero_row():
    pred, g = torch.zeros(2, 13), torch.ones(2, 7)
    pose, grad = R6.rot6d_to_pose(pred), R6.rot6d_to_pose_backward(pred, g)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(grad).all())


def test_fixture_rows_are_away_from_the_sign_flip_and_the_clamp(golden11):
    """What make_golden_v11.py selected its seeds for, on the stored data: |w| >= 1e-3 on every x_noisy, head and Gram-Schmidt
    quaternion, |a1| and |a2 - (a2.b1) b1| > 1e-6, no ground-truth rotation near pi -- for the three steps and for every
    trajectory entry."""
    for spec in T6.TRAIN3D_6DOF:
        name = spec["name"]
        assert golden11[f"{name}/noise_tr"].shape[1] == 9
        for key in ("x_noisy", "prediction"):
            rows = golden11[f"{name}/{key}"]
            assert rows.shape[1] == 13 and float(np.abs(rows[:, 0]).min()) >= T6.W_MIN, (name, key)
        w, n1, n2 = R6.gs_margins(torch.from_numpy(golden11[f"{name}/prediction"]))
        assert w >= T6.W_MIN and n1 > T6.A_MIN and n2 > T6.A_MIN, (name, w, n1, n2)
        gt = T6.build_case(spec)["x_start"]
        assert float((2 * torch.acos(gt[:, 0].double().clamp(-1, 1)) - np.pi).abs().min()) > 1e-3
        dead = [k for k in golden11.files if k.startswith(f"{name}/grad_stats/mlp_r.")]
        assert len(dead) == 4 and all(float(golden11[k][1]) == 0.0 for k in dead)           # the head's quaternion carries no loss
        assert float(golden11[f"{name}/grad_stats/mlp_t.2.weight"][1]) > 0
    traj = torch.from_numpy(golden11["loop/traj"])
    assert traj.shape == (T6.LOOP_ITERS, sum(T6.SIZES), 13)
    assert float(traj[..., 0].abs().min()) >= T6.W_MIN
    w, n1, n2 = R6.gs_margins(traj)
    assert w >= T6.W_MIN and n1 > T6.A_MIN and n2 > T6.A_MIN, (w, n1, n2)
    pose = torch.from_numpy(golden11["loop/pose7"])
    assert float((R6.rot6d_to_pose(traj[-1].double()) - pose.double()).abs().max()) < 1e-6          # the evaluation's plain divisions = F.normalize
    assert golden11["loop/metrics"].shape == (len(T6.SIZES), 4)


def test_mode_keeps_the_refusals_of_the_7_channel_model():
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    m = module_6dof(steps=20)
    x = torch.zeros(3, 7)
    for lt in ("l1", "split"):
        with pytest.raises(NotImplementedError):
            m.p_losses(x, None, loss_type=lt)                         # before t is touched
    m = module_6dof(steps=20, model_mean_type=ModelMeanType.EPSILON)
    with pytest.raises(NotImplementedError, match="TypeError"):
        m.p_losses(x, None, loss_type="all")
    with pytest.raises(NotImplementedError):
        GNN_Diffusion(steps=20, sampling="DDIM", backbone="vn_dgcnn", use_6dof=True, use_vn_dgcnn_equiv_inv_mp=True)
    with pytest.raises(NotImplementedError):
        Eff_GAT_3d(steps=20, input_channels=13, t_channels=9, backbone="vn_dgcnn", use_vn_dgcnn_equiv_inv_mp=True)


def test_tensors_off_the_device_raise_daerror():
    from diffassemble_amd import _lib
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import Rot6dToPoseFn, rot6d_to_pose
    m = module_6dof(steps=20)
    P = 3
    x = torch.zeros(P, 7)
    x[:, 0] = 1.0
    t = torch.zeros(P, dtype=torch.long)
    with pytest.raises(_lib.DaError):
        m.q_sample_se3(x, t, (torch.zeros(P, 9), torch.ones(P, 3), torch.full((P,), 0.5)))
    with pytest.raises(_lib.DaError):
        rot6d_to_pose(torch.ones(P, 13))
    with pytest.raises(_lib.DaError):
        Rot6dToPoseFn.apply(torch.ones(P, 13, requires_grad=True))
    with pytest.raises(_lib.DaError):
        m.p_losses(x, t, noise=(torch.zeros(P, 9), torch.ones(P, 3), torch.full((P,), 0.5)), loss_type="all")
