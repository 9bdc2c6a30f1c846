"""Host-side checks of the 3D assembly losses (diffassemble_amd/losses3d.py): the C ABI carries the new entry points, host
tensors never compute, bad arguments raise before anything is launched, and the piece -> (shape, slot) map follows the
reference's masked-assignment order (utils_3d.py ``x[valid_mask] = ...``).  No GPU."""
import pytest
import torch


def _inputs(P=5, N=8, n_batch=2, n_parts=4):
    g = torch.Generator().manual_seed(0)
    valids = torch.tensor([[1, 1, 0, 1], [0, 1, 0, 1]], dtype=torch.bool)
    return torch.randn(P, 7, generator=g), torch.randn(P, 7, generator=g), torch.randn(P, N, 3, generator=g), valids, n_batch, n_parts


def test_module_imports_and_symbols_are_exported_and_bound():
    from diffassemble_amd import _lib, losses3d
    h = _lib.lib()
    for name in ("da_loss3d_forward", "da_loss3d_backward", "da_loss3d_workspace_bytes"):
        assert name in _lib.PROTOTYPES and getattr(h, name).argtypes == _lib.PROTOTYPES[name][1]
    assert h.da_abi_version() == _lib.ABI_VERSION == 19                      # additive: the ABI number stays
    assert h.da_loss3d_workspace_bytes(32, 20, 1000) > 0 and h.da_loss3d_workspace_bytes(0, 20, 1000) == 0
    for fn in ("trans_l2_loss", "rot_cosine_loss", "shape_cd_loss", "assembly_losses"):
        assert callable(getattr(losses3d, fn))


def test_entry_points_check_their_arguments_before_launching():
    from diffassemble_amd import _lib
    h = _lib.lib()
    rc = h.da_loss3d_forward(5, 8, 2, 4, 7, None, None, None, None, 1.0, 1.0, 1.0, None, None, None, None, 0, None)
    assert rc == 1 and b"null argument" in h.da_last_error()
    rc = h.da_loss3d_forward(5, 8, 2, 65, 7, None, None, None, None, 1.0, 1.0, 1.0, None, None, None, None, 0, None)
    assert rc == 1 and b"n_parts" in h.da_last_error()
    rc = h.da_loss3d_backward(9, 8, 2, 4, 7, None, None, None, None, None, None, None, None, 0, None)
    assert rc == 1 and b"do not fit" in h.da_last_error()
    rc = h.da_loss3d_backward(5, 8, 2, 4, 0, None, None, None, None, None, None, None, None, 0, None)
    assert rc == 1 and b"terms" in h.da_last_error()


def test_host_tensors_raise_daerror():
    from diffassemble_amd import _lib, losses3d
    pred, gt, pts, valids, n_batch, n_parts = _inputs()
    with pytest.raises(_lib.DaError):
        losses3d.assembly_losses(pred, gt, pts, n_batch, valids, n_parts=n_parts)
    with pytest.raises(_lib.DaError):
        losses3d.trans_l2_loss(pred[:, 4:], gt[:, 4:], n_batch=n_batch, valids=valids, n_parts=n_parts)
    with pytest.raises(_lib.DaError):
        losses3d.rot_cosine_loss(pred[:, :4], gt[:, :4], valids, n_batch, n_parts=n_parts)
    with pytest.raises(_lib.DaError):
        losses3d.shape_cd_loss(pts, pred[:, 4:], gt[:, 4:], pred[:, :4], gt[:, :4], n_parts=n_parts, n_batch=n_batch, valids=valids)


def test_split_is_not_implemented_and_model_surface():
    from diffassemble_amd import losses3d
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion
    pred, gt, pts, valids, n_batch, n_parts = _inputs()
    with pytest.raises(NotImplementedError):
        losses3d.assembly_losses(pred, gt, pts, n_batch, valids, n_parts=n_parts, loss_type="split")
    with pytest.raises(NotImplementedError):
        losses3d.assembly_losses(pred, gt, pts, n_batch, valids, n_parts=n_parts, loss_type="l1")
    assert callable(GNN_Diffusion.pose_losses)


def test_shape_and_valids_mismatches_raise():
    from diffassemble_amd import losses3d
    pred, gt, pts, valids, n_batch, n_parts = _inputs()
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred, gt[:4], pts, n_batch, valids, n_parts=n_parts)              # poses disagree
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred[:, :6], gt[:, :6], pts, n_batch, valids, n_parts=n_parts)    # not [P, 7]
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred, gt, pts[:4], n_batch, valids, n_parts=n_parts)              # pts of another P
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred, gt, pts, n_batch, valids, n_parts=5)                        # valids is not n_batch x n_parts
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred, gt, pts, n_batch, torch.ones(2, 4, dtype=torch.bool), n_parts=n_parts)   # 8 slots, 5 pieces
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred, gt, pts, n_batch, valids.repeat(1, 20), n_parts=80)         # more slots than the kernels hold
    with pytest.raises(ValueError):
        losses3d.assembly_losses(pred, gt, None, n_batch, valids, n_parts=n_parts)
    with pytest.raises(ValueError):
        losses3d.shape_cd_loss(pts, pred[:, 4:], gt[:, 4:], pred[:, :4], gt[:, :4], n_parts=n_parts)                # no n_batch / valids


def test_slot_map_follows_the_masked_assignment_order():
    from diffassemble_amd import losses3d
    n_batch, n_parts = 3, 20
    valids = torch.zeros(n_batch, n_parts, dtype=torch.bool)
    valids[0, [0, 1, 3]] = True                          # 1 1 0 1 0 ...: a hole
    valids[1, [2, 19]] = True                            # does not start at slot 0
    valids[2] = True
    P = int(valids.sum())
    got = losses3d.slot_map(valids, n_batch, n_parts, P)
    assert got.dtype == torch.int32 and got.shape == (P, 2)
    x = torch.full((n_batch, n_parts), -1, dtype=torch.long)
    x[valids] = torch.arange(P)                          # the reference's assignment: piece k lands where x == k
    want = torch.stack([(x == k).nonzero()[0] for k in range(P)])
    assert torch.equal(got.long(), want)
    assert torch.equal(losses3d.slot_map(valids.reshape(-1).float(), n_batch, n_parts, P), got)      # any layout / dtype of valids
