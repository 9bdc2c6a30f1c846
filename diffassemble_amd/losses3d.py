"""The 3D model's training losses of ``loss_type="all"`` (puzzle_diff/model/utils_3d.py:585-890 as called at
spatial_diffusion_3d_test_double_diffusion.py:500-562), forward and backward in HIP (diffassemble_amd/csrc/da_loss3d.hip,
DESIGN.md 3i): ``trans_l2_loss``, ``rot_cosine_loss``, ``shape_cd_loss`` with the reference's names and argument lists, and
``assembly_losses``, the weighted ``loss_dict``.

Pieces are rows: rotations [P, 4] (quaternion, real part first), translations [P, 3], fragments ``pts`` [P, N, 3];
``valids`` [n_batch, n_parts] (any shape with that many entries) marks the slots that hold a piece, and the k-th piece takes
the k-th true entry in row-major order, as the reference's ``x[valid_mask] = ...`` does.  Everything runs on the ROCm device
on the current stream, without a host synchronisation (the step can be captured); host tensors raise ``DaError``.  The
gradient reaches the first pose only (``trans1`` / ``rot1`` / ``prediction``): the target carries none in the reference."""
import torch

from . import _lib

TRANS_LOSS_W, ROT_PT_CD_LOSS_W, TRANSFORM_PT_CD_LOSS_W, ROT_LOSS_W, ROT_PT_L2_LOSS_W = 1.0, 0.0, 10.0, 0.2, 0.0
MAX_PARTS = 64


def slot_map(valids, n_batch, n_parts, n_pieces):
    """int32 [n_pieces, 2]: (shape, slot) of every piece -- the position of the k-th true entry of ``valids`` in row-major
    order.  Plain torch ops of fixed output shape on the device of ``valids``: no host synchronisation.  (When ``valids``
    holds fewer than ``n_pieces`` true entries the surplus pieces get shape ``n_batch``, which the kernels leave out.)"""
    flat = valids.reshape(-1) != 0
    if flat.numel() != n_batch * n_parts:
        raise ValueError(f"valids has {flat.numel()} entries, expected n_batch * n_parts = {n_batch} * {n_parts}")
    if n_pieces > flat.numel():
        raise ValueError(f"{n_pieces} pieces do not fit {n_batch} shapes of {n_parts} slots")
    if flat.device.type != "cuda" and int(flat.sum()) != n_pieces:          # (a host tensor: the count is free to check)
        raise ValueError(f"valids marks {int(flat.sum())} slots for {n_pieces} pieces")
    csum = torch.cumsum(flat.to(torch.int32), 0, dtype=torch.int32)
    pos = torch.searchsorted(csum, torch.arange(1, n_pieces + 1, dtype=torch.int32, device=flat.device))
    return torch.stack((pos // n_parts, pos % n_parts), 1).to(torch.int32)


class _Loss3d(torch.autograd.Function):
    """(pred [P, 7], gt [P, 7], pts [P, N, 3] | None, map) -> per-shape losses [3, n_batch] (trans, shape Chamfer, rotation)
    and ``weights`` x their means over the shapes [3] (weighted inside the kernel's fp64 reduction: one rounding per
    output); backward: d / d pred from the saved nearest indices."""

    @staticmethod
    def forward(ctx, pred, gt, pts, pmap, n_batch, n_parts, terms, weights):
        dev = pred.device
        P = pred.shape[0]
        N = pts.shape[1] if pts is not None else 1
        L = _lib.lib()
        pred_c, gt_c = pred.detach().to(torch.float32).contiguous(), gt.detach().to(torch.float32).contiguous()
        pts_c = pts.detach().to(torch.float32).contiguous() if pts is not None else None
        ws = torch.empty(L.da_loss3d_workspace_bytes(n_batch, n_parts, N), dtype=torch.uint8, device=dev)
        cd = bool(terms & _lib.LOSS3D_SHAPE_CD)
        dist = torch.empty(2, P, N, dtype=torch.float32, device=dev) if cd else None
        idx = torch.empty(2, P, N, dtype=torch.int32, device=dev) if cd else None
        out = torch.empty(3 * n_batch + 3, dtype=torch.float32, device=dev)
        _lib.check(L.da_loss3d_forward(P, N, n_batch, n_parts, terms, _lib.ptr(pts_c), _lib.ptr(pred_c), _lib.ptr(gt_c), _lib.ptr(pmap),
                                       weights[0], weights[1], weights[2], _lib.ptr(dist), _lib.ptr(idx), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        ctx.save_for_backward(pred_c, gt_c, pts_c, pmap, idx, ws)
        ctx.dims = (P, N, n_batch, n_parts, terms)
        ctx.weights = weights
        ctx.pred_dtype = pred.dtype
        ctx.mark_non_differentiable(*(t for t in (dist, idx) if t is not None))
        return out[:3 * n_batch].view(3, n_batch), out[3 * n_batch:], dist, idx

    @staticmethod
    def backward(ctx, g_shape, g_mean, _gd, _gi):
        pred_c, gt_c, pts_c, pmap, idx, ws = ctx.saved_tensors
        P, N, n_batch, n_parts, terms = ctx.dims
        g = torch.zeros(3, n_batch, dtype=torch.float32, device=pred_c.device)
        if g_shape is not None:
            g = g + g_shape.to(torch.float32)
        if g_mean is not None:
            gm = g_mean.to(torch.float32)              # (python scalars only: a host tensor here would be a copy inside a captured graph)
            g = g + torch.stack([gm[k] * (ctx.weights[k] / n_batch) for k in range(3)])[:, None]
        g = g.contiguous()
        grad = torch.empty(P, 7, dtype=torch.float32, device=pred_c.device)
        _lib.check(_lib.lib().da_loss3d_backward(P, N, n_batch, n_parts, terms, _lib.ptr(pts_c), _lib.ptr(pred_c), _lib.ptr(gt_c),
                                                 _lib.ptr(pmap), _lib.ptr(idx), _lib.ptr(g), _lib.ptr(grad), _lib.ptr(ws), ws.numel(),
                                                 _lib.stream_ptr(pred_c.device)))
        return grad.to(ctx.pred_dtype), None, None, None, None, None, None, None


def _run(pred, gt, pts, n_batch, valids, n_parts, terms, who, weights=(1.0, 1.0, 1.0)):
    if pred.dim() != 2 or pred.shape[1] != 7 or gt.shape != pred.shape:
        raise ValueError(f"{who}: poses must be two [P, 7] tensors (got {tuple(pred.shape)} and {tuple(gt.shape)})")
    P = pred.shape[0]
    if n_batch is None or valids is None:
        raise ValueError(f"{who}: n_batch and valids are required (the reference's n_batch=None branch is not on the 3D training path)")
    if not 0 < n_parts <= MAX_PARTS or n_batch <= 0 or P <= 0:
        raise ValueError(f"{who}: need 0 < n_parts <= {MAX_PARTS}, n_batch > 0 and at least one piece")
    if pts is not None and (pts.dim() != 3 or pts.shape[0] != P or pts.shape[2] != 3 or pts.shape[1] == 0):
        raise ValueError(f"{who}: pts must be [P, N, 3] with P = {P} (got {tuple(pts.shape)})")
    if (terms & _lib.LOSS3D_SHAPE_CD) and pts is None:
        raise ValueError(f"{who}: the shape term needs pts")
    pmap = slot_map(valids, n_batch, n_parts, P)
    tensors = [t for t in (pred, gt, pts, valids) if t is not None]
    if any(t.device.type != "cuda" for t in tensors):
        raise _lib.DaError(f"{who}: the tensors must live on the ROCm device (diffassemble_amd has no CPU / eager fallback)")
    if any(t.device != pred.device for t in tensors):
        raise ValueError(f"{who}: the tensors live on different devices")
    return _Loss3d.apply(pred, gt, pts, pmap.contiguous(), n_batch, n_parts, terms, tuple(float(w) for w in weights))


def _poses(rot, trans, like):
    """[P, 7] from a rotation and / or a translation (the missing half: identity / zero, which no requested term reads)."""
    P = like.shape[0]
    if rot is None:
        rot = torch.zeros(P, 4, dtype=like.dtype, device=like.device)
    if trans is None:
        trans = torch.zeros(P, 3, dtype=like.dtype, device=like.device)
    if rot.dim() != 2 or rot.shape[1] != 4 or trans.dim() != 2 or trans.shape[1] != 3 or rot.shape[0] != trans.shape[0]:
        raise ValueError(f"rotations must be [P, 4] quaternions and translations [P, 3] (got {tuple(rot.shape)}, {tuple(trans.shape)})")
    return torch.cat((rot, trans), 1)


def trans_l2_loss(trans1, trans2, n_batch=None, valids=None, n_parts=20):
    """utils_3d.py:862-890: per shape, the mean over its valid parts of |t1 - t2|^2 -> [n_batch]."""
    out = _run(_poses(None, trans1, trans1), _poses(None, trans2, trans2), None, n_batch, valids, n_parts, _lib.LOSS3D_TRANS, "trans_l2_loss")
    return out[0][0]


def rot_cosine_loss(rot1, rot2, valids, n_batch, n_parts=20):
    """utils_3d.py:624-679 for quaternions: per shape, the mean over its valid parts of 1 - |q1 . q2|, after
    ``Rotation3D._process_zero_quat`` (norm <= 0.5 -> (1, 0, 0, 0), no gradient) -> [n_batch]."""
    out = _run(_poses(rot1, None, rot1), _poses(rot2, None, rot2), None, n_batch, valids, n_parts, _lib.LOSS3D_ROT, "rot_cosine_loss")
    return out[0][2]


def shape_cd_loss(pts, trans1, trans2, rot1, rot2, ret_pts=False, n_parts=20, training=True, n_batch=None, valids=None):
    """utils_3d.py:768-859 (its ``n_batch`` branch, which ignores ``training``): the two-sided squared Chamfer distance between
    the assembled shape under (rot1, trans1) and under (rot2, trans2), summed over the valid points and divided by
    n_parts * N -> [n_batch].  ``pts`` is detached, as in the reference.  The posed clouds are never formed, so ``ret_pts``
    is not available."""
    if ret_pts:
        raise NotImplementedError("shape_cd_loss: ret_pts=True (the posed clouds are never materialised)")
    out = _run(_poses(rot1, trans1, rot1), _poses(rot2, trans2, rot2), pts, n_batch, valids, n_parts, _lib.LOSS3D_SHAPE_CD, "shape_cd_loss")
    return out[0][1]


def shape_cd_matches(pts, trans1, trans2, rot1, rot2, n_parts=20, n_batch=None, valids=None):
    """The search behind ``shape_cd_loss``: (dist, idx), each [2, P, N] -- for every point of every piece the squared distance
    to the nearest point of the other shape and that point's index ``slot * N + point`` in the reference's padded frame
    ([0]: first pose -> second, [1]: second -> first).  No gradient."""
    out = _run(_poses(rot1, trans1, rot1).detach(), _poses(rot2, trans2, rot2).detach(), pts, n_batch, valids, n_parts, _lib.LOSS3D_SHAPE_CD,
               "shape_cd_matches")
    return out[2], out[3]


def assembly_losses(prediction, target, pts, n_batch, valids, n_parts=20, loss_type="all"):
    """The ``loss_dict`` of ``loss_type="all"`` (spatial_diffusion_3d_test_double_diffusion.py:500-562): prediction / target
    [P, 7] (quaternion wxyz | translation), pts [P, N, 3].  Keys ``trans_loss``, ``rot_pt_cd_loss``, ``transform_pt_cd_loss``,
    ``rot_loss``, ``rot_pt_l2_loss``: the means over the shapes with the reference's weights 1.0 / 0.0 / 10.0 / 0.2 / 0.0
    already applied.  The two zero-weight terms (``rot_points_cd_loss``, ``rot_points_l2_loss``) are exact zeros and are NOT
    computed (in the reference they cost two more searches and contribute 0 * value).  One fused forward and one fused
    backward serve the three live terms.

    ``valids`` must mark exactly P slots.  On the device this is NOT checked (counting would synchronise with the host and
    break graph capture): with fewer true entries the surplus pieces are silently left out of every term, with more the
    later entries are silently ignored."""
    if loss_type == "split":
        raise NotImplementedError('loss_type="split": the reference\'s own call of it (trans_l2_loss without valids) cannot run')
    if loss_type != "all":
        raise NotImplementedError(f"loss_type={loss_type!r}")
    _, mean, _, _ = _run(prediction, target, pts, n_batch, valids, n_parts, _lib.LOSS3D_ALL, "assembly_losses",
                         weights=(TRANS_LOSS_W, TRANSFORM_PT_CD_LOSS_W, ROT_LOSS_W))
    zero = mean.new_zeros(())
    return {"trans_loss": mean[0], "rot_pt_cd_loss": zero, "transform_pt_cd_loss": mean[1], "rot_loss": mean[2], "rot_pt_l2_loss": zero.clone()}
