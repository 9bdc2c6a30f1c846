"""Evaluation metrics of the 3D ``validation_step`` / ``test_step`` (host glue: torch ops on whatever device the
sampled poses live on; runs once per Batch AFTER the sampling loop, not on the per-timestep path).

Counterparts of puzzle_diff/model/utils_3d.py ``trans_metrics`` (:362-383), ``rot_metrics`` (:415-450, 'rmse' and
'geodesic'), ``geodesic_distance`` (:916-945) and ``calc_part_acc`` (:1089-1129).  The reference routes the last one
through pytorch3d's CUDA ``knn_points`` (model/chamfer_distance.py:148-149), which does not exist on ROCm: on the device
the K = 1 search both ways is ``da_nearest_sq`` (diffassemble_amd/csrc/da_pcd_encoder.hip; b tiles staged in LDS, the
[P, N, N] distance tensor is never formed).  Host tensors take the cdist route below.  Poses are (unit quaternion wxyz |
translation) rows, [P, 7]; fragments [P, N, 3].

``batch_metrics`` scores every object of a Batch at once: on the device it is ONE library call (``da_metrics3d``,
diffassemble_amd/csrc/da_metrics3d.hip, DESIGN 3k: one workgroup per part poses the fragment twice in LDS, a segmented mean
per object finishes) and the caller copies [G, 4] to the host once; on host tensors it is the loop over the objects through
the four functions above it, which states the semantics."""
import math

import torch


def _rotate(q, v):
    """points v [P, N, 3] by unit quaternions q [P, 4] (real part first)."""
    w, u = q[:, None, :1], q[:, None, 1:].expand(-1, v.shape[1], -1)
    t = 2.0 * torch.cross(u, v, dim=-1)
    return v + w * t + torch.cross(u, t, dim=-1)


def _rmat(q):
    r, i, j, k = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    return torch.stack((1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                        s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                        s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)), -1).reshape(q.shape[:-1] + (3, 3))


def trans_metrics(t1, t2):
    """RMSE over xyz per part, mean over parts (utils_3d.py:362-383, metric='rmse')."""
    return ((t1 - t2).pow(2).mean(-1) ** 0.5).mean()


def _euler_zyx_deg(q):
    q0, q1, q2, q3 = q.unbind(-1)
    x = torch.atan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
    y = torch.asin(torch.clamp(2 * (q0 * q2 - q1 * q3), -1, 1))
    z = torch.atan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3))
    return torch.stack((x, y, z), -1) * (180.0 / math.pi)


def rot_metrics(q1, q2, metric="rmse"):
    """utils_3d.py:415-450: 'rmse' of the zyx Euler angles in degrees (differences wrap at 360) or 'geodesic'."""
    if metric == "geodesic":
        tr = torch.einsum("bij,bij->b", _rmat(q1), _rmat(q2))
        return torch.acos(torch.clamp(0.5 * (tr - 1), -1 + 1e-6, 1 - 1e-6)).mean()
    d = (_euler_zyx_deg(q1) - _euler_zyx_deg(q2)).abs()
    d = torch.minimum(d, 360.0 - d)
    return (d.pow(2).mean(-1) ** 0.5).mean()


def calc_part_acc(pts, t1, t2, q1, q2, thr=0.01):
    """utils_3d.py:1089-1129: parts whose two-sided mean squared Chamfer distance between the two posed copies of the
    fragment is below ``thr``, as a fraction of the parts."""
    a = _rotate(q1, pts) + t1[:, None, :]
    b = _rotate(q2, pts) + t2[:, None, :]
    if a.device.type == "cuda":
        from .pcd_encoder import nearest_sq
        d_ab, d_ba = nearest_sq(a, b)
        loss = d_ab.mean(1) + d_ba.mean(1)
    else:                                       # poses already moved to the host by the caller
        d = torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist").pow(2)   # exact differences: the threshold sits near 0
        loss = d.min(2)[0].mean(1) + d.min(1)[0].mean(1)
    return (loss < thr).sum() / loss.numel()


def _part_chamfer(pts, t1, t2, q1, q2):
    """The per-part loss ``calc_part_acc`` thresholds (host tensors), [P]."""
    a = _rotate(q1, pts) + t1[:, None, :]
    b = _rotate(q2, pts) + t2[:, None, :]
    d = torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist").pow(2)
    return d.min(2)[0].mean(1) + d.min(1)[0].mean(1)


def _pose_rows(x):
    """Pose rows as the library reads them: fp32, unit inner stride -> (tensor, leading dimension >= 7)."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < 7):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else 7)


def batch_metrics(pcds, pred, gt, ptr=None, batch=None, thr=0.01, return_per_part=False):
    """The four pose metrics of every object of a Batch: [G, 4] = (rmse_t, rmse_r, gd_r, part_acc), each the value the
    per-object calls ``trans_metrics`` / ``rot_metrics('rmse')`` / ``rot_metrics('geodesic')`` / ``calc_part_acc`` give on
    the object's parts.  ``pred`` / ``gt`` [P, 7]; ``pcds`` [P, N, 3] or None (part_acc is NaN then).  The objects are
    consecutive rows: give ``ptr`` (int [G + 1]) or the sorted ``batch`` vector [P] (``ptr`` is then built on the device with
    bincount + cumsum).  An object without parts gets a NaN row.  ``return_per_part``: also [P, 4] = (rmse_t, rmse_r, gd_r,
    Chamfer loss) per part.  On a ROCm device this is one call of ``da_metrics3d``; on host tensors the loop below."""
    if (ptr is None) == (batch is None):
        raise ValueError("batch_metrics: give either ptr or a sorted batch vector")
    if pred.dim() != 2 or pred.shape[1] != 7 or gt.shape != pred.shape:
        raise ValueError(f"batch_metrics: poses are [P, 7] rows (got {tuple(pred.shape)}, {tuple(gt.shape)})")
    P = pred.shape[0]
    if pcds is not None and (pcds.dim() != 3 or pcds.shape[0] != P or pcds.shape[2] != 3):
        raise ValueError(f"batch_metrics: pcds is [P, N, 3] with P = {P} (got {tuple(pcds.shape)})")
    if ptr is None:
        if batch.shape != (P,):
            raise ValueError(f"batch_metrics: batch is [P] with P = {P} (got {tuple(batch.shape)})")
        G = int(batch.max()) + 1
        ptr = torch.zeros(G + 1, dtype=torch.int32, device=batch.device)
        ptr[1:] = torch.cumsum(torch.bincount(batch, minlength=G), 0)
    G = ptr.numel() - 1
    if pred.device.type == "cuda":
        from . import _lib
        dev = pred.device
        pr, ld_pred = _pose_rows(pred)
        tg, ld_gt = _pose_rows(gt.to(dev))
        pts = None if pcds is None else pcds.detach().to(dev, torch.float32).contiguous()
        ptr = ptr.to(dev, torch.int32).contiguous()
        per_part = torch.empty(P, 4, dtype=torch.float32, device=dev)
        per_object = torch.empty(G, 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().da_metrics3d(P, 0 if pts is None else pts.shape[1], G, _lib.ptr(pr), ld_pred, _lib.ptr(tg), ld_gt,
                                               _lib.ptr(pts), _lib.ptr(ptr), float(thr), _lib.ptr(per_part), _lib.ptr(per_object),
                                               _lib.stream_ptr(dev)))
        return (per_object, per_part) if return_per_part else per_object
    bounds = ptr.tolist()
    nan = float("nan")
    per_object = torch.full((G, 4), nan, dtype=pred.dtype)
    for g in range(G):
        s, e = bounds[g], bounds[g + 1]
        if e <= s:
            continue
        q1, t1, q2, t2 = pred[s:e, :4], pred[s:e, 4:7], gt[s:e, :4], gt[s:e, 4:7]
        per_object[g, 0] = trans_metrics(t1, t2)
        per_object[g, 1] = rot_metrics(q1, q2, "rmse")
        per_object[g, 2] = rot_metrics(q1, q2, "geodesic")
        if pcds is not None:
            per_object[g, 3] = calc_part_acc(pcds[s:e], t1, t2, q1, q2, thr)
    if not return_per_part:
        return per_object
    per_part = torch.full((P, 4), nan, dtype=pred.dtype)
    for p in range(P):
        q1, t1, q2, t2 = pred[p:p + 1, :4], pred[p:p + 1, 4:7], gt[p:p + 1, :4], gt[p:p + 1, 4:7]
        per_part[p, 0] = trans_metrics(t1, t2)
        per_part[p, 1] = rot_metrics(q1, q2, "rmse")
        per_part[p, 2] = rot_metrics(q1, q2, "geodesic")
        if pcds is not None:
            per_part[p, 3] = _part_chamfer(pcds[p:p + 1], t1, t2, q1, q2)[0]
    return per_object, per_part
