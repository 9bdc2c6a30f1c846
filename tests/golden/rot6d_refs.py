"""The contract of ``da_rot6d_to_pose`` / ``da_rot6d_to_pose_backward`` in torch, dtype-generic, and the restatement of the
``use_6dof`` noising (spatial_diffusion_3d_test_double_diffusion.py:421-441 with the nine Gaussian channels of :424-431).

Forward (:480-490): a1 = pred[:, 7:10], a2 = pred[:, 10:13],
    b1 = a1 / max(|a1|, 1e-12),  u = a2 - (a2.b1) b1,  b2 = u / max(|u|, 1e-12),  b3 = b1 x b2,
    pose7 = [matrix_to_quaternion(stack([b1, b2, b3], -1)) | pred[:, 4:7]].
Backward, ONE closed form for all four branches of matrix_to_quaternion.  R = [b1 b2 b3] is a rotation for every (a1, a2), so
only the differential along SO(3) is ever used: for dR = [dw]x R the quaternion moves by dq = (0, dw) (x) q / 2, which gives
    m := dL/dw = (w g_v - g_w v + v x g_v) / 2          (q = (w, v) the forward's output, g = dL/dq),
and the frame turns by dw = (b3.db2) b1 - (b3.db1) b2 + (b2.db1) b3 with db1 = (I - b1 b1^T) da1 / n1 and
b3.db2 = (b3.da2 - d b3.db1) / n2 (n1 = |a1|, n2 = |u|, d = a2.b1):
    d a2 = (m.b1) b3 / n2,        d a1 = ((m.b3) b2 - ((m.b2) + (m.b1) d / n2) b3) / n1.
Columns 0:4 of d_pred are zero (the loss never reads the head's quaternion) and 4:7 pass through."""
import math

import torch
import torch.nn.functional as F

from oracle import so3
from oracle.pyg_restatement import matrix_to_quaternion, quaternion_to_matrix

EPS = 1e-12


def frame(pred):
    a1, a2 = pred[:, 7:10], pred[:, 10:13]
    n1 = a1.norm(dim=-1, keepdim=True).clamp(min=EPS)
    b1 = a1 / n1
    d = (a2 * b1).sum(-1, keepdim=True)
    u = a2 - d * b1
    n2 = u.norm(dim=-1, keepdim=True).clamp(min=EPS)
    b2 = u / n2
    b3 = torch.cross(b1, b2, dim=-1)
    return b1, b2, b3, n1, n2, d


def rot6d_to_pose(pred):
    b1, b2, b3, _, _, _ = frame(pred)
    return torch.cat([matrix_to_quaternion(torch.stack([b1, b2, b3], dim=-1)), pred[:, 4:7]], 1)


def rot6d_to_pose_backward(pred, d_pose):
    b1, b2, b3, n1, n2, d = frame(pred)
    q = matrix_to_quaternion(torch.stack([b1, b2, b3], dim=-1))
    w, v = q[:, :1], q[:, 1:]
    gw, gv = d_pose[:, :1], d_pose[:, 1:4]
    m = 0.5 * (w * gv - gw * v + torch.cross(v, gv, dim=-1))
    mb1, mb2, mb3 = ((m * b).sum(-1, keepdim=True) for b in (b1, b2, b3))
    k2 = mb1 / n2
    d_a1 = (mb3 * b2 - (mb2 + k2 * d) * b3) / n1
    d_a2 = k2 * b3
    return torch.cat([torch.zeros_like(pred[:, :4]), d_pose[:, 4:7], d_a1, d_a2], 1)


def rot6d_to_pose_autograd(pred, d_pose):
    """The same gradient by torch autograd through the reference's expression (F.normalize / cross / stack / matrix_to_quaternion)."""
    p = pred.clone().requires_grad_(True)
    a1, a2 = p[:, 7:10], p[:, 10:13]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (a2 * b1).sum(-1, keepdim=True) * b1, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    pose = torch.cat([matrix_to_quaternion(torch.stack([b1, b2, b3], dim=-1)), p[:, 4:7]], 1)
    (pose * d_pose).sum().backward()
    return p.grad.detach(), pose.detach()


def gs_margins(pred):
    """(min |w| of the Gram-Schmidt quaternion, min |a1|, min |a2 - (a2.b1) b1|) of [.., 13] rows, in fp64."""
    p = pred.reshape(-1, pred.shape[-1]).double()
    a1, a2 = p[:, 7:10], p[:, 10:13]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    u = a2 - (a2 * b1).sum(-1, keepdim=True) * b1
    return float(rot6d_to_pose(p)[:, 0].abs().min()), float(a1.norm(dim=-1).min()), float(u.norm(dim=-1).min())


def special_rows():
    """[8, 13] fp64 rows (columns 0:7 zero): a1 parallel to e_x; a2 nearly parallel to a1 (sine 1e-2); |a1| = 1e-3; a rotation whose
    quaternion has w = +-1e-3 (either side of the standardisation); w = 1 (identity); a rotation by 2 (generic); long vectors."""
    def rows_of(R, s1=1.0, s2=1.0, mix=0.0):
        a1 = s1 * R[:, 0]
        return torch.cat([torch.zeros(7, dtype=torch.float64), a1, s2 * R[:, 1] + mix * a1])

    eye = torch.eye(3, dtype=torch.float64)
    out = [rows_of(eye, 2.0, 0.7, 0.3)]
    a1 = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    perp = torch.linalg.cross(a1, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    a2 = math.sqrt(1 - 1e-4) * a1 / a1.norm() + 1e-2 * perp / perp.norm()
    out.append(torch.cat([torch.zeros(7, dtype=torch.float64), a1, 1.3 * a2]))
    R = so3.skew_to_rmat(torch.tensor([[0.4, -0.2, 0.9]], dtype=torch.float64))[0]
    out.append(rows_of(R, 1e-3, 0.5, 2.0))
    axis = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
    for wq in (1e-3, -1e-3):
        q = torch.cat([torch.tensor([wq], dtype=torch.float64), math.sqrt(1 - wq * wq) * axis])
        out.append(rows_of(quaternion_to_matrix(q[None])[0], 0.9, 1.1, -0.4))
    out.append(rows_of(eye))
    out.append(rows_of(so3.skew_to_rmat(torch.tensor([[1.2, 1.2, -1.0]], dtype=torch.float64))[0], 1.0, 1.0, 0.0))
    out.append(rows_of(R, 40.0, 25.0, 3.0))
    return torch.stack(out)


def noising_restatement_6d(m, trap, x_start, t, noise_tr, axes, unif, dtype):
    """p_losses :421-441 with use_6dof: x_start [P, 7], noise_tr [P, 9] -> x_noisy [P, 13] = [noised quaternion | q_sample of
    [t | R0[:, :, 0] | R0[:, :, 1]]]; the rotation half as in the 7-channel model (IsotropicGaussianSO3.sample on the fp32 CDF table
    ``trap`` [steps, 999], trap_start / trap_end from the FIRST piece's row), arithmetic in ``dtype``."""
    sac, somac = m.sqrt_alphas_cumprod.to(dtype), m.sqrt_one_minus_alphas_cumprod.to(dtype)
    x = x_start.to(dtype)
    R0 = quaternion_to_matrix(x[:, :4])
    x_tr = torch.cat([x[:, 4:], R0[:, :, 0], R0[:, :, 1]], 1)
    tr = sac[t, None] * x_tr + somac[t, None] * noise_tr.to(dtype)
    idx1 = (trap[t] <= unif[:, None]).sum(1).clamp(max=998)
    idx0 = (idx1 - 1).clamp(min=0)
    row0 = trap[t[0]].to(dtype)
    ts, te = row0[idx0], row0[idx1]
    wgt = ((unif.to(dtype) - ts) / (te - ts).clamp(min=1e-6)).clamp(0, 1)
    loc = (math.pi * torch.linspace(0, 1.0, 1000) ** 3.0)[1:].to(dtype)
    ang = torch.lerp(loc[idx0], loc[idx1], wgt)
    a = axes.to(dtype)
    a = a / a.norm(dim=-1, keepdim=True)
    noise = torch.matrix_exp(so3.vec2skew(a * ang[:, None]))
    rot = so3.so3_scale(R0, sac[t]) @ noise
    return torch.cat([matrix_to_quaternion(rot), tr], 1)
