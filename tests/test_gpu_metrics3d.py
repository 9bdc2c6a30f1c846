"""GPU tests of the batched 3D pose metrics: ``da_metrics3d`` (diffassemble_amd/csrc/da_metrics3d.hip) through the C ABI and
through ``metrics3d.batch_metrics``, and the 3D module's ``validation_step`` on top of it.

Reference: the fp64 evaluation of the same expressions on the fp32 inputs (oracle/metrics3d.py with ``.double()`` inputs, one
part or one object at a time; the per-part Chamfer loss is the ``loss`` line of its ``part_accuracy``).  Bound: the rule
tests/test_gpu_train3d.py applies to per-piece kernels (``within_4x``) -- per column, in max-abs terms scaled by the column's
largest value, the kernel's error against fp64 is at most 4x the error of the torch-fp32 host functions (``batch_metrics`` on
CPU tensors) against the same fp64 value, floored at 16 fp32 ulps.

Inputs.  ``|2 (q0 q2 - q1 q3)| <= 0.99`` for both pose sets of the compared cases (asserted): beyond it asin amplifies fp32
rounding without bound, in torch as in the kernel.  The rotation noise of the random rows stays away from zero (0.3 .. 1 x the
case's scale): at a vanishing angle acos does the same, and identical / opposite / half-turn / gimbal poses are the SPECIAL
rows below.  The seeds were searched on the CPU so that every part's fp64 Chamfer loss is at least 1e-3 x thr away from thr
(asserted; three orders of magnitude above fp32's error on a mean of 1000 terms), which makes ``part_acc`` exact, and so that
the losses straddle thr.

Measured on MI355X (torch-fp32 error / HIP error, per column and case): see DESIGN 3k."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases as C
from oracle import metrics3d as OM
from oracle import pyg_restatement as R

pytestmark = pytest.mark.gpu
ULP16 = 16 * 2.0 ** -23
THR = 0.01
SENTINEL = -7.25
COLS = ("rmse_t", "rmse_r", "gd_r", "chamfer")

# name -> (N, parts per object, noise scale, seed).  N: 1; 63 / 64 / 65 around one wave; 257: a thread owns two points;
# 1000: the shape of the benchmark; 1025: a second LDS tile.  Objects of 1, 2 and 20 parts; 65 objects: more than one
# workgroup of the finishing kernel (4 objects each).
CASES = {
    "n1_p1_g1": (1, (1,), 0.10, 0),
    "n63_obj_1_2_20": (63, (1, 2, 20), 0.08, 0),
    "n64_obj_2_1": (64, (2, 1), 0.08, 0),
    "n65_obj_3": (65, (3,), 0.08, 1),
    "n257_obj_2_3": (257, (2, 3), 0.10, 1),
    "n1000_obj_1_2_20": (1000, (1, 2, 20), 0.16, 0),
    "n1025_obj_2": (1025, (2,), 0.16, 0),
    "n5_65_objects": (5, tuple(1 + g % 3 for g in range(65)), 0.10, 0),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def asin_arg(q):
    q = q.double()
    return (2 * (q[:, 0] * q[:, 2] - q[:, 1] * q[:, 3])).abs()


def make_case(N, counts, noise, seed):
    """(pcds [P, N, 3], pred [P, 7], gt [P, 7], ptr int32 [G + 1]); rows whose asin argument passes 0.99 are drawn again."""
    rng = np.random.default_rng(seed)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))  # noqa: E731
    P = sum(counts)
    pred, gt = [], []
    while len(gt) < P:
        g = torch.cat([torch.nn.functional.normalize(f(1, 4), dim=-1), f(1, 3) * 0.5], 1)
        p = g + float(rng.uniform(0.3, 1.0)) * noise * f(1, 7)
        p[:, :4] = torch.nn.functional.normalize(p[:, :4], dim=-1)
        if float(asin_arg(g[:, :4])) <= 0.99 and float(asin_arg(p[:, :4])) <= 0.99:
            gt.append(g)
            pred.append(p)
    pcds = f(P, N, 3) * 0.3
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return pcds.contiguous(), torch.cat(pred).contiguous(), torch.cat(gt).contiguous(), ptr


def chamfer64(pts, t1, t2, q1, q2):
    """oracle/metrics3d.py part_accuracy up to its ``loss`` (fp64 in, fp64 out), [P]."""
    a = R.quaternion_apply(q1[:, None, :].expand(-1, pts.shape[1], -1), pts) + t1[:, None, :]
    b = R.quaternion_apply(q2[:, None, :].expand(-1, pts.shape[1], -1), pts) + t2[:, None, :]
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    return d.min(2)[0].mean(1) + d.min(1)[0].mean(1)


def reference64(pcds, pred, gt, ptr):
    """fp64 per_part [P, 4] (one part at a time) and per_object [G, 4] (one object at a time; column 3 = part_acc)."""
    pd, gd, cd = pred.double(), gt.double(), pcds.double()
    P, b = pred.shape[0], ptr.tolist()
    per_part = torch.empty(P, 4, dtype=torch.float64)
    for p in range(P):
        s = slice(p, p + 1)
        per_part[p, 0] = OM.trans_rmse(pd[s, 4:], gd[s, 4:])
        per_part[p, 1] = OM.rot_rmse(pd[s, :4], gd[s, :4])
        per_part[p, 2] = OM.geodesic(pd[s, :4], gd[s, :4])
        per_part[p, 3] = chamfer64(cd[s], pd[s, 4:], gd[s, 4:], pd[s, :4], gd[s, :4])[0]
    per_object = torch.empty(len(b) - 1, 4, dtype=torch.float64)
    for g in range(len(b) - 1):
        s = slice(b[g], b[g + 1])
        per_object[g, 0] = OM.trans_rmse(pd[s, 4:], gd[s, 4:])
        per_object[g, 1] = OM.rot_rmse(pd[s, :4], gd[s, :4])
        per_object[g, 2] = OM.geodesic(pd[s, :4], gd[s, :4])
        per_object[g, 3] = (per_part[s, 3] < THR).sum() / (b[g + 1] - b[g])
    return per_part, per_object


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs, the fp64 reference and the torch-fp32 host values of one case: computed once, shared, never modified."""
    from diffassemble_amd.metrics3d import batch_metrics
    pcds, pred, gt, ptr = make_case(*CASES[name])
    part64, obj64 = reference64(pcds, pred, gt, ptr)
    obj32, part32 = batch_metrics(pcds, pred, gt, ptr=ptr, thr=THR, return_per_part=True)
    return SimpleNamespace(pcds=pcds, pred=pred, gt=gt, ptr=ptr, part64=part64, obj64=obj64, part32=part32, obj32=obj32)


def run_direct(dev, pcds, pred, gt, ptr, thr=THR, guard=3):
    """``da_metrics3d`` through the C ABI: ld_pred = 7, gt in rows of 8 floats whose pad column is NaN, outputs filled with a
    sentinel and followed by guard rows (asserted untouched).  Returns per_part [P, 4], per_object [G, 4] on the host."""
    from diffassemble_amd import _lib
    P, G = pred.shape[0], ptr.numel() - 1
    pr = pred.to(dev).contiguous()
    g8 = torch.full((P, 8), float("nan"), device=dev)
    g8[:, :7] = gt.to(dev)
    pts = None if pcds is None else pcds.to(dev).contiguous()
    pt = ptr.to(dev, torch.int32).contiguous()
    pp = torch.full((P + guard, 4), SENTINEL, device=dev)
    po = torch.full((G + guard, 4), SENTINEL, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().da_metrics3d(P, 0 if pts is None else pts.shape[1], G, _lib.ptr(pr), 7, _lib.ptr(g8), 8, _lib.ptr(pts),
                                           _lib.ptr(pt), thr, _lib.ptr(pp), _lib.ptr(po), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    pp, po = pp.cpu(), po.cpu()
    assert bool((pp[P:] == SENTINEL).all()) and bool((po[G:] == SENTINEL).all()), "a guard row was written"
    return pp[:P], po[:G]


@functools.lru_cache(maxsize=None)
def hip_data(name):
    d = case_data(name)
    return run_direct(torch.device("cuda:0"), d.pcds, d.pred, d.gt, d.ptr)


def within_4x(name, hip, f32, f64):
    """tests/test_gpu_train3d.py's rule, for one column."""
    scale = float(f64.abs().max())
    if scale == 0.0:
        scale = 1.0
    e32 = float((f32.double() - f64).abs().max()) / scale
    ehip = float((hip.double() - f64).abs().max()) / scale
    print(f"{name}: scale {scale:.3e}  torch-fp32 err {e32:.3e}  HIP err {ehip:.3e}")
    assert math.isfinite(ehip) and ehip <= max(4 * e32, ULP16), (name, e32, ehip)


@pytest.mark.parametrize("name", list(CASES))
def test_per_part_and_per_object_vs_fp64(dev, name):
    d = case_data(name)
    assert float(asin_arg(d.pred[:, :4]).max()) <= 0.99 and float(asin_arg(d.gt[:, :4]).max()) <= 0.99      # the input condition
    pp, po = hip_data(name)
    assert bool(torch.isfinite(pp).all()) and bool(torch.isfinite(po).all())
    for c, col in enumerate(COLS):
        within_4x(f"{name} per_part {col}", pp[:, c], d.part32[:, c], d.part64[:, c])
    for c, col in enumerate(COLS[:3]):
        within_4x(f"{name} per_object {col}", po[:, c], d.obj32[:, c], d.obj64[:, c])


@pytest.mark.parametrize("name", list(CASES))
def test_part_acc_is_exact(dev, name):
    d = case_data(name)
    margin = float(((d.part64[:, 3] - THR).abs() / THR).min())
    print(f"{name}: smallest |chamfer - thr| / thr = {margin:.3e}; part_acc per object {d.obj64[:, 3].tolist()[:8]}")
    assert margin >= 1e-3                                                    # the input condition: no part sits on the threshold
    _, po = hip_data(name)
    assert torch.equal(po[:, 3], d.obj64[:, 3].float())                      # count / parts, one fp32 rounding
    assert torch.equal(po[:, 3], d.obj32[:, 3])


def test_part_acc_threshold_is_exercised(dev):
    """Across the cases the losses fall on both sides of thr, and inside one object too."""
    mixed = 0
    for name in CASES:
        acc = case_data(name).obj64[:, 3]
        mixed += int(((acc > 0) & (acc < 1)).sum())
    assert mixed >= 1
    _, po = hip_data("n1000_obj_1_2_20")
    assert 0.0 < float(po[2, 3]) < 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_null_clouds_determinism_and_public_route(dev, name):
    from diffassemble_amd.metrics3d import batch_metrics
    d = case_data(name)
    pp, po = hip_data(name)
    pp0, po0 = run_direct(dev, None, d.pred, d.gt, d.ptr)
    assert bool(torch.isnan(pp0[:, 3]).all()) and bool(torch.isnan(po0[:, 3]).all())
    assert torch.equal(pp0[:, :3], pp[:, :3]) and torch.equal(po0[:, :3], po[:, :3])
    pp2, po2 = run_direct(dev, d.pcds, d.pred, d.gt, d.ptr)                   # a second run: the same bits
    assert torch.equal(pp2, pp) and torch.equal(po2, po)
    g8 = torch.zeros(d.gt.shape[0], 8, device=dev)
    g8[:, :7] = d.gt.to(dev)
    batch = torch.repeat_interleave(torch.arange(d.ptr.numel() - 1), (d.ptr[1:] - d.ptr[:-1]).long()).to(dev)
    for kw in (dict(ptr=d.ptr.to(dev)), dict(batch=batch)):
        o, p = batch_metrics(d.pcds.to(dev), d.pred.to(dev), g8[:, :7], thr=THR, return_per_part=True, **kw)
        assert torch.equal(o.cpu(), po) and torch.equal(p.cpu(), pp)
    o = batch_metrics(None, d.pred.to(dev), d.gt.to(dev), ptr=d.ptr.to(dev))
    assert torch.equal(o[:, :3].cpu(), po[:, :3]) and bool(torch.isnan(o[:, 3]).all())


def test_object_without_parts_is_a_nan_row(dev):
    d = case_data("n63_obj_1_2_20")
    pp, po = hip_data("n63_obj_1_2_20")
    ptr = torch.tensor([0, 1, 1, 3, 23], dtype=torch.int32)                  # object 1 is empty
    pp4, po4 = run_direct(dev, d.pcds, d.pred, d.gt, ptr)
    assert torch.equal(pp4, pp) and bool(torch.isnan(po4[1]).all()) and torch.equal(po4[[0, 2, 3]], po)


def test_nan_pose_gives_nan_chamfer_as_on_the_host(dev):
    """A diverged pose: torch.min passes NaN, so the host route's Chamfer loss of that part is NaN; the kernel's too.  The part
    counts as a miss in ``part_acc`` and no other row moves."""
    from diffassemble_amd.metrics3d import batch_metrics
    d = case_data("n63_obj_1_2_20")
    pp, po = hip_data("n63_obj_1_2_20")
    pred = d.pred.clone()
    pred[1, 5] = float("nan")                                                # first part of the two-part object
    ppn, pon = run_direct(dev, d.pcds, pred, d.gt, d.ptr)
    _, host = batch_metrics(d.pcds, pred, d.gt, ptr=d.ptr, return_per_part=True)
    assert math.isnan(float(host[1, 3])) and math.isnan(float(ppn[1, 3])) and math.isnan(float(ppn[1, 0]))
    keep = [r for r in range(pp.shape[0]) if r != 1]
    assert torch.equal(ppn[keep], pp[keep]) and torch.equal(pon[[0, 2]], po[[0, 2]])
    assert float(pon[1, 3]) == float(pp[2, 3] < THR) / 2


# ------------------------------------------------------------------------------------------------ special rows
def special_rows():
    """identical | q against -q | w < 0 on both sides | a half turn | half turn against itself plus noise | gimbal (sin y = +1 and -1
    exactly, LAST two rows).  One object; N = 65."""
    rng = np.random.default_rng(5)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))  # noqa: E731
    P, N = 7, 65
    while True:
        gt = torch.cat([torch.nn.functional.normalize(f(P, 4), dim=-1), f(P, 3) * 0.5], 1)
        gt[2, :4] *= -torch.sign(gt[2, 0])                                   # w < 0 on both sides
        gt[4, :4] = torch.tensor([0.0, 0.0, 0.0, 1.0])                       # a half turn about z against its noisy copy
        pred = gt + 0.1 * f(P, 7)
        pred[:, :4] = torch.nn.functional.normalize(pred[:, :4], dim=-1)
        pred[0] = gt[0]                                                      # identical poses
        pred[1, :4] = -gt[1, :4]                                             # the same rotation, the other sign
        pred[3, :4] = torch.tensor([0.0, 1.0, 0.0, 0.0])                     # a half turn about x against a random pose
        pred[5, :4] = torch.tensor([0.5, 0.5, 0.5, -0.5])                    # 2 (q0 q2 - q1 q3) = +1 exactly
        pred[6, :4] = torch.tensor([0.5, 0.5, -0.5, 0.5])                    # ... = -1 exactly
        if float(asin_arg(pred[:5, :4]).max()) <= 0.99 and float(asin_arg(gt[:, :4]).max()) <= 0.99:
            break
    assert float(pred[2, 0]) < 0 and float(gt[2, 0]) < 0
    assert asin_arg(pred[5:, :4]).tolist() == [1.0, 1.0]
    pcds = f(P, N, 3) * 0.3
    return pcds.contiguous(), pred.contiguous(), gt.contiguous(), torch.tensor([0, P], dtype=torch.int32)


def test_special_rows(dev):
    from diffassemble_amd.metrics3d import batch_metrics
    pcds, pred, gt, ptr = special_rows()
    pp, po = run_direct(dev, pcds, pred, gt, ptr)
    assert bool(torch.isfinite(pp).all()) and bool(torch.isfinite(po).all())
    part64, _ = reference64(pcds, pred, gt, ptr)
    _, part32 = batch_metrics(pcds, pred, gt, ptr=ptr, return_per_part=True)
    for c, col in enumerate(COLS):                                           # all rows but the gimbal rows, against the host fp32 functions' error
        within_4x(f"special rows {col}", pp[:5, c], part32[:5, c], part64[:5, c])
    # identical poses: zero distances, and gd_r at the clamp is torch-fp32's value (acos of fp32(1 - 1e-6)), not fp64's
    assert float(pp[0, 0]) == 0.0 and float(pp[0, 1]) == 0.0 and float(pp[0, 3]) == 0.0
    clamp32 = float(torch.acos(torch.tensor(1 - 1e-6, dtype=torch.float32)))
    assert abs(float(pp[0, 2]) - clamp32) <= ULP16 * clamp32 and abs(float(pp[0, 2]) - math.acos(1 - 1e-6)) > 1e-3 * clamp32
    assert abs(float(pp[0, 2]) - float(part32[0, 2])) <= ULP16 * clamp32
    # q against -q: the same Euler angles, the same rotation matrix, the same posed points
    assert float(pp[1, 1]) == 0.0 and abs(float(pp[1, 2]) - clamp32) <= ULP16 * clamp32
    for r in (5, 6):                                                         # gimbal rows: only a sane angle is asked
        assert 0.0 <= float(pp[r, 1]) <= 180.0


# ------------------------------------------------------------------------------------------------ the 3D module
def test_validation_step_scores_through_batch_metrics(dev):
    """validation_step on a ragged three-object Batch (20 / 7 / 13 parts, categories repeating): every per-category metric
    equals the mean over the category's objects of the host route of ``batch_metrics`` on the returned poses; without clouds
    the part accuracy is not updated."""
    from diffassemble_amd.metrics3d import batch_metrics
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType, _metric_was_updated
    lp = C.LOOPS3D[0]
    spec = C.by_name(lp["base"])
    case = C.build_case(spec, "3d")
    m = GNN_Diffusion(steps=lp["T"], sampling="DDIM", inference_ratio=lp["ratio"], noise_weight=lp["noise_weight"],
                      model_mean_type=ModelMeanType.START_X, backbone="vn_dgcnn", architecture=spec["arch"])
    m.model.load_state_dict(case["sd"], strict=False)
    m = m.to(dev).eval()
    m.model.precision = "fp32"
    P = case["x"].shape[0]
    rng = np.random.default_rng(3)
    pcds = torch.from_numpy(rng.standard_normal((P, 200, 3)).astype(np.float32)) * 0.3
    gt = case["x"].clone()
    cats = ["everyday", "artifact", "everyday"]
    batch = SimpleNamespace(x=gt.to(dev), pcds=pcds.to(dev), edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev),
                            pcd_feats=case["feats"].to(dev), category=cats)
    m.initialize_torchmetrics(["everyday", "artifact"])
    torch.manual_seed(0)
    final = m.validation_step(batch, 0).cpu()
    assert final.shape == (P, 7) and bool(torch.isfinite(final).all())
    host = batch_metrics(pcds, final, gt, batch=case["batch"])
    assert host.shape == (3, 4)
    for cat in ("everyday", "artifact"):
        rows = [g for g, c in enumerate(cats) if c == cat]
        for c, k in enumerate(("rmse_t", "rmse_r", "gd_r", "part_acc")):
            got, want = float(m.metrics[f"{k}_{cat}"].compute()), float(host[rows, c].double().mean())
            print(f"{k}_{cat}: module {got:.6f}  host route {want:.6f}")
            assert abs(got - want) < (1e-6 if k == "part_acc" else 1e-4), (k, cat, got, want)
    m.initialize_torchmetrics(["everyday", "artifact"])
    batch.pcds = None
    m.validation_step(batch, 0)
    assert _metric_was_updated(m.metrics["rmse_t_everyday"]) and _metric_was_updated(m.metrics["gd_r_artifact"])
    assert not _metric_was_updated(m.metrics["part_acc_everyday"]) and not _metric_was_updated(m.metrics["part_acc_artifact"])
