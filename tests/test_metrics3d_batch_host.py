"""Host-side checks of the batched 3D pose metrics (diffassemble_amd/metrics3d.py ``batch_metrics``, C entry point
``da_metrics3d``): the C ABI carries the entry point, bad arguments are refused before anything is launched, and the host route
of ``batch_metrics`` -- the CPU statement of what the kernels compute -- reproduces the reference's own values
(golden_v2.npz, "metrics3d_*") and the oracle restatement on a ragged Batch.  No GPU.

The three fixture cases have different N (200, 1000, 64) and a Batch holds one N, so they are GROUPED BY N: each case is the
single object of its own Batch (padding by repeating points would need the common multiple 8000 to keep the means).  Their
pose metrics, which do not depend on N, are also checked as the three objects of ONE Batch with ``pcds=None``."""
import math
import os
import re

import numpy as np
import pytest
import torch

import cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ("rmse_t", "rmse_r", "gd_r", "part_acc")


def close(v, ref):
    """The tolerance tests/test_oracle.py applies to the same fixtures."""
    return abs(float(v) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))


def ragged_batch(counts=(20, 7, 13), N=50, noise=0.08, seed=11):
    """Poses and clouds of objects with ``counts`` parts; the noise scale puts the Chamfer losses on both sides of 0.01."""
    rng = np.random.default_rng(seed)
    P = sum(counts)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))  # noqa: E731
    pcds = f(P, N, 3) * 0.3
    gt = torch.cat([torch.nn.functional.normalize(f(P, 4), dim=-1), f(P, 3) * 0.5], 1)
    scale = torch.from_numpy(rng.uniform(0.0, noise, (P, 1)).astype(np.float32))
    pred = gt + scale * f(P, 7)
    pred[:, :4] = torch.nn.functional.normalize(pred[:, :4], dim=-1)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    batch = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    return pcds, pred, gt, ptr, batch


def test_header_library_and_binding_carry_da_metrics3d():
    from diffassemble_amd import _lib, metrics3d
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())
    assert ("int da_metrics3d(int n_parts, int n_points, int n_objects, const float *pred, int ld_pred, const float *gt, int ld_gt, "
            "const float *pcds, const int32_t *ptr, float thr, float *per_part, float *per_object, void *stream);") in text
    for cite in ("362-383", "415-450", "916-945", "1089-1129", "895-960", "1036-1080"):
        assert cite in text.split("int da_metrics3d(")[0][-2000:], cite      # the comment names the reference lines it replaces
    h = _lib.lib()
    assert "da_metrics3d" in _lib.PROTOTYPES and h.da_metrics3d.argtypes == _lib.PROTOTYPES["da_metrics3d"][1]
    assert len(_lib.PROTOTYPES["da_metrics3d"][1]) == 13
    assert h.da_abi_version() == _lib.ABI_VERSION == 19                      # additive: the ABI number stays
    assert callable(metrics3d.batch_metrics)


def test_entry_point_checks_its_arguments_before_launching():
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = 1 << 12                                                           # a non-null address: every refusal below comes before any use
    assert h.da_metrics3d(4, 8, 1, None, 7, None, 7, None, None, 0.01, None, None, None) == 1 and b"null argument" in h.da_last_error()
    assert h.da_metrics3d(4, 8, 1, one, 7, one, 7, one, None, 0.01, one, one, None) == 1 and b"null argument" in h.da_last_error()
    for sizes in ((0, 8, 1), (4, 0, 1), (4, 8, 0), (-1, 8, 1)):
        assert h.da_metrics3d(*sizes, one, 7, one, 7, one, one, 0.01, one, one, None) == 1 and b"bad sizes" in h.da_last_error(), sizes
    for lds in ((6, 7), (7, 6), (0, 8)):
        assert h.da_metrics3d(4, 8, 1, one, lds[0], one, lds[1], one, one, 0.01, one, one, None) == 1 and b"7 floats" in h.da_last_error(), lds


def test_batch_metrics_refuses_inconsistent_arguments():
    from diffassemble_amd.metrics3d import batch_metrics
    pcds, pred, gt, ptr, batch = ragged_batch()
    with pytest.raises(ValueError):
        batch_metrics(pcds, pred, gt)                                       # neither ptr nor batch
    with pytest.raises(ValueError):
        batch_metrics(pcds, pred, gt, ptr=ptr, batch=batch)                 # both
    with pytest.raises(ValueError):
        batch_metrics(pcds, pred[:, :6], gt[:, :6], ptr=ptr)
    with pytest.raises(ValueError):
        batch_metrics(pcds, pred, gt[:-1], ptr=ptr)
    with pytest.raises(ValueError):
        batch_metrics(pcds[:-1], pred, gt, ptr=ptr)
    with pytest.raises(ValueError):
        batch_metrics(pcds, pred, gt, batch=batch[:-1])


@pytest.mark.parametrize("ms", C.METRICS3D, ids=lambda s: s["name"])
def test_host_route_reproduces_the_reference_fixtures(ms):
    """Grouped by N: the case is the one object of its Batch; all four values against the reference's own."""
    from diffassemble_amd.metrics3d import batch_metrics
    g2 = C.load_golden2()
    pcds, pred, gt = C.metrics3d_inputs(ms)
    got = batch_metrics(pcds, pred, gt, ptr=torch.tensor([0, ms["P"]], dtype=torch.int32))
    assert got.shape == (1, 4) and got.dtype == torch.float32
    for c, k in enumerate(KEYS):
        assert close(got[0, c], g2[f"{ms['name']}/{k}"]), (k, float(got[0, c]), float(g2[f"{ms['name']}/{k}"]))
    same = batch_metrics(pcds, pred, gt, batch=torch.zeros(ms["P"], dtype=torch.long))
    assert torch.equal(same, got)


def test_three_fixture_cases_as_the_objects_of_one_batch_pose_metrics():
    from diffassemble_amd.metrics3d import batch_metrics
    g2 = C.load_golden2()
    ins = [C.metrics3d_inputs(ms) for ms in C.METRICS3D]
    pred, gt = torch.cat([i[1] for i in ins]), torch.cat([i[2] for i in ins])
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([ms["P"] for ms in C.METRICS3D])]), dtype=torch.int32)
    got = batch_metrics(None, pred, gt, ptr=ptr)
    assert got.shape == (3, 4) and torch.isnan(got[:, 3]).all()             # no clouds: no part accuracy
    for g, ms in enumerate(C.METRICS3D):
        for c, k in enumerate(KEYS[:3]):
            assert close(got[g, c], g2[f"{ms['name']}/{k}"]), (ms["name"], k)


def test_ragged_batch_equals_the_oracle_per_object():
    """20 / 7 / 13 parts: every object's four values equal oracle/metrics3d.py on that object's rows; ``ptr`` and ``batch`` agree;
    the per-part table averages to the per-object one; an object without parts is a NaN row."""
    from diffassemble_amd.metrics3d import batch_metrics
    from oracle import metrics3d as OM
    pcds, pred, gt, ptr, batch = ragged_batch()
    got, per_part = batch_metrics(pcds, pred, gt, ptr=ptr, return_per_part=True)
    assert got.shape == (3, 4) and per_part.shape == (40, 4)
    assert torch.equal(batch_metrics(pcds, pred, gt, batch=batch), got)
    b = ptr.tolist()
    for g in range(3):
        s = slice(b[g], b[g + 1])
        want = (OM.trans_rmse(pred[s, 4:], gt[s, 4:]), OM.rot_rmse(pred[s, :4], gt[s, :4]), OM.geodesic(pred[s, :4], gt[s, :4]),
                OM.part_accuracy(pcds[s], pred[s, 4:], gt[s, 4:], pred[s, :4], gt[s, :4]))
        for c in range(3):
            assert close(got[g, c], want[c]), (g, KEYS[c], float(got[g, c]), float(want[c]))
        assert abs(float(got[g, 3]) - float(want[3])) < 1e-6
        assert torch.allclose(per_part[s, :3].mean(0), got[g, :3], rtol=1e-5, atol=0)
        assert abs(float((per_part[s, 3] < 0.01).float().mean()) - float(got[g, 3])) < 1e-6
    assert 0.0 < float(got[0, 3]) < 1.0                                      # the threshold is exercised
    holes = torch.tensor([0, 20, 20, 27, 40], dtype=torch.int32)             # object 1 has no parts
    got4 = batch_metrics(pcds, pred, gt, ptr=holes)
    assert torch.isnan(got4[1]).all() and torch.equal(got4[[0, 2, 3]], got)
    assert math.isnan(float(batch_metrics(None, pred, gt, ptr=ptr)[0, 3]))
