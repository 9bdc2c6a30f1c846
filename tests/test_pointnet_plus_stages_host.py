"""Host half of the PointNet++ encoder's stage-level tests (the kernels: tests/test_gpu_pointnet_plus_stages.py): that the injected
stage inputs of tests/golden/pointnet_plus_refs.py (``stage_cases``) and the elementwise comparison at the stage's ``tol`` have teeth,
shown on the contract alone.

tol = 8 x E32 x max |stage64|, E32 = max |stage32 - stage64| / max |stage64|: the deviation of a plain fp32 evaluation of the stage
(folded weights, BLAS dot products) from fp64, recomputed on every run; 8 for the kernels' other summation order.

* every row position of a group decides some output cell by more than 2 tol (``decisive_positions`` has no zero);
* the contract with one wrong step of the kind a kernel makes -- a row left out of a maximum, groups written one output row off,
  fragment 0's points read for fragment 1, the coordinate columns dropped, a tile of the head dropped -- is outside tol;
* the refactored ``eval_forward`` gives the bits of the one it replaces.
Nothing here loads the library (the workspace layout of ``da_pointnet_plus_workspace_offsets`` is checked in the GPU file)."""
import functools
import os

import numpy as np
import pytest
import torch

import pointnet_plus_refs as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "pointnet_plus_v1.npz"))
RTOL32 = 1e-4
CASES = R.stage_cases()
SA_CASES = [n for n, c in CASES.items() if c.stage != "head"]
COVERED = [n for n, c in CASES.items() if c.coverage]          # all but N = 1, where every row of a group is the same point


@functools.lru_cache(maxsize=None)
def weights():
    return R.state(torch.float64), R.folded32(R.state())


@functools.lru_cache(maxsize=None)
def reference(name):
    return R.stage_reference(CASES[name], *weights())


def within(a, ref, tol):
    return bool(((a - ref).abs() <= tol).all())


def test_cases_are_the_issue_shapes_and_in_range():
    shapes = {n: (c.stage, c.P, c.N) for n, c in CASES.items()}
    assert shapes == {"sa1": ("sa1", 2, 64), "sa1_n2048": ("sa1", 2, 2048), "sa1_n1": ("sa1", 1, 1), "sa2": ("sa2", 2, 64),
                      "sa3": ("sa3", 3, 64), "head": ("head", 5, 64)}
    for n in ("sa1", "sa1_n2048"):
        g = CASES[n].grp1
        assert (np.sort(g, -1)[..., 1:] != np.sort(g, -1)[..., :-1]).all(-1).mean() > 0.95          # distinct members but for the edge groups
    c = CASES["sa1"]
    assert (c.grp1[0, 3] == c.grp1[0, 3, 0]).all() and {0, 63} <= set(c.grp1[1, 4].tolist()) and c.fps1[1, 5] == 63 and c.fps1[1, 511] == 63
    assert (CASES["sa1_n2048"].grp1[1] == 2047).any(-1).all() and CASES["sa1_n2048"].fps1[1, 511] == 2047
    c = CASES["sa2"]
    assert {0, 511} <= set(c.fps2[0].tolist()) and (c.grp2[1, 3] == c.grp2[1, 3, 0]).all() and {0, 511} <= set(c.grp2[0, 4].tolist())
    assert len(set(c.grp2[1, 7].tolist())) == 64 and not np.array_equal(c.l1[0], c.l1[1]) and (c.l1 >= 0).all() and (c.l1 == 0).mean() > 0.4
    part = CASES["head"].part
    top = np.sort(part, 1)
    assert (part >= 0).all() and (top[:, 3] - top[:, 2] >= R.HEAD_MARGIN * 0.999).all()
    share = np.stack([(part.argmax(1) == t).mean(1) for t in range(4)])
    assert share.min() > 0.2 and share.max() < 0.3, share                                            # each tile wins about a quarter, per fragment


@pytest.mark.parametrize("name", list(CASES))
def test_bound_comes_from_the_fp32_reference_and_is_tighter_than_rtol32(name):
    _, out64, out32, e32, tol = reference(name)
    print(f"pointnet_plus stage {name}: E32 {e32:.3e}, tol {tol:.3e} (max |stage64| {float(out64.abs().max()):.4g})")
    assert 0 < R.STAGE_TOL_FACTOR * e32 <= RTOL32
    assert within(out32.double(), out64, tol / R.STAGE_TOL_FACTOR * 1.0000001)


@pytest.mark.parametrize("name", COVERED)
def test_every_row_position_is_decisive(name):
    pre, _, _, _, tol = reference(name)
    if name == "head":
        # tol is in the units of the head's OUTPUT, two dense layers behind the maximum; a tile's lead is in the units of its input,
        # `part`.  Here: each tile leads by the margin it was built with; at tol: test_a_dropped_head_tile_is_seen
        hits = R.decisive_positions(pre, -2, 0.25 * R.HEAD_MARGIN)
    else:
        hits = R.decisive_positions(pre, -2, tol)
    print(f"pointnet_plus stage {name}: {len(hits)} positions, fewest decisive cells {int(hits.min())}")
    assert len(hits) == {"sa1": 32, "sa2": 64, "sa3": 128, "head": 4}[CASES[name].stage]
    assert int(hits.min()) > 0, hits.tolist()


def test_decisive_positions_counts_clear_maxima_only():
    x = torch.tensor([[[1.0, 5.0], [3.0, 5.1], [2.0, 0.0]]])                  # [1, rows 3, channels 2]
    assert R.decisive_positions(x, -2, 0.4).tolist() == [0, 1, 0]             # row 1 wins channel 0 by 1 > 0.8; channel 1 by 0.1 only
    assert R.decisive_positions(x, -2, 0.04).tolist() == [0, 2, 0]
    assert R.decisive_positions(x.transpose(1, 2), -1, 0.04).tolist() == [0, 2, 0]


# ------------------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("name", [n for n in COVERED if n != "head"])
def test_leaving_any_row_out_of_the_maximum_is_seen(name):
    pre, out64, _, _, tol = reference(name)
    top = pre.topk(2, dim=-2)
    for j in range(pre.shape[-2]):
        without = torch.where(top.indices[..., 0, :] == j, top.values[..., 1, :], top.values[..., 0, :])
        if j in (0, pre.shape[-2] - 1):                # the shortcut is the plain thing
            keep = [i for i in range(pre.shape[-2]) if i != j]
            assert torch.equal(without, pre[..., keep, :].max(dim=-2).values)
        assert not within(without, out64, tol), j


@pytest.mark.parametrize("name", [n for n in COVERED if n not in ("sa3", "head")])
def test_groups_written_one_output_row_off_are_seen(name):
    _, out64, _, _, tol = reference(name)
    for shift in (1, -1):
        assert not within(torch.roll(out64, shift, dims=1), out64, tol)
    p = out64.shape[0] - 1                             # only the last fragment's rows off by one
    moved = out64.clone()
    moved[p] = torch.roll(out64[p], 1, dims=0)
    assert not within(moved, out64, tol)


@pytest.mark.parametrize("name", [n for n in COVERED if n != "head"])
def test_another_fragments_points_are_seen(name):
    c = CASES[name]
    _, out64, _, _, tol = reference(name)
    pts = c.pts.copy()
    pts[1:] = pts[0]
    got = R.stage_sa(weights()[0], int(c.stage[2]), R.stage_rows(c, torch.float64, pts=pts))[1]
    assert within(got[0], out64[0], 0.0)
    for p in range(1, c.P):
        assert not within(got[p], out64[p], tol), p


@pytest.mark.parametrize("name", ["sa2", "sa3"])
def test_dropped_coordinate_columns_are_seen(name):
    c = CASES[name]
    _, out64, _, _, tol = reference(name)
    got = R.stage_sa(weights()[0], int(c.stage[2]), R.stage_rows(c, torch.float64, xyz=False))[1]
    for p in range(c.P):
        assert not within(got[p], out64[p], tol), p


def test_a_dropped_head_tile_is_seen():
    pre, out64, _, _, tol = reference("head")
    for t in range(4):
        got = R.head(weights()[0], pre[:, [k for k in range(4) if k != t]])
        for p in range(pre.shape[0]):
            assert not within(got[p], out64[p], tol), (t, p)
    # and a fragment's tiles taken from its neighbour
    assert not within(R.head(weights()[0], torch.roll(pre, 1, dims=0)), out64, tol)


# ------------------------------------------------------------------------------------------------------------ the refactoring
def _bn_eval(sd, name, y):
    r = 1.0 / torch.sqrt(sd[f"{name}.running_var"] + R.EPS)
    return sd[f"{name}.weight"] * (y - sd[f"{name}.running_mean"]) * r + sd[f"{name}.bias"]


def _stack(sd, level, rows):
    for i in range(3):
        w = sd[f"sa{level}.mlp_convs.{i}.weight"][:, :, 0, 0]
        rows = torch.relu(_bn_eval(sd, f"sa{level}.mlp_bns.{i}", rows @ w.t() + sd[f"sa{level}.mlp_convs.{i}.bias"]))
    return rows


def eval_forward_in_one_piece(sd, pts, sel):
    """The contract's eval_forward as it stood before stage_sa / head were factored out of it, kept word for word."""
    out = []
    for p in range(pts.shape[0]):
        x = pts[p]
        f1, g1, f2, g2 = (torch.from_numpy(sel[k][p]) for k in ("fps1", "grp1", "fps2", "grp2"))
        l1_xyz = x[f1]
        l1 = _stack(sd, 1, torch.cat([x[g1] - l1_xyz[:, None, :], x[g1]], -1)).max(dim=1).values
        l2_xyz = l1_xyz[f2]
        l2 = _stack(sd, 2, torch.cat([l1_xyz[g2] - l2_xyz[:, None, :], l1[g2]], -1)).max(dim=1).values
        l3 = _stack(sd, 3, torch.cat([l2_xyz, l2], -1)).max(dim=0).values
        h = torch.relu(_bn_eval(sd, "bn1", l3 @ sd["fc1.weight"].t() + sd["fc1.bias"]))
        out.append(torch.relu(_bn_eval(sd, "bn2", h @ sd["fc2.weight"].t() + sd["fc2.bias"])))
    return torch.stack(out) if out else pts.new_zeros(0, 256)


@pytest.mark.parametrize("P,N", [(1, 1), (1, 64), (2, 513)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_eval_forward_keeps_its_bits(P, N, dtype):
    """The fixture stores the REFERENCE's fp32 outputs, no digest of the contract's (an fp64 product's last bits are the BLAS build's,
    not the project's): the digest is taken of both formulations here, on one machine.  tests/test_pointnet_plus_host.py goes on
    holding eval_forward against the fixture."""
    pre = f"case/{P}x{N}/"
    pts = R.make_cloud(P, N, int(GOLD[pre + "cloud_seed"]))
    sel = R.select(pts, GOLD[pre + "start1"], GOLD[pre + "start2"])
    sd, x = R.state(dtype), torch.from_numpy(pts).to(dtype)
    new, old = R.eval_forward(sd, x, sel), eval_forward_in_one_piece(sd, x, sel)
    assert new.shape == (P, 256) and R.digest(new.numpy()) == R.digest(old.numpy())
    chain = R.eval_chain(sd, x, sel)
    assert R.digest(chain["out"].numpy()) == R.digest(old.numpy())
    if dtype == torch.float64 and N > 1:
        ref = torch.from_numpy(GOLD[pre + "eval_out"]).double()
        assert float((new - ref).abs().max() / ref.abs().max()) <= max(16 * float(GOLD[pre + "dev/eval_out"]), 1e-5)
