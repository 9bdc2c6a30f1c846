"""GPU tests of the 2D Batch scoring: ``da_score2d`` (diffassemble_amd/csrc/da_score2d.hip) through the C ABI and through
``score2d.batch_scores``, and ``GNN_Diffusion.validation_step`` on top of it.

Two expectations:
  (a) the composition the scoring used on the device before: ``engine.greedy_assign`` for both assignments plus the torch loop
      (``score2d._loop_scores`` fed device tensors, reached with ``score2d.USE_KERNEL = False``).  The kernel's distances, ties
      and clamps are da_greedy_assign's, so the assigned cells are IDENTICAL on any input: near-ties, exact ties, NaN.
  (b) the host route on CPU copies, for the inputs of tests/test_score2d_host.py whose greedy choices are all clear by 1e-5
      (relative, checked there in fp64) and whose cosines stay 1e-3 away from cos(pi / 4).
Everything compared is an integer or a flag: there is no tolerance."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import cases as C
import test_score2d_host as H
from oracle import weights as W

pytestmark = pytest.mark.gpu
POISON = 0x5B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@contextlib.contextmanager
def kernel_off():
    from diffassemble_amd import score2d
    old, score2d.USE_KERNEL = score2d.USE_KERNEL, False
    try:
        yield
    finally:
        score2d.USE_KERNEL = old


def scores(c, device, use_batch=False):
    """(piece_ok, correct, cell_pred, cell_gt) of a case on ``device``, everything back on the host."""
    from diffassemble_amd.score2d import batch_scores
    kw = dict(batch=c["batch"].to(device)) if use_batch else dict(ptr=c["ptr"].to(device))
    out = batch_scores(c["pred"].to(device), c["gt"].to(device), c["dims"], rotation=c["rotation"], return_cells=True, **kw)
    return tuple(t.cpu() for t in out)


def assert_same(got, want, what):
    for name, a, b in zip(("piece_ok", "correct", "cell_pred", "cell_gt"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), (what, name, a.tolist()[:40], b.tolist()[:40])


def check(c, dev, host_too):
    got = scores(c, dev)
    with kernel_off():
        assert_same(got, scores(c, dev), "(a) greedy_assign twice + the torch loop")
    if host_too:
        assert_same(got, scores(c, torch.device("cpu")), "(b) host route")
    return got


def raw_call(c, dev, cells=True, poison=POISON, max_n=None, max_m=None):
    """da_score2d through the C ABI on poisoned outputs -> (rc, piece_ok uint8, per_puzzle, cell_pred, cell_gt) on the host."""
    from diffassemble_amd import _lib
    from diffassemble_amd.score2d import _grid
    pred, gt = c["pred"].to(dev).contiguous(), c["gt"].to(dev).contiguous()
    dims = c["dims"].tolist()
    grid = torch.cat([_grid(r, k, dev) for r, k in dims]).contiguous()
    n = (c["ptr"][1:] - c["ptr"][:-1]).tolist()
    m = [r * k for r, k in dims]
    ptr_cell = torch.tensor([0] + list(torch.tensor(m).cumsum(0)), dtype=torch.int32, device=dev)
    ptr_piece = c["ptr"].to(dev, torch.int32)
    N, G = pred.shape[0], len(dims)
    ok = torch.full((N,), poison, dtype=torch.uint8, device=dev)
    per = torch.full((G, 4), -7, dtype=torch.int32, device=dev)
    cp, cg = (torch.full((N,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    rc = _lib.lib().da_score2d(G, _lib.ptr(pred), pred.shape[1], _lib.ptr(gt), gt.shape[1], _lib.ptr(grid), 2, _lib.ptr(ptr_piece),
                               _lib.ptr(ptr_cell), max_n or max(n), max_m or max(m), int(c["rotation"]),
                               _lib.ptr(cp) if cells else None, _lib.ptr(cg) if cells else None, _lib.ptr(ok), _lib.ptr(per),
                               _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, ok.cpu(), per.cpu(), cp.cpu(), cg.cpu()


# ------------------------------------------------------------------------------------------------ against both expectations
@pytest.mark.parametrize("name", sorted(H.NOISY))
def test_noisy_cases_equal_the_parent_composition_and_the_host_route(dev, name):
    """1 x 1, 2 x 3, 3 x 3 with 7 pieces, 6 x 6 with and without rotation, 23 x 23 (529 rows: more than the 512 threads of one
    half of the workgroup, so the strided row loops run), and the ragged Batch mixing four sizes in one launch."""
    c = H.noisy_case(name)
    got = check(c, dev, host_too=True)
    assert_same(scores(c, dev, use_batch=True), got, "batch vector instead of ptr")
    if c["pred"].shape[0] >= 36:
        assert 0 < int(got[0].sum()) < got[0].numel()                       # right and wrong pieces both occur


def test_exact_ties(dev):
    """Every piece on one point (all rows tie at every step), and a ground truth exactly on the cell centres (every winning
    distance an exact zero): row-major tie-breaking, identical to da_greedy_assign's; the exact ground truth recovers its cells."""
    g = torch.Generator().manual_seed(1)
    puzzles = ((6, 6), (2, 3), (5, 4))
    preds, gts, perms = [], [], []
    for rows, cols in puzzles:
        grid = H.grid_of(rows, cols)
        perm = torch.randperm(rows * cols, generator=g)
        perms.append(perm)
        gts.append(grid[perm])
        preds.append(torch.tensor([[0.1, -0.3]]).repeat(rows * cols, 1))
    counts = [r * k for r, k in puzzles]
    c = dict(pred=torch.cat(preds), gt=torch.cat(gts), dims=torch.tensor(puzzles), rotation=False,
             ptr=torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32),
             batch=torch.repeat_interleave(torch.arange(3), torch.tensor(counts)))
    ok, correct, cp, cg = check(c, dev, host_too=False)
    assert torch.equal(cg, torch.cat(perms))
    lo = 0
    for n in counts:
        assert sorted(cp[lo:lo + n].tolist()) == list(range(n))             # still a permutation of the cells
        lo += n
    same = dict(c, pred=c["gt"].clone())
    ok, correct, cp, cg = check(same, dev, host_too=True)                   # zeros are zeros on the host too
    assert bool(ok.all()) and bool(correct.all()) and torch.equal(cp, cg)


def test_puzzle_beyond_48_kb_of_lds(dev):
    """36 x 36 = 1296 cells need 52 KB of LDS: the launch that has to raise the kernel's dynamic-LDS limit first, with a 2 x 3
    puzzle in the same Batch.  Expectation (a) only: no seed keeps 1.7 million pairs clear of near-ties."""
    g = torch.Generator().manual_seed(2)
    puzzles = ((36, 36), (2, 3))
    perms = [torch.randperm(r * k, generator=g) for r, k in puzzles]
    gts = [H.grid_of(r, k)[p] for (r, k), p in zip(puzzles, perms)]
    preds = [x + 0.35 * (2.0 / (max(r, k) - 1)) * torch.randn(x.shape, generator=g) for x, (r, k) in zip(gts, puzzles)]
    c = dict(pred=torch.cat(preds), gt=torch.cat(gts), dims=torch.tensor(puzzles), rotation=False,
             ptr=torch.tensor([0, 1296, 1302], dtype=torch.int32), batch=torch.repeat_interleave(torch.arange(2), torch.tensor([1296, 6])))
    from diffassemble_amd.score2d import _lds_bytes
    assert 48 * 1024 < _lds_bytes(1296, 1296) <= 160 * 1024
    ok, correct, cp, cg = check(c, dev, host_too=False)
    assert sorted(cp[:1296].tolist()) == list(range(1296)) and torch.equal(cg, torch.cat(perms))      # exact ground truth: its own cells
    assert 0 < int(ok.sum()) < ok.numel()


def test_wide_rows_and_unequal_leading_dimensions(dev):
    """``pred`` with four columns and rotation off, ``gt`` as the first two columns of six (ld_gt = 6 != ld_pred = 4): the columns
    the call has no business with hold NaN."""
    from diffassemble_amd.score2d import batch_scores
    c = H.noisy_case("ragged")
    want = scores(c, dev)
    N = c["pred"].shape[0]
    pred4 = torch.full((N, 4), float("nan"))
    pred4[:, :2] = c["pred"]
    gt6 = torch.full((N, 6), float("nan"))
    gt6[:, :2] = c["gt"]
    gt_view = gt6.to(dev)[:, :2]
    assert gt_view.stride() == (6, 1)
    got = batch_scores(pred4.to(dev), gt_view, c["dims"], ptr=c["ptr"], rotation=False, return_cells=True)
    assert_same(tuple(t.cpu() for t in got), want, "ld_pred 4, ld_gt 6")


@pytest.mark.parametrize("rotation", [False, True])
def test_non_finite_poses(dev, rotation):
    """One NaN row, one Inf row and an all-NaN puzzle in a ragged Batch: the call returns, every flag is 0 or 1, the cells are
    cells, the composition (a) agrees, and the puzzles without such rows score as they do in the clean Batch."""
    c = H.noisy_case("ragged_rot" if rotation else "ragged")
    clean = scores(c, dev)
    b = c["ptr"].tolist()
    bad = dict(c, pred=c["pred"].clone())
    bad["pred"][b[1]:b[2]] = float("nan")                                   # puzzle 1 (2 x 3): every row
    bad["pred"][b[3] + 4] = float("nan")                                    # puzzle 3 (6 x 6): one NaN row, one Inf row
    bad["pred"][b[3] + 9, 0] = float("inf")
    got = check(bad, dev, host_too=False)
    rc, ok, per, cp, cg = raw_call(bad, dev)
    assert rc == 0 and set(ok.tolist()) <= {0, 1} and set(per[:, 0].tolist()) <= {0, 1}
    for g, (rows, cols) in enumerate(c["dims"].tolist()):
        assert 0 <= int(cp[b[g]:b[g + 1]].min()) and int(cp[b[g]:b[g + 1]].max()) < rows * cols
    for g in (0, 2):                                                        # untouched puzzles
        for k in (0, 2, 3):
            assert torch.equal(got[k][b[g]:b[g + 1]], clean[k][b[g]:b[g + 1]]), (g, k)
        assert bool(got[1][g]) == bool(clean[1][g])
    assert torch.equal(got[3], clean[3])                                    # the ground truth's cells never saw the NaNs
    if rotation:
        assert not bool(got[0][b[1]:b[2]].any()) and not bool(got[0][b[3] + 4])      # a NaN cosine compares false


def test_zero_rotation_vector_is_wrong_and_no_nan_escapes(dev):
    c = H.noisy_case("6x6_rot")
    c["pred"][:, :2] = c["gt"][:, :2]                                       # positions right: the rotation decides
    c["pred"][:, 2:] = c["gt"][:, 2:]
    c["pred"][5, 2:] = 0.0
    c["gt"][11, 2:] = 0.0
    ok, correct, cp, cg = check(c, dev, host_too=True)
    want = torch.ones(36, dtype=torch.bool)
    want[5] = want[11] = False
    assert torch.equal(ok, want) and correct.tolist() == [False] and torch.equal(cp, cg)
    rc, raw, per, _, _ = raw_call(c, dev)
    assert rc == 0 and per.tolist() == [[0, 34, 36, 34]]


# ------------------------------------------------------------------------------------------------ the C entry point
def test_poisoned_outputs_are_fully_overwritten_and_cells_may_be_null(dev):
    c = H.noisy_case("ragged_rot")
    rc, ok, per, cp, cg = raw_call(c, dev)
    assert rc == 0
    assert POISON not in ok.tolist() and -7 not in per.flatten().tolist() and -7 not in cp.tolist() and -7 not in cg.tolist()
    want = scores(c, dev)
    assert torch.equal(ok.bool(), want[0]) and torch.equal(per[:, 0].bool(), want[1])
    assert torch.equal(cp.long(), want[2]) and torch.equal(cg.long(), want[3])
    n = c["ptr"][1:] - c["ptr"][:-1]
    b = c["ptr"].tolist()
    for g in range(len(n)):
        flags = ok[b[g]:b[g + 1]]
        pos = cp[b[g]:b[g + 1]] == cg[b[g]:b[g + 1]]
        row = per[g].tolist()
        assert row[:3] == [int(flags.all()), int(flags.sum()), int(pos.sum())] and row[1] <= min(row[2], row[3]) <= int(n[g])
    rc2, ok2, per2, cp2, cg2 = raw_call(c, dev, cells=False)
    assert rc2 == 0 and torch.equal(ok2, ok) and torch.equal(per2, per)
    assert set(cp2.tolist()) == {-7} and set(cg2.tolist()) == {-7}           # NULL tables: nothing written anywhere else
    c0 = H.noisy_case("ragged")
    assert raw_call(c0, dev)[2][:, 3].tolist() == n.tolist()                 # rotation off: every piece counts as n_rot_ok


def test_refusals_come_before_any_launch(dev):
    """More pieces than cells (max_n > max_m) and a puzzle beyond one workgroup's LDS: error code, message, outputs untouched."""
    from diffassemble_amd import _lib
    c = H.noisy_case("2x3")
    for kw, msg in ((dict(max_n=7, max_m=6), b"more pieces than cells"), (dict(max_n=4096, max_m=4096), b"too large")):
        rc, ok, per, cp, cg = raw_call(c, dev, **kw)
        assert rc == 1 and msg in _lib.lib().da_last_error(), kw
        assert set(ok.tolist()) == {POISON} and set(per.flatten().tolist()) == {-7} and set(cp.tolist()) == {-7}


def test_kernel_guard_marks_a_puzzle_with_more_pieces_than_cells(dev):
    """Inside a ragged Batch (max_n <= max_m holds) the workgroup of a puzzle with n > m writes all_correct = -1 and nothing
    else; the other puzzles are scored.  ``batch_scores`` never lets such a Batch reach the kernel: it takes the loop."""
    from diffassemble_amd.score2d import batch_scores
    c = H.noisy_case("ragged")
    want = raw_call(c, dev)
    b = c["ptr"].tolist()
    squeezed = dict(c, dims=torch.tensor([[1, 1], [2, 3], [2, 3], [6, 6]]))      # puzzle 2: 7 pieces, 6 cells
    for which in ("gt", "pred"):                                                 # its choices on the smaller grid are clear too
        assert H.smallest_greedy_gap(c[which][b[2]:b[3]], H.grid_of(2, 3)) >= H.GAP
    rc, ok, per, cp, cg = raw_call(squeezed, dev)
    assert rc == 0 and per[2].tolist() == [-1, -7, -7, -7]
    assert set(ok[b[2]:b[3]].tolist()) == {POISON} and set(cp[b[2]:b[3]].tolist()) == {-7}
    for g in (0, 1, 3):
        assert torch.equal(per[g], want[2][g]) and torch.equal(ok[b[g]:b[g + 1]], want[1][b[g]:b[g + 1]])
    got = batch_scores(c["pred"].to(dev), c["gt"].to(dev), squeezed["dims"], ptr=c["ptr"], return_sizes=True)
    host = batch_scores(c["pred"], c["gt"], squeezed["dims"], ptr=c["ptr"], return_sizes=True)
    assert got[2].tolist() == host[2].tolist() == [[1, 1, 1], [6, 2, 3], [6, 2, 3], [36, 6, 6]]
    assert torch.equal(got[0], host[0]) and torch.equal(got[1], host[1])


# ------------------------------------------------------------------------------------------------ the 2D module
def test_validation_step_metrics_equal_the_fallback_loop(dev):
    """validation_step on a 6 x 6 puzzle and a 6 x 6 puzzle with six pieces missing: every metric's value and number of updates
    equal those of the loop (feature route off) on the same poses."""
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
    spec = C.by_name("k36_loop_sharp")
    case = C.build_case(spec)
    m = GNN_Diffusion(steps=50, sampling="DDIM", model_mean_type=ModelMeanType.START_X, visual_pretrained=False, noise_weight=1.0)
    m.model.load_state_dict(case["sd"], strict=False)
    m = m.to(dev).eval()
    m.model.precision = "fp32"
    sizes = [36, 30]
    ei, bvec = W.collate([W.dense_edge_index(n, True) for n in sizes], sizes)
    grid = H.grid_of(6, 6)
    g = torch.Generator().manual_seed(0)
    x_gt = torch.cat([grid[torch.randperm(36, generator=g)[:n]] for n in sizes])
    feats = torch.cat([case["feats"], case["feats"].flip(0)[:30]])
    batch = SimpleNamespace(x=x_gt.to(dev), patches=None, edge_index=ei.to(dev), batch=bvec.to(dev),
                            patches_dim=torch.tensor([[6, 6], [6, 6]]), patch_feats=feats.to(dev))

    def run():
        m.initialize_torchmetrics([(6, 6)])
        calls = {k: [] for k in m.metrics}
        for k, metric in m.metrics.items():
            metric.update = (lambda k, inner: lambda v: (calls[k].append(torch.as_tensor(v).numel()), inner(v))[1])(k, metric.update)
        img = m.validation_step(batch, 0)
        return img, calls, {k: float(metric.compute()) for k, metric in m.metrics.items()}

    torch.manual_seed(4)
    img, calls, values = run()
    assert img.shape == (66, 2) and bool(torch.isfinite(img).all())
    m.p_sample_loop = lambda *a, **k: ([img], None)                          # the same poses for the loop
    with kernel_off():
        img2, calls2, values2 = run()
    assert img2 is img and calls == calls2 and values == values2
    assert calls["overall__piece_acc"] == [36, 30] and calls["overall_acc"] == [1, 1] and values["overall_nImages"] == 2
    assert calls["(6, 6)__piece_acc"] == [36, 30] and calls["(6, 6)_nImages"] == [1, 1]
