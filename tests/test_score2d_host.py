"""Host-side checks of the 2D Batch scoring (diffassemble_amd/score2d.py ``batch_scores``, C entry point ``da_score2d``): the C
ABI carries the entry point, bad arguments are refused before anything is launched, and the host route of ``batch_scores``
reproduces a literal restatement of the reference's ``validation_step`` arithmetic (spatial_diffusion.py:775-856, 915-955).
No GPU.

The input generators below are shared with tests/test_gpu_score2d.py.  The GPU test compares the kernel (fp32 distances,
uncontracted) with the host route (torch.norm on the host): the two may round a distance differently by an ulp, which can only
change a greedy choice where two candidate distances are that close.  So every NOISY case must satisfy a condition ON THE
INPUTS (not a tolerance on the kernel): in the fp64 greedy run of both of its assignment problems, the winning distance of
every step is at least 1e-5 (relative) below the runner-up among the pairs still free.  Random draws violate it now and then
(a 23 x 23 puzzle has 280 000 pairs; gaps down to 2e-6 were seen), so the seeds were searched on the CPU and are fixed here;
``test_noisy_inputs_keep_every_greedy_choice_clear`` asserts the condition for each.  Rotation inputs keep every cosine at
least 1e-3 away from cos(pi / 4): at exactly 45 degrees the comparison is decided by fp32 rounding alone."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GAP = 1e-5
COS45 = math.cos(math.pi / 4)

# name -> (puzzles as (rows, cols, pieces removed), rotation, seed)
NOISY = {
    "1x1": (((1, 1, 0),), False, 0),
    "2x3": (((2, 3, 0),), False, 0),
    "3x3_7_pieces": (((3, 3, 2),), False, 0),
    "6x6": (((6, 6, 0),), False, 0),
    "6x6_rot": (((6, 6, 0),), True, 0),
    "23x23": (((23, 23, 0),), False, 639),          # smallest gap 2.5e-5, the widest of seeds 0 .. 699 (most are below 1e-5)
    "ragged": (((1, 1, 0), (2, 3, 0), (3, 3, 2), (6, 6, 0)), False, 1),
    "ragged_rot": (((1, 1, 0), (2, 3, 0), (3, 3, 2), (6, 6, 0)), True, 0),
}
HOST_CASES = ("1x1", "2x3", "3x3_7_pieces", "ragged", "ragged_rot")          # small enough for the literal loop


def grid_of(rows, cols):
    """The puzzle's cell centres as validation_step builds them (spatial_diffusion.py:931-934)."""
    y = torch.linspace(-1, 1, rows)
    x = torch.linspace(-1, 1, cols)
    return torch.stack(torch.meshgrid(x, y, indexing="xy"), -1).reshape(-1, 2)


def make_case(puzzles, rotation, seed):
    """A Batch: per puzzle a random subset of the cells, the ground truth a little off its cell, the prediction further off
    (about a third of the cell spacing: some pieces land on a neighbour's cell).  With ``rotation`` the ground truth points
    along a multiple of 90 degrees and the prediction is turned by a random angle whose cosine stays 1e-3 away from cos(pi / 4),
    with a random length.  -> dict(pred, gt, dims [G, 2], ptr int32 [G + 1], batch [N], rotation)."""
    rng = np.random.default_rng(seed)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))  # noqa: E731
    preds, gts, counts = [], [], []
    for rows, cols, removed in puzzles:
        grid = grid_of(rows, cols)
        n = rows * cols - removed
        keep = torch.from_numpy(rng.permutation(rows * cols)[:n].copy())
        step = 2.0 / max(max(rows, cols) - 1, 1)
        gt = grid[keep] + 0.02 * step * f(n, 2)
        pred = gt + 0.35 * step * f(n, 2)
        if rotation:
            a = torch.from_numpy(rng.integers(0, 4, n).astype(np.float32)) * (math.pi / 2)
            turn = []
            while len(turn) < n:
                d = float(rng.uniform(-math.pi, math.pi))
                if abs(math.cos(d) - COS45) > 2e-3:
                    turn.append(d)
            b = a + torch.tensor(turn, dtype=torch.float32)
            length = torch.from_numpy(rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))
            gt = torch.cat((gt, torch.stack((torch.cos(a), torch.sin(a)), 1)), 1)
            pred = torch.cat((pred, length * torch.stack((torch.cos(b), torch.sin(b)), 1)), 1)
        preds.append(pred)
        gts.append(gt)
        counts.append(n)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    batch = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    dims = torch.tensor([[r, c] for r, c, _ in puzzles])
    return dict(pred=torch.cat(preds).contiguous(), gt=torch.cat(gts).contiguous(), dims=dims, ptr=ptr, batch=batch, rotation=rotation)


def noisy_case(name):
    return make_case(*NOISY[name])


def smallest_greedy_gap(pos, grid):
    """fp64 greedy run of ``pos`` [n, 2] against ``grid`` [m, 2]: the smallest relative gap, over the steps, between the
    winning distance and the runner-up among the pairs free at that step (inf when a step has a single free pair)."""
    d = np.linalg.norm(pos.double().numpy()[:, None, :] - grid.double().numpy()[None, :, :], axis=2)
    n, m = d.shape
    order = np.argsort(d, axis=None, kind="stable")
    dist = d.reshape(-1)[order]
    row_free, col_free = np.ones(n, bool), np.ones(m, bool)
    worst, k, done = math.inf, 0, 0
    while done < min(n, m):
        while not (row_free[order[k] // m] and col_free[order[k] % m]):
            k += 1
        q = k + 1
        while q < order.size and not (row_free[order[q] // m] and col_free[order[q] % m]):
            q += 1
        if q < order.size:
            worst = min(worst, (dist[q] - dist[k]) / dist[q] if dist[q] > 0 else 0.0)
        row_free[order[k] // m] = col_free[order[k] % m] = False
        done += 1
    return worst


def reference_scores(case):
    """The reference's per-puzzle arithmetic, literally: the TorchScript loop of greedy_cost_assignment
    (spatial_diffusion.py:179-216), the two sorts by row, the comparison, the cosine test (:931-955)."""
    def greedy(pos1, pos2):
        dist = torch.norm(pos1[:, None] - pos2, dim=2)
        mask = torch.ones_like(dist, dtype=torch.bool)
        out = []
        while mask.sum() > 0:
            mv, mi = dist[mask].min(dim=0)
            i, j = mask.nonzero()[int(mi)]
            out.append((int(i), int(j), int(mv)))
            mask[i, :] = 0
            mask[:, j] = 0
        return torch.tensor(out, dtype=torch.int64).reshape(-1, 3)

    img, x, flags, verdicts, cells_pred, cells_gt = case["pred"], case["gt"], [], [], [], []
    for i in range(int(case["batch"].max()) + 1):
        idx = torch.where(case["batch"] == i)[0]
        gt_pos, pos = x[idx, :2], img[idx, :2]
        n_patches = case["dims"][i].tolist()
        real_grid = grid_of(n_patches[0], n_patches[1])
        gt_ass = greedy(gt_pos, real_grid)
        gt_ass = gt_ass[torch.sort(gt_ass[:, 0])[1]]
        pred_ass = greedy(pos, real_grid)
        pred_ass = pred_ass[torch.sort(pred_ass[:, 0])[1]]
        correct = (gt_ass[:, 1] == pred_ass[:, 1]).all()
        piece_accuracy = gt_ass[:, 1] == pred_ass[:, 1]
        if case["rotation"]:
            rot_correct = torch.cosine_similarity(img[idx, 2:], x[idx, 2:]) > math.cos(math.pi / 4)
            correct = correct and rot_correct.all()
            piece_accuracy = rot_correct * piece_accuracy
        flags.append(piece_accuracy)
        verdicts.append(bool(correct))
        cells_pred.append(pred_ass[:, 1])
        cells_gt.append(gt_ass[:, 1])
    return torch.cat(flags), torch.tensor(verdicts), torch.cat(cells_pred), torch.cat(cells_gt)


def test_header_library_and_binding_carry_da_score2d():
    from diffassemble_amd import _lib, score2d
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())
    assert ("int da_score2d(int n_puzzles, const float *pred, int ld_pred, const float *gt, int ld_gt, const float *grid, int ld_grid, "
            "const int32_t *ptr_piece, const int32_t *ptr_cell, int max_n, int max_m, int rotation, int32_t *cell_pred, "
            "int32_t *cell_gt, uint8_t *piece_ok, int32_t *per_puzzle, void *stream);") in text
    comment = text.split("int da_score2d(")[0][-2500:]
    for cite in ("spatial_diffusion.py:775-856, 915-955", "row-major", "n_g <= m_g"):      # the lines it replaces, the tie rule, the precondition
        assert cite in comment, cite
    h = _lib.lib()
    assert "da_score2d" in _lib.PROTOTYPES and h.da_score2d.argtypes == _lib.PROTOTYPES["da_score2d"][1]
    assert len(_lib.PROTOTYPES["da_score2d"][1]) == 17
    assert h.da_abi_version() == _lib.ABI_VERSION == 19                      # additive: the ABI number stays
    assert callable(score2d.batch_scores)


def test_entry_point_checks_its_arguments_before_launching():
    """Every refusal below comes before any use of a pointer or of the device: null arguments, bad sizes, more pieces than
    cells, a puzzle beyond one workgroup's LDS."""
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = 1 << 12                                                           # a non-null address

    def call(G=1, ld=(2, 2, 2), max_n=4, max_m=4, rot=0, ptrs=(one,) * 9):
        pred, gt, grid, pp, pc, cp, cg, ok, per = ptrs
        return h.da_score2d(G, pred, ld[0], gt, ld[1], grid, ld[2], pp, pc, max_n, max_m, rot, cp, cg, ok, per, None)

    for missing in (0, 1, 2, 3, 4, 7, 8):                                   # cell_pred / cell_gt (5, 6) may be NULL
        assert call(ptrs=tuple(None if k == missing else one for k in range(9))) == 1 and b"null argument" in h.da_last_error(), missing
    for kw in (dict(G=0), dict(max_n=0), dict(max_m=0), dict(ld=(1, 2, 2)), dict(ld=(2, 1, 2)), dict(ld=(2, 2, 1)),
               dict(rot=1, ld=(3, 4, 2)), dict(rot=1, ld=(4, 2, 2))):
        assert call(**kw) == 1 and b"bad sizes" in h.da_last_error(), kw
    assert call(max_n=5, max_m=4) == 1 and b"more pieces than cells" in h.da_last_error()
    assert call(max_n=4096, max_m=4096) == 1 and b"too large" in h.da_last_error()      # 10 x 4096 words + 96 > 160 KB
    assert call(max_n=1, max_m=13600) == 1 and b"too large" in h.da_last_error()


def test_batch_scores_refuses_inconsistent_arguments():
    from diffassemble_amd import _lib
    from diffassemble_amd.score2d import batch_scores
    c = noisy_case("ragged_rot")
    pred, gt, dims, ptr, batch = c["pred"], c["gt"], c["dims"], c["ptr"], c["batch"]
    for args, kw in (((pred, gt, dims), {}),                                             # neither ptr nor batch
                     ((pred, gt, dims), dict(ptr=ptr, batch=batch)),                     # both
                     ((pred[:, :1], gt, dims), dict(ptr=ptr)),
                     ((pred[:, :3], gt, dims), dict(ptr=ptr, rotation=True)),
                     ((pred, gt[:-1], dims), dict(ptr=ptr)),
                     ((pred[0], gt[0], dims), dict(ptr=ptr)),
                     ((pred, gt, dims[:-1]), dict(ptr=ptr)),
                     ((pred, gt, dims.flatten()), dict(ptr=ptr)),
                     ((pred, gt, dims.float()), dict(ptr=ptr)),
                     ((pred, gt, dims * 0), dict(ptr=ptr)),
                     ((pred, gt, dims), dict(batch=batch[:-1])),
                     ((pred, gt, dims[:-1]), dict(batch=batch)),                         # batch names a puzzle dims does not have
                     ((pred, gt, dims), dict(ptr=ptr.flip(0))),
                     ((pred, gt, dims), dict(ptr=ptr - 1))):
        with pytest.raises(ValueError):
            batch_scores(*args, **kw)
    with pytest.raises(_lib.DaError):                                                    # neither a host nor a ROCm tensor
        batch_scores(pred.to("meta"), gt.to("meta"), dims, ptr=ptr)


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_route_reproduces_the_reference_arithmetic(name):
    from diffassemble_amd.score2d import batch_scores
    c = noisy_case(name)
    want_ok, want_correct, want_cp, want_cg = reference_scores(c)
    ok, correct, cp, cg, sizes = batch_scores(c["pred"], c["gt"], c["dims"], ptr=c["ptr"], rotation=c["rotation"], return_cells=True,
                                              return_sizes=True)
    assert ok.dtype == torch.bool and correct.dtype == torch.bool
    assert torch.equal(ok, want_ok.bool()) and torch.equal(correct, want_correct)
    assert torch.equal(cp, want_cp) and torch.equal(cg, want_cg)
    counts = (c["ptr"][1:] - c["ptr"][:-1]).long()
    assert torch.equal(sizes, torch.cat((counts[:, None], c["dims"]), 1))
    again = batch_scores(c["pred"], c["gt"], c["dims"].tolist(), batch=c["batch"], rotation=c["rotation"])
    assert len(again) == 2 and torch.equal(again[0], ok) and torch.equal(again[1], correct)
    if name.startswith("ragged"):
        assert 0 < int(ok.sum()) < ok.numel()                               # right and wrong pieces both occur


def test_2x3_pins_the_xy_cell_order():
    """Cell j of a rows x cols puzzle is (x_{j % cols}, y_{j // cols}): a piece at the right end of the top row is cell 2."""
    from diffassemble_amd.score2d import batch_scores
    gt = torch.tensor([[1.0, -1.0], [-1.0, 1.0], [0.0, 1.0]])
    ptr, dims = torch.tensor([0, 3], dtype=torch.int32), torch.tensor([[2, 3]])
    ok, correct, cp, cg = batch_scores(gt.flip(0), gt, dims, ptr=ptr, return_cells=True)
    assert cg.tolist() == [2, 3, 4] and cp.tolist() == [4, 3, 2]
    assert ok.tolist() == [False, True, False] and correct.tolist() == [False]
    assert batch_scores(gt, gt, dims, ptr=ptr)[1].tolist() == [True]


def test_more_pieces_than_cells_keeps_the_reference_row_count():
    """n > m stays on the loop: min(n, m) flags for that puzzle, as the reference's comparison of the two sorted lists gives."""
    from diffassemble_amd.score2d import batch_scores
    g = torch.Generator().manual_seed(0)
    pred, gt = torch.rand(9, 2, generator=g) * 2 - 1, torch.rand(9, 2, generator=g) * 2 - 1
    ok, correct, sizes = batch_scores(pred, gt, [[2, 2], [2, 2]], ptr=torch.tensor([0, 6, 9]), return_sizes=True)
    assert ok.numel() == 4 + 3 and correct.numel() == 2 and sizes.tolist() == [[4, 2, 2], [3, 2, 2]]


def test_product_file_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "diffassemble_amd", "score2d.py")).read()
    assert "import oracle" not in src and "from oracle" not in src


@pytest.mark.parametrize("name", sorted(NOISY))
def test_noisy_inputs_keep_every_greedy_choice_clear(name):
    c = noisy_case(name)
    b = c["ptr"].tolist()
    for g, (rows, cols) in enumerate(c["dims"].tolist()):
        grid = grid_of(rows, cols)
        for which in ("gt", "pred"):
            gap = smallest_greedy_gap(c[which][b[g]:b[g + 1], :2], grid)
            assert gap >= GAP, (name, g, which, gap)
    if c["rotation"]:
        cos = torch.cosine_similarity(c["pred"][:, 2:].double(), c["gt"][:, 2:].double())
        assert float((cos - COS45).abs().min()) >= 1e-3
        assert 0 < int((cos > COS45).sum()) < cos.numel()
