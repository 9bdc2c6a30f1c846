"""Puzzle and piece accuracy of the continuous 2D ``validation_step`` / ``test_step`` (host glue; runs once per Batch AFTER the
sampling loop, not on the per-timestep path).

Counterpart of the scoring in puzzle_diff/model/spatial_diffusion.py:775-856, 915-955: per puzzle the reference assigns the
ground-truth positions and the predicted positions greedily to the puzzle's grid (``greedy_cost_assignment``, :179-216), sorts
both assignments by piece, and calls a piece right when both put it on the same cell (and, with ``rotation``, when
``cosine_similarity`` of the two (cos, sin) pairs exceeds cos(pi / 4)); a puzzle is right when all its pieces are.

``batch_scores`` scores every puzzle of a Batch at once.  On a ROCm device it is ONE library call (``da_score2d``,
diffassemble_amd/csrc/da_score2d.hip, DESIGN 3n: one workgroup per puzzle runs both assignments side by side in LDS and
compares them) between two host copies: the sizes before it (piece counts and ``dims``, whichever of them lives on the device)
and the flags after it.  On host tensors it is ``_loop_scores``, the per-puzzle loop ``GNN_Diffusion._eval_step`` used to hold,
which states the semantics; device Batches the kernel does not take (a puzzle with more pieces than cells, or too large for one
workgroup's LDS) go through the same loop, which then calls ``da_greedy_assign``."""
import math

import torch

USE_KERNEL = True          # False: device tensors take the loop too (tests and tests/tools/score2d_bench.py compare the two routes)
_LDS_BYTES = 160 * 1024
_GRIDS = {}


def _lds_bytes(n, m):
    """What da_score2d reserves for a puzzle of n pieces and m cells (s2_lds_floats, da_score2d.hip)."""
    return 4 * (2 * m + 2 * (3 * n + m) + 96)


def _grid(rows, cols, device):
    """The cell centres of a rows x cols puzzle, [rows * cols, 2], as validation_step builds them (torch's linspace bits)."""
    y = torch.linspace(-1, 1, rows, device=device)
    x = torch.linspace(-1, 1, cols, device=device)
    return torch.stack(torch.meshgrid(x, y, indexing="xy"), -1).reshape(-1, 2)


def _cached_grids(dims, device):
    """The grids of the Batch's puzzles, concatenated [sum(rows * cols), 2]; each grid is cached per (rows, cols, device)."""
    parts = []
    for rows, cols in dims:
        k = (rows, cols, str(device))
        if k not in _GRIDS:
            _GRIDS[k] = _grid(rows, cols, device).contiguous()
        parts.append(_GRIDS[k])
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _rows(x, cols):
    """Pose rows as the library reads them: fp32, unit inner stride -> (tensor, leading dimension >= cols)."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < cols):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else max(cols, x.shape[1]))


def _loop_scores(pred, gt, dims, batch, rotation):
    """The per-puzzle scoring loop of ``GNN_Diffusion._eval_step`` (spatial_diffusion.py:775-856, 915-955) on whatever device
    the poses live on.  ``dims``: host list of (rows, cols); ``batch``: the sorted puzzle index of every piece.  Returns four
    lists with one entry per puzzle: the piece flags (bool [min(n, m)]), the puzzle's verdict (bool), and the cells assigned
    to the pieces by the ground truth and by the prediction."""
    from .model.spatial_diffusion import greedy_cost_assignment
    device = pred.device
    G = len(dims)
    grids = []
    for i in range(G):
        y = torch.linspace(-1, 1, dims[i][0], device=device)
        x = torch.linspace(-1, 1, dims[i][1], device=device)
        grids.append(torch.stack(torch.meshgrid(x, y, indexing="xy"), -1).reshape(-1, 2))
    counts = torch.bincount(batch, minlength=G)
    ptr = torch.zeros(G + 1, dtype=torch.int32, device=device)
    ptr[1:] = torch.cumsum(counts, 0)
    batched = pred.is_cuda and all(g.shape[0] == int(c) for g, c in zip(grids, counts))
    if batched:                                        # both assignments of every puzzle: two launches
        from .engine import greedy_assign
        grid_all = torch.cat(grids)
        gt_all = greedy_assign(gt[:, :2], grid_all, ptr, ptr)
        pred_all = greedy_assign(pred[:, :2], grid_all, ptr, ptr)
    flags, verdicts, cells_gt, cells_pred = [], [], [], []
    for i in range(G):
        idx = torch.where(batch == i)[0]
        if batched:
            lo, hi = int(ptr[i]), int(ptr[i + 1])
            gt_ass, pred_ass = gt_all[lo:hi], pred_all[lo:hi]
        else:
            gt_ass = greedy_cost_assignment(gt[idx, :2], grids[i])
            pred_ass = greedy_cost_assignment(pred[idx, :2], grids[i])
        gt_ass = gt_ass[torch.sort(gt_ass[:, 0])[1]]
        pred_ass = pred_ass[torch.sort(pred_ass[:, 0])[1]]
        piece_accuracy = (gt_ass[:, 1] == pred_ass[:, 1]).to(device)
        correct = bool(piece_accuracy.all())
        if rotation:
            rot_correct = torch.cosine_similarity(pred[idx, 2:], gt[idx, 2:]) > math.cos(math.pi / 4)
            correct = correct and bool(rot_correct.all())
            piece_accuracy = rot_correct * piece_accuracy
        flags.append(piece_accuracy)
        verdicts.append(correct)
        cells_gt.append(gt_ass[:, 1])
        cells_pred.append(pred_ass[:, 1])
    return flags, verdicts, cells_gt, cells_pred


def _host_sizes(N, G, dims, batch, ptr, device):
    """Piece counts and dims as host lists, with at most ONE copy from the device (skipped for whichever is a host tensor)."""
    if ptr is not None:
        src = ptr.reshape(-1).long()
    elif batch.device.type == "cpu":
        src = torch.bincount(batch, minlength=G)
    else:
        src = torch.bincount(batch.to(device), minlength=G)
    d = dims.reshape(-1).long()
    if src.device.type != "cpu" and d.device.type != "cpu":
        host = torch.cat((src, d.to(src.device))).cpu()
        src, d = host[:src.numel()], host[src.numel():]
    src, d = src.cpu().tolist(), d.cpu().reshape(G, 2).tolist()
    if ptr is not None:
        if src[0] != 0 or src[-1] != N or any(b < a for a, b in zip(src, src[1:])):
            raise ValueError(f"batch_scores: ptr must rise from 0 to N = {N} (got {src[:4]} ... {src[-1]})")
        counts = [b - a for a, b in zip(src, src[1:])]
    else:
        if len(src) != G:
            raise ValueError(f"batch_scores: batch names puzzle {len(src) - 1} but dims has {G} rows")
        counts = src
    if any(r < 1 or c < 1 for r, c in d):
        raise ValueError("batch_scores: dims holds a non-positive size")
    return counts, d


def batch_scores(pred, gt, dims, batch=None, ptr=None, rotation=False, return_cells=False, return_sizes=False):
    """Piece and puzzle accuracy of every puzzle of a Batch: ``(piece_ok, correct)`` = bool [N] (the reference's
    ``piece_accuracy`` of the puzzles, concatenated) and bool [G], both on the host.

    ``pred`` / ``gt`` [N, >= 2]: x, y and, with ``rotation`` ([N, 4]), (cos, sin); ``dims`` int [G, 2]: the ``patches_dim`` of
    the Batch, (rows, cols) per puzzle.  The puzzles are consecutive rows: give ``ptr`` (int [G + 1]) or the sorted ``batch``
    vector [N].  ``return_cells``: also the cell (local index, int64) every piece is assigned to, by the prediction and by the
    ground truth.  ``return_sizes``: also a host int64 [G, 3] = (flags of the puzzle in ``piece_ok``, rows, cols).
    A puzzle with more pieces than cells has min(n, m) flags, as in the reference; everywhere else flags = pieces.
    On a ROCm device this is one call of ``da_score2d`` between two host copies; on host tensors the reference's loop."""
    if (ptr is None) == (batch is None):
        raise ValueError("batch_scores: give either ptr or a sorted batch vector")
    need = 4 if rotation else 2
    if pred.dim() != 2 or gt.dim() != 2 or pred.shape[0] != gt.shape[0] or pred.shape[0] < 1:
        raise ValueError(f"batch_scores: poses are [N, >= {need}] rows, N >= 1 (got {tuple(pred.shape)}, {tuple(gt.shape)})")
    if (rotation and (pred.shape[1] != 4 or gt.shape[1] != 4)) or pred.shape[1] < 2 or gt.shape[1] < 2:
        raise ValueError(f"batch_scores: rotation={bool(rotation)} needs {'[N, 4]' if rotation else '[N, >= 2]'} poses "
                         f"(got {tuple(pred.shape)}, {tuple(gt.shape)})")
    dims = torch.as_tensor(dims)
    if dims.dim() != 2 or dims.shape[1] != 2 or dims.shape[0] < 1 or dims.is_floating_point():
        raise ValueError(f"batch_scores: dims is an integer [G, 2] tensor (got {tuple(dims.shape)}, {dims.dtype})")
    N, G = pred.shape[0], dims.shape[0]
    if ptr is not None and ptr.numel() != G + 1:
        raise ValueError(f"batch_scores: ptr has G + 1 = {G + 1} entries (got {ptr.numel()})")
    if batch is not None and tuple(batch.shape) != (N,):
        raise ValueError(f"batch_scores: batch is [N] with N = {N} (got {tuple(batch.shape)})")
    dev = pred.device
    if dev.type not in ("cpu", "cuda"):
        from . import _lib
        raise _lib.DaError(f"batch_scores needs ROCm or host tensors (got {dev})")
    gt = gt.to(dev)
    counts, dims_h = _host_sizes(N, G, dims, batch, ptr, dev)
    cells = [r * c for r, c in dims_h]
    fused = (dev.type == "cuda" and USE_KERNEL and all(n <= m for n, m in zip(counts, cells))
             and _lds_bytes(max(counts), max(cells)) <= _LDS_BYTES)
    if not fused:
        if batch is None:
            batch = torch.repeat_interleave(torch.arange(G), torch.tensor(counts))
        flags, verdicts, cells_gt, cells_pred = _loop_scores(pred, gt, dims_h, batch.to(dev), rotation)
        piece_ok, correct = torch.cat(flags).bool().cpu(), torch.tensor(verdicts, dtype=torch.bool)
        cell_pred, cell_gt = torch.cat(cells_pred), torch.cat(cells_gt)
    else:
        from . import _lib
        pr, ld_pred = _rows(pred, need)
        tg, ld_gt = _rows(gt, need)
        grid = _cached_grids([tuple(d) for d in dims_h], dev)
        bounds = torch.zeros(2, G + 1, dtype=torch.int64)
        bounds[0, 1:] = torch.tensor(counts).cumsum(0)
        bounds[1, 1:] = torch.tensor(cells).cumsum(0)
        bounds = bounds.to(torch.int32).to(dev)
        out = torch.empty(16 * G + N, dtype=torch.uint8, device=dev)          # per_puzzle int32 [G, 4], then piece_ok [N]: one copy back
        cell_tab = torch.empty(2, N, dtype=torch.int32, device=dev) if return_cells else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().da_score2d(G, _lib.ptr(pr), ld_pred, _lib.ptr(tg), ld_gt, _lib.ptr(grid), 2, _lib.ptr(bounds[0]),
                                             _lib.ptr(bounds[1]), max(counts), max(cells), int(bool(rotation)),
                                             _lib.ptr(cell_tab[0]) if return_cells else None,
                                             _lib.ptr(cell_tab[1]) if return_cells else None,
                                             out.data_ptr() + 16 * G, out.data_ptr(), _lib.stream_ptr(dev)))
        host = out.cpu()
        per_puzzle = host[:16 * G].view(torch.int32).view(G, 4)
        if bool((per_puzzle[:, 0] < 0).any()):
            raise _lib.DaError("da_score2d refused a puzzle with more pieces than cells")
        piece_ok, correct = host[16 * G:].bool(), per_puzzle[:, 0].bool()
        if return_cells:
            cell_pred, cell_gt = cell_tab[0].long(), cell_tab[1].long()
    res = (piece_ok, correct)
    if return_cells:
        res += (cell_pred, cell_gt)
    if return_sizes:
        res += (torch.tensor([[min(n, m), r, c] for n, m, (r, c) in zip(counts, cells, dims_h)], dtype=torch.int64),)
    return res
