"""A 2D Batch from whole images: cut every picture into 32 x 32 pieces, turn them, drop some, and lay out every tensor the
2D modules read (host glue; runs once per Batch, before the encoder).

Counterpart of the reference's puzzle_diff/dataset/puzzle_dataset.py: ``divide_images_into_patches`` (:175-190) and the
``get()`` of ``Puzzle_Dataset`` (:257-300), ``Puzzle_Dataset_Pad`` (``zero_margin`` :326-332), ``Puzzle_Dataset_ROT_MP``
(:403-485), ``Puzzle_Dataset_MP`` (:507-544) and ``Puzzle_Dataset_ROT`` (:580-700), followed by PyG's collation of the samples
into one Batch.  The reference makes one ``PIL.Image.fromarray``, one ``.rotate`` and one ``np.array`` per piece on the host.
The rule, in this project's words:

* the picture of a ``(rows, cols)`` puzzle is uint8 RGB ``[32 * rows, 32 * cols, 3]``; cell ``(i, j)`` is piece ``i * cols + j``,
  its crop ``[3, 32, 32]`` fp32 = ``uint8 / 255``, its position ``(x_j, y_i)`` with ``x = torch.linspace(-1, 1, cols)`` and
  ``y = torch.linspace(-1, 1, rows)`` (torch's own values: in fp32 they are not ``-1 + i * step``);
* with ``rotation`` piece p is turned counter-clockwise by ``rot_index[p]`` quarter turns (``PIL.Image.rotate(r * 90)`` of a
  square tile = ``np.rot90(tile, r)``: exact transposes), ``rot = one_hot(r) @ [[1, 0], [0, 1], [-1, 0], [0, -1]]`` (int64) and
  ``x`` gets ``rot`` as its fp32 columns 2 .. 3; with ``all_equivariant`` the crops are ``[N, 4, 3, 32, 32]``, view k turned by
  ``(r + k) % 4``;
* with missing pieces only the cells of the puzzle's kept list remain, in the list's order (the reference keeps the head of a
  shuffled ``range(n)``, unsorted), ``n - ceil(n * missing_perc / 100)`` of them;
* ``padding`` zeroes that many outermost pixels on every side of every (turned) crop;
* ``edge_index`` is the complete graph with self loops of every puzzle's present pieces, source-major
  (``dense_to_sparse(torch.ones(n, n))``), shifted by the puzzle's first piece; ``batch`` / ``ptr`` as PyG collates them.

Differences from the reference, on purpose:

* with missing pieces the reference leaves ``rot``, ``rot_index`` and ``indexes`` at full length and unpermuted while ``x``
  and ``patches`` are permuted and shortened (:462-485).  Here all five follow the kept list: row p of each describes the
  same piece;
* ``rot`` (all ``(1, 0)``) and ``rot_index`` (all 0) exist without ``rotation`` too, and ``indexes`` exists in every mode;
* the random draws are made here on the host with torch under ``generator`` (per puzzle: the turns, then the kept cells), or
  handed in; the reference draws the kept cells with Python's ``random.shuffle``;
* the ``random=True`` shuffle and the Exphander graphs stay with the caller (``edges=None`` leaves ``edge_index`` unset); the
  PIL resize and the flip / crop augmentations are ``resize2d.make_batch_from_pictures``, which resizes on the device and then
  calls ``make_batch`` (the flip coin and the crop box are drawn by the caller).

``make_batch`` on a ROCm device is two library calls (``da_puzzle_batch`` and ``da_complete_edges``,
diffassemble_amd/csrc/da_puzzle_batch.hip) after ONE upload of the small tables and one of the pictures when they
lie on the host.  For host input without ``device`` it is ``_loop_batch``, the per-piece route in PIL and torch in the
reference's order of operations: a Batch of CPU tensors is a reasonable thing to ask for, and the rule that kernels have no
fallback concerns the model's arithmetic."""
import math

import numpy as np
import torch

PATCH = 32
TILE_BYTES = 3 * PATCH * PATCH                      # one cell of a picture
MAX_EDGE_BYTES = 1 << 28                            # cap of edges="complete": 16 bytes per edge
_ROTS = ((1, 0), (0, 1), (-1, 0), (0, -1))


class PuzzleBatch:
    """What ``make_batch`` returns: a plain attribute object with ``x`` fp32 [N, 2 or 4], ``patches`` fp32 [N, 3, 32, 32] or
    [N, 4, 3, 32, 32], ``indexes`` / ``rot_index`` / ``batch`` int64 [N], ``rot`` int64 [N, 2], ``edge_index`` int64 [2, E]
    (absent with ``edges=None``), ``ptr`` int64 [G + 1], ``patches_dim`` int64 [G, 2], ``ind_name`` int64 [G] and
    ``num_graphs``.  Further attributes (``expander_perm``, ``patch_feats``, ...) may be assigned freely."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def keys(self):
        return list(self.__dict__)

    def to(self, device):
        return PuzzleBatch(**{k: v.to(device) if torch.is_tensor(v) else v for k, v in self.__dict__.items()})

    def __repr__(self):
        body = ", ".join(f"{k}={list(v.shape)}" if torch.is_tensor(v) else f"{k}={v!r}" for k, v in self.__dict__.items())
        return f"PuzzleBatch({body})"


def _image(img, g, who="make_batch"):
    """One picture as a uint8 [H, W, 3] tensor (on whatever device it lies); ``who`` names the caller in the errors."""
    if not torch.is_tensor(img):
        if hasattr(img, "mode") and hasattr(img, "size") and not isinstance(img, np.ndarray):          # a PIL image
            if img.mode != "RGB":
                raise ValueError(f"{who}: image {g} is a PIL image of mode {img.mode!r}; convert it to 'RGB'")
        arr = np.array(img)                         # a copy: PIL hands out read-only memory
        if arr.dtype != np.uint8:
            raise ValueError(f"{who}: image {g} is uint8 [H, W, 3] (got dtype {arr.dtype})")
        img = torch.from_numpy(np.ascontiguousarray(arr))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"{who}: image {g} is uint8 [H, W, 3] (got {img.dtype} {tuple(img.shape)})")
    return img


def _dims(patch_per_dim, G):
    try:
        d = np.asarray(patch_per_dim, dtype=np.int64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"make_batch: patch_per_dim is (rows, cols) or one pair per puzzle (got {patch_per_dim!r})") from e
    if d.shape == (2,):
        d = np.tile(d, (G, 1))
    if d.shape != (G, 2) or (d < 1).any():
        raise ValueError(f"make_batch: patch_per_dim is (rows, cols) or one pair per puzzle, {G} here, all positive (got {patch_per_dim!r})")
    return [(int(r), int(c)) for r, c in d]


def _int_array(v, what):
    """A flat int64 numpy array of integers handed in as a tensor (any device), an array or a sequence."""
    if torch.is_tensor(v):
        if v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"make_batch: {what} holds integers (got {v.dtype})")
        return v.detach().cpu().reshape(-1).to(torch.int64).numpy()
    arr = np.asarray(v)
    if arr.size and arr.dtype.kind not in "iu":
        raise ValueError(f"make_batch: {what} holds integers (got {arr.dtype})")
    return arr.reshape(-1).astype(np.int64)


def _draws(dims, rotation, missing_perc, rot_index, keep, generator):
    """Per puzzle the quarter turns of all its cells and the kept cells in output order (int64 arrays); what is not handed in is
    drawn here."""
    G = len(dims)
    total = sum(r * c for r, c in dims)
    if rot_index is not None:
        if not rotation:
            raise ValueError("make_batch: rot_index needs rotation=True")
        flat = _int_array(rot_index, "rot_index")
        if len(flat) != total:
            raise ValueError(f"make_batch: rot_index has one entry per cell, {total} here (got {len(flat)})")
        if ((flat < 0) | (flat > 3)).any():
            raise ValueError("make_batch: rot_index entries are quarter turns 0 .. 3")
    if keep is not None and (isinstance(keep, (str, bytes)) or not hasattr(keep, "__len__") or len(keep) != G):
        raise ValueError(f"make_batch: keep is one list of kept cells per puzzle, {G} here")
    if not 0 <= missing_perc <= 100:
        raise ValueError(f"make_batch: missing_perc is a percentage 0 .. 100 (got {missing_perc})")
    turns, keeps, lo = [], [], 0
    for g, (rows, cols) in enumerate(dims):
        n = rows * cols
        left = n - math.ceil(n * missing_perc / 100)
        if left < 1:
            raise ValueError(f"make_batch: missing_perc = {missing_perc} leaves no piece of puzzle {g} ({rows} x {cols})")
        if not rotation:
            turns.append(np.zeros(n, np.int64))
        elif rot_index is not None:
            turns.append(flat[lo:lo + n])
        else:
            turns.append(torch.randint(0, 4, (n,), generator=generator).numpy())
        if keep is not None:
            kg = _int_array(keep[g], f"keep[{g}]")
            if ((kg < 0) | (kg >= n)).any():
                raise ValueError(f"make_batch: keep[{g}] names cells 0 .. {n - 1} of a {rows} x {cols} puzzle")
            if len(np.unique(kg)) != len(kg):
                raise ValueError(f"make_batch: keep[{g}] repeats a cell")
            if not len(kg):
                raise ValueError(f"make_batch: keep[{g}] leaves no piece of puzzle {g}")
            if missing_perc and len(kg) != left:
                raise ValueError(f"make_batch: keep[{g}] has {len(kg)} cells, missing_perc = {missing_perc} leaves {left} of {n}")
        elif left < n:
            kg = torch.randperm(n, generator=generator)[:left].numpy()
        else:
            kg = np.arange(n)
        keeps.append(kg)
        lo += n
    return turns, keeps


def _zero_margin(t, padding):
    if padding > 0:
        t[..., :padding, :] = 0
        t[..., -padding:, :] = 0
        t[..., :, :padding] = 0
        t[..., :, -padding:] = 0
    return t


def _complete_edges_host(counts):
    out, lo = [], 0
    for n in counts:
        out.append(torch.ones(n, n).nonzero().t() + lo)
        lo += n
    return torch.cat(out, 1).contiguous()


def _loop_batch(images, dims, turns, keeps, rotation=False, all_equivariant=False, padding=0):
    """The per-piece host route: ``images`` uint8 [H, W, 3] host tensors, ``dims`` (rows, cols) per puzzle, ``turns`` / ``keeps``
    of ``_draws``.  Every step is the reference's, in its order: ToTensor, unfold, linspace / meshgrid, per piece the uint8
    round trip, ``Image.fromarray``, ``.rotate(r * 90)``, ``np.array``, ``/ 255``, then the kept list.  Returns the per-piece
    tensors (x, patches, indexes, rot, rot_index, batch) of the whole Batch."""
    Image = None
    if rotation:
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("make_batch on host tensors turns the pieces through PIL, which is not installed; "
                              "pass device= to build the Batch on the ROCm device") from e
    rots = torch.tensor(_ROTS)
    xs, ps, idx, rt, ri, bt = [], [], [], [], [], []
    for g, (img, (rows, cols)) in enumerate(zip(images, dims)):
        chw = img.permute(2, 0, 1).contiguous().to(torch.float32).div(255)                          # ToTensor
        patches = chw.permute(1, 2, 0).unfold(0, PATCH, PATCH).unfold(1, PATCH, PATCH)
        y, x = torch.linspace(-1, 1, rows), torch.linspace(-1, 1, cols)
        xy = torch.stack(torch.meshgrid(x, y, indexing="xy"), -1).reshape(-1, 2)
        patches = patches.reshape(rows * cols, 3, PATCH, PATCH)
        r = torch.as_tensor(np.asarray(turns[g]), dtype=torch.long)
        rot = torch.nn.functional.one_hot(r, 4) @ rots
        if rotation:
            tiles = (patches * 255).long().numpy().transpose(0, 2, 3, 1).astype(np.uint8)
            turned = [Image.fromarray(tiles[p]).rotate(int(q) * 90) for p, q in enumerate(turns[g])]

            def tensor_of(pic):
                return torch.tensor(np.array(pic)).permute(2, 0, 1).float() / 255

            if all_equivariant:
                patches = torch.stack([torch.stack([tensor_of(pic.rotate(k * 90)) for k in range(4)]) for pic in turned])
            else:
                patches = torch.stack([tensor_of(pic) for pic in turned])
            xy = torch.cat([xy, rot], 1)
        kept = torch.as_tensor(np.asarray(keeps[g]), dtype=torch.long)
        xs.append(xy[kept])
        ps.append(_zero_margin(patches[kept].clone(), padding))
        idx.append(torch.arange(rows * cols)[kept])
        rt.append(rot[kept])
        ri.append(r[kept])
        bt.append(torch.full((len(keeps[g]),), g, dtype=torch.long))
    return torch.cat(xs), torch.cat(ps), torch.cat(idx), torch.cat(rt), torch.cat(ri), torch.cat(bt)


def _tables(dims, turns, keeps, names, with_edges):
    """Everything small the device route needs as ONE host buffer, and the byte range and dtype of every part.
    int64: edge table [G, 3], ptr [G + 1], patches_dim [G, 2], ind_name [G]; int32: pieces [N, 4], puzzles [G, 8]; fp32: the
    linspace tables, the 256 values of uint8 / 255."""
    G = len(dims)
    counts = [len(k) for k in keeps]
    N = sum(counts)
    sides = sorted({s for d in dims for s in d})
    lin_at, lin, lo = {}, [], 0
    for s in sides:
        lin_at[s] = lo
        lin.append(torch.linspace(-1, 1, s))
        lo += s
    lin = torch.cat(lin).numpy()
    unit = (torch.arange(256, dtype=torch.uint8).float() / 255).numpy()
    edge = np.zeros((G, 3), np.int64)
    ptr = np.zeros(G + 1, np.int64)
    puzzles = np.zeros((G, 8), np.int32)
    pieces = np.zeros((N, 4), np.int32)
    off = e0 = 0
    for g, ((rows, cols), n) in enumerate(zip(dims, counts)):
        edge[g] = (e0, ptr[g], n)
        ptr[g + 1] = ptr[g] + n
        puzzles[g, 0:2] = np.array([off], dtype=np.int64).view(np.int32)
        puzzles[g, 2:] = (rows, cols, ptr[g], n, lin_at[cols], lin_at[rows])
        pieces[ptr[g]:ptr[g + 1], 0] = g
        pieces[ptr[g]:ptr[g + 1], 1] = keeps[g]
        pieces[ptr[g]:ptr[g + 1], 2] = np.asarray(turns[g])[np.asarray(keeps[g], dtype=np.int64)]
        off += rows * cols * TILE_BYTES
        e0 += n * n
    parts = [("edge", edge), ("ptr", ptr), ("patches_dim", np.asarray(dims, np.int64).reshape(G, 2)), ("ind_name", np.asarray(names, np.int64)),
             ("pieces", pieces), ("puzzles", puzzles), ("lin", lin), ("unit", unit)]
    where, size = {}, 0
    for name, arr in parts:
        size = (size + 15) & ~15                                  # the kernel reads the piece table with 16-byte loads
        where[name] = (size, size + arr.nbytes, arr.dtype, arr.shape)
        size += arr.nbytes
    buf = np.zeros(size, np.uint8)
    for name, arr in parts:
        a, b = where[name][:2]
        buf[a:b] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    return buf, where, N, e0 if with_edges else 0, len(lin)


_TORCH_OF = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


def make_batch(images, patch_per_dim, *, rotation=False, all_equivariant=False, missing_perc=0, padding=0, rot_index=None, keep=None,
               generator=None, edges="complete", ind_name=None, device=None):
    """The Batch of G puzzles cut from G pictures (see the module docstring for the rule and the differences from the reference).

    ``images``: a list of G uint8 ``[32 * rows_g, 32 * cols_g, 3]`` arrays, tensors or PIL RGB images, or one ``[G, H, W, 3]``
    tensor, already resized (``make_batch_from_pictures`` resizes first).  ``patch_per_dim``: one ``(rows, cols)``
    for all puzzles or one per puzzle.  The reference's dataset classes are the arguments: ``Puzzle_Dataset`` the defaults,
    ``Puzzle_Dataset_ROT`` ``rotation=True`` (and ``all_equivariant``), ``Puzzle_Dataset_MP`` ``missing_perc``,
    ``Puzzle_Dataset_ROT_MP`` both, ``Puzzle_Dataset_Pad`` ``padding`` (0 .. 16).
    ``rot_index``: the quarter turns 0 .. 3 of every cell of every puzzle, ``[sum rows * cols]``; ``keep``: per puzzle the kept
    cells in output order (unsorted is fine), ``n - ceil(n * missing_perc / 100)`` of them, or of any length from 1 to n with
    ``missing_perc`` left at 0.  What is not given is drawn on the host (``torch.randint`` / ``torch.randperm`` under
    ``generator``, per puzzle the turns first), never on the device.
    ``edges``: ``"complete"`` or None (no ``edge_index``: attach your own graph).  ``ind_name``: G integers (default 0 .. G - 1).
    ``device``: where the Batch is built; default: where the pictures lie.  Anything wrong raises ``ValueError``."""
    if torch.is_tensor(images):
        if images.dim() != 4:
            raise ValueError(f"make_batch: images is a list of [H, W, 3] pictures or one [G, H, W, 3] tensor (got {tuple(images.shape)})")
        images = list(images.unbind(0))
    images = [_image(img, g) for g, img in enumerate(images)]
    G = len(images)
    if G < 1:
        raise ValueError("make_batch: no image")
    dims = _dims(patch_per_dim, G)
    for g, (img, (rows, cols)) in enumerate(zip(images, dims)):
        if tuple(img.shape[:2]) != (PATCH * rows, PATCH * cols):
            raise ValueError(f"make_batch: image {g} is {img.shape[0]} x {img.shape[1]}, a {rows} x {cols} puzzle of {PATCH}-pixel pieces "
                             f"needs {PATCH * rows} x {PATCH * cols}: resize it first")
    if all_equivariant and not rotation:
        raise ValueError("make_batch: all_equivariant needs rotation=True")
    if isinstance(padding, bool) or int(padding) != padding or not 0 <= padding <= PATCH // 2:
        raise ValueError(f"make_batch: padding is an integer 0 .. {PATCH // 2} (got {padding!r})")
    padding = int(padding)
    if edges not in ("complete", None):
        raise ValueError(f"make_batch: edges is 'complete' or None (got {edges!r})")
    names = list(range(G)) if ind_name is None else _int_array(ind_name, "ind_name").tolist()
    if len(names) != G:
        raise ValueError(f"make_batch: ind_name has one integer per puzzle, {G} here (got {len(names)})")
    turns, keeps = _draws(dims, bool(rotation), missing_perc, rot_index, keep, generator)
    counts = [len(k) for k in keeps]
    n_edges = sum(n * n for n in counts)
    if edges == "complete" and 16 * n_edges > MAX_EDGE_BYTES:
        raise ValueError(f"make_batch: the complete graphs have {n_edges} edges = {16 * n_edges} bytes of edge_index, above {MAX_EDGE_BYTES}: "
                         "pass edges=None and attach a sparser graph (or the dense plan) yourself")
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((img.device for img in images if img.device.type != "cpu"), torch.device("cpu"))
    if dev.type not in ("cpu", "cuda"):
        from . import _lib
        raise _lib.DaError(f"make_batch needs a ROCm device or the host (got {dev})")
    views, x_cols = (4 if all_equivariant else 1), (4 if rotation else 2)
    if dev.type == "cpu":
        x, patches, indexes, rot, rot_idx, bvec = _loop_batch([img.cpu() for img in images], dims, turns, keeps, bool(rotation),
                                                              bool(all_equivariant), padding)
        out = PuzzleBatch(x=x, patches=patches, indexes=indexes, rot=rot, rot_index=rot_idx)
        if edges == "complete":
            out.edge_index = _complete_edges_host(counts)
        ptr = [0]
        for n in counts:
            ptr.append(ptr[-1] + n)
        out.batch, out.ptr = bvec, torch.tensor(ptr, dtype=torch.long)
        out.patches_dim, out.ind_name = torch.tensor(dims, dtype=torch.long).reshape(G, 2), torch.tensor(names, dtype=torch.long)
        out.num_graphs = G
        return out
    from . import _lib
    host, where, N, E, n_lin = _tables(dims, turns, keeps, names, edges == "complete")
    if all(img.device.type == "cpu" for img in images):
        flat = torch.cat([img.reshape(-1) for img in images]).to(dev)                                  # one copy of the pictures
    else:
        flat = torch.cat([img.to(dev).reshape(-1) for img in images]) if G > 1 else images[0].to(dev).contiguous().reshape(-1)
    small = torch.from_numpy(host).to(dev)                                                              # one copy of the tables

    def part(name):
        a, b, dtype, shape = where[name]
        return small[a:b].view(_TORCH_OF[dtype]).view(shape)

    patches = torch.empty((N, 4, 3, PATCH, PATCH) if views == 4 else (N, 3, PATCH, PATCH), dtype=torch.float32, device=dev)
    x = torch.empty((N, x_cols), dtype=torch.float32, device=dev)
    rot = torch.empty((N, 2), dtype=torch.long, device=dev)
    rot_idx, indexes, bvec = (torch.empty(N, dtype=torch.long, device=dev) for _ in range(3))
    out = PuzzleBatch(x=x, patches=patches, indexes=indexes, rot=rot, rot_index=rot_idx)
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        _lib.check(_lib.lib().da_puzzle_batch(G, N, _lib.ptr(flat), flat.numel(), _lib.ptr(part("puzzles")), _lib.ptr(part("pieces")),
                                              _lib.ptr(part("lin")), n_lin, _lib.ptr(part("unit")), padding, views, x_cols, _lib.ptr(patches),
                                              _lib.ptr(x), _lib.ptr(rot), _lib.ptr(rot_idx), _lib.ptr(indexes), _lib.ptr(bvec), st))
        if edges == "complete":
            out.edge_index = torch.empty((2, E), dtype=torch.long, device=dev)
            _lib.check(_lib.lib().da_complete_edges(G, _lib.ptr(part("edge")), E, _lib.ptr(out.edge_index), st))
    out.batch, out.ptr, out.patches_dim, out.ind_name = bvec, part("ptr"), part("patches_dim"), part("ind_name")
    out.num_graphs = G
    return out
