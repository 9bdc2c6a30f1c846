"""Build tests/golden/resize2d_v1.npz: what ``PIL.Image.resize`` returns for small pictures, and what the reference's own
dataset classes (puzzle_diff/dataset/puzzle_dataset.py) return for pictures that are NOT at their final size.

BUILD-CONTAINER ONLY (needs PIL and, for part (b), the reference checkout; never runs with the suite).

(a) Resize cases (``CASES``).  The source of case k is ``source(kind, seed, height, width)``: ``np.random.default_rng(seed)
    .integers(0, 256, (height, width, 3), dtype=np.uint8)`` for ``"noise"``, a 0 / 255 checkerboard of single pixels for
    ``"checker"`` (it overshoots both ways under bicubic and Lanczos, so both clamps run).  Every case runs with the three
    filters: ``Image.fromarray(source).resize((out_w, out_h), filter, box)``.  Stored: the table of the cases (``cases`` int64
    [K, 6] = kind, seed, height, width, out_h, out_w; ``boxes`` float64 [K, 4], NaN for no box), ``out/<k>/<filter>`` uint8,
    ``pil_version``.  No source picture is stored.  The cases: up- and downscaling, a 1 x 1 source, sizes that are not a multiple
    of the kernel's 32-column tile, strong downscaling (7 x 300 and 40 x 1000 -> 32 x 32), one pass skipped (height or width
    unchanged), an integer box, a fractional box, a size-preserving box (the ``hard`` augmentation's second stage).
(b) Reference chain (``CHAIN``).  ``Puzzle_Dataset.get()`` (PIL's default, bicubic, :266) and ``Puzzle_Dataset_ROT.get()``
    (Lanczos, :590) loaded through ``ref_import.import_reference_dataset()`` with the stand-ins of
    ``make_puzzle_batch_golden.py``, on three noise pictures of other sizes than their puzzles'.  Stored per mode (``plain`` /
    ``rot``) and puzzle: x, patches (uint8, after asserting that ``uint8 / 255`` reproduces the fp32 crops), indexes and, for
    ``rot``, rot and rot_index; ``chain`` int64 [3, 5] = seed, height, width, rows, cols.

The archive is written with fixed time stamps: it regenerates byte for byte.

    python tests/golden/make_resize2d_golden.py
"""
import os
import random as pyrandom
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_puzzle_batch_golden import write_archive  # noqa: E402

FIXTURE = os.path.join(HERE, "resize2d_v1.npz")
FILTERS = ("bilinear", "bicubic", "lanczos")
NOISE, CHECKER = 0, 1
# kind, seed, source height, width, output height, width, box (left, upper, right, lower) or None
CASES = (
    (NOISE, 7001, 1, 1, 32, 32, None),
    (NOISE, 7002, 2, 3, 33, 65, None),
    (NOISE, 7003, 33, 17, 64, 32, None),
    (NOISE, 7004, 97, 131, 40, 56, None),
    (NOISE, 7005, 218, 178, 96, 96, None),
    (NOISE, 7006, 7, 300, 32, 32, None),
    (NOISE, 7007, 40, 1000, 32, 32, None),
    (NOISE, 7008, 97, 131, 97, 40, None),                  # height unchanged: the vertical pass is skipped
    (NOISE, 7009, 97, 131, 40, 131, None),                 # width unchanged: the horizontal pass is skipped
    (NOISE, 7010, 97, 131, 64, 48, (3, 5, 120, 90)),
    (NOISE, 7011, 97, 131, 64, 32, (0.3, 0.7, 130.4, 95.75)),
    (NOISE, 7012, 64, 64, 64, 64, (8, 10, 60, 55)),         # size-preserving box
    (CHECKER, 0, 33, 17, 65, 33, None),
    (CHECKER, 0, 97, 131, 96, 96, None),
)
# seed, source height, width, rows, cols
CHAIN = ((7101, 218, 178, 2, 3), (7102, 50, 70, 3, 2), (7103, 100, 37, 1, 2))


def source(kind, seed, height, width):
    if kind == CHECKER:
        yy, xx = np.mgrid[0:height, 0:width]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def main():
    import PIL
    from PIL import Image
    codes = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    blob = {"pil_version": np.array(PIL.__version__),
            "cases": np.array([c[:6] for c in CASES], np.int64),
            "boxes": np.array([c[6] if c[6] is not None else (np.nan,) * 4 for c in CASES], np.float64),
            "chain": np.array(CHAIN, np.int64)}
    for k, (kind, seed, h, w, oh, ow, box) in enumerate(CASES):
        pic = Image.fromarray(source(kind, seed, h, w))
        for name in FILTERS:
            out = np.array(pic.resize((ow, oh), codes[name], box))
            assert out.shape == (oh, ow, 3) and out.dtype == np.uint8
            blob[f"out/{k}/{name}"] = out

    from ref_import import import_reference_dataset
    m = import_reference_dataset()
    m.pyg_data.Data = lambda **kw: SimpleNamespace(**kw)
    m.transforms.ToTensor = lambda: (lambda pic: torch.from_numpy(np.array(pic)).permute(2, 0, 1).contiguous().float() / 255)

    def compose(fns):
        def run(v):
            for fn in fns:
                v = fn(v)
            return v
        return run

    m.transforms.Compose = compose
    m.pyg.utils = SimpleNamespace(dense_to_sparse=lambda adj: (adj.nonzero().t(), None))
    unit = torch.arange(256, dtype=torch.uint8).float() / 255
    pictures = [Image.fromarray(source(NOISE, seed, h, w)) for seed, h, w, _, _ in CHAIN]
    for mi, mode in enumerate(("plain", "rot")):
        for g, (_, h, w, rows, cols) in enumerate(CHAIN):
            assert (h, w) != (32 * rows, 32 * cols)
            kw = dict(dataset=pictures, dataset_get_fn=lambda v: v, patch_per_dim=[(rows, cols)])
            torch.manual_seed(500 * mi + 10 * g)
            pyrandom.seed(500 * mi + 10 * g)
            d = (m.Puzzle_Dataset(**kw) if mode == "plain" else m.Puzzle_Dataset_ROT(**kw)).get(g)
            bytes_ = (d.patches * 255).long()
            assert d.patches.dtype == torch.float32 and torch.equal(unit[bytes_], d.patches)
            key = f"chain/{mode}/{g}/"
            blob[key + "patches"] = bytes_.to(torch.uint8).numpy()
            blob[key + "x"], blob[key + "indexes"] = d.x.numpy(), d.indexes.reshape(-1).numpy()
            if mode == "rot":
                blob[key + "rot"], blob[key + "rot_index"] = d.rot.numpy(), d.rot_index.numpy()
    write_archive(FIXTURE, blob)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
