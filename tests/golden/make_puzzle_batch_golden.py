"""Build tests/golden/puzzle_batch_v1.npz: what the reference's own dataset classes (puzzle_diff/dataset/puzzle_dataset.py)
return for four small puzzles cut from noise pictures.

BUILD-CONTAINER ONLY (needs the reference checkout and PIL; never runs with the suite).  The reference file is loaded from
where it lies through ``ref_import.import_reference_dataset()``.  In the loaded module's namespace only what the stubs lack is
put in place: ``pyg_data.Data`` becomes a recording namespace, the ``ToTensor`` / ``Compose`` pair becomes
``uint8 HWC -> fp32 CHW / 255``, ``pyg.utils.dense_to_sparse`` becomes ``adj.nonzero().t()``, and the module's ``random`` is
wrapped so that the list ``random.shuffle`` leaves behind is recorded.  Then the reference's own ``get()`` runs, one puzzle at a
time, for

    plain   Puzzle_Dataset                          rot     Puzzle_Dataset_ROT
    roteq   Puzzle_Dataset_ROT(all_equivariant)     mp      Puzzle_Dataset_MP(missing_perc=30)
    rotmp   Puzzle_Dataset_ROT_MP(missing_perc=30)

on the puzzles (2, 3), (3, 2), (1, 4), (3, 3).  The pictures are already at their final size, so the reference's resize
returns a copy.  ``Puzzle_Dataset_Pad.get`` cannot run as shipped (its line 346 is broken): ``zero_margin`` is called directly
on the plain crops of puzzle 0 with padding 3 (``pad3``).

The pictures are noise from two byte values per picture (eight colours per pixel): every transposition of a tile is
distinguishable, and the file stays small (the crops are stored as uint8 after asserting that ``uint8 / 255`` reproduces the
reference's fp32 crops exactly; the full range of byte values is covered by the table test and the device tests).  The seeds
of the rotation modes are the first at which every turn 0 .. 3 occurs in the puzzle.  Stored per mode and puzzle: x, patches
(uint8), edge_index, ind_name, patches_dim and, where the reference returns them, indexes, rot, rot_index (with missing pieces:
full length and unpermuted, as the reference leaves them) and ``keep``, the head of the shuffled list.  The archive is written
with fixed time stamps: it regenerates byte for byte.

    python tests/golden/make_puzzle_batch_golden.py
"""
import io
import math
import os
import random as pyrandom
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FIXTURE = os.path.join(HERE, "puzzle_batch_v1.npz")
PUZZLES = ((2, 3), (3, 2), (1, 4), (3, 3))
MODES = ("plain", "rot", "roteq", "mp", "rotmp")
MISSING = 30
PAD = 3


def noise_picture(g, rows, cols):
    rng = np.random.default_rng(4100 + g)
    palette = rng.choice(256, 2, replace=False).astype(np.uint8)
    return palette[rng.integers(0, 2, (32 * rows, 32 * cols, 3))]


def write_archive(path, blob):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(blob):
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.asarray(blob[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, raw.getvalue(), compresslevel=9)


def main():
    from PIL import Image
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
    shuffled = []

    def recording_shuffle(seq):
        pyrandom.shuffle(seq)
        shuffled.append(list(seq))

    m.random = SimpleNamespace(shuffle=recording_shuffle)

    def dataset(mode, pictures, dims):
        kw = dict(dataset=pictures, dataset_get_fn=lambda v: v, patch_per_dim=[dims])
        if mode == "plain":
            return m.Puzzle_Dataset(**kw)
        if mode in ("rot", "roteq"):
            return m.Puzzle_Dataset_ROT(all_equivariant=mode == "roteq", **kw)
        if mode == "mp":
            return m.Puzzle_Dataset_MP(missing_perc=MISSING, **kw)
        return m.Puzzle_Dataset_ROT_MP(missing_perc=MISSING, **kw)

    pictures = [Image.fromarray(noise_picture(g, *d)) for g, d in enumerate(PUZZLES)]
    unit = torch.arange(256, dtype=torch.uint8).float() / 255
    blob = {"puzzles": np.array(PUZZLES, np.int64), "missing_perc": np.array(MISSING), "unit": unit.numpy()}
    for g, pic in enumerate(pictures):
        blob[f"image/{g}"] = np.array(pic)
    for mi, mode in enumerate(MODES):
        for g, dims in enumerate(PUZZLES):
            n = dims[0] * dims[1]
            seed = 1000 * mi + 100 * g
            while True:
                torch.manual_seed(seed)
                pyrandom.seed(seed)
                shuffled.clear()
                d = dataset(mode, pictures, dims).get(g)
                if not hasattr(d, "rot_index") or sorted(set(d.rot_index.tolist())) == [0, 1, 2, 3]:
                    break
                seed += 1
            key = f"{mode}/{g}/"
            blob[key + "seed"] = np.array(seed)
            bytes_ = (d.patches * 255).long()
            assert d.patches.dtype == torch.float32 and torch.equal(bytes_.to(torch.uint8).float() / 255, d.patches)
            assert torch.equal(unit[bytes_], d.patches)
            blob[key + "patches"] = bytes_.to(torch.uint8).numpy()
            assert d.x.dtype == torch.float32 and d.edge_index.dtype == torch.int64
            blob[key + "x"], blob[key + "edge_index"] = d.x.numpy(), d.edge_index.contiguous().numpy()
            blob[key + "ind_name"], blob[key + "patches_dim"] = d.ind_name.numpy(), d.patches_dim.numpy()
            for name in ("indexes", "rot", "rot_index"):
                if hasattr(d, name):
                    assert getattr(d, name).dtype == torch.int64
                    blob[key + name] = getattr(d, name).numpy()
            if mode in ("mp", "rotmp"):
                assert len(shuffled) == 1
                left = n - math.ceil(n * MISSING / 100)
                blob[key + "keep"] = np.array(shuffled[0][:left], np.int64)
                assert d.x.shape[0] == left
            else:
                assert not shuffled
    pad = m.Puzzle_Dataset_Pad.zero_margin(SimpleNamespace(padding=PAD), unit[torch.from_numpy(blob["plain/0/patches"]).long()].clone())
    blob["pad3/0/patches"] = (pad * 255).long().to(torch.uint8).numpy()
    assert torch.equal(unit[torch.from_numpy(blob["pad3/0/patches"]).long()], pad)
    write_archive(FIXTURE, blob)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
