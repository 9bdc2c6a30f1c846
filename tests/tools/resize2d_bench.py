"""Timing of the device resize (diffassemble_amd/resize2d.py, csrc/da_resize2d.hip): 64 noise pictures of 218 x 178 (height x
width, the CelebA size) resized to 384 x 384 (a 12 x 12 puzzle) and to 960 x 960 (30 x 30), bicubic and Lanczos.

Arms, each after 5 warm-ups, median of the repetitions:
  resize_images(device)  the whole call on ONE stacked device tensor, host clock between two device synchronisations: the
                         descriptors (the tables are cached after the first call), their one upload, ONE ``da_resize2d`` launch
  resize_images(host)    the same on host pictures: plus the one packed upload of the pictures
  da_resize2d            the launch alone (fused route), everything prepared, device events around it
  two_pass               the same through the two-pass route (two launches and the workspace)
  copy                   ``Tensor.copy_`` of as many bytes as the launch reads and writes together, device to device: the
                         yardstick of a kernel that has to read every source byte and write every output byte once
  PIL                    ``Image.resize`` in a loop over ``--host-pictures`` pictures on this machine's CPU (one core), scaled to
                         the Batch; absent where PIL is not installed
  make_batch_from_pictures / make_batch   the resize plus the Batch builder end to end (rotation on, ``edges=None``), next to
                         the builder alone on pictures that are already resized
The device result must equal the host route ``_loop_resize`` on the first picture (and PIL where present) first.  GB/s = (source
bytes + output bytes) / time.  One JSON line per (size, filter).

    python tests/tools/resize2d_bench.py [--reps 30] [--sizes 384 960] [--host-pictures 4]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffassemble_amd import _lib, make_batch, make_batch_from_pictures, resize_images  # noqa: E402
from diffassemble_amd import resize2d as R  # noqa: E402
from puzzle_batch_bench import WARMUP, event_timed, host_timed  # noqa: E402

G, SRC_H, SRC_W = 64, 218, 178


def launches(d_imgs, size, resample, dev, reps):
    """da_resize2d through the C ABI with everything prepared: the fused route, the two-pass route, and the copy yardstick."""
    shapes, sizes = [(SRC_H, SRC_W)] * G, [(size, size)] * G
    boxes = [(0.0, 0.0, float(SRC_W), float(SRC_H))] * G
    pics, tables, out_bytes, tiles, hblocks, vblocks, ws_bytes, window = R._descriptors(shapes, sizes, resample, boxes, [False] * G)
    assert window <= R.WINDOW_ROWS
    small = torch.from_numpy(np.concatenate([pics.reshape(-1), tables])).to(dev)
    d_pics, d_tables = small[:pics.size], small[pics.size:]
    flat, out = d_imgs.reshape(-1), torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    h = _lib.lib()

    def run(route):
        _lib.check(h.da_resize2d(G, _lib.ptr(flat), flat.numel(), _lib.ptr(d_pics), _lib.ptr(d_tables), d_tables.numel(), _lib.ptr(out),
                                 out.numel(), _lib.ptr(work), ws_bytes, route, tiles, hblocks, vblocks, st))

    fused = event_timed(lambda: run(0), reps)
    two = event_timed(lambda: run(1), reps)
    n = flat.numel() + out_bytes
    a, b = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    return fused, two, event_timed(lambda: a.copy_(b), reps), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[384, 960])
    ap.add_argument("--filters", nargs="+", default=["bicubic", "lanczos"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-pictures", type=int, default=4)
    a = ap.parse_args()
    assert a.reps >= 20, "median of at least 20 repetitions"
    assert torch.cuda.is_available(), "resize2d_bench needs the GPU"
    dev = torch.device("cuda:0")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    imgs = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (G, SRC_H, SRC_W, 3), dtype=np.uint8))
    d_imgs = imgs.to(dev)
    hp = min(a.host_pictures, G)
    for size in a.sizes:
        side = size // 32
        rot_index = torch.randint(0, 4, (G * side * side,), generator=torch.Generator().manual_seed(0))
        kw = dict(rotation=True, rot_index=rot_index, edges=None)
        for resample in a.filters:
            got = resize_images(d_imgs, (size, size), resample=resample)
            assert R.last_route() == "fused"
            want = R._loop_resize(imgs[0].numpy(), (size, size), resample)
            assert torch.equal(got[0].cpu(), torch.from_numpy(want)), (size, resample)
            assert torch.equal(resize_images(d_imgs, (size, size), resample=resample, route="two_pass"), got)
            res = {"pictures": G, "source": [SRC_H, SRC_W], "size": size, "resample": resample, "warmup": WARMUP, "reps": a.reps}
            if Image is not None:
                code = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[resample]
                pil = [Image.fromarray(imgs[g].numpy()) for g in range(hp)]
                assert np.array_equal(np.array(pil[0].resize((size, size), code)), want)
                res["PIL"] = host_timed(lambda: [p.resize((size, size), code) for p in pil], 5, warmup=1, sync=False)
                res["PIL"]["batch_ms"] = round(res["PIL"]["median_ms"] * G / hp, 1)
                res["PIL"]["pictures"] = hp
            fused, two, copy, nbytes = launches(d_imgs, size, resample, dev, a.reps)
            res.update({"bytes": nbytes, "da_resize2d": fused, "two_pass": two, "copy": copy,
                        "resize_images(device)": host_timed(lambda: resize_images(d_imgs, (size, size), resample=resample), a.reps),
                        "resize_images(host)": host_timed(lambda: resize_images(imgs, (size, size), resample=resample, device=dev), a.reps),
                        "make_batch_from_pictures": host_timed(lambda: make_batch_from_pictures(d_imgs, (side, side), resample=resample, **kw),
                                                               a.reps),
                        "make_batch": host_timed(lambda: make_batch(got, (side, side), **kw), a.reps)})
            for arm in ("da_resize2d", "two_pass", "copy", "resize_images(device)", "resize_images(host)"):
                res[arm]["GB_per_s"] = round(nbytes / (res[arm]["median_ms"] * 1e-3) / 1e9, 1)
            res["copy_over_kernel"] = round(copy["median_ms"] / fused["median_ms"], 3)                   # achieved fraction of a copy
            if Image is not None:
                res["PIL_over_resize_images"] = round(res["PIL"]["batch_ms"] / res["resize_images(device)"]["median_ms"], 1)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
