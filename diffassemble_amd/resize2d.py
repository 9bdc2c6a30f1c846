"""Resize a 2D Batch's pictures on the device, bit-equal to ``PIL.Image.resize`` (host glue; runs once per Batch, before
``make_batch``).

Counterpart of the ``img.resize((32 * cols, 32 * rows))`` at the head of every ``get()`` of the reference's
puzzle_diff/dataset/puzzle_dataset.py (:266, :344, :413, :517 with PIL's default, bicubic; :590, ``Puzzle_Dataset_ROT``, with
Lanczos) and of its augmentations (:155-172): ``weak`` is ``RandomHorizontalFlip``, ``hard`` adds
``RandomCropAndResizedToOriginal``, a bicubic resize of a crop box back to the picture's own size.  The rule is
``PIL.Image.resize(size, resample, box)`` for mode RGB, 8 bits per channel, filters bicubic, bilinear and Lanczos, in this
project's words:

* per axis, in Python floats (C doubles): ``scale = (in1 - in0) / out`` (the difference alone in C floats), ``filterscale =
  max(scale, 1)``, ``support = filter_support * filterscale`` (bilinear 1, bicubic 2, Lanczos 3); for output index ``xx``: ``center = in0 + (xx + 0.5) *
  scale``, ``xmin = max(int(center - support + 0.5), 0)``, ``xmax = min(int(center + support + 0.5), in_size) - xmin`` (``int``
  truncates), weights ``filter((x + xmin - center + 0.5) * (1 / filterscale))`` for ``x < xmax``, summed in index order and each
  divided by the sum when it is not zero; the integer coefficient is ``int(0.5 + w * 2**22)``, ``int(-0.5 + w * 2**22)`` for a
  negative ``w``.  The box is held in C floats, as PIL holds it;
* the filters: bilinear ``1 - |x|`` below 1; bicubic with ``a = -0.5``: ``((a + 2) |x| - (a + 3)) x^2 + 1`` below 1,
  ``(((|x| - 5) |x| + 8) |x| - 4) a`` below 2; Lanczos ``sinc(x) sinc(x / 3)`` for ``-3 <= x < 3`` with ``math.sin``;
* two passes, horizontal first.  A pass runs only if its axis changes size or its box does not span the axis; with neither the
  result is a copy.  Every output byte is ``clamp((2**21 + sum(byte * coefficient)) >> 22, 0, 255)`` in int32, the shift
  arithmetic.  The horizontal result is stored as uint8 before the vertical pass reads it, and only the source rows the
  vertical pass reads are made;
* ``flips[g]`` mirrors the stage's OUTPUT left to right: ``RandomHorizontalFlip`` after the resize, the reference's order.  (The
  truncations in ``xmin`` are not mirror-symmetric: flipping the source is not the same bytes.)

What is not built: modes other than 8-bit RGB, the nearest, box and Hamming filters, ``reducing_gap``, decoding.  The flip coin
and the crop box are drawn by the caller, like every random draw of this project.

``resize_images`` on a ROCm device is ONE library call (``da_resize2d``, diffassemble_amd/csrc/da_resize2d.hip)
after one packed upload of the pictures when they lie on the host and one of the descriptors and tables.  The tables (int32
coefficients and bounds) are made here, one per distinct ``(in_size, in0, in1, out_size, filter)``, and cached.  For host input
without ``device`` it is ``_loop_resize``, the per-picture numpy route, which is also what the kernel is tested against."""
import functools
import math

import numpy as np
import torch

from .puzzle_batch import PATCH, _dims, _image, make_batch

PRECISION_BITS = 22
FILTERS = ("bilinear", "bicubic", "lanczos")
_PIL_CODES = {2: "bilinear", 3: "bicubic", 1: "lanczos"}         # PIL.Image.Resampling
ROUTES = (None, "fused", "two_pass")
TILE_ROWS, TILE_COLS, BLOCK = 64, 32, 256                        # da_resize2d.hip: RS_TH, RS_TW, RS_THREADS
WINDOW_ROWS = 256                                                # RS_WINDOW = da_resize2d_window_rows()
PIC_INTS = 24                                                    # ints of one picture's descriptor (include/diffassemble_hip.h)


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTER = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


@functools.lru_cache(maxsize=512)
def _axis_tables(in_size, in0, in1, out_size, resample):
    """(bounds int32 [out, 2] = (first source index, count), coefficients int32 [out, ksize]) of one axis, read-only."""
    fn, fsupport = _FILTER[resample]
    scale = float(np.float32(in1) - np.float32(in0)) / out_size          # PIL subtracts the box ends as C floats
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ss = 1.0 / filterscale
    rows, bounds = [], np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = max(min(int(center + support + 0.5), in_size) - xmin, 0)
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w])
        bounds[xx] = (xmin, xmax)
    coeffs = np.zeros((out_size, max(1, max(len(r) for r in rows))), np.int32)
    for xx, r in enumerate(rows):
        coeffs[xx, :len(r)] = r
    if int(np.abs(coeffs).max()) >= 1 << (PRECISION_BITS + 1):                      # the kernel multiplies in 24 bits
        raise ValueError(f"resize_images: a weight of {in_size} -> {out_size} ({resample}, box {in0} .. {in1}) reaches 2 or more")
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


@functools.lru_cache(maxsize=512)
def _identity_tables(size):
    bounds = np.stack([np.arange(size), np.ones(size, np.int64)], 1).astype(np.int32)
    coeffs = np.full((size, 1), 1 << PRECISION_BITS, np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def _resample(resample):
    name = _PIL_CODES.get(resample, resample) if isinstance(resample, int) and not isinstance(resample, bool) else resample
    if isinstance(name, str) and name.lower() in FILTERS:
        return name.lower()
    raise ValueError(f"resize_images: resample is 'bicubic', 'bilinear' or 'lanczos' (got {resample!r})")


def resize_tables(in_size, out_size, resample="bicubic", in0=0.0, in1=None):
    """The bound table int32 ``[out_size, 2]`` (first source index, count) and the coefficient table int32 ``[out_size, ksize]``
    of one axis: ``in_size`` source samples, the box ``[in0, in1)`` (default: the whole axis) resized to ``out_size``.  Cached:
    an identical request returns the same (read-only) arrays."""
    in1 = float(in_size) if in1 is None else in1
    if int(in_size) < 1 or int(out_size) < 1 or not 0 <= in0 < in1 <= in_size:
        raise ValueError(f"resize_tables: sizes are positive and 0 <= in0 < in1 <= in_size (got {in_size}, {out_size}, {in0}, {in1})")
    return _axis_tables(int(in_size), float(np.float32(in0)), float(np.float32(in1)), int(out_size), _resample(resample))


def _plan(shape, size, resample, box):
    """The two axes' tables of one picture, PIL's pass skipping applied: (h bounds, h coeffs, v bounds, v coeffs, first source
    row the vertical pass reads, rows it reads)."""
    (H, W), (oh, ow) = shape, size
    x0, y0, x1, y1 = box
    if ow != W or x0 != 0 or x1 != W:
        hb, hc = _axis_tables(W, x0, x1, ow, resample)
    else:
        hb, hc = _identity_tables(W)
    if oh != H or y0 != 0 or y1 != H:
        vb, vc = _axis_tables(H, y0, y1, oh, resample)
    else:
        vb, vc = _identity_tables(H)
    row0 = int(vb[0, 0])
    return hb, hc, vb, vc, row0, int(vb[-1, 0] + vb[-1, 1]) - row0


def _pass(src, bounds, coeffs, out_len):
    """One pass along axis 1 of ``src`` uint8 [R, in, 3] -> uint8 [R, out_len, 3], in int32 like PIL."""
    out = np.empty((src.shape[0], out_len, 3), np.uint8)
    s32 = src.astype(np.int32)
    for xx in range(out_len):
        lo, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full((src.shape[0], 3), 1 << (PRECISION_BITS - 1), np.int32)
        for k in range(n):
            acc += s32[:, lo + k, :] * coeffs[xx, k]
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def _loop_resize(img, size, resample="bicubic", box=None, flip=False):
    """The per-picture host route and the contract of the kernel: ``img`` uint8 numpy [H, W, 3] -> uint8 [size[0], size[1], 3],
    what ``PIL.Image.fromarray(img).resize((size[1], size[0]), resample, box)`` returns, mirrored left to right with ``flip``.
    ``box``: (left, upper, right, lower) already as C floats, or None."""
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    oh, ow = size
    box = (0.0, 0.0, float(W), float(H)) if box is None else box
    hb, hc, vb, vc, row0, rows = _plan((H, W), (oh, ow), resample, box)
    mid = _pass(img[row0:row0 + rows], hb, hc, ow)                                   # uint8 before the vertical pass reads it
    vb = np.stack([vb[:, 0] - row0, vb[:, 1]], 1)
    out = _pass(mid.transpose(1, 0, 2), vb, vc, oh).transpose(1, 0, 2)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def _sizes(sizes, G):
    try:
        d = np.asarray(sizes, dtype=np.int64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"resize_images: sizes is (height, width) or one pair per picture (got {sizes!r})") from e
    if d.shape == (2,):
        d = np.tile(d, (G, 1))
    if d.shape != (G, 2) or (d < 1).any() or (d > 1 << 24).any():
        raise ValueError(f"resize_images: sizes is (height, width) or one pair per picture, {G} here, all positive (got {sizes!r})")
    return [(int(h), int(w)) for h, w in d]


def _boxes(boxes, images):
    G = len(images)
    if boxes is None:
        boxes = [None] * G
    if isinstance(boxes, (str, bytes)) or not hasattr(boxes, "__len__") or len(boxes) != G:
        raise ValueError(f"resize_images: boxes is one (left, upper, right, lower) or None per picture, {G} here")
    out = []
    for g, (b, img) in enumerate(zip(boxes, images)):
        H, W = int(img.shape[0]), int(img.shape[1])
        if b is None:
            out.append((0.0, 0.0, float(W), float(H)))
            continue
        try:
            x0, y0, x1, y1 = (float(np.float32(v)) for v in b)                       # PIL keeps the box in C floats
        except (TypeError, ValueError) as e:
            raise ValueError(f"resize_images: boxes[{g}] is (left, upper, right, lower) (got {b!r})") from e
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise ValueError(f"resize_images: boxes[{g}] = {tuple(b)} is empty or lies outside the {H} x {W} picture")
        out.append((x0, y0, x1, y1))
    return out


def _flips(flips, G):
    if flips is None:
        return [False] * G
    if torch.is_tensor(flips):
        flips = flips.detach().cpu().reshape(-1).tolist()
    if isinstance(flips, (str, bytes)) or not hasattr(flips, "__len__") or len(flips) != G:
        raise ValueError(f"resize_images: flips is one boolean per picture, {G} here")
    return [bool(f) for f in flips]


def _pictures(images, who):
    if torch.is_tensor(images):
        if images.dim() != 4:
            raise ValueError(f"{who}: images is a list of [H, W, 3] pictures or one [G, H, W, 3] tensor (got {tuple(images.shape)})")
        images = list(images.unbind(0))
    images = [_image(img, g, who) for g, img in enumerate(images)]
    if len(images) < 1:
        raise ValueError(f"{who}: no image")
    for g, img in enumerate(images):
        if img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError(f"{who}: image {g} is empty ({img.shape[0]} x {img.shape[1]})")
    return images


def _descriptors(shapes, sizes, resample, boxes, flips):
    """``_descriptors_of`` on hashable copies of the arguments: a Batch shaped like an earlier one costs a dictionary lookup."""
    return _descriptors_of(tuple(shapes), tuple(sizes), resample, tuple(boxes), tuple(bool(f) for f in flips))


@functools.lru_cache(maxsize=64)
def _descriptors_of(shapes, sizes, resample, boxes, flips):
    """The descriptors int32 [G, 24] and the packed tables int32 of one call (include/diffassemble_hip.h), and what the launch
    needs: (pictures, tables, output bytes, tiles, h blocks, v blocks, workspace bytes, largest window of a tile)."""
    G = len(shapes)
    pics = np.zeros((G, PIC_INTS), np.int32)
    at, parts, n_ints = {}, [], 0

    def place(arr):
        nonlocal n_ints
        if id(arr) not in at:
            at[id(arr)] = n_ints
            parts.append(arr.reshape(-1))
            n_ints += arr.size
        return at[id(arr)]

    def words(v):
        return np.array([v], np.int64).view(np.int32)

    src = dst = ws = tiles = hblocks = vblocks = window = 0
    for g, ((H, W), (oh, ow)) in enumerate(zip(shapes, sizes)):
        hb, hc, vb, vc, row0, rows = _plan((H, W), (oh, ow), resample, boxes[g])
        tiles_x = -(-ow // TILE_COLS)
        pics[g, 0:2], pics[g, 4:6], pics[g, 21:23] = words(src), words(dst), words(ws)
        pics[g, 2:4], pics[g, 6:8], pics[g, 8] = (H, W), (oh, ow), int(flips[g])
        pics[g, 9:12] = (place(hb), place(hc), hc.shape[1])
        pics[g, 12:15] = (place(vb), place(vc), vc.shape[1])
        pics[g, 15:21] = (tiles, tiles_x, hblocks, vblocks, row0, rows)
        for y0 in range(0, oh, TILE_ROWS):
            y1 = min(y0 + TILE_ROWS, oh) - 1
            window = max(window, int(vb[y1, 0] + vb[y1, 1] - vb[y0, 0]))
        tiles += tiles_x * -(-oh // TILE_ROWS)
        hblocks += -(-rows * ow // BLOCK)
        vblocks += -(-oh * ow // BLOCK)
        src += 3 * H * W
        dst += (3 * oh * ow + 15) & ~15                              # every output picture starts 16-byte aligned
        ws += (3 * rows * ow + 15) & ~15
        if max(tiles, hblocks, vblocks) >= 1 << 31:
            raise ValueError("resize_images: more than 2^31 - 1 tiles in one call; split the Batch")
    tables = np.concatenate(parts)
    pics.setflags(write=False)
    tables.setflags(write=False)
    return pics, tables, dst, tiles, hblocks, vblocks, ws, window


_last_route = None                                                   # the route of the latest device call ("fused" / "two_pass")


def _launch(flat, pics, tables, out, tiles, hblocks, vblocks, ws_bytes, route, dev):
    """``da_resize2d`` on the packed pictures ``flat`` (device uint8) into ``out`` (device uint8, flat)."""
    from . import _lib
    h = _lib.lib()
    small = torch.from_numpy(np.concatenate([pics.reshape(-1), tables])).to(dev)     # one copy of descriptors and tables
    d_pics, d_tables = small[:pics.size], small[pics.size:]
    two = route == "two_pass"
    work = None
    if two:
        need = h.da_resize2d_workspace_bytes(len(pics), pics.ctypes.data)
        assert need == ws_bytes, (need, ws_bytes)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(h.da_resize2d(len(pics), _lib.ptr(flat), flat.numel(), _lib.ptr(d_pics), _lib.ptr(d_tables), d_tables.numel(), _lib.ptr(out),
                                 out.numel(), _lib.ptr(work), ws_bytes if two else 0, 1 if two else 0, tiles, hblocks, vblocks,
                                 _lib.stream_ptr(dev)))
    return out


def _pack(images, stacked, dev):
    """The pictures back to back as one flat device tensor: host pictures go up in ONE copy, a stacked device tensor is read in
    place (the kernel reads bytes: no picture needs an aligned start)."""
    if stacked is not None and stacked.device == dev and stacked.is_contiguous():
        return stacked.reshape(-1)
    if all(img.device.type == "cpu" for img in images):
        return torch.cat([img.reshape(-1) for img in images]).to(dev)
    return torch.cat([img.to(dev).reshape(-1) for img in images])


def resize_images(images, sizes, *, resample="bicubic", boxes=None, flips=None, route=None, device=None):
    """``PIL.Image.resize`` of G pictures, byte for byte (see the module docstring for the rule).

    ``images``: a list of G uint8 ``[H, W, 3]`` arrays, tensors (host or ROCm) or PIL RGB images, or one ``[G, H, W, 3]`` tensor.
    ``sizes``: one ``(height, width)`` for all pictures or one per picture.  ``resample``: ``"bicubic"`` (PIL's default),
    ``"bilinear"`` or ``"lanczos"`` (or PIL's ``Resampling`` codes of the three).  ``boxes``: per picture None or PIL's ``box``
    ``(left, upper, right, lower)``, integers or fractions: the region of the source that is resized.  ``flips``: per picture,
    mirror the OUTPUT left to right.  ``route``: None picks the fused kernel unless a tile of some picture needs more than 256
    source rows (strong downscaling), then the two-pass route; ``"fused"`` / ``"two_pass"`` force one (the same bytes).
    ``device``: where the work is done; default: where the pictures lie.  Returns uint8 pictures on that device: one
    ``[G, H, W, 3]`` tensor when all sizes agree, otherwise a list.  Anything wrong raises ``ValueError``."""
    global _last_route
    stacked = images if torch.is_tensor(images) and images.dim() == 4 and images.dtype == torch.uint8 else None
    images = _pictures(images, "resize_images")
    G = len(images)
    sizes = _sizes(sizes, G)
    resample = _resample(resample)
    boxes = _boxes(boxes, images)
    flips = _flips(flips, G)
    if route not in ROUTES:
        raise ValueError(f"resize_images: route is None, 'fused' or 'two_pass' (got {route!r})")
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((img.device for img in images if img.device.type != "cpu"), torch.device("cpu"))
    if dev.type not in ("cpu", "cuda"):
        from . import _lib
        raise _lib.DaError(f"resize_images needs a ROCm device or the host (got {dev})")
    same = all(s == sizes[0] for s in sizes)
    if dev.type == "cpu":
        outs = [torch.from_numpy(_loop_resize(img.cpu().numpy(), sizes[g], resample, boxes[g], flips[g])) for g, img in enumerate(images)]
        return torch.stack(outs) if same else outs
    shapes = [(int(img.shape[0]), int(img.shape[1])) for img in images]
    pics, tables, out_bytes, tiles, hblocks, vblocks, ws_bytes, window = _descriptors(shapes, sizes, resample, boxes, flips)
    if route == "fused" and window > WINDOW_ROWS:
        raise ValueError(f"resize_images: route='fused' holds at most {WINDOW_ROWS} source rows per tile, this call needs {window}; "
                         "use route='two_pass' (or None)")
    route = route or ("fused" if window <= WINDOW_ROWS else "two_pass")
    flat = _pack(images, stacked, dev)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    _launch(flat, pics, tables, out, tiles, hblocks, vblocks, ws_bytes, route, dev)
    _last_route = route
    if same:
        oh, ow = sizes[0]
        if (3 * oh * ow) % 16 == 0 or G == 1:
            return out[:G * 3 * oh * ow].view(G, oh, ow, 3)
    outs, lo = [], 0
    for oh, ow in sizes:
        outs.append(out[lo:lo + 3 * oh * ow].view(oh, ow, 3))
        lo += (3 * oh * ow + 15) & ~15
    return torch.stack(outs) if same else outs


def last_route():
    """The route the latest device call of ``resize_images`` took: ``"fused"`` or ``"two_pass"`` (None before the first)."""
    return _last_route


def make_batch_from_pictures(pictures, patch_per_dim, *, resample="bicubic", flips=None, crop_boxes=None, **make_batch_kwargs):
    """``make_batch`` of pictures of any size: the reference's ``get()`` from its ``img.resize`` on.

    Every picture is resized to ``(32 * rows, 32 * cols)`` with ``resample`` (``"bicubic"``: ``Puzzle_Dataset``, ``_Pad``, ``_MP``,
    ``_ROT_MP``; ``"lanczos"``: ``Puzzle_Dataset_ROT``) and mirrored where ``flips`` says so: the ``weak`` augmentation.  With
    ``crop_boxes`` (per picture None or ``(left, upper, right, lower)`` in the RESIZED picture: ``(j, i, j + w, i + h)`` of
    ``RandomResizedCrop.get_params``) a second, bicubic stage resizes that box back to the same size: the ``hard`` augmentation.
    The box is PIL's ``box``: where the filter's support reaches beyond it, pixels outside the box are read (torchvision's
    ``resized_crop`` crops a PIL image first; resize cropped views with ``resize_images`` for that).
    Then ``make_batch(..., **make_batch_kwargs)`` as it stands.  The coin and the box are the caller's draws."""
    images = _pictures(pictures, "make_batch_from_pictures")
    dims = _dims(patch_per_dim, len(images))
    sizes = [(PATCH * r, PATCH * c) for r, c in dims]
    device = make_batch_kwargs.get("device")
    out = resize_images(pictures if torch.is_tensor(pictures) else images, sizes, resample=resample, flips=flips, device=device)
    if crop_boxes is not None:
        out = resize_images(out, sizes, resample="bicubic", boxes=crop_boxes, device=device)
    return make_batch(out if torch.is_tensor(out) else list(out), patch_per_dim, **make_batch_kwargs)
