"""Host-side checks of the device resize (diffassemble_amd/resize2d.py ``resize_images`` / ``make_batch_from_pictures``, C entry
points ``da_resize2d`` and ``da_resize2d_workspace_bytes``).  No GPU.

tests/golden/resize2d_v1.npz holds what ``PIL.Image.resize`` returned for 14 small cases with three filters and what the
reference's own dataset classes returned for pictures that were not at their final size (made by
tests/golden/make_resize2d_golden.py; the sources are regenerated from their seeds).  The host route ``_loop_resize`` must equal
it byte for byte, and PIL itself over a sweep where PIL is installed; tests/test_gpu_resize2d.py then holds the kernel to the
fixture and to ``_loop_resize``.  Every comparison is exact equality of bytes: there is no tolerance.  The helpers are shared
with the GPU file."""
import functools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "resize2d_v1.npz")
FILTERS = ("bilinear", "bicubic", "lanczos")
CHAIN_MODES = {"plain": ("bicubic", {}), "rot": ("lanczos", dict(rotation=True))}


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        blob = {k: z[k] for k in z.files}
    for v in blob.values():
        v.setflags(write=False)
    return blob


def source(kind, seed, height, width):
    """The generator's ``source``: noise from a seed, or a 0 / 255 checkerboard."""
    if kind == 1:
        yy, xx = np.mgrid[0:height, 0:width]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """[(source uint8 [H, W, 3], (out_h, out_w), box or None)] of the fixture, in its order."""
    out = []
    for row, box in zip(fixture()["cases"], fixture()["boxes"]):
        kind, seed, h, w, oh, ow = (int(v) for v in row)
        src = source(kind, seed, h, w)
        src.setflags(write=False)
        out.append((src, (oh, ow), None if np.isnan(box[0]) else tuple(float(v) for v in box)))
    return out


def want(k, resample):
    return fixture()[f"out/{k}/{resample}"]


def chain_pictures():
    return [source(0, int(seed), int(h), int(w)) for seed, h, w, _, _ in fixture()["chain"]]


def chain_dims():
    return [(int(r), int(c)) for _, _, _, r, c in fixture()["chain"]]


def chain_ref(mode, name):
    """Attribute ``name`` of the reference's samples of a mode, concatenated in puzzle order (crops as fp32)."""
    parts = [torch.from_numpy(fixture()[f"chain/{mode}/{g}/{name}"].copy()) for g in range(len(chain_dims()))]
    v = torch.cat(parts)
    return (torch.arange(256, dtype=torch.uint8).float() / 255)[v.long()] if name == "patches" else v


def c_box(box, img):
    from diffassemble_amd import resize2d as R
    return R._boxes([box], [img])[0]


def loop(img, size, resample="bicubic", box=None, flip=False):
    from diffassemble_amd import resize2d as R
    return R._loop_resize(img, size, resample, c_box(box, img), flip)


RAGGED = dict(shapes=[(1, 1), (37, 53), (64, 80), (90, 31), (45, 45)], sizes=[(32, 32), (70, 41), (64, 96), (33, 65), (45, 45)],
              boxes=[None, (2, 3, 50, 30), None, (0.5, 1.25, 30.5, 88.0), (5, 6, 40, 41)], flips=[True, True, False, False, True])


def ragged_pictures():
    rng = np.random.default_rng(99)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in RAGGED["shapes"]]


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_small_and_covers_the_paths():
    assert os.path.getsize(FIXTURE) < 500 * 1000
    table = fixture()["cases"]
    assert len(table) == 14 and {int(k) for k in table[:, 0]} == {0, 1}
    assert any(h == oh for _, _, h, w, oh, ow in table) and any(w == ow for _, _, h, w, oh, ow in table)      # a skipped pass each
    assert sum(not np.isnan(b[0]) for b in fixture()["boxes"]) == 3
    for k in range(len(table)):
        for f in FILTERS:
            assert want(k, f).shape == (int(table[k, 4]), int(table[k, 5]), 3) and want(k, f).dtype == np.uint8
    for f in ("bicubic", "lanczos"):                                                                        # both clamps run
        assert want(12, f).min() == 0 and want(12, f).max() == 255
    assert str(fixture()["pil_version"])


@pytest.mark.parametrize("resample", FILTERS)
def test_host_route_equals_every_case_of_the_fixture(resample):
    for k, (src, size, box) in enumerate(cases()):
        got = loop(src, size, resample, box)
        assert got.dtype == np.uint8 and np.array_equal(got, want(k, resample)), (k, resample, int((got != want(k, resample)).sum()))


def test_flip_mirrors_the_output():
    src, size, box = cases()[10]
    assert np.array_equal(loop(src, size, "bicubic", box, flip=True), want(10, "bicubic")[:, ::-1])


# ------------------------------------------------------------------------------------------------ PIL itself
SOURCES = [(1, 1), (3, 2), (17, 33), (131, 97), (218, 178), (7, 300), (40, 1000)]        # (height, width): 1x1 ... 1000x40 as width x height
OUTPUTS = [(32, 32), (32, 64), (65, 33), (96, 96)]


@pytest.mark.parametrize("resample", FILTERS)
def test_host_route_equals_pil_over_a_sweep(resample):
    Image = pytest.importorskip("PIL.Image")
    code = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[resample]
    n = 0
    for h, w in SOURCES:
        src = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        pic = Image.fromarray(src)
        todo = [(size, None) for size in OUTPUTS] + [((h, 40), None), ((40, w), None)]                      # one pass skipped
        if h >= 3 and w >= 3:
            todo += [((32, 32), (1, 1, w - 1, h - 1)), ((65, 33), (0.3, 0.7, w - 0.6, h - 1.25)), ((h, w), (1, 0, w - 1, h - 1)),
                     ((h, w), (0, 0, w, h))]                                                                # the last is PIL's copy
        for (oh, ow), box in todo:
            ref = np.array(pic.resize((ow, oh), code, box))
            got = loop(src, (oh, ow), resample, box)
            assert np.array_equal(got, ref), (h, w, oh, ow, box, int((got != ref).sum()))
            n += 1
    assert n == 7 * 6 + 5 * 4


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("resample", FILTERS)
def test_tables_sum_to_one_and_stay_inside_the_source(resample):
    from diffassemble_amd.resize2d import resize_tables
    for in_size, out_size, in0, in1 in ((1, 32, 0, None), (178, 384, 0, None), (218, 32, 0, None), (1000, 32, 0, None), (97, 97, 3.5, 90.25),
                                        (131, 64, 0.3, 130.4)):
        bounds, coeffs = resize_tables(in_size, out_size, resample, in0, in1)
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32 and bounds.shape == (out_size, 2) and coeffs.shape[0] == out_size
        first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (first >= 0).all() and (count >= 1).all() and (first + count <= in_size).all() and count.max() == coeffs.shape[1]
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()                          # what the kernel's window relies on
        for xx in range(out_size):
            assert abs(int(coeffs[xx, :count[xx]].astype(np.int64).sum()) - (1 << 22)) <= count[xx], (in_size, out_size, xx)
            assert not coeffs[xx, count[xx]:].any()


def test_an_identical_request_hits_the_cache():
    from diffassemble_amd import resize2d as R
    a = R.resize_tables(55, 77, "lanczos", 1.5, 50)
    hits = R._axis_tables.cache_info().hits
    b = R.resize_tables(55, 77, "lanczos", 1.5, 50)
    assert R._axis_tables.cache_info().hits == hits + 1 and a[0] is b[0] and a[1] is b[1]
    assert not a[0].flags.writeable and not a[1].flags.writeable


def test_descriptors_tile_the_outputs_and_pick_the_route():
    from diffassemble_amd import resize2d as R
    pics = ragged_pictures()
    boxes = R._boxes(RAGGED["boxes"], pics)
    d, tables, out_bytes, tiles, hblocks, vblocks, ws, window = R._descriptors(RAGGED["shapes"], RAGGED["sizes"], "bicubic", boxes,
                                                                                RAGGED["flips"])
    assert d.shape == (5, 24) and d.dtype == np.int32 and tables.dtype == np.int32 and window <= R.WINDOW_ROWS
    assert d[:, 15].tolist() == [0, 1, 5, 8, 11] and tiles == 13                                             # 1, 2 x 2, 1 x 3, 1 x 3 ... tiles
    assert (d[:, 4] % 16 == 0).all() and out_bytes >= sum(3 * h * w for h, w in RAGGED["sizes"])
    assert d[:, 8].tolist() == [1, 1, 0, 0, 1]
    assert (d[:, 9:11].max() < len(tables)) and (d[:, 12:14].max() < len(tables))
    big = R._descriptors([(600, 600)], [(32, 32)], "bicubic", [(0.0, 0.0, 600.0, 600.0)], [False])
    assert big[-1] > R.WINDOW_ROWS                                                                           # route=None goes two-pass
    thin = R._descriptors([(40, 1000)], [(32, 32)], "bicubic", [(0.0, 0.0, 1000.0, 40.0)], [False])
    assert thin[-1] <= R.WINDOW_ROWS                                                                         # 40 source rows: the fused route


# ------------------------------------------------------------------------------------------------ arguments and results
def test_host_call_returns_a_tensor_or_a_list():
    from diffassemble_amd import resize_images
    src = [c[0] for c in cases()[3:5]]
    one = resize_images(src, (40, 56))
    assert torch.is_tensor(one) and one.dtype == torch.uint8 and tuple(one.shape) == (2, 40, 56, 3) and one.device.type == "cpu"
    assert np.array_equal(one[0].numpy(), want(3, "bicubic"))
    many = resize_images([torch.from_numpy(src[0].copy()), src[1]], [(40, 56), (96, 96)], resample="lanczos")
    assert isinstance(many, list) and np.array_equal(many[0].numpy(), want(3, "lanczos")) and np.array_equal(many[1].numpy(), want(4, "lanczos"))
    stacked = resize_images(torch.from_numpy(np.stack([src[0], src[0]])), (40, 56), flips=[False, True])
    assert torch.equal(stacked[1], stacked[0].flip(1))
    same = resize_images([src[0]], src[0].shape[:2])
    assert np.array_equal(same[0].numpy(), src[0])


def test_pil_pictures_are_accepted():
    Image = pytest.importorskip("PIL.Image")
    from diffassemble_amd import resize_images
    src = cases()[3][0]
    assert np.array_equal(resize_images([Image.fromarray(src)], (40, 56), resample=Image.BICUBIC)[0].numpy(), want(3, "bicubic"))
    with pytest.raises(ValueError, match="resize_images: image 0 is a PIL image of mode 'L'; convert it to 'RGB'"):
        resize_images([Image.fromarray(src[:, :, 0])], (8, 8))


def test_arguments_are_validated():
    from diffassemble_amd import resize_images
    img = np.zeros((10, 12, 3), np.uint8)
    with pytest.raises(ValueError, match=r"resize_images: image 0 is uint8 \[H, W, 3\] \(got dtype float32\)"):
        resize_images([img.astype(np.float32)], (8, 8))
    with pytest.raises(ValueError, match=r"resize_images: image 1 is uint8 \[H, W, 3\]"):
        resize_images([img, torch.zeros(10, 12, 4, dtype=torch.uint8)], (8, 8))
    with pytest.raises(ValueError, match=r"one \[G, H, W, 3\] tensor"):
        resize_images(torch.zeros(10, 12, 3, dtype=torch.uint8), (8, 8))
    with pytest.raises(ValueError, match="no image"):
        resize_images([], (8, 8))
    with pytest.raises(ValueError, match=r"sizes is \(height, width\) or one pair per picture, 2 here"):
        resize_images([img, img], [(8, 8)] * 3)
    with pytest.raises(ValueError, match="all positive"):
        resize_images([img], (0, 8))
    for box in ((0, 0, 13, 10), (-1, 0, 5, 5), (4, 0, 4, 5), (0, 8, 5, 3)):
        with pytest.raises(ValueError, match=r"boxes\[0\] = .* is empty or lies outside the 10 x 12 picture"):
            resize_images([img], (8, 8), boxes=[box])
    with pytest.raises(ValueError, match="boxes is one"):
        resize_images([img], (8, 8), boxes=[None, None])
    with pytest.raises(ValueError, match="flips is one boolean per picture, 1 here"):
        resize_images([img], (8, 8), flips=[True, False])
    with pytest.raises(ValueError, match="resample is 'bicubic', 'bilinear' or 'lanczos'"):
        resize_images([img], (8, 8), resample="nearest")
    with pytest.raises(ValueError, match="route is None, 'fused' or 'two_pass'"):
        resize_images([img], (8, 8), route="auto")


def test_the_feature_is_exported_and_device_input_without_a_device_is_refused():
    """Fails on the parent commit: there is no ``resize_images``."""
    import diffassemble_amd
    from diffassemble_amd import _lib
    from diffassemble_amd import resize2d as R
    assert diffassemble_amd.resize_images is R.resize_images and diffassemble_amd.make_batch_from_pictures is R.make_batch_from_pictures
    assert {"resize_images", "make_batch_from_pictures"} <= set(diffassemble_amd.__all__)
    with pytest.raises(_lib.DaError, match="resize_images needs a ROCm device or the host"):
        R.resize_images(torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="meta"), (4, 4))
    with pytest.raises(_lib.DaError, match="resize_images needs a ROCm device or the host"):
        R.resize_images([np.zeros((8, 8, 3), np.uint8)], (4, 4), device="meta")
    src = open(os.path.join(ROOT, "diffassemble_amd", "resize2d.py")).read()
    assert not re.search(r"^(import PIL|from PIL|import oracle|from oracle)", src, re.M)                     # needs neither to import


def test_make_batch_from_pictures_on_the_host_equals_the_reference_chain():
    """The whole host chain against the reference's ``get()`` on pictures that are not at their final size."""
    pytest.importorskip("PIL.Image")                                                                          # _loop_batch turns pieces through PIL
    from diffassemble_amd import make_batch_from_pictures
    for mode, (resample, kw) in CHAIN_MODES.items():
        turns = chain_ref(mode, "rot_index") if kw else None
        got = make_batch_from_pictures(chain_pictures(), chain_dims(), resample=resample, rot_index=turns, **kw)
        for name in ("x", "patches", "indexes") + (("rot", "rot_index") if kw else ()):
            assert torch.equal(getattr(got, name), chain_ref(mode, name)), (mode, name)


def test_make_batch_itself_still_refuses_wrong_sized_pictures():
    from diffassemble_amd import make_batch
    with pytest.raises(ValueError, match="resize it first"):
        make_batch(chain_pictures()[:1], chain_dims()[:1])


# ------------------------------------------------------------------------------------------------ ABI
def test_header_library_and_binding_carry_the_entry_points():
    import ctypes as C
    from diffassemble_amd import _lib
    from diffassemble_amd import resize2d as R
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())
    assert ("int da_resize2d(int n_pictures, const uint8_t *src, long long src_bytes, const int32_t *pictures, const int32_t *tables, "
            "long long n_table, uint8_t *dst, long long dst_bytes, uint8_t *workspace, size_t workspace_bytes, int route, long long n_tiles, "
            "long long n_hblocks, long long n_vblocks, void *stream);") in text
    assert "size_t da_resize2d_workspace_bytes(int n_pictures, const int32_t *pictures_host);" in text
    h = _lib.lib()
    assert len(_lib.PROTOTYPES["da_resize2d"][1]) == 15 and h.da_resize2d.argtypes == _lib.PROTOTYPES["da_resize2d"][1]
    assert h.da_resize2d_window_rows() == R.WINDOW_ROWS
    assert h.da_abi_version() == _lib.ABI_VERSION                                                             # additive: the number stays
    pics = np.zeros((2, R.PIC_INTS), np.int32)
    pics[:, 7], pics[:, 20] = (5, 32), (3, 10)
    assert h.da_resize2d_workspace_bytes(2, pics.ctypes.data) == 48 + 960
    assert h.da_resize2d_workspace_bytes(0, pics.ctypes.data) == 0 and h.da_resize2d_workspace_bytes(2, None) == 0
    one = C.c_void_p(1 << 20)                                                                                # never dereferenced: all refused

    def call(G=1, src=one, src_bytes=3, pictures=one, tables=one, n_table=8, dst=one, dst_bytes=3, work=None, work_bytes=0, route=0, tiles=1,
             hb=1, vb=1):
        return h.da_resize2d(G, src, src_bytes, pictures, tables, n_table, dst, dst_bytes, work, work_bytes, route, tiles, hb, vb, None)

    for name in ("src", "pictures", "tables", "dst"):
        assert call(**{name: None}) == 1 and b"null argument" in h.da_last_error(), name
    for kw in (dict(G=0), dict(src_bytes=0), dict(n_table=0), dict(dst_bytes=-1)):
        assert call(**kw) == 1 and b"bad sizes" in h.da_last_error(), kw
    assert call(route=2) == 1 and b"route is 0 (fused) or 1 (two-pass)" in h.da_last_error()
    assert call(tiles=0) == 1 and b"tiles in one launch" in h.da_last_error()
    assert call(tiles=1 << 31) == 1 and b"tiles in one launch" in h.da_last_error()
    assert call(route=1) == 1 and b"needs a workspace" in h.da_last_error()
    assert call(route=1, work=one, work_bytes=16, hb=0) == 1 and b"blocks in one launch" in h.da_last_error()
