"""GPU tests of the device resize: ``da_resize2d`` (diffassemble_amd/csrc/da_resize2d.hip) through ``resize_images`` and
``make_batch_from_pictures``.

Three expectations, all exact: tests/golden/resize2d_v1.npz, what ``PIL.Image.resize`` and the reference's dataset classes
returned (see tests/test_resize2d_host.py, which also proves the host route ``_loop_resize`` equal to it and to PIL),
``_loop_resize`` itself on a ragged Batch, and ``make_batch`` of ``_loop_resize``'s pictures.  The shapes are small: the
kernel's paths are the two routes, full and partial tiles in both directions (outputs wider than 32 and taller than 64), rows
that are and are not multiples of 16 bytes, the skipped passes, boxes and the flip, and every one of them runs below 100 x 100
pixels; only the route choice needs a taller source (1000 and 600 rows).  Every comparison is ``torch.equal`` on bytes."""
import numpy as np
import pytest
import torch

import test_resize2d_host as H

pytestmark = pytest.mark.gpu

ROUTES = ("fused", "two_pass")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("resample", H.FILTERS)
def test_every_fixture_case_in_one_ragged_call(resample, route, dev):
    """All 14 cases as ONE call per filter and route (ragged sources, outputs and boxes): byte-equal to what PIL returned."""
    from diffassemble_amd import resize2d as R
    cases = H.cases()
    got = R.resize_images([c[0] for c in cases], [c[1] for c in cases], resample=resample, boxes=[c[2] for c in cases], route=route, device=dev)
    assert R.last_route() == route and isinstance(got, list) and len(got) == len(cases)
    for k, g in enumerate(got):
        w = torch.from_numpy(H.want(k, resample).copy())
        assert g.device.type == "cuda" and g.dtype == torch.uint8 and tuple(g.shape) == tuple(w.shape)
        assert torch.equal(g.cpu(), w), (k, resample, route, int((g.cpu() != w).sum()))


@pytest.mark.parametrize("resample", ["bicubic", "lanczos"])
def test_both_routes_equal_the_host_route_on_a_ragged_batch(resample, dev):
    """Five pictures, five source and output sizes, a 1 x 1 source, boxes and flips mixed, rows of 123 and 135 bytes (no
    multiple of 16), outputs above one tile both ways; host pictures and device pictures."""
    from diffassemble_amd import resize2d as R
    pics = H.ragged_pictures()
    want = [torch.from_numpy(H.loop(p, s, resample, b, f)) for p, s, b, f in zip(pics, H.RAGGED["sizes"], H.RAGGED["boxes"], H.RAGGED["flips"])]
    for route in ROUTES:
        for given in (pics, [torch.from_numpy(p).to(dev) for p in pics]):
            got = R.resize_images(given, H.RAGGED["sizes"], resample=resample, boxes=H.RAGGED["boxes"], flips=H.RAGGED["flips"], route=route,
                                  device=dev)
            assert R.last_route() == route
            for k, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g.cpu(), w), (k, resample, route, int((g.cpu() != w).sum()))


def test_strong_downscaling_takes_the_two_pass_route(dev):
    """A tile of a 1000- or 600-row source resized to 32 rows reads more than 256 source rows: route=None goes two-pass and
    forcing the fused route is refused; a 40-row source with 1000 columns stays fused."""
    from diffassemble_amd import resize2d as R
    rng = np.random.default_rng(5)
    for (h, w), route in (((1000, 40), "two_pass"), ((600, 600), "two_pass"), ((40, 1000), "fused")):
        pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = R.resize_images([pic], (32, 32), device=dev)
        assert R.last_route() == route, (h, w)
        assert tuple(got.shape) == (1, 32, 32, 3) and torch.equal(got[0].cpu(), torch.from_numpy(H.loop(pic, (32, 32)))), (h, w)
        if route == "two_pass":
            with pytest.raises(ValueError, match="route='fused' holds at most 256 source rows per tile"):
                R.resize_images([pic], (32, 32), route="fused", device=dev)


@pytest.mark.parametrize("mode", list(H.CHAIN_MODES))
def test_make_batch_from_pictures_equals_the_reference_datasets(mode, dev):
    """Pictures that are not at their final size -> resize (bicubic: Puzzle_Dataset, Lanczos: Puzzle_Dataset_ROT) -> pieces: every
    per-piece tensor bit-equal to what the reference's get() returned."""
    from diffassemble_amd import make_batch_from_pictures
    resample, kw = H.CHAIN_MODES[mode]
    turns = H.chain_ref(mode, "rot_index") if kw else None
    got = make_batch_from_pictures(H.chain_pictures(), H.chain_dims(), resample=resample, rot_index=turns, device=dev, **kw)
    names = ("x", "patches", "indexes", "rot", "rot_index") if kw else ("x", "patches", "indexes")
    for name in names:
        g, w = getattr(got, name), H.chain_ref(mode, name)
        assert g.device.type == "cuda" and g.dtype == w.dtype and torch.equal(g.cpu(), w), (mode, name)
    if not kw:
        assert bool((got.rot_index == 0).all()) and got.rot.cpu().tolist() == [[1, 0]] * 14
    assert got.ptr.tolist() == [0, 6, 12, 14] and got.num_graphs == 3


def test_hard_augmentation_equals_make_batch_of_the_two_stage_host_result(dev):
    from diffassemble_amd import make_batch, make_batch_from_pictures
    import test_puzzle_batch_host as P
    pics, dims = H.chain_pictures(), H.chain_dims()
    flips = [True, False, True]
    crops = [(5, 3, 90, 60), None, (2.5, 1.0, 60.25, 30.0)]
    staged = []
    for pic, (rows, cols), flip, crop in zip(pics, dims, flips, crops):
        one = H.loop(pic, (32 * rows, 32 * cols), "bicubic", None, flip)
        staged.append(torch.from_numpy(one if crop is None else H.loop(one, (32 * rows, 32 * cols), "bicubic", crop)))
    turns = torch.arange(14) % 4
    want = make_batch(staged, dims, rotation=True, rot_index=turns)
    got = make_batch_from_pictures([torch.from_numpy(p).to(dev) for p in pics], dims, flips=flips, crop_boxes=crops, rotation=True, rot_index=turns)
    P.assert_batch_equal(got, want)
    weak = make_batch_from_pictures(pics, dims, flips=flips, device=dev)
    firsts = [torch.from_numpy(H.loop(pic, (32 * r, 32 * c), "bicubic", None, f)) for pic, (r, c), f in zip(pics, dims, flips)]
    P.assert_batch_equal(weak, make_batch(firsts, dims))


@pytest.mark.parametrize("route", ROUTES)
def test_nothing_outside_the_callers_buffer_is_written(route, dev):
    """The ragged Batch written into the middle of a buffer filled with a pattern: the bytes before and behind the output, and
    the padding between the pictures, keep the pattern; the pictures are right."""
    from diffassemble_amd import resize2d as R
    pics = H.ragged_pictures()
    boxes = R._boxes(H.RAGGED["boxes"], pics)
    d, tables, out_bytes, tiles, hblocks, vblocks, ws, _ = R._descriptors(H.RAGGED["shapes"], H.RAGGED["sizes"], "bicubic", boxes, H.RAGGED["flips"])
    guard = 4096
    pattern = (torch.arange(out_bytes + 2 * guard, dtype=torch.int64) * 37 % 251).to(torch.uint8)
    buf = pattern.to(dev)
    flat = torch.cat([torch.from_numpy(p).reshape(-1) for p in pics]).to(dev)
    R._launch(flat, d, tables, buf[guard:guard + out_bytes], tiles, hblocks, vblocks, ws, route, dev)
    torch.cuda.synchronize()
    back = buf.cpu()
    assert torch.equal(back[:guard], pattern[:guard]) and torch.equal(back[guard + out_bytes:], pattern[guard + out_bytes:])
    lo = guard
    for k, (p, (oh, ow), b, f) in enumerate(zip(pics, H.RAGGED["sizes"], H.RAGGED["boxes"], H.RAGGED["flips"])):
        n = 3 * oh * ow
        assert torch.equal(back[lo:lo + n].view(oh, ow, 3), torch.from_numpy(H.loop(p, (oh, ow), "bicubic", b, f))), k
        pad = ((n + 15) & ~15) - n
        assert torch.equal(back[lo + n:lo + n + pad], pattern[lo + n:lo + n + pad]), k
        lo += n + pad
    assert lo == guard + out_bytes


def test_final_sized_pictures_come_back_unchanged(dev):
    """Neither pass runs (PIL returns a copy): one stacked device tensor, read in place."""
    from diffassemble_amd import resize_images
    import test_puzzle_batch_host as P
    imgs = torch.stack(P.noise_images([(2, 3)] * 3, 21)).to(dev)
    for route in ROUTES:
        got = resize_images(imgs, (64, 96), route=route)
        assert got.data_ptr() != imgs.data_ptr() and torch.equal(got, imgs)
    flipped = resize_images(imgs, (64, 96), flips=[True, False, True])
    assert torch.equal(flipped[0], imgs[0].flip(1)) and torch.equal(flipped[1], imgs[1])
