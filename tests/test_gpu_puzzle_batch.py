"""GPU tests of the Batch builder: ``da_puzzle_batch`` and ``da_complete_edges`` (diffassemble_amd/csrc/da_puzzle_batch.hip)
through the C ABI and through ``make_batch``.

Two expectations, both exact: tests/golden/puzzle_batch_v1.npz, what the reference's dataset classes returned (see
tests/test_puzzle_batch_host.py, which also proves the host route ``_loop_batch`` equal to it), and ``_loop_batch`` itself on fresh
noise pictures with every byte value.  All shapes are 32-pixel pieces on at most 4 x 4 cells: the kernel's paths are the four
turns, the two view counts, the border, ragged puzzles and kept lists, and every one of them runs at that size.  Every
comparison is ``torch.equal``: the feature copies bytes and looks a table up."""
import numpy as np
import pytest
import torch

import test_puzzle_batch_host as H
from oracle import weights as W

pytestmark = pytest.mark.gpu

POISON = -7          # of the int64 outputs (-1 is a legitimate entry of rot)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("mode,views", [("rot", 1), ("roteq", 4)])
def test_c_abi_on_poisoned_outputs_equals_the_reference(mode, views, dev):
    """The four fixture puzzles as one ragged Batch in one call, outputs pre-filled with NaN / -7: bit-equal to what the
    reference returned, nothing left unwritten."""
    from diffassemble_amd import _lib
    from diffassemble_amd import puzzle_batch as P
    dims = H.puzzles()
    turns = [H.ref(mode, g, "rot_index").tolist() for g in range(4)]
    assert all(sorted(set(t)) == [0, 1, 2, 3] for t in turns)                 # every turn in every puzzle
    keeps = [list(range(r * c)) for r, c in dims]
    host, where, N, E, n_lin = P._tables(dims, turns, keeps, [0, 1, 2, 3], True)
    small = torch.from_numpy(host).to(dev)

    def part(name):
        a, b, dtype, shape = where[name]
        return small[a:b].view(P._TORCH_OF[dtype]).view(shape)

    flat = torch.cat([i.reshape(-1) for i in H.images()]).to(dev)
    patches = torch.full((N, views, 3, 32, 32), float("nan"), device=dev)
    x = torch.full((N, 4), float("nan"), device=dev)
    rot = torch.full((N, 2), POISON, dtype=torch.long, device=dev)
    rot_index, indexes, batch = (torch.full((N,), POISON, dtype=torch.long, device=dev) for _ in range(3))
    edge_index = torch.full((2, E), POISON, dtype=torch.long, device=dev)
    h = _lib.lib()
    _lib.check(h.da_puzzle_batch(4, N, _lib.ptr(flat), flat.numel(), _lib.ptr(part("puzzles")), _lib.ptr(part("pieces")), _lib.ptr(part("lin")),
                                 n_lin, _lib.ptr(part("unit")), 0, views, 4, _lib.ptr(patches), _lib.ptr(x), _lib.ptr(rot), _lib.ptr(rot_index),
                                 _lib.ptr(indexes), _lib.ptr(batch), _lib.stream_ptr(dev)))
    _lib.check(h.da_complete_edges(4, _lib.ptr(part("edge")), E, _lib.ptr(edge_index), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert not torch.isnan(patches).any() and not torch.isnan(x).any()
    for t in (rot, rot_index, indexes, batch, edge_index):
        assert not (t == POISON).any()
    want = H.expected(mode)
    got = P.PuzzleBatch(x=x, patches=patches if views == 4 else patches[:, 0], indexes=indexes, rot=rot, rot_index=rot_index,
                        edge_index=edge_index, batch=batch, ptr=part("ptr"), patches_dim=part("patches_dim"), ind_name=part("ind_name"),
                        num_graphs=4)
    H.assert_batch_equal(got, want, mode)


def test_c_abi_two_column_x_and_the_border(dev):
    """x_cols = 2 writes [N, 2] rows and nothing beyond; padding = 3 equals the reference's zero_margin."""
    from diffassemble_amd import make_batch
    got = make_batch([H.images()[0].to(dev)], H.puzzles()[0], padding=3)
    assert got.x.shape == (6, 2) and torch.equal(got.x.cpu(), H.ref("plain", 0, "x"))
    assert torch.equal(got.patches.cpu(), H.ref("pad3", 0, "patches"))


# ------------------------------------------------------------------------------------------------ make_batch against the host route
DIMS = [(2, 3), (4, 4), (1, 2), (3, 2)]          # with 30 % missing: 4, 11, 1 and 4 pieces left
MODE_KW = {"plain": {}, "rot": dict(rotation=True), "roteq": dict(rotation=True, all_equivariant=True), "mp": dict(missing_perc=30),
           "rotmp": dict(rotation=True, missing_perc=30)}


@pytest.mark.parametrize("padding", [0, 3])
@pytest.mark.parametrize("mode", list(MODE_KW))
def test_make_batch_on_the_device_equals_the_host_route(mode, padding, dev):
    from diffassemble_amd import make_batch
    imgs = H.noise_images(DIMS, 31 + padding)
    want = make_batch(imgs, DIMS, padding=padding, generator=torch.Generator().manual_seed(5), **MODE_KW[mode])
    assert want.x.device.type == "cpu"
    for given in ([i.to(dev) for i in imgs], imgs):                          # pictures on the device, and on the host with device=
        got = make_batch(given, DIMS, padding=padding, generator=torch.Generator().manual_seed(5), device=dev, **MODE_KW[mode])
        assert all(getattr(got, k).device.type == "cuda" for k in H.ATTRS)
        H.assert_batch_equal(got, want, (mode, padding))
    if mode == "rot":
        assert sorted(set(want.rot_index.tolist())) == [0, 1, 2, 3]
    if "missing_perc" in MODE_KW[mode]:
        assert want.ptr.tolist() == [0, 4, 15, 16, 20]


@pytest.mark.parametrize("rotation", [False, True])
def test_kept_lists(rotation, dev):
    """Drop the first piece, drop the last piece, out of order, and a puzzle with a single piece left."""
    from diffassemble_amd import make_batch
    dims = [(2, 3), (2, 3), (2, 2), (3, 3), (4, 4)]
    keep = [[1, 2, 3, 4, 5], [0, 1, 2, 3, 4], [3, 0, 2, 1], [7], [15, 0, 9, 3, 12, 5]]
    imgs = H.noise_images(dims, 77)
    kw = dict(keep=keep, rotation=rotation, generator=torch.Generator().manual_seed(2))
    want = make_batch(imgs, dims, **kw)
    kw["generator"] = torch.Generator().manual_seed(2)
    got = make_batch([i.to(dev) for i in imgs], dims, **kw)
    H.assert_batch_equal(got, want)
    assert got.indexes.tolist() == sum(keep, []) and got.ptr.tolist() == [0, 5, 10, 14, 15, 21]
    assert got.edge_index.shape == (2, 25 + 25 + 16 + 1 + 36)


def test_one_stacked_device_tensor_is_read_in_place(dev):
    from diffassemble_amd import make_batch
    imgs = torch.stack(H.noise_images([(2, 2)] * 3, 4))
    want = make_batch(imgs, (2, 2), rotation=True, rot_index=torch.arange(12) % 4)
    got = make_batch(imgs.to(dev), (2, 2), rotation=True, rot_index=(torch.arange(12) % 4).to(dev))
    H.assert_batch_equal(got, want)


def test_complete_edges_of_1_5_and_6_pieces(dev):
    from diffassemble_amd import make_batch
    dims = [(1, 1), (2, 3), (2, 3)]
    got = make_batch([i.to(dev) for i in H.noise_images(dims, 1)], dims, keep=[[0], [5, 0, 1, 2, 4], [0, 1, 2, 3, 4, 5]])
    want = torch.cat([torch.ones(n, n).nonzero().t() + lo for n, lo in ((1, 0), (5, 1), (6, 6))], 1)
    assert got.edge_index.dtype == torch.int64 and torch.equal(got.edge_index.cpu(), want)
    assert W.collate([W.dense_edge_index(n, True) for n in (1, 5, 6)], [1, 5, 6])[0].shape == want.shape


# ------------------------------------------------------------------------------------------------ the contract, end to end
def test_a_batch_goes_through_eval_step_and_the_renderer(dev):
    """make_batch(rotation=True) -> GNN_Diffusion(backbone='resnet18equiv')._eval_step (encoder, sampling loop, scoring) ->
    render2d.batch_frames: it runs, and the shapes agree."""
    from diffassemble_amd import make_batch
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
    from diffassemble_amd.render2d import batch_frames
    m = GNN_Diffusion(steps=50, sampling="DDIM", inference_ratio=10, noise_weight=1.0, rotation=True, model_mean_type=ModelMeanType.START_X,
                      visual_pretrained=False, backbone="resnet18equiv")
    dsd, esd = W.make_denoiser_state(50, 4, 4, seed=5), W.make_encoder_state(5)
    missing, unexpected = m.model.load_state_dict({**dsd, **{"visual_backbone." + k: v for k, v in esd.items()}}, strict=False)
    assert not unexpected, unexpected
    m = m.to(dev).eval()
    m.model.precision = "fp32"
    dims = [(3, 3), (2, 3)]
    batch = make_batch([i.to(dev) for i in H.noise_images(dims, 12)], dims, rotation=True, keep=[list(range(9)), [4, 0, 5, 2]],
                       generator=torch.Generator().manual_seed(1), ind_name=[12, 5])
    torch.manual_seed(3)
    img = m.test_step(batch, 0)
    assert img.shape == batch.x.shape == (13, 4) and img.device.type == "cuda" and bool(torch.isfinite(img).all())
    frames = batch_frames(batch.patches, [img, batch.x], batch.patches_dim, batch=batch.batch, rotation=True)
    assert len(frames) == 2 and [tuple(f.shape) for f in frames[0]] == [(96, 96, 4), (64, 96, 4)]
    assert m.render_frames(batch, [img])[0][1].shape == (64, 96, 4)


def test_image_to_pieces_to_image(dev):
    """Rendering the ground-truth x of an unrotated, complete Batch gives the input pictures back: RGB exactly, alpha 255.
    (Square puzzles: the renderer scales x by the row count, the reference's pairing, so only they tile their canvas.)"""
    from diffassemble_amd import make_batch
    from diffassemble_amd.render2d import batch_frames
    dims = [(4, 4), (2, 2), (1, 1)]
    imgs = H.noise_images(dims, 8)
    batch = make_batch(imgs, dims, device=dev)
    frames = batch_frames(batch.patches, batch.x, batch.patches_dim, batch=batch.batch)[0]
    for g, img in enumerate(imgs):
        f = frames[g].cpu()
        assert torch.equal(f[..., :3], img) and bool((f[..., 3] == 255).all()), g
