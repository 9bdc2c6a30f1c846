"""GPU tests of the 2D renderer: ``da_render2d`` (diffassemble_amd/csrc/da_render2d.hip) through ``render2d.batch_frames`` and
through ``GNN_Diffusion.render_frames`` / ``test_step``.

The expectation is the numpy contract of tests/golden/render2d_refs.py, which tests/test_render2d_host.py proves equal to the
frames the reference's PIL compositing produced.  The contract is run on the angles the host layer computes on this machine
(``render2d.piece_angles``; they may differ from the recorded ones in the last bit of an atan2), so nothing here depends on a
libm; where they equal the recorded angles bit for bit, the reference's own frames and hashes are checked too.
Every comparison is ``torch.equal`` on bytes: there is no tolerance."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import render2d_refs as R
import test_render2d_host as H
from oracle import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def device_frames(name, dev, **kw):
    from diffassemble_amd.render2d import batch_frames
    c = H.cases()[name]
    return batch_frames(torch.from_numpy(H.crops_of(name)).to(dev), H.poses_of(name).to(dev), c["dims"], batch=H.batch_of(name).to(dev),
                        steps=c["steps"], **kw)


@pytest.mark.parametrize("name", R.CASES)
def test_kernel_frames_equal_the_contract(name, dev):
    c = H.cases()[name]
    frames = device_frames(name, dev)
    want = H.contract_frames(name)
    assert len(frames) == len(c["steps"]) and all(len(f) == len(c["dims"]) for f in frames)
    for (k, g), w in want.items():
        f = frames[k][g]
        assert f.dtype == torch.uint8 and f.device.type == "cuda" and tuple(f.shape) == w.shape
        assert torch.equal(f.cpu(), torch.from_numpy(w.copy())), (name, k, g, int((f.cpu() != torch.from_numpy(w.copy())).any(-1).sum()))
    if c["deg"] is None or np.array_equal(H.host_angles(name), c["deg"]):               # equal angles: the reference's own bytes
        for (k, g), digest in c["sha"].items():
            assert R.sha256(frames[k][g].cpu().numpy()) == digest, (name, k, g)
        for (k, g), frame in c["frames"].items():
            assert torch.equal(frames[k][g].cpu(), torch.from_numpy(frame)), (name, k, g)


def test_frames_are_views_of_one_buffer_in_step_then_puzzle_order(dev):
    frames = device_frames("ragged", dev)
    base = frames[0][0].untyped_storage()
    sizes = [64 * 96 * 4, 96 * 64 * 4, 32 * 32 * 4]
    assert base.nbytes() == 2 * sum(sizes)
    off = 0
    for k in range(2):
        for g in range(3):
            f = frames[k][g]
            assert f.untyped_storage().data_ptr() == base.data_ptr() and f.is_contiguous()
            assert f.storage_offset() == off and f.numel() == sizes[g]
            off += sizes[g]


def test_two_calls_give_equal_bytes(dev):
    for name in ("stack4x5", "pile30"):
        a, b = device_frames(name, dev), device_frames(name, dev)
        assert a[0][0].data_ptr() != b[0][0].data_ptr() and torch.equal(a[0][0], b[0][0])


def test_no_rotation_takes_the_identity_map(dev):
    """rotation=False on [N, 4] poses ignores the (cos, sin) columns (the kernel's NULL coefficient table)."""
    c = H.cases()["stack4x5"]
    got = device_frames("stack4x5", dev, rotation=False)[0][0]
    want = R.render(H.crops_of("stack4x5"), c["pos"][0], c["dims"][0])
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_strided_poses_and_a_list_of_steps(dev):
    """The loop's trajectory as a wider tensor's view ([K, N, 4] inside [K, N, 7], steps strided) and as a list of tensors."""
    from diffassemble_amd.render2d import batch_frames
    c = H.cases()["ragged"]
    crops, poses, batch = torch.from_numpy(H.crops_of("ragged")).to(dev), H.poses_of("ragged").to(dev), H.batch_of("ragged").to(dev)
    wide = torch.full((6, 12, 7), float("nan"), device=dev)
    wide[::2, :, 2:6] = poses
    view = wide[::2, :, 2:6]
    assert not view.is_contiguous()
    want = H.contract_frames("ragged")
    for got in (batch_frames(crops, view, c["dims"], batch=batch, steps=[0, 2]),
                batch_frames(crops, list(poses.unbind(0)), c["dims"], batch=batch, steps=[0, 2]),
                batch_frames(crops, wide[::4, :, 2:6], c["dims"], batch=batch)):          # steps 0 and 2, strided, no copy
        for (k, g), w in want.items():
            assert torch.equal(got[k][g].cpu(), torch.from_numpy(w.copy())), (k, g)


def test_a_non_finite_pose_is_not_drawn_on_the_device(dev):
    from diffassemble_amd.render2d import batch_frames
    c = H.cases()["clip3x5"]
    crops = H.crops_of("clip3x5")
    pos = np.repeat(c["pos"][:1], 3, 0).copy()
    pos[0, 5, 0], pos[1, 5, 1], pos[2, 5] = np.nan, np.inf, (-np.inf, np.nan)
    keep = [i for i in range(15) if i != 5]
    want = torch.from_numpy(R.render(crops[keep], c["pos"][0][keep], (3, 5)))
    got = batch_frames(torch.from_numpy(crops).to(dev), torch.from_numpy(pos).to(dev), [[3, 5]])
    assert all(torch.equal(got[k][0].cpu(), want) for k in range(3))


# ------------------------------------------------------------------------------------------------ the 2D module
def _module_and_batch(dev):
    """GNN_Diffusion(rotation=True) with random weights and a Batch of a 6 x 6 puzzle and a 6 x 6 puzzle with six pieces
    missing; 5 loop steps."""
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=50, sampling="DDIM", inference_ratio=10, model_mean_type=ModelMeanType.START_X, visual_pretrained=False,
                      noise_weight=1.0, rotation=True)
    m.model.load_state_dict(W.make_denoiser_state(50, 4, 4, seed=5), strict=False)
    m = m.to(dev).eval()
    m.model.precision = "fp32"
    sizes = [36, 30]
    ei, bvec = W.collate([W.dense_edge_index(n, True) for n in sizes], sizes)
    g = torch.Generator().manual_seed(3)
    a = torch.rand(66, generator=g) * 6.2831853
    x_gt = torch.cat((torch.rand(66, 2, generator=g) * 2 - 1, torch.cos(a)[:, None], torch.sin(a)[:, None]), 1)
    batch = SimpleNamespace(x=x_gt.to(dev), patches=torch.from_numpy(R.make_crops(9, 66)).to(dev), edge_index=ei.to(dev), batch=bvec.to(dev),
                            patches_dim=torch.tensor([[6, 6], [6, 6]]), patch_feats=torch.randn(66, 1088, generator=g).to(dev),
                            ind_name=torch.tensor([12, 5]))
    return m, batch


def _contract_of_loop(imgs, batch):
    """{(k, g): frame} of the contract for the loop's poses, on the host layer's angles."""
    from diffassemble_amd.render2d import piece_angles
    crops = batch.patches.cpu().numpy()
    out = {}
    for k, img in enumerate(imgs):
        pose, deg = img.cpu().numpy(), piece_angles(img[:, 2:4]).numpy()
        for g, (lo, hi) in enumerate(((0, 36), (36, 66))):
            out[(k, g)] = torch.from_numpy(R.render(crops[lo:hi], pose[lo:hi], (6, 6), deg[lo:hi]))
    return out


def test_render_frames_on_the_loops_own_trajectory(dev):
    m, batch = _module_and_batch(dev)
    torch.manual_seed(1)
    imgs, _ = m.p_sample_loop(batch.x.shape, batch.patches, batch.edge_index, batch=batch.batch, patch_feats=batch.patch_feats)
    assert len(imgs) == 5 and imgs[0].shape == (66, 4)
    frames = m.render_frames(batch, imgs)
    want = _contract_of_loop(imgs, batch)
    assert len(frames) == 5 and all(len(f) == 2 for f in frames)
    for (k, g), w in want.items():
        assert tuple(frames[k][g].shape) == (192, 192, 4) and torch.equal(frames[k][g].cpu(), w), (k, g)
    assert int((want[(4, 0)][..., 3] == 255).sum()) > 0                                    # something was drawn
    picked = m.render_frames(batch, imgs, steps=[4, 1])
    assert torch.equal(picked[0][1], frames[4][1]) and torch.equal(picked[1][0], frames[1][0])


def test_test_step_writes_every_step_and_changes_nothing_else(dev, tmp_path):
    """save_eval_images = True: K files per puzzle, named by ind_name and step, whose pixels are the frames; off (the default):
    no file, and the returned poses are bit-equal to those of the run that saved."""
    Image = pytest.importorskip("PIL.Image")
    m, batch = _module_and_batch(dev)
    m.eval_image_dir = str(tmp_path / "off")
    assert m.save_eval_images is False
    torch.manual_seed(2)
    img_off = m.test_step(batch, 0)
    assert not os.path.exists(m.eval_image_dir)
    kept = []
    loop = m.p_sample_loop
    m.p_sample_loop = lambda *a, **k: (kept.append(loop(*a, **k)), kept[-1])[1]
    m.save_eval_images = True
    m.eval_image_dir = str(tmp_path / "on")
    m.eval_image_max_bytes = 2 * 2 * 192 * 192 * 4                                           # two steps per launch: three chunks
    torch.manual_seed(2)
    img_on = m.test_step(batch, 0)
    assert torch.equal(img_on, img_off)
    imgs = kept[0][0]
    want = _contract_of_loop(imgs, batch)
    assert sorted(os.listdir(m.eval_image_dir)) == sorted(f"{n:03d}_{s:03d}.png" for n in (12, 5) for s in range(5))
    for g, n in enumerate((12, 5)):
        for s in range(5):
            with Image.open(os.path.join(m.eval_image_dir, f"{n:03d}_{s:03d}.png")) as im:
                assert im.mode == "RGBA" and torch.equal(torch.from_numpy(np.asarray(im).copy()), want[(s, g)]), (g, s)
