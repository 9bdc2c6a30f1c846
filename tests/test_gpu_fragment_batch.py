"""GPU tests of the 3D Batch builder: ``da_mesh_cum_area`` and ``da_fragment_batch`` (diffassemble_amd/csrc/da_fragment_batch.hip)
through ``make_batch3d``, against the host route ``_loop_batch3d`` (which tests/test_fragment_batch_host.py holds bit-equal to a
literal per-part loop) on the meshes and fixed draws of that module: 27 parts in objects of 2, 5 and 20, face counts 1, 4, 12,
80, 255, 256, 257 and 1300 (the scan's chunk is 256), zero-area faces, one huge face among tiny ones, a cube at 1e3, picks that
are exactly 0, and N = 1, 7, 256, 257, 1000 (the workgroup has 256 threads).

Bounds.  The sampled faces are EQUAL: the host test proves that no pick of these draws lies within 64 F 2^-53 cum[-1] of a
boundary, more than a reordered fp64 sum can move one.  ``pcds`` and the centroid columns of ``x``:
|out - fp32(ref64)| <= ulp32(ref) + 2^-40 max|vertex of the part|: one fp32 rounding may flip, and the centroid is a sum of N
terms in another order (N 2^-53 max|vertex| << 2^-40 max|vertex| for N + F <= 8192), which matters only where centring
cancels.  Everything else is equal."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_fragment_batch_host as H

pytestmark = pytest.mark.gpu

EXACT = ("batch", "ptr", "valids", "edge_index", "data_id")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def part_scale(meshes, src):
    """max |vertex| of every output part."""
    flat = [np.abs(v).max() for obj in meshes for v, _ in obj]
    return torch.tensor([flat[s] for s in src], dtype=torch.float64)


def assert_close_to_host(got, want, scale, what=""):
    """``got`` (device) against ``want`` (host route) under the bounds of the module docstring; prints the worst figures first."""
    g_p, w_p = got.pcds.cpu().double(), want.pcds.double()
    g_c, w_c = got.x[:, 4:].cpu().double(), want.x[:, 4:].double()
    worst = []
    for g, w, s in ((g_p, w_p, scale[:, None, None]), (g_c, w_c, scale[:, None])):
        ulp = torch.from_numpy(np.spacing(np.abs(w.numpy()).astype(np.float32)).astype(np.float64))
        bound = ulp + 2.0 ** -40 * s
        err = (g - w).abs()
        worst.append((float((err / bound).max()), float(err.max())))
        assert bool((err <= bound).all()), (what, worst)
    print(f"{what}: worst error / bound: pcds {worst[0][0]:.3f} (abs {worst[0][1]:.3e}), centroid {worst[1][0]:.3f} (abs {worst[1][1]:.3e}); "
          f"pcds bit-equal {float((g_p == w_p).double().mean()):.4%}")
    assert torch.equal(got.x[:, :4].cpu(), want.x[:, :4]), what
    for k in EXACT:
        if hasattr(want, k):
            a, b = getattr(got, k), getattr(want, k)
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b), (what, k)
    assert got.category == want.category and got.num_graphs == want.num_graphs


@pytest.mark.parametrize("N", H.N_LIST)
def test_device_equals_the_host_route(N, dev):
    from diffassemble_amd import make_batch3d
    want = H.host_batch(N)
    got = make_batch3d(H.case_meshes(), num_points=N, category=["a", "b", "c"], data_id=[7, 8, 9], return_face_index=True, device=dev,
                       **H.case_draws(N))
    for k in ("x", "pcds", "face_index") + EXACT:
        assert getattr(got, k).device.type == "cuda", k
    assert got.face_index.dtype == torch.int32
    assert torch.equal(got.face_index.cpu(), want.face_index)                 # no case exempted
    assert_close_to_host(got, want, part_scale(H.case_meshes(), range(27)), f"N = {N}")


def packed_on(dev):
    meshes = H.case_meshes()
    parts = [p for obj in meshes for p in obj]
    return dict(vertices=torch.from_numpy(np.concatenate([v for v, _ in parts])).to(dev),
                faces=torch.from_numpy(np.concatenate([f for _, f in parts]).astype(np.int32)).to(dev),
                vert_ptr=np.concatenate([[0], np.cumsum([len(v) for v, _ in parts])]), face_ptr=np.concatenate([[0], np.cumsum([len(f) for _, f in parts])]),
                parts_per_object=list(H.COUNTS))


def assert_same(a, b, keys=("x", "pcds", "face_index") + EXACT):
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_two_calls_are_bit_equal_and_host_meshes_equal_device_meshes(dev):
    from diffassemble_amd import make_batch3d
    N = 257
    kw = dict(num_points=N, return_face_index=True, device=dev, **H.case_draws(N))
    first = make_batch3d(H.case_meshes(), **kw)
    assert_same(first, make_batch3d(H.case_meshes(), **kw))
    on_device = make_batch3d(packed_on(dev), **{k: v for k, v in kw.items() if k != "device"})        # device: where the meshes lie
    assert on_device.pcds.device.type == "cuda"
    assert_same(first, on_device)
    draws_on_device = make_batch3d(packed_on(dev), **{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()})
    assert_same(first, draws_on_device)


@pytest.mark.parametrize("name,kw", [("rot_range", dict(rot_range=25.0)), ("shuffle_parts", dict(shuffle_parts=True)), ("missing", dict(missing=30)),
                                     ("degree", dict(degree=40)), ("all", dict(rot_range=180.0, shuffle_parts=True, missing=20, degree=70))])
def test_options_on_the_device_equal_the_host_route(name, kw, dev):
    from diffassemble_amd import fragment_batch as F
    from diffassemble_amd import make_batch3d
    meshes = [H.case_meshes()[1], H.case_meshes()[0]]                          # 5 and 2 parts
    want = make_batch3d(meshes, num_points=65, generator=torch.Generator().manual_seed(9), **kw)
    got = make_batch3d(meshes, num_points=65, generator=torch.Generator().manual_seed(9), device=dev, **kw)
    src = np.concatenate(F._draws([5, 2], 65, kw.get("rot_range", -1), kw.get("shuffle_parts", False), kw.get("missing", 0), kw.get("degree", 0),
                                  torch.Generator().manual_seed(9))[4])
    assert got.x.shape == want.x.shape and got.edge_index.shape == want.edge_index.shape
    assert_close_to_host(got, want, part_scale(meshes, src), name)
    if "missing" in kw:
        assert got.x.shape[0] < 7


def test_bad_face_indices_and_perm_values_on_the_device_are_clamped(dev):
    """Part 6 gets face indices and perm values outside their ranges, handed in on the device (where nothing checks them): the
    call returns, every other part is unchanged, and part 6 is what the host route gives for the clamped values."""
    from diffassemble_amd import make_batch3d
    N = 7
    draws = {k: v.to(dev) for k, v in H.case_draws(N).items()}
    good = packed_on(dev)
    clean = make_batch3d(good, num_points=N, return_face_index=True, **draws)
    bad = dict(good, faces=good["faces"].clone())
    f0 = int(good["face_ptr"][6])
    bad["faces"][f0 + 3] = torch.tensor([1 << 30, -5, 2], dtype=torch.int32, device=dev)
    bad["faces"][f0 + 200, 1] = 257 + 40
    bad_draws = dict(draws, point_perm=draws["point_perm"].clone())
    bad_draws["point_perm"][6, 0], bad_draws["point_perm"][6, 3] = N + 1000, -3
    got = make_batch3d(bad, num_points=N, return_face_index=True, **bad_draws)
    torch.cuda.synchronize()
    others = [k for k in range(27) if k != 6]
    for k in ("x", "pcds", "face_index"):
        assert torch.equal(getattr(got, k)[others], getattr(clean, k)[others]), k
    assert_same(got, clean, EXACT)
    meshes = H.case_meshes()
    f = meshes[1][4][1].copy()                                                 # part 6 = object 1, part 4 (F = 255, V = 257)
    f[3], f[200, 1] = [256, 0, 2], 256
    meshes[1][4] = (meshes[1][4][0], f)
    perm = H.case_draws(N)["point_perm"].clone()
    perm[6, 0], perm[6, 3] = N - 1, 0
    want = make_batch3d(meshes, num_points=N, return_face_index=True, **dict(H.case_draws(N), point_perm=perm))
    assert torch.equal(got.face_index.cpu(), want.face_index)
    assert_close_to_host(got, want, part_scale(meshes, range(27)), "clamped")


def test_non_finite_vertices_propagate_as_on_the_host(dev):
    """A NaN vertex in a middle face of part 2, one in the third scan chunk of part 9 (F = 1300) and an Inf vertex in part 8: the
    total area is not finite, every pick finds the first such face as numpy.searchsorted does, and the part comes out non-finite
    exactly where the host route's does; the other parts keep their bounds."""
    from diffassemble_amd import make_batch3d
    N = 65
    want = H.nonfinite_batch(N)
    got = make_batch3d(H.nonfinite_meshes(), num_points=N, return_face_index=True, device=dev, **H.case_draws(N))
    assert torch.equal(got.face_index.cpu(), want.face_index)
    bad = sorted(v[0] for v in H.NONFINITE.values())
    for k in ("pcds", "x"):
        g, w = getattr(got, k).cpu()[bad], getattr(want, k)[bad]
        assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(torch.isinf(g), torch.isinf(w)), k
        assert torch.equal(g[torch.isinf(w)], w[torch.isinf(w)]) and torch.equal(g[torch.isfinite(w)], w[torch.isfinite(w)]), k
    assert bool(torch.isnan(got.pcds[[2, 9]]).all()) and not bool(torch.isfinite(got.pcds[8]).any())
    ok = [k for k in range(27) if k not in bad]

    def rows(b):
        return SimpleNamespace(pcds=b.pcds[ok], x=b.x[ok], category=b.category, num_graphs=b.num_graphs)

    assert_close_to_host(rows(got), rows(want), part_scale(H.case_meshes(), ok), "beside non-finite parts")
    assert_same(SimpleNamespace(**{k: getattr(got, k).cpu() for k in EXACT}), want, EXACT)


def test_a_batch_goes_through_the_3d_training_step(dev):
    """make_batch3d -> GNN_Diffusion(backbone="pointnet").training_step: 2 objects of 2 and 3 parts at N = 1.  The backbone is FROZEN
    (the configuration of the existing PointNet step test), so the encoder runs its eval path, which takes n_points >= 1
    (da_pointnet_forward); a trainable backbone's batch statistics need two points in all.  No tensor is assembled by hand."""
    import test_gpu_pointnet as PT
    from diffassemble_amd import make_batch3d
    meshes = [H.case_meshes()[0], H.case_meshes()[1][:3]]
    batch = make_batch3d(meshes, num_points=1, max_num_part=6, category=["everyday", "everyday"], generator=torch.Generator().manual_seed(4),
                         device=dev)
    assert batch.x.shape == (5, 7) and batch.pcds.shape == (5, 1, 3) and batch.valids.shape == (12,) and len(batch.data_id) == 2
    m = PT.diffusion_module(dev, freeze=True).train()
    m.log = lambda *a, **kw: None
    torch.manual_seed(3)
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
