"""Stage-level GPU tests of the PointNet++ fragment encoder (da_pointnet_plus.hip): k_pnp_sa<1|2|3> and k_pnp_head each alone on
injected inputs, the natural pipeline tensor by tensor, staged against whole execution, the seam between two passes over the
workspace, and the selection kernels at the sizes where their loops turn over.  Beside tests/test_gpu_pointnet_plus.py, which holds
the final [P, 256] row; the inputs and the comparison are shown to have teeth in tests/test_pointnet_plus_stages_host.py.

The bound of a matrix stage is elementwise: |kernel - stage64| <= tol = 8 x E32 x max |stage64|, with
E32 = max |stage32 - stage64| / max |stage64| the deviation of a plain fp32 evaluation of the same stage (folded weights, BLAS dot
products; tests/golden/pointnet_plus_refs.py) from fp64, recomputed from the reference on every run, never from the kernel.  8: the
kernels sum in another order (MFMA 32x32x2 blocks, k in slices of 8; the head 64 lanes and a shuffle tree) -- both are
O(sqrt(K) u) walks.  8 E32 <= RTOL32 is asserted: the bound can only be tighter than the project's 1e-4.  Every test prints E32,
tol and the kernel's err / tol (pytest -s).

Every index a test writes into the workspace is in range (asserted by stage_cases): the kernels do not bounds-check them."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointnet_plus_refs as R

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet_plus_v1.npz"))
RTOL32 = 1e-4
CASES = R.stage_cases()
INPUTS = {"sa1": ("fps1", "grp1"), "sa2": ("fps1", "fps2", "grp2", "l1"), "sa3": ("fps1", "fps2", "l2"), "head": ("part",)}
OUTPUT = {"sa1": "l1", "sa2": "l2", "sa3": "part", "head": None}
TENSORS = ("fps1", "grp1", "fps2", "grp2", "l1", "l2", "part")
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    from diffassemble_amd.pointnet_plus_encoder import PointNetPlusEngine
    return PointNetPlusEngine(R.state(), device=dev)


@functools.lru_cache(maxsize=None)
def weights():
    return R.state(torch.float64), R.folded32(R.state())


def held(what, got, ref64, e32, tol):
    """Print the figures, then the elementwise bound."""
    got, scale = got.detach().double().cpu(), float(ref64.abs().max())
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()), what
    err = float((got - ref64).abs().max())
    print(f"pointnet_plus {what}: E32 {e32:.3e}, tol {tol:.3e} (max |ref64| {scale:.4g}), kernel err {err:.3e} = {err / tol:.3f} tol "
          f"= {err / scale:.3e} relative")
    assert 0 < R.STAGE_TOL_FACTOR * e32 <= RTOL32, (what, e32)
    assert bool(((got - ref64).abs() <= tol).all()), (what, err, tol)


# ------------------------------------------------------------------------------------------------------------ one stage alone
@pytest.mark.parametrize("name", list(CASES))
def test_stage_alone_from_injected_inputs(dev, eng, name):
    from diffassemble_amd.pointnet_plus_encoder import STAGES
    c = CASES[name]
    _, out64, _, e32, tol = R.stage_reference(c, *weights())
    pts, start = torch.from_numpy(c.pts).to(dev), (torch.zeros(c.P, dtype=torch.int64), torch.zeros(c.P, dtype=torch.int64))
    eng.forward(pts, start)                            # sizes the workspace of this P (and leaves in-range indices everywhere)
    v = eng.workspace_views(c.P)
    inputs = {k: torch.from_numpy(getattr(c, k)).to(v[k].dtype) for k in INPUTS[c.stage]}
    for k, t in inputs.items():
        assert v[k].shape == t.shape, (k, tuple(v[k].shape), tuple(t.shape))
        v[k].copy_(t.to(dev))
    out = torch.full((c.P, 256), SENTINEL, device=dev)
    result = out if c.stage == "head" else v[OUTPUT[c.stage]]
    others = {k: v[k].clone() for k in TENSORS if k != OUTPUT[c.stage]}
    runs = []
    for _ in range(2):
        result.fill_(float("nan"))                     # nothing of the sizing call survives in the result
        assert eng.run_stages(pts, start, out, STAGES[c.stage]) is out
        runs.append(result.clone())
    for k in TENSORS:                                  # the inputs, and every tensor that is not this stage's, bit for bit
        if k != OUTPUT[c.stage]:
            assert torch.equal(v[k], others[k]), k
    for k, t in inputs.items():
        assert torch.equal(v[k].cpu(), t), k
    if c.stage != "head":
        assert bool((out == SENTINEL).all())
    assert torch.equal(runs[0], runs[1])
    got = runs[0].double().cpu()
    if c.stage == "sa3":                               # four tiles of 32 points: their maximum is the stage's
        assert runs[0].shape == (c.P, 4, 1024)
        pre = R.stage_sa(weights()[0], 3, R.stage_rows(c, torch.float64))[0]              # [P, 128, 1024]
        held(f"stage {name} per tile", got, pre.reshape(c.P, 4, 32, 1024).max(dim=2).values, e32, tol)
        got = got.max(dim=1).values
    held(f"stage {name}", got, out64, e32, tol)


# ------------------------------------------------------------------------------------------------------------ the natural pipeline
@functools.lru_cache(maxsize=None)
def natural(P, N):
    """A stored case, computed once and left unchanged: cloud, starts, the contract's selections, every tensor of the chain in fp64
    and in plain fp32."""
    pre = f"case/{P}x{N}/"
    pts = R.make_cloud(P, N, int(GOLD[pre + "cloud_seed"]))
    start = (torch.from_numpy(GOLD[pre + "start1"].astype(np.int64)), torch.from_numpy(GOLD[pre + "start2"].astype(np.int64)))
    sel = R.select(pts, start[0].numpy(), start[1].numpy())
    sd64, fw = weights()
    return SimpleNamespace(pts=torch.from_numpy(pts), start=start, sel=sel, c64=R.eval_chain(sd64, torch.from_numpy(pts).double(), sel),
                           c32=R.eval_chain(None, torch.from_numpy(pts), sel, fw=fw))


@pytest.mark.parametrize("P,N", [(1, 64), (2, 513)])
def test_natural_pipeline_tensor_by_tensor(dev, eng, P, N):
    c = natural(P, N)
    out = eng.forward(c.pts.to(dev), c.start)
    v = eng.workspace_views(P)
    for k in ("fps1", "grp1", "fps2", "grp2"):         # the level-2 selections run on `sel`-indexed points: not the stand-alone entries
        assert v[k].dtype == torch.int32 and np.array_equal(v[k].cpu().numpy(), c.sel[k]), k
    got = dict(l1=v["l1"], l2=v["l2"], l3=v["part"].max(dim=1).values, out=out)
    for k in ("l1", "l2", "l3", "out"):
        held(f"natural {P}x{N} {k}", got[k], c.c64[k], *R.stage_bound(c.c64[k], c.c32[k]))


def test_staged_equals_whole(dev, eng):
    from diffassemble_amd.pointnet_plus_encoder import STAGES
    c = natural(2, 513)
    pts = c.pts.to(dev)
    whole = eng.forward(pts, c.start).clone()
    v = eng.workspace_views(2)
    want = {k: v[k].clone() for k in TENSORS}
    assert list(STAGES.values()) == [1, 2, 4, 8, 16, 32, 64, 128]
    selections = sum(STAGES[k] for k in ("fps1", "ball1", "fps2", "ball2"))
    matrix = sum(STAGES[k] for k in ("sa1", "sa2", "sa3", "head"))
    for sets in (list(STAGES.values()), [selections, matrix], [255]):
        for k in TENSORS:
            v[k].zero_()                               # index 0 is in range everywhere
        out = torch.full((2, 256), SENTINEL, device=dev)
        for bits in sets:
            eng.run_stages(pts, c.start, out, bits)
        for k in TENSORS:
            assert torch.equal(v[k], want[k]), (sets, k)
        assert torch.equal(out, whole), sets


# ------------------------------------------------------------------------------------------------------------ two passes over the workspace
@pytest.mark.parametrize("N", [32, 600])
def test_chunk_seam(dev, N):
    """chunk + 1 fragments: the second pass starts at fragment `chunk` of points, start1, start2 and out, on the workspace of the
    first.  Five distinct fragments with five distinct pairs of starts, cyclically; fragment `chunk` is not fragment 0's.
    * points + p0 * fs and out + p0 * ld_out: every row bit-equal to its fragment's, within RTOL32 of the contract, a strided out.
    * start1 + p0 and start2 + p0: after the call the workspace holds the second pass's fragment in its first slot and the first
      pass's in the others; its fps1 / fps2 (which begin with the starts) and groups equal the contract's selections of THOSE
      fragments, and the contract's selections differ when the starts are fragment 0's (asserted).  At N = 32 that is the only hold
      on the starts: sa1 picks every point and no ball fills, so the row does not depend on them.  At N = 600 it does -- the
      contract's rows move by more than 1e-3 of the largest when start1 alone or start2 alone is fragment 0's (asserted) -- and the
      rows hold them too."""
    from diffassemble_amd.pointnet_plus_encoder import PointNetPlusEngine
    e = PointNetPlusEngine(R.state(), device=dev)      # its own engine: the half gigabyte goes with it
    chunk, B = e.chunk, 5
    P = chunk + 1
    assert chunk >= B and chunk % B != 0               # fragment `chunk` differs from fragment 0, the one a lost offset would read
    base = R.make_cloud(B, N, R.STAGE_SEED + 60 + N)
    s1, s2 = np.array([0, N - 1, 7, N // 2, N - 7]), np.array([0, 511, 100, 301, 77])
    which = torch.arange(P) % B
    pts = torch.from_numpy(base)[which].to(dev)
    start = (torch.from_numpy(s1)[which], torch.from_numpy(s2)[which])
    sd64, fw = weights()
    x64 = torch.from_numpy(base).double()
    sel = R.select(base, s1, s2)
    want = R.eval_forward(sd64, x64, sel)
    assert float((want[:, None] - want[None]).abs().amax(-1).add(torch.eye(B) * 9).min()) > 1e-2          # five different rows
    for lost in (0, 1):                                # what a launch without `+ p0` would select, and (N = 600) compute
        other = R.select(base, s1 * (lost != 0), s2 * (lost != 1))
        key = ("fps1", "fps2")[lost]
        assert all((other[key][p] != sel[key][p]).any() for p in range(1, B)), key
        if N > 512:
            moved = (R.eval_forward(sd64, x64, other) - want).abs().amax(-1) / want.abs().max()
            assert float(moved[1:].min()) > 1e-3, (key, moved)
    out = e.forward(pts, start)
    print(f"pointnet_plus chunk seam: P = {P}, N = {N}, workspace {e._ws.numel() / 2 ** 20:.1f} MiB")
    assert e._ws.numel() == e.lib.da_pointnet_plus_workspace_bytes(chunk, N)
    assert torch.equal(out, out[:B][which.to(dev)])    # EVERY row is its fragment's
    v = e.workspace_views(chunk)                       # slot 0: fragment `chunk` (second pass); slot j > 0: fragment j (first pass)
    held_by = np.arange(chunk) % B
    held_by[0] = chunk % B
    for k in ("fps1", "fps2"):
        assert np.array_equal(v[k].cpu().numpy(), sel[k][held_by]), k
    for k in ("grp1", "grp2"):
        for slot in (0, 1, chunk - 1):
            assert np.array_equal(v[k][slot].cpu().numpy(), sel[k][held_by[slot]]), (k, slot)
    assert int(v["fps1"][0, 0]) == s1[chunk % B] != s1[0] and int(v["fps2"][0, 0]) == s2[chunk % B] != s2[0]
    for i in (0, chunk - 1, chunk):
        err = float((out[i].double().cpu() - want[i % B]).abs().max() / want.abs().max())
        print(f"pointnet_plus chunk seam N = {N}: row {i} rel err {err:.3e}")
        assert err <= RTOL32
        alone = e.forward(pts[i:i + 1], tuple(s[i:i + 1] for s in start))
        assert torch.equal(alone[0], out[i]), i
    buf = torch.full((P, 400), SENTINEL, device=dev)
    view = buf[:, 64:320]
    assert e.forward(pts, start, out=view).data_ptr() == view.data_ptr() and torch.equal(view, out)
    assert bool((buf[:, :64] == SENTINEL).all()) and bool((buf[:, 320:] == SENTINEL).all())
    with pytest.raises(Exception, match="workspace_views"):
        e.workspace_views(P)


# ------------------------------------------------------------------------------------------------------------ the workspace layout
SIZES = (512 * 4, 512 * 32 * 4, 128 * 4, 128 * 64 * 4, 512 * 128 * 4, 128 * 256 * 4, 4 * 1024 * 4)          # bytes per fragment


def test_workspace_offsets_are_the_layout_of_workspace_bytes():
    """Needs the built library, not the device: it stands here, with the tests that run the library."""
    import ctypes as C
    from diffassemble_amd import _lib
    from diffassemble_amd import pointnet_plus_encoder as E
    lib = _lib.lib()
    chunk = lib.da_pointnet_plus_workspace_offsets(0, None)
    assert chunk >= 1 and [n for n, _, _ in E.WORKSPACE_TENSORS] == list(TENSORS)
    assert tuple(4 * int(np.prod(s)) for _, _, s in E.WORKSPACE_TENSORS) == SIZES
    for P in (1, 2, 3, 5, 7, chunk - 1, chunk, chunk + 1, 3 * chunk):
        off = (C.c_size_t * 7)(*([12345] * 7))
        assert lib.da_pointnet_plus_workspace_offsets(P, off) == chunk
        off, held = list(off), min(P, chunk)
        assert off[0] == 0 and all(o % 256 == 0 for o in off)
        for i in range(6):                             # ascending, no overlap, no more than the alignment between two tensors
            assert off[i] + held * SIZES[i] <= off[i + 1] < off[i] + held * SIZES[i] + 256, (P, i)
        end = off[6] + held * SIZES[6]
        assert (end + 255) // 256 * 256 == lib.da_pointnet_plus_workspace_bytes(P, 1000), P
    untouched = (C.c_size_t * 7)(*([12345] * 7))
    assert lib.da_pointnet_plus_workspace_offsets(0, untouched) == chunk and list(untouched) == [12345] * 7


# ------------------------------------------------------------------------------------------------------------ selection seams
SEAM_N = (2, 63, 65, 255, 256, 257, 2047)              # the ball query walks 64 points a step, the sampling keeps lane + 256 i


@pytest.mark.parametrize("N", SEAM_N)
def test_fps_at_the_seams(dev, N):
    from diffassemble_amd import pointnet_plus_encoder as E
    pts = R.make_cloud(2, N, R.STAGE_SEED + 70 + N)
    start = np.array([0, N - 1])
    for npoint in (1, N, N + 3):
        want = R.fps(pts, npoint, start)
        got = E.fps(torch.from_numpy(pts).to(dev), npoint, torch.from_numpy(start))
        assert got.shape == (2, npoint) and np.array_equal(got.cpu().numpy(), want), npoint
        if npoint == N:
            assert all(len(set(w.tolist())) == N for w in want)               # every point once ...
        if npoint == N + 3:
            assert not want[:, N:].any()                                         # ... then index 0


@pytest.mark.parametrize("N", SEAM_N)
def test_ball_query_at_the_seams(dev, N):
    """nsample 1 / 33 / 64 / 65 at a radius chosen (on the reference) so that the walk ends in different 64-point steps.  Asserted on
    the reference, wherever N allows it:
    * nsample 1 and 33, N >= 63: inside the FIRST 64 points some centre has more than nsample members (the members found past
      nsample in that step are left out) and some centre fewer (it walks on, or is padded).  Fewer than 1 needs a centre past the
      first 64 points with no neighbour among them, so N >= 65: point N - 1 of the last fragment lies far from all others and is a
      centre.  N = 2: two members for nsample 1 is all there can be.
    * nsample 64 and 65, N >= 255: no first step of 64 points can exceed them; some centre has fewer members in the first step and
      some centre's count passes nsample strictly inside a LATER step.
    * N = 63 and 65: some centre stays short of nsample 33 and up over the whole fragment and is padded with its first member.
    21 centres: not a multiple of the four a workgroup takes."""
    from diffassemble_amd import pointnet_plus_encoder as E
    P, S = 3, 7
    pts = R.make_cloud(P, N, R.STAGE_SEED + 90 + N)
    if N >= 65:
        pts[P - 1, N - 1] = (4.0, -4.0, 4.0)          # alone: a centre beyond the first step whose only member is itself
    rng = np.random.default_rng(R.STAGE_SEED + 91 + N)
    centre = rng.integers(0, N, (P, S))
    centre[0, 0], centre[P - 1, S - 1] = 0, N - 1
    d = np.stack([R.d2(pts[p][centre[p]][:, None, :], pts[p][None]) for p in range(P)])              # [P, S, N]
    near = d[d < 4.0].astype(np.float64)               # the distances among the cloud proper
    for nsample in (1, 33, 64, 65):
        # the share of the points inside the ball, on average: about nsample of the first 64, or 0.6 so that 64 / 65 fall in step two
        share = (0.25 if N > 2 else 0.75) if nsample == 1 else 33 / 64 if nsample == 33 else 0.6
        radius = float(np.sqrt(np.quantile(near, share)))
        want = R.ball_query(pts, centre, radius, nsample)
        count = np.cumsum(~(d > np.float32(radius ** 2)), -1)
        ends = count[..., np.minimum(np.arange(63, N + 63, 64), N - 1)]         # after each step of 64
        before = np.concatenate([np.zeros_like(ends[..., :1]), ends[..., :-1]], -1)
        passes = (before < nsample) & (ends > nsample)                          # strictly inside a step
        if nsample < 64:
            assert (ends[..., 0] > nsample).any() or (N == 2 and nsample == 33), (N, nsample)
            if N >= (65 if nsample == 1 else 63):
                assert (ends[..., 0] < nsample).any(), (N, nsample)
        elif N >= 255:
            assert (ends[..., 0] < nsample).any() and passes[..., 1:].any(), (N, nsample)
        if N in (63, 65) and nsample >= 33:
            assert count[..., -1].min() < nsample, (N, nsample)
        got = E.ball_query(torch.from_numpy(pts).to(dev), torch.from_numpy(centre), radius, nsample)
        assert got.shape == (P, S, nsample) and np.array_equal(got.cpu().numpy(), want), (N, nsample)
