"""The hidden layer projected by its own attention kernel (k_attn_res<.., 64>, da_attn_opt.hip; da_config.disable_folds bit 64 clear, the default): the
K / V-resident kernel of a (graph, head) computes that head's Q | K | V | skip columns of its graph in its prologue -- K | V straight
into its LDS image, Q / skip rows to memory in the projection kernels' layouts -- and no projection kernel runs.  Same
TransformerConv layer as every other path (reference backbones/Transformer_GNN.py:32,38; PyG lin_query / lin_key / lin_value /
lin_skip): same 16-step MFMA chain per output, bias behind the reduction, same rounding to bf16, so Q, skip and the layer's output
must equal the two-kernel layer's (disable_folds bit 64 set) BIT FOR BIT.  The switch is set in-process (`_lib.set_config`).

Which shapes the form takes is a statement about LDS, restated here from the kernel's layout and not read back from the library:
64-key stages of 8 KB for the K | V image, 512 B of words, the K and V weight blocks (2 * kin / 16 KB), 128 bias floats, and the
Q / skip weight blocks either inside the image's last stages (when those lie behind the eight stages the waves' first slabs fill) or
behind everything else; 160 KB in all.  1216 pieces (19 stages) are beyond it at either reduction length: the layer then keeps
the projection kernel, still on the resident attention kernel."""
import ctypes as C

import pytest
import torch

import test_gpu_softmax_fallbacks as F

pytestmark = pytest.mark.gpu
H = F.H


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def takes(max_nodes, kin):
    """LDS of k_attn_res<.., 64> for a Batch whose largest graph has max_nodes pieces (see the module docstring)."""
    img, wb = ((max_nodes + 63) // 64) * 8192, 2 * (kin // 16) * 1024
    base = img + 512 + wb + 512
    lds = base if img >= 8 * 8192 + wb else base + wb
    return 512 <= max_nodes <= 1216 and lds <= 160 * 1024


FOLD_ATTN_PROJ = 64          # da_config.disable_folds: set = the projection kernel stays in front of the resident attention kernel


class proj_switch:
    """`with proj_switch(3): ...` -- the switch, restored on exit: 3 = the attention kernel projects its layer (bit clear), 2 = two kernels."""

    def __init__(self, level):
        self.level = level

    def __enter__(self):
        from diffassemble_amd import _lib
        self.old = _lib.config().disable_folds
        _lib.set_config(disable_folds=(self.old & ~FOLD_ATTN_PROJ) | (0 if self.level == 3 else FOLD_ATTN_PROJ))

    def __exit__(self, *exc):
        from diffassemble_amd import _lib
        _lib.set_config(disable_folds=self.old)


def layer_inputs(sizes, kin, kind="m44", seed=13):
    """F.build_layer's layer (bf16-exact values, carrier features in the LAST two input columns) at a reduction length of 256 or,
    keeping the last 128 input features, 128 -- the reduction of the denoiser's first conv."""
    row, key, who = F.offsets_for(kind, sizes)
    x, ws, bs = F.build_layer(sizes, 32, False, seed, row, key, True)
    if kin == 128:
        x, ws = x[:, 128:].contiguous(), [w_[:, 128:].contiguous() for w_ in ws]
    return x, ws, bs, who


def make_plan(dev, sizes, loops):
    from diffassemble_amd.graph_plan import build_plan
    from oracle import weights as W
    ei, batch = W.collate([W.dense_edge_index(n, loops) for n in sizes], sizes)
    return build_plan(ei.to(dev), batch.to(dev), 0)


def run_conv(plan, x, ws, bs, level):
    """da_conv_dense_ex (the conv-level entry, Q rows pre-scaled by the caller) with the switch at `level` (see proj_switch), on a scratch
    of our own: returns (layer output [N, 256], Q rows [H, N, 32], skip rows [N, 256], launch counters)."""
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    dev = plan.row_map.device
    xb = x.to(dev).bfloat16().contiguous()
    wb = torch.cat(ws).to(dev).bfloat16().contiguous()
    bb = torch.cat(bs).to(dev).float().contiguous()
    g = plan.c_struct(need_csr=False)
    lib = _lib.lib()
    N, HC = xb.shape[0], H * 32
    nbytes = int(lib.da_attn_dense_scratch_bytes(_lib.PREC_BF16, C.byref(g), H, 32))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((N, HC), dtype=torch.bfloat16, device=dev)
    with proj_switch(level), torch.cuda.device(dev):
        E.launch_counters(reset=True)
        _lib.check(lib.da_conv_dense_ex(_lib.PREC_BF16, C.byref(g), H, 32, xb.shape[1], _lib.ptr(xb), _lib.ptr(wb), _lib.ptr(bb), None, 0,
                                        _lib.ptr(out), _lib.ptr(scratch), _lib.CONV_Q_PRESCALED, _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        cnt = E.launch_counters(reset=True)
    n_pad = int(plan.n_pad)
    hb = -(-((n_pad + 64) * HC * 2) // 256) * 256          # one region of the scratch: Q | K | V | skip (da_conv_dense_ex)
    q = scratch[:H * n_pad * 64].view(torch.bfloat16).view(H, n_pad, 32)[:, plan.row_map[:N].long()]
    s = scratch[3 * hb:3 * hb + N * HC * 2].view(torch.bfloat16).view(N, HC)
    return out.cpu(), q.cpu(), s.cpu(), cnt


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


SHAPES = [[512], [513], [900], [960], [1216], [640, 900]]


@pytest.mark.parametrize("loops", [True, False], ids=["self_loops", "no_diagonal"])
@pytest.mark.parametrize("kin", [256, 128])
@pytest.mark.parametrize("sizes", SHAPES, ids=["512", "513", "900", "960", "1216", "640_900"])
def test_prologue_projection_equals_the_two_kernel_layer_bit_for_bit(dev, sizes, kin, loops):
    """512: sixteen slabs, no wave has a second one, the Q / skip weights sit BEHIND the image; 513: seventeen, exactly one wave has a
    second slab and it holds one valid row; 900: 29 slabs, a 4-row last slab, 60 padded rows in the last stage; 960: fifteen full
    stages, the largest image beside the weights at a reduction of 256; 1216: beyond the LDS (stays on the projection kernel);
    640 + 900: ragged, slots at their own offsets (no uniform padding)."""
    x, ws, bs, _ = layer_inputs(sizes, kin)
    plan = make_plan(dev, sizes, loops)
    o2, q2, s2, c2 = run_conv(plan, x, ws, bs, 2)
    o3, q3, s3, c3 = run_conv(plan, x, ws, bs, 3)
    assert c2["resident_launches"] == 1 and c2["resident_projection_launches"] == 0, c2
    assert c3["resident_launches"] == 1, c3
    assert c3["resident_projection_launches"] == (1 if takes(max(sizes), kin) else 0), c3      # 1: no projection kernel ran
    assert torch.isfinite(o3.float()).all()
    assert same_bits(q3, q2), float((q3.float() - q2.float()).abs().max())
    assert same_bits(s3, s2), float((s3.float() - s2.float()).abs().max())
    assert same_bits(o3, o2), float((o3.float() - o2.float()).abs().max())
    if kin == 256 and sizes == [900]:          # ... and the layer is the TransformerConv layer (fp64 PyG formula, the resident kernel's tolerance)
        assert F.rel(o3.float(), F.reference(x, ws, bs, sizes, loops, 32, False, True)) < 1e-2


def test_per_wave_fallback_on_keys_projected_in_place(dev):
    """One key near the end of every graph at +115 (the `late_outlier` construction): row sums leave the optimistic window, every wave
    re-runs its slab with the running-max recurrence -- over the K | V rows its workgroup projected into LDS."""
    from diffassemble_amd import engine as E
    sizes = [900, 640]
    x, ws, bs, who = layer_inputs(sizes, 256, kind="late_outlier", seed=0)
    assert who == "all"
    plan = make_plan(dev, sizes, True)
    o2, q2, s2, _ = run_conv(plan, x, ws, bs, 2)
    E.debug_counters(reset=True)
    o3, q3, s3, c3 = run_conv(plan, x, ws, bs, 3)
    # (run_conv's launch-counter read reset the fallback counters with everything else: count the re-runs in a run of their own)
    with proj_switch(3):
        E.debug_counters(reset=True)
        out = E.conv_dense_ex(plan, x.to(dev), torch.cat(ws).to(dev), torch.cat(bs).to(dev), H, 32, None, 0, "bf16", prescale_q="done", folded=False)
        torch.cuda.synchronize()
        cnt = E.debug_counters(reset=True)
    assert c3["resident_projection_launches"] == 1, c3
    assert cnt["opt_gen_workgroups"] > 0, cnt
    assert same_bits(o3, o2) and same_bits(q3, q2) and same_bits(s3, s2)
    assert same_bits(out.cpu(), o3)
    assert F.rel(o3.float(), F.reference(x, ws, bs, sizes, True, 32, False, True)) < 1e-2


def test_small_and_hybrid_batches_keep_their_kernels_with_the_switch_on(dev):
    from diffassemble_amd import engine as E
    from diffassemble_amd.graph_plan import build_plan
    # 144-piece puzzles: the ring kernel behind the projection kernel
    sizes = [144] * 4
    x, ws, bs, _ = layer_inputs(sizes, 256)
    plan = make_plan(dev, sizes, True)
    o2, q2, s2, c2 = run_conv(plan, x, ws, bs, 2)
    o3, q3, s3, c3 = run_conv(plan, x, ws, bs, 3)
    assert c3["resident_launches"] == 0 and c3["resident_projection_launches"] == 0, c3
    assert same_bits(o3, o2) and same_bits(q3, q2) and same_bits(s3, s2)
    # a hybrid Batch with a graph of resident size: the adjacency-masked kernel behind the projection kernel
    sizes = [600, 200]
    x, ws, bs, _ = layer_inputs(sizes, 256)
    ei, batch = F.hybrid_graph(sizes, 7)
    plan = build_plan(ei.to(dev), batch.to(dev), 0, hybrid="force")
    assert plan.hybrid == 1
    outs = []
    for level in (2, 3):
        with proj_switch(level):
            E.launch_counters(reset=True)
            o = E.conv_dense_ex(plan, x.to(dev), torch.cat(ws).to(dev), torch.cat(bs).to(dev), H, 32, None, 0, "bf16", prescale_q="done", folded=False)
            torch.cuda.synchronize()
            cnt = E.launch_counters(reset=True)
        assert cnt["resident_launches"] == 0 and cnt["resident_projection_launches"] == 0, (level, cnt)
        outs.append(o.cpu())
    assert same_bits(outs[0], outs[1])
    assert F.rel(outs[1].float(), F.reference_edges(x, ws, bs, ei, 32, False, True)) < 1e-2


def test_900_piece_forward_and_ddim_trajectory_fixtures_with_the_switch_on_and_off(dev):
    """The reference's own 900-piece forward and DDIM trajectory (tests/golden/golden_v2.npz), bf16, with the switch on and off: both inside
    the fixtures' tolerance, and equal to each other bit for bit.  A denoiser keeps the setting it was CREATED with: the one created with the
    switch on still projects in the attention kernel after the switch went off, the one created with it off never does."""
    import cases as CS
    from diffassemble_amd import DenoiserEngine, Schedule, _lib
    from diffassemble_amd import engine as E
    from oracle import diffusion as ODF
    import test_gpu_benched_mode as B
    golden2 = CS.load_golden2()
    spec = CS.by_name("rot900_g1")
    case = CS.build_case(spec)
    lp = CS.LOOPS2D_BIG[0]
    assert lp["base"] == "rot900_g1"
    sch = Schedule(ODF.make_schedule(lp["T"]), dev)
    x0 = torch.from_numpy(golden2[f"{lp['name']}/x_init"]).to(dev)
    res = {}
    for level in (3, 2):
        with proj_switch(level):
            eng = DenoiserEngine(case["sd"], variant="2d", arch=spec["arch"], virt_nodes=spec["V"], precision="bf16", device=dev)
            plan = eng.plan(case["edge_index"], case["batch"])
            E.launch_counters(reset=True)
            out = eng.forward(plan, case["x"].to(dev), case["t"].to(dev), case["feats"].to(dev))
            torch.cuda.synchronize()
            cnt = E.launch_counters(reset=True)
            traj, _ = eng.sample_loop(plan, sch, x0, case["feats"].to(dev), ratio=lp["ratio"], mean_type=_lib.MEAN_START_X,
                                      max_iters=lp["max_iters"], use_graph=True)
            torch.cuda.synchronize()
        with proj_switch(5 - level):          # the other setting: the denoiser's snapshot decides, not the switch at call time
            E.launch_counters(reset=True)
            out_b = eng.forward(plan, case["x"].to(dev), case["t"].to(dev), case["feats"].to(dev))
            torch.cuda.synchronize()
            cnt_b = E.launch_counters(reset=True)
        assert cnt["resident_launches"] > 0, cnt
        assert (cnt["resident_projection_launches"] > 0) == (level == 3), (level, cnt)
        assert cnt_b == cnt, (level, cnt, cnt_b)
        assert torch.equal(out_b, out)
        assert B.rel(out, golden2["rot900_g1/out"]) < B.RTOLBF, (level, B.rel(out, golden2["rot900_g1/out"]))
        assert B.rel(traj, golden2[f"{lp['name']}/imgs"]) < B.RTOLBF, (level, B.rel(traj, golden2[f"{lp['name']}/imgs"]))
        res[level] = (out.cpu(), traj.cpu())
    assert torch.equal(res[3][0], res[2][0])
    assert torch.equal(res[3][1], res[2][1])
