"""The folded last layer with Q projected in the prologue of its attention kernel (k_attn_optt<144, true, false, .., 8192>, da_attn_opt.hip;
da_config.disable_folds bit 256 = DA_FOLD_LAST_QPROJ clear): the projection kernel in front of the attention writes the K | V' columns only
(QkvScatter::col0), every wave of the attention kernel computes the Q fragments of its own 32-query slab on the matrix pipe, and no Q row is
ever written or read.  Same TransformerConv layer as the two-kernel form (reference backbones/Transformer_GNN.py:32,38; PyG lin_query): the
same 16-step MFMA chain per output, the bias behind the reduction, the same pre-scale and the same rounding to bf16, so K, V' and the per-head
outputs must equal the two-kernel layer's (bit 256 set) BIT FOR BIT.  The switch is set in-process (`_lib.set_config`); a denoiser keeps the
setting it was created with.

Layer level: da_conv_dense_ex (DA_CONV_FOLDED_V32 | DA_CONV_Q_PRESCALED, C = 144, Din = 256) on a scratch of our own whose Q region is
pre-filled with a bf16 NaN pattern -- with the bit clear it must come back untouched (nobody wrote it), and the outputs must be finite
(nobody read it).  Built on the helpers of test_gpu_softmax_fallbacks.py."""
import ctypes as C
import gc

import pytest
import torch

import test_gpu_softmax_fallbacks as F

pytestmark = pytest.mark.gpu
H, CH = F.H, 144
FOLD_LAST_QPROJ = 256          # da_config.disable_folds: set = the projection kernel keeps its Q columns (two-kernel form)
NAN_BITS = 0x7FC1              # a bf16 quiet NaN no kernel of the library produces


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


class qproj:
    """`with qproj(True): ...` -- disable_folds bit 256 clear (Q in the attention kernel) or set (two kernels), restored on exit."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from diffassemble_amd import _lib
        self.old = _lib.config().disable_folds
        _lib.set_config(disable_folds=(self.old & ~FOLD_LAST_QPROJ) | (0 if self.on else FOLD_LAST_QPROJ))

    def __exit__(self, *exc):
        from diffassemble_amd import _lib
        _lib.set_config(disable_folds=self.old)


def make_plan(dev, sizes, loops):
    from diffassemble_amd.graph_plan import build_plan
    from oracle import weights as W
    ei, batch = W.collate([W.dense_edge_index(n, loops) for n in sizes], sizes)
    return build_plan(ei.to(dev), batch.to(dev), 0)


def run_layer(plan, x, ws, bs, on):
    """The folded layer with the switch as asked: (per-head outputs [H, N, 32], the scratch's Q region, its K | V' regions, launch counters,
    fallback counters)."""
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    dev = plan.row_map.device
    xb = x.to(dev).bfloat16().contiguous()
    wb = torch.cat(ws).to(dev).bfloat16().contiguous()
    bb = torch.cat(bs).to(dev).float().contiguous()
    g = plan.c_struct(need_csr=False)
    lib = _lib.lib()
    N, HC = xb.shape[0], H * CH
    nbytes = int(lib.da_attn_dense_scratch_bytes(_lib.PREC_BF16, C.byref(g), H, CH))
    hb = -(-((int(plan.n_pad) + 64) * HC * 2) // 256) * 256          # one region of the scratch: Q | K | V' | (skip) (da_conv_dense_ex)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    scratch[:hb].view(torch.int16).fill_(NAN_BITS)
    out = torch.empty((H, N, 32), dtype=torch.bfloat16, device=dev)
    with qproj(on), torch.cuda.device(dev):
        E.launch_counters(reset=True)
        _lib.check(lib.da_conv_dense_ex(_lib.PREC_BF16, C.byref(g), H, CH, xb.shape[1], _lib.ptr(xb), _lib.ptr(wb), _lib.ptr(bb), None, 0,
                                        _lib.ptr(out), _lib.ptr(scratch), _lib.CONV_Q_PRESCALED | _lib.CONV_FOLDED_V32, _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        fell = E.debug_counters(reset=False)
        cnt = E.launch_counters(reset=True)
    return out.cpu(), scratch[:hb].view(torch.int16).cpu(), scratch[hb:3 * hb].cpu(), cnt, fell


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def check_pair(dev, sizes, loops, kind="m44", seed=13):
    row, key, who = F.offsets_for(kind, sizes)
    x, ws, bs = F.build_layer(sizes, CH, True, seed, row, key, True)
    plan = make_plan(dev, sizes, loops)
    o2, q2, kv2, c2, f2 = run_layer(plan, x, ws, bs, False)
    o1, q1, kv1, c1, f1 = run_layer(plan, x, ws, bs, True)
    assert c1["last_qproj_launches"] == 1, c1                        # the form was taken ...
    assert c2["last_qproj_launches"] == 0, c2                        # ... and the other setting did not move the counter
    assert bool((q1 == NAN_BITS).all()), "the Q region was written with the bit clear"
    assert not bool((q2 == NAN_BITS).all())                          # (the two-kernel form does write it: the pattern is a live check)
    assert torch.isfinite(o1.float()).all()
    assert torch.equal(kv1, kv2), "K | V' regions differ"
    assert same_bits(o1, o2), float((o1.float() - o2.float()).abs().max())
    return (x, ws, bs, who), (o1, f1), (o2, f2)


SIZES = [[1], [31], [32], [33], [128], [129], [144], [160], [5, 64, 130], [900]]


@pytest.mark.parametrize("loops", [True, False], ids=["self_loops", "no_diagonal"])
@pytest.mark.parametrize("sizes", SIZES, ids=["_".join(map(str, s)) for s in SIZES])
def test_q_in_the_prologue_equals_the_two_kernel_layer_bit_for_bit(dev, sizes, loops):
    """1: one query, one key; 31 / 32 / 33: a partial slab, a full one, a second slab with one row; 128 / 129: a full query tile, a second tile with one
    query (three waves of it without a slab); 144 / 160: configuration 2's graph, five full slabs; 5 + 64 + 130: ragged, slots at their own
    offsets; 900: the benched graph (29 slabs, a 4-row last slab)."""
    if sizes == [1] and not loops:
        # a lone piece without its self loop is a graph without any edge: no plan calls it dense and da_conv_dense_ex refuses it.  The case runs
        # the piece beside the smallest loop-free graph that has an edge (as test_gpu_softmax_fallbacks does): its only row has NO incoming edge
        sizes = [1, 2]
    (x, ws, bs, _), (o1, _), _ = check_pair(dev, sizes, loops)
    if sizes in ([5, 64, 130], [900]):          # ... and the layer is the TransformerConv layer (fp64 PyG formula, the optimistic kernel's tolerance)
        assert F.rel(o1.float(), F.reference(x, ws, bs, sizes, loops, CH, True, True)) < 1e-2


def test_workgroup_fallback_reuses_the_projected_fragments(dev):
    """Logits outside the optimistic window (every row at -80 log2-units through the carrier columns): the workgroups re-run their tiles with the
    running-max recurrence, on the Q fragments their prologue projected."""
    sizes = [130, 37, 64]
    (x, ws, bs, who), (o1, f1), (o2, f2) = check_pair(dev, sizes, True, kind="m80", seed=0)
    assert who == "all"
    assert f1["opt_gen_workgroups"] > 0, f1
    assert f2["opt_gen_workgroups"] > 0, f2
    assert F.rel(o1.float(), F.reference(x, ws, bs, sizes, True, CH, True, True)) < 1e-2


# ---------------------------------------------------------------------------------------------------------------- denoiser level
def engines_both_settings(dev, cfg_name):
    """(model, engine created with bit 256 clear, engine created with it set) over ONE set of weights."""
    import bench
    from diffassemble_amd import DenoiserEngine
    model = bench.build_module(bench.CONFIGS[cfg_name], dev, "bf16")
    sd = model.model._denoiser_state()
    gnn = model.model.gnn_backbone
    engs = []
    for on in (True, False):
        with qproj(on):
            engs.append(DenoiserEngine(sd, variant=model.model.variant, arch=gnn.arch, virt_nodes=getattr(gnn, "virt_nodes", 0), precision="bf16", device=dev))
    return model, engs[0], engs[1]


def test_denoiser_forward_and_captured_loop_are_bit_identical(dev):
    """A 64- and a 96-piece puzzle, default folds: one forward and one captured 3-step sampling loop per denoiser.  The denoiser's snapshot decides,
    not the switch at call time: both run with the switch at its default."""
    import bench
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    from oracle import weights as W
    sizes = [64, 96]
    model, eng1, eng0 = engines_both_settings(dev, "3p")
    ei, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], sizes)
    gen = torch.Generator(device=dev).manual_seed(11)
    feats = torch.randn((sum(sizes), 1088), generator=gen, device=dev)
    x = torch.randn((sum(sizes), 4), generator=gen, device=dev)
    res = []
    for eng, want in ((eng1, 1), (eng0, 0)):
        plan = eng.plan(ei.to(dev), batch.to(dev))
        E.launch_counters(reset=True)
        out = eng.forward(plan, x, 37, feats)
        torch.cuda.synchronize()
        cnt = E.launch_counters(reset=True)
        assert cnt["last_qproj_launches"] == want, cnt                # one per forward for the denoiser created with the bit clear
        _, xf = eng.sample_loop(plan, model._schedule(), x, feats, ratio=bench.CONFIGS["3p"]["ratio"], mean_type=_lib.MEAN_START_X, max_iters=3,
                                keep_trajectory=False, use_graph=True)
        torch.cuda.synchronize()
        res.append((out.cpu().clone(), xf.cpu().clone()))
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[0][0], res[1][0]), float((res[0][0] - res[1][0]).abs().max())
    assert torch.equal(res[0][1], res[1][1]), float((res[0][1] - res[1][1]).abs().max())
    del eng, eng0, eng1, plan, model          # (the denoisers hold captured graphs: released here, not whenever the collector gets to them)
    gc.collect()


def test_hybrid_batches_and_the_3d_model_keep_their_kernels(dev):
    """A masked (hybrid) Batch and a 3D denoiser, created with the bit clear: the counter does not move."""
    import bench
    from diffassemble_amd import engine as E
    gen = torch.Generator(device=dev).manual_seed(5)
    with qproj(True):
        _, eng, _ = engines_both_settings(dev, "3")
        plan = eng.plan_expander(bench.expander_perms(bench.CONFIGS["3"], 2, 3).to(dev), 90)
        E.launch_counters(reset=True)
        out = eng.forward(plan, torch.randn((plan.n_real, 4), generator=gen, device=dev), 37, torch.randn((plan.n_real, 1088), generator=gen, device=dev))
        torch.cuda.synchronize()
        cnt = E.launch_counters(reset=True)
        assert torch.isfinite(out).all() and cnt["last_qproj_launches"] == 0, cnt
        _, eng3, _ = engines_both_settings(dev, "4")
        ei, batch = bench.dense_batch(2, 20, dev)
        plan3 = eng3.plan(ei, batch)
        E.launch_counters(reset=True)
        out3 = eng3.forward(plan3, torch.randn((plan3.n_real, 7), generator=gen, device=dev), 37, torch.randn((plan3.n_real, 768), generator=gen, device=dev))
        torch.cuda.synchronize()
        cnt3 = E.launch_counters(reset=True)
        assert torch.isfinite(out3).all() and cnt3["last_qproj_launches"] == 0, cnt3
    del eng, eng3, plan, plan3
    gc.collect()
