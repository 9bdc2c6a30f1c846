"""Hidden layers hand their rows to the next layer in MFMA operand order (da_config.disable_folds bit 128 clear; da_conv_dense_ex flags
DA_CONV_X_FM / DA_CONV_OUT_FM): where two consecutive layers are projected by their own attention kernel (k_attn_res<.., 64>, da_attn_opt.hip), the
first one's epilogue stores its rows "fragment-major" (FM) over the padded slots and the second one's prologue reads them so -- every request
of a wave is one contiguous KB instead of 32-byte pieces of 64 rows.  Same TransformerConv layer as every other path (reference
backbones/Transformer_GNN.py:32,38): a change of LAYOUT only, so everything must equal the row-major path bit for bit.

The layout, restated here from its definition and not read back from the library: rows live in the padded slot space (slot of node v =
plan.row_map[v]; a graph's slots start at pad_ptr[g], a multiple of 64); for rows of length L = 16 KS bf16,

    byte offset of x[slot row r][16 s + 8 half + e]  =  ((r >> 5) * KS + s) * 1024  +  (half * 32 + (r & 31)) * 16  +  2 e      (e = 0 .. 7)

Rows behind a graph (slot rows >= n_g): the producer writes zeros into those of a 32-row slab the graph owns and never touches later slabs; the
consumer must not care what they hold (every FM input here carries NaN bits there)."""
import ctypes as C
import types

import pytest
import torch

import test_gpu_attn_qsf as Q
import test_gpu_softmax_fallbacks as F

H = F.H
HC = H * 32
NAN_BITS = 0x7FC0          # a bf16 quiet NaN, as int16
FOLD_ATTN_PROJ, FOLD_X_FM = 64, 128          # da_config.disable_folds
CONV_X_FM, CONV_OUT_FM = 4, 8                # da_conv_dense_ex flags (include/diffassemble_hip.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- host side of the layout
def slot_rows(x_rows, plan, fill=0):
    """[N, L] bf16 node rows -> [n_pad, L] int16 slot rows; slots without a node hold `fill`."""
    n = x_rows.shape[0]
    rows = torch.full((int(plan.n_pad), x_rows.shape[1]), fill, dtype=torch.int16)
    rows[plan.row_map[:n].long().cpu()] = x_rows.cpu().contiguous().view(torch.int16)
    return rows


def to_fm(x_rows, plan, kin, fill=0):
    """Node rows [N, kin] (bf16) -> the FM buffer over the plan's padded slots, flat int16 [n_pad * kin]: element index
    ((r >> 5) * KS + s) * 512 + (half * 32 + (r & 31)) * 8 + e, i.e. the axes [slab][s][half][r & 31][e]."""
    assert x_rows.shape[1] == kin and kin % 16 == 0 and int(plan.n_pad) % 32 == 0
    rows = slot_rows(x_rows, plan, fill)
    return rows.view(int(plan.n_pad) // 32, 32, kin // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def from_fm(buf, plan, kin):
    """The inverse: flat FM buffer -> (node rows [N, kin] bf16, all slot rows [n_pad, kin] int16)."""
    n_pad = int(plan.n_pad)
    rows = buf.cpu().view(torch.int16).view(n_pad // 32, kin // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).contiguous().view(n_pad, kin)
    n = int(plan.graph_ptr[-1])
    return rows[plan.row_map[:n].long().cpu()].view(torch.bfloat16), rows


def host_plan(sizes):
    """The slot tables of a Batch of complete graphs, by hand (64-aligned slots, nodes in order): what to_fm / from_fm read of a plan."""
    gp, pp = [0], [0]
    for n in sizes:
        gp.append(gp[-1] + n)
        pp.append(pp[-1] + (n + 63) // 64 * 64)
    row_map = torch.cat([torch.arange(n) + pp[g] for g, n in enumerate(sizes)]).to(torch.int32)
    return types.SimpleNamespace(n_pad=pp[-1], row_map=row_map, graph_ptr=torch.tensor(gp, dtype=torch.int32), pad_ptr=torch.tensor(pp, dtype=torch.int32))


def test_host_round_trip_and_the_layout_formula():
    plan = host_plan([640, 900])          # ragged: the second graph's slots start at 640, its nodes at 640 too, n_pad 1600
    g = torch.Generator().manual_seed(5)
    for kin in (256, 128):
        x = torch.randn(1540, kin, generator=g).bfloat16()
        buf = to_fm(x, plan, kin, fill=NAN_BITS)
        back, rows = from_fm(buf, plan, kin)
        assert torch.equal(back.view(torch.int16), x.view(torch.int16))
        assert (rows[1540:] == NAN_BITS).all() and buf.numel() == 1600 * kin
    # the formula, literally, on one 2-slab graph (40 pieces in a 64-row slot), reduction 128
    plan, kin, ks = host_plan([40]), 128, 8
    x = torch.randn(40, kin, generator=g).bfloat16()
    buf = to_fm(x, plan, kin, fill=NAN_BITS)
    xi = x.view(torch.int16)
    for r in range(64):
        for s in range(ks):
            for half in range(2):
                byte = ((r >> 5) * ks + s) * 1024 + (half * 32 + (r & 31)) * 16
                got = buf[byte // 2:byte // 2 + 8]
                want = xi[r, 16 * s + 8 * half:16 * s + 8 * half + 8] if r < 40 else torch.full((8,), NAN_BITS, dtype=torch.int16)
                assert torch.equal(got, want), (r, s, half)


# ---------------------------------------------------------------------------------------------------------------- layer level
def run_conv_fm(plan, x, ws, bs, x_fm, out_fm):
    """da_conv_dense_ex with the projection in the attention kernel (Q.proj_switch(3)) and the given layout flags; FM input carries NaN bits in
    every slot row without a node, the output buffer is NaN bits all over.  Returns (output node rows [N, 256] bf16, all output slot rows
    (FM output) or None, Q rows, counters)."""
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    dev = plan.row_map.device
    kin = x.shape[1]
    xb = x.bfloat16()
    xin = to_fm(xb, plan, kin, fill=NAN_BITS).to(dev) if x_fm else xb.to(dev).contiguous()
    wb = torch.cat(ws).to(dev).bfloat16().contiguous()
    bb = torch.cat(bs).to(dev).float().contiguous()
    g = plan.c_struct(need_csr=False)
    lib = _lib.lib()
    N, n_pad = x.shape[0], int(plan.n_pad)
    scratch = torch.zeros(int(lib.da_attn_dense_scratch_bytes(_lib.PREC_BF16, C.byref(g), H, 32)), dtype=torch.uint8, device=dev)
    out = torch.full(((n_pad if out_fm else N) * HC,), NAN_BITS, dtype=torch.int16, device=dev)
    flags = _lib.CONV_Q_PRESCALED | (CONV_X_FM if x_fm else 0) | (CONV_OUT_FM if out_fm else 0)
    with Q.proj_switch(3), torch.cuda.device(dev):
        E.launch_counters(reset=True)
        rc = lib.da_conv_dense_ex(_lib.PREC_BF16, C.byref(g), H, 32, kin, _lib.ptr(xin), _lib.ptr(wb), _lib.ptr(bb), None, 0, _lib.ptr(out),
                                  _lib.ptr(scratch), flags, _lib.stream_ptr(dev))
        err = lib.da_last_error() if rc else b""
        torch.cuda.synchronize()
        cnt = E.launch_counters(reset=True)
    if rc:
        return rc, err, cnt, out.cpu()
    q = scratch[:H * n_pad * 64].view(torch.bfloat16).view(H, n_pad, 32)[:, plan.row_map[:N].long()].cpu()
    if out_fm:
        o, rows = from_fm(out, plan, HC)
    else:
        o, rows = out.cpu().view(torch.bfloat16).view(N, HC), None
    return o, rows, q, cnt


_plain = {}


def plain(dev, sizes, kin, loops):
    """The row-major call (the existing test's level 3), once per shape: (plan, inputs, output, Q rows)."""
    key = (tuple(sizes), kin, loops)
    if key not in _plain:
        x, ws, bs, _ = Q.layer_inputs(sizes, kin)
        plan = Q.make_plan(dev, sizes, loops)
        o, q, _, c = Q.run_conv(plan, x, ws, bs, 3)
        assert c["resident_projection_launches"] == 1 and c["resident_fm_input_launches"] == 0, c
        _plain[key] = (plan, (x, ws, bs), o, q)
    return _plain[key]


@pytest.mark.gpu
@pytest.mark.parametrize("loops", [True, False], ids=["self_loops", "no_diagonal"])
@pytest.mark.parametrize("kin", [256, 128])
@pytest.mark.parametrize("sizes", [[512], [513], [900], [960], [640, 900]], ids=["512", "513", "900", "960", "640_900"])
def test_fm_layer_equals_the_row_major_layer_bit_for_bit(dev, sizes, kin, loops):
    """513: a second slab holding one valid row; 900: a 4-row last slab and 60 padded rows in the last stage; 640 + 900: ragged slot offsets
    (pad0 / 32 differs from node0 / 32); 512: the weights behind the image; 960: no padded row at all.  Both flags, then each alone."""
    plan, (x, ws, bs), o0, q0 = plain(dev, sizes, kin, loops)
    for x_fm, out_fm in ((True, True), (True, False), (False, True)):
        o, rows, q, cnt = run_conv_fm(plan, x, ws, bs, x_fm, out_fm)
        assert cnt["resident_launches"] == 1 and cnt["resident_projection_launches"] == 1, (x_fm, out_fm, cnt)
        assert cnt["resident_fm_input_launches"] == (1 if x_fm else 0), (x_fm, out_fm, cnt)
        assert torch.isfinite(o.float()).all(), (x_fm, out_fm)
        assert Q.same_bits(q, q0), (x_fm, out_fm, float((q.float() - q0.float()).abs().max()))
        assert Q.same_bits(o, o0), (x_fm, out_fm, float((o.float() - o0.float()).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[513], [900]], ids=["513", "900"])
def test_producer_zeroes_the_padding_rows_of_slabs_it_owns(dev, sizes):
    """Output NaN bits all over before the launch: afterwards slot rows n_g .. of the graph's last 32-row slab are zeros, the slabs behind it still
    hold the NaN bits (nobody owns them), every row of a node is finite."""
    plan, (x, ws, bs), o0, _ = plain(dev, sizes, 256, True)
    o, rows, _, _ = run_conv_fm(plan, x, ws, bs, False, True)
    assert Q.same_bits(o, o0)
    n_g, slot = sizes[0], int(plan.n_pad)
    owned = (n_g + 31) // 32 * 32
    assert owned > n_g and slot > owned
    assert torch.isfinite(rows[:n_g].view(torch.bfloat16).float()).all()
    assert (rows[n_g:owned] == 0).all()
    assert (rows[owned:] == NAN_BITS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[1216], [144]], ids=["1216", "144"])
@pytest.mark.parametrize("flag", ["DA_CONV_X_FM", "DA_CONV_OUT_FM"])
def test_fm_flags_are_rejected_where_the_layer_is_not_projected_in_its_attention_kernel(dev, sizes, flag):
    """1216 pieces are beyond the LDS (the projection kernel stays), 144 below the resident kernel's range: an error that names the flag, no launch."""
    x, ws, bs, _ = Q.layer_inputs(sizes, 256)
    plan = Q.make_plan(dev, sizes, True)
    rc, err, cnt, out = run_conv_fm(plan, x, ws, bs, flag == "DA_CONV_X_FM", flag == "DA_CONV_OUT_FM")
    assert isinstance(rc, int) and rc != 0
    assert flag.encode() in err, err
    assert cnt["resident_launches"] == 0 and cnt["resident_projection_launches"] == 0 and cnt["resident_fm_input_launches"] == 0, cnt
    assert (out == NAN_BITS).all()          # nothing was written


# ---------------------------------------------------------------------------------------------------------------- denoiser level
class folds:
    """`with folds(x_fm=True): ...` -- disable_folds with bit 64 clear (layers projected by their attention kernel) and bit 128 as asked."""

    def __init__(self, x_fm):
        self.x_fm = x_fm

    def __enter__(self):
        from diffassemble_amd import _lib
        self.old = _lib.config().disable_folds
        _lib.set_config(disable_folds=(self.old & ~(FOLD_ATTN_PROJ | FOLD_X_FM)) | (0 if self.x_fm else FOLD_X_FM))

    def __exit__(self, *exc):
        from diffassemble_amd import _lib
        _lib.set_config(disable_folds=self.old)


def forward_both_settings(dev, cfg_name, make_plan):
    """One forward per setting of bit 128, a denoiser created per setting: ((output, counters) with the bit clear, (...) with it set)."""
    import bench
    from diffassemble_amd import DenoiserEngine
    from diffassemble_amd import engine as E
    cfg = bench.CONFIGS[cfg_name]
    model = bench.build_module(cfg, dev, "bf16")
    sd = model.model._denoiser_state()
    gnn = model.model.gnn_backbone
    res = []
    for x_fm in (True, False):
        with folds(x_fm):
            eng = DenoiserEngine(sd, variant=model.model.variant, arch=gnn.arch, virt_nodes=getattr(gnn, "virt_nodes", 0), precision="bf16", device=dev)
        plan = make_plan(eng)
        gen = torch.Generator(device=dev).manual_seed(11)
        feats = torch.randn((plan.n_real, 1088), generator=gen, device=dev)
        x = torch.randn((plan.n_real, 4), generator=gen, device=dev)
        E.launch_counters(reset=True)
        out = eng.forward(plan, x, 37, feats)
        torch.cuda.synchronize()
        res.append((out.cpu(), E.launch_counters(reset=True)))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[900, 900], [640, 900]], ids=["900_900", "640_900"])
def test_denoiser_forward_is_bit_identical_with_the_rows_handed_over_fragment_major(dev, sizes):
    """Three hidden layers projected by their attention kernel; layers 1 and 2 read what layers 0 and 1 wrote fragment-major (the first conv's
    input and the last hidden layer's output stay row-major)."""
    import bench
    from oracle import weights as W

    def make_plan(eng):
        ei, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], sizes)
        return eng.plan(ei.to(dev), batch.to(dev))

    (o1, c1), (o0, c0) = forward_both_settings(dev, "3p", make_plan)
    assert c1["resident_projection_launches"] == 3 and c1["resident_fm_input_launches"] == 2, c1
    assert c0["resident_projection_launches"] == 3 and c0["resident_fm_input_launches"] == 0, c0
    assert torch.isfinite(o1).all()
    assert torch.equal(o1, o0), float((o1 - o0).abs().max())


@pytest.mark.gpu
def test_small_and_hybrid_batches_are_untouched_by_the_switch(dev):
    import bench

    def small(eng):
        ei, batch = bench.dense_batch(4, 144, dev)
        return eng.plan(ei, batch)

    def hybrid(eng):
        perms = bench.expander_perms(bench.CONFIGS["3"], 2, 3).to(dev)
        return eng.plan_expander(perms, 90)

    for cfg_name, make_plan in (("3p", small), ("3", hybrid)):
        (o1, c1), (o0, c0) = forward_both_settings(dev, cfg_name, make_plan)
        assert c1["resident_fm_input_launches"] == 0 and c0["resident_fm_input_launches"] == 0, (cfg_name, c1, c0)
        assert c1 == c0, (cfg_name, c1, c0)
        assert torch.isfinite(o1).all() and torch.equal(o1, o0), cfg_name
