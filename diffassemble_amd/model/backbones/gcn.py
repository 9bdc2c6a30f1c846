"""Counterpart of puzzle_diff/model/backbones/gcn.py:5-22 (``GCN``): two PyG ``GCNConv`` layers with default settings,
GELU after each, ``(x, None)`` out.  Parameter names match PyG's (``lin.weight`` without a bias, ``bias`` added after
the aggregation) so reference checkpoints load unchanged.  Inside ``Eff_GAT`` / ``Eff_GAT_3d`` the stack runs in the one
``da_denoiser_forward`` call; ``forward`` here is the standalone layer pair through the kernel-level ABI."""
import torch
import torch.nn as nn

from ... import _lib
from ... import engine as E
from ...graph_plan import build_plan


class GCNConv(nn.Module):
    """Parameter holder of one PyG ``GCNConv(in_channels, out_channels)`` (add_self_loops, normalize, bias: the defaults)."""

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        if kwargs.get("improved") or kwargs.get("cached") or kwargs.get("add_self_loops") is False \
                or kwargs.get("normalize") is False or kwargs.get("bias") is False:
            raise NotImplementedError("only the configuration the reference uses (PyG defaults) is supported")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.xavier_uniform_(self.lin.weight)             # PyG: glorot weight, zero bias
        nn.init.zeros_(self.bias)


class GCN(nn.Module):
    arch = "gcn"
    virt_nodes = 0

    def __init__(self, input_size, hidden_dim, output_size) -> None:
        super().__init__()
        self.module_list = nn.ModuleList([GCNConv(input_size, out_channels=hidden_dim),
                                          GCNConv(hidden_dim, out_channels=output_size)])

    @torch.no_grad()
    def forward(self, x, edge_index, batch=None, *args, precision="fp32"):
        """gcn.py:16-22 through da_linear + da_gcn_aggregate: conv 0 projects, then aggregates (bias + GELU fused);
        conv 1 aggregates, then projects (bias + GELU in the GEMM epilogue) -- both aggregations at the hidden width."""
        if batch is None:
            batch = torch.zeros(x.shape[0], dtype=torch.long, device=x.device)
        plan = build_plan(edge_index, batch, 0, hybrid="off")
        c0, c1 = self.module_list
        p = E.linear(x, c0.lin.weight, None, _lib.ACT_NONE, None, precision)
        h = E.gcn_aggregate(plan, p, c0.bias, _lib.ACT_GELU, precision)
        y = E.gcn_aggregate(plan, h, None, _lib.ACT_NONE, precision)
        return E.linear(y, c1.lin.weight, c1.bias, _lib.ACT_GELU, None, precision).float(), None
