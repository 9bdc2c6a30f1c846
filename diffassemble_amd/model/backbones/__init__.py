"""Counterpart of puzzle_diff/model/backbones/__init__.py:1-8 (minus the import of the
missing ``backbone_vist`` file).  The hot-path denoisers are real, inference and training;
the ablation architectures the drivers merely import are placeholders that fail on construction (out of scope)."""
from .efficient_gat import Eff_GAT
from .efficient_gat_3d import Eff_GAT_3d
from .efficient_gat_discrete import Eff_GAT_Discrete
from .efficient_gat_discrete_rotation import Eff_GAT_Discrete_ROT
from .exophormer_gnn import Exophormer_GNN
from .gcn import GCN, GCNConv
from .Transformer_GNN import Transformer_GNN
from .transformer_conv import TransformerConv


def _out_of_scope(name):
    class _Placeholder:  # noqa: D401
        def __init__(self, *a, **k):
            raise NotImplementedError(
                f"{name} is an ablation architecture outside the accelerated hot path "
                "(SURVEY.md section 2); only its import name is kept for the drivers.")
    _Placeholder.__name__ = name
    return _Placeholder


Dark_TFConv = _out_of_scope("Dark_TFConv")
Eff_GAT_Vist = _out_of_scope("Eff_GAT_Vist")

__all__ = ["Eff_GAT", "Eff_GAT_3d", "Exophormer_GNN", "GCN", "GCNConv", "Transformer_GNN", "TransformerConv",
           "Dark_TFConv", "Eff_GAT_Discrete", "Eff_GAT_Discrete_ROT", "Eff_GAT_Vist"]
