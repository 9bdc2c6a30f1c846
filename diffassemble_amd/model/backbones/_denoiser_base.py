"""Shared engine plumbing of ``Eff_GAT`` / ``Eff_GAT_3d``: lazily packs the module's
parameters into a ``DenoiserEngine`` (HIP library), caches the graph plan of the current
Batch and the staged piece features so the T sampling steps of one Batch re-use them."""
import os

import torch
import torch.nn as nn

from ...engine import DenoiserEngine
from ...train import DenoiserTrainFn, TrainEngine


def default_precision():
    return os.environ.get("DIFFASSEMBLE_PRECISION", "bf16")


class _Held:
    """Cache key over caller tensors that cannot go stale: it keeps a strong reference to every keyed
    tensor, so the caching allocator cannot hand their addresses to a different same-shaped tensor while
    the entry lives, and then compares (address, shape, stride, dtype, ``_version``) -- ``_version`` is
    shared by all views of a storage, so in-place edits through any alias miss.  (A key on ``data_ptr``
    alone hit for the NEXT Batch of a Lightning loop: batch i is freed before batch i+1 is moved to the
    device and gets the same addresses with ``_version == 0`` -- a fresh random expander per sample,
    puzzle_dataset.py:194-212, silently ran on the previous sample's plan.)"""

    __slots__ = ("tensors", "sig", "extra")

    def __init__(self, tensors, extra=()):
        self.tensors = tuple(tensors)
        self.sig = tuple(self._sig(t) for t in self.tensors)
        self.extra = tuple(extra)

    @staticmethod
    def _sig(t):
        return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype, t._version)

    def matches(self, tensors, extra=()):
        return (len(tensors) == len(self.tensors) and tuple(extra) == self.extra
                and all(self._sig(t) == s for t, s in zip(tensors, self.sig)))


class DenoiserBase(nn.Module):
    variant = "2d"

    def _denoiser_state(self):
        skip = ("visual_backbone.", "pcd_backbone.", "linear1.", "linear2.", "mean", "std")
        return {k: v for k, v in self.state_dict().items() if not k.startswith(skip)}

    def _param_version(self):
        # the fused optimizer updates the flat parameter buffer through a raw pointer (no ``_version``
        # bump): its step counter is part of the key, so packed inference weights never outlive a step
        te = getattr(self, "_train_engine", None)
        return (tuple((p.data_ptr(), p._version) for p in self.parameters()), te.version if te is not None else 0)

    def engine(self, device=None, precision=None) -> DenoiserEngine:
        """The packed HIP denoiser for the module's CURRENT parameters (rebuilt when a
        parameter was modified in place, moved, or the precision changed)."""
        precision = precision or getattr(self, "precision", None) or default_precision()
        device = torch.device(device) if device is not None else next(self.parameters()).device
        key = (self._param_version(), precision, str(device))
        if getattr(self, "_engine_key", None) != key:
            gnn = self.gnn_backbone
            self._engine = DenoiserEngine(self._denoiser_state(), variant=self.variant, arch=gnn.arch,
                                          virt_nodes=getattr(gnn, "virt_nodes", 0), precision=precision,
                                          device=device)
            self._engine_key = key
            self._plan_key = self._feat_key = None
        return self._engine

    def _plan_for(self, eng, edge_index, batch, expander=None):
        """``expander=(perms [G, n], degree)``: the Batch's graphs are Exphander graphs described by their permutations
        (diffassemble_amd.expander); the plan is then built in closed form and ``edge_index`` may be None."""
        key = getattr(self, "_plan_key", None)
        if expander is not None:
            perms, degree = expander
            if key is None or not key.matches((perms,), (id(eng), "expander", int(degree))):
                self._plan = eng.plan_expander(perms, degree)
                self._plan_key = _Held((perms,), (id(eng), "expander", int(degree)))
                self._feat_key = None
            return self._plan
        if key is None or not key.matches((edge_index, batch), (id(eng),)):
            self._plan = eng.plan(edge_index, batch)
            self._plan_key = _Held((edge_index, batch), (id(eng),))
            self._feat_key = None
        return self._plan

    def _release_dense_plan_key(self):
        """After a whole sampling loop ran off a DENSE plan: stop pinning the Batch's edge list.  The plan of a complete graph does
        not need it (graph_plan.py), but the cache key and the plan hold the caller's int64 ``edge_index`` alive -- 830 MB for 64 dense
        900-piece puzzles -- until the NEXT Batch is planned, i.e. two Batches' edge lists would be resident at the peak of a
        validation loop.  The next call re-plans (~4 ms per 64 x 900 Batch, against a 76 ms loop)."""
        plan = getattr(self, "_plan", None)
        if plan is not None and getattr(plan, "dense", 0):
            # the engine keeps the plan object alive for its cached hipGraph (device arrays of the plan), so the edge list has to
            # leave the plan itself; nothing reads it again (alpha is only returned by the per-step path, which plans afresh)
            plan._edge_index = None

            def _gone():
                raise RuntimeError("this GraphPlan's edge list was released after its sampling loop (complete graphs do not "
                                   "need it); plan the Batch again to get attention weights / a CSR")
            plan.edge_index_fn = _gone
            self._plan_key = self._feat_key = None
            self._plan = None

    def _stage_features(self, eng, plan, feats):
        key = getattr(self, "_feat_key", None)
        if key is None or not key.matches((feats,), (id(plan),)):
            eng.set_features(plan, feats)
            self._feat_key = _Held((feats,), (id(plan),))

    def train_engine(self, device=None) -> TrainEngine:
        """Flat-buffer training engine (diffassemble_amd/train.py); rebinds the live parameters as views
        of one flat fp32 buffer the first time (and again if their storage was replaced)."""
        te = getattr(self, "_train_engine", None)
        if te is None or not te.still_bound():
            te = TrainEngine(self, device if device is not None else next(self.parameters()).device)
            self._train_engine = te
        return te

    def _wants_grad(self):
        return self.training and torch.is_grad_enabled() and self.time_emb.weight.requires_grad

    def _run_train(self, xy_pos, time, edge_index, feats, batch):
        """forward_with_feats under autograd: da_train_forward now, da_train_backward when the loss is
        back-propagated (attention weights are not returned on this path, as p_losses asks)."""
        te = self.train_engine(xy_pos.device)
        key = getattr(self, "_tplan_key", None)
        if key is None or not key.matches((edge_index, batch), (id(te),)):
            from ...graph_plan import build_plan
            # (the GCN aggregates complete graphs in closed form and everything else over the CSR: no hybrid split)
            self._tplan = build_plan(edge_index.to(te.device), batch.to(te.device), te.virt_nodes,
                                     hybrid="off" if te.arch == "gcn" else None).with_source_csr()
            self._tplan_key = _Held((edge_index, batch), (id(te),))
        out = DenoiserTrainFn.apply(te, self._tplan, xy_pos, time, feats, te.anchor)
        return out, None

    @torch.no_grad()
    def _run(self, xy_pos, time, edge_index, feats, batch, return_attentions=True):
        eng = self.engine(xy_pos.device)
        plan = self._plan_for(eng, edge_index, batch)
        self._stage_features(eng, plan, feats)
        all_layers = self.gnn_backbone.arch == "transformer"
        if self.gnn_backbone.arch == "gcn":         # GCN.forward returns (x, None) (gcn.py:22): no attention weights
            return eng.forward(plan, xy_pos, time, None), None
        if return_attentions:
            out, alpha = eng.forward(plan, xy_pos, time, None, return_alpha=True, alpha_all_layers=all_layers)
            attentions = ([(plan.edge_index, alpha[l]) for l in range(alpha.shape[0])] if all_layers
                          else [(plan.edge_index, alpha)])
        else:
            out = eng.forward(plan, xy_pos, time, None)
            attentions = None
        return out, attentions
