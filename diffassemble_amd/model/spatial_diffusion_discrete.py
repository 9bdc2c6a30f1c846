"""Counterpart of puzzle_diff/model/spatial_diffusion_discrete.py: ``GNN_Diffusion`` of the discrete position diffusion (D3PM
with the uniform transition over ``backbones.Eff_GAT_Discrete``), with the reference's constructor, attributes and Lightning
hooks.  INFERENCE is built -- forward, reverse step, the captured sampling loop with classifier-free guidance, validation /
test / predict steps; the training side (``p_losses``, ``q_sample``, ``vb_terms_bpd``, ``training_step``) raises
``NotImplementedError``.

* ``forward_with_feats`` -> one ``da_denoiser_forward_idx`` call
* ``p_sample_ddpm``      -> forward (two under guidance) + ``da_d3pm_step``
* ``p_sample_loop``      -> ``da_sample_loop_idx``: every iteration enqueued by one C call, replayed as one hipGraph launch

Differences from the reference, on purpose:
* no ``Q_onestep`` / ``Q_onestep_transpose`` / ``overline_Q`` buffers ([steps, K, K] fp32 each: 1.9 GB at K = 900, steps = 600).
  For the uniform kernel ``overline_Q[t] = a_t I + (1 - a_t) / K 11^T`` with ``a_t = alphas_cumprod[t]`` and
  ``overline_Q[t] overline_Q[p]^-1 = r I + (1 - r) / K 11^T`` with ``r = a_t / a_p``: the reverse step needs two scalars per
  node.  A reference checkpoint that carries the three tables loads: the keys are dropped;
* the closed form is evaluated instead of fp32 matrix products and ``torch.linalg.inv`` (the reference's inverse
  loses digits at steps = 600; the closed form is the exact one);
* the Gumbel uniforms of the captured loop come from a counter-based generator inside the step kernel (seeded from torch's
  generator once per loop), not from one ``torch.rand`` call per step: the draws differ from the reference's stream;
* ``validation_step`` dumps no images.
"""
import torch
import torch.nn.functional as F

from . import backbones
from . import spatial_diffusion as sd

_Q_TABLES = ("Q_onestep", "Q_onestep_transpose", "overline_Q")
_NOT_BUILT = "discrete training is not built yet"


class GNN_Diffusion(sd.GNN_Diffusion):
    def __init__(self, puzzle_sizes, loss_type="vb", lambda_loss=0.01, *args, **kwargs):
        K = puzzle_sizes[0][0] * puzzle_sizes[0][1]
        if "input_channels" not in kwargs:
            kwargs["input_channels"] = K
        if "output_channels" not in kwargs:
            kwargs["output_channels"] = K
        super().__init__(*args, **kwargs)
        self.lambda_loss = lambda_loss
        self.puzzle_sizes = puzzle_sizes[0]
        self.loss_type = loss_type
        self.K = K
        self.discrete = True
        self.save_hyperparameters()

    def init_backbone(self):
        self.model = backbones.Eff_GAT_Discrete(steps=self.steps, input_channels=self.input_channels,
                                                output_channels=self.output_channels)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a reference checkpoint carries the three [steps, K, K] transition tables; this module has their closed form instead
        for k in _Q_TABLES:
            state_dict.pop(prefix + k, None)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ------------------------------------------------------------------ training side: not built
    def training_step(self, batch, batch_idx):
        raise NotImplementedError(_NOT_BUILT)

    def p_losses(self, *args, **kwargs):
        raise NotImplementedError(_NOT_BUILT)

    def q_sample(self, *args, **kwargs):
        raise NotImplementedError(_NOT_BUILT)

    def vb_terms_bpd(self, *args, **kwargs):
        raise NotImplementedError(_NOT_BUILT)

    # ------------------------------------------------------------------ reverse process
    def q_posterior_logits(self, x_t, x_start_logits, t, previous_t, K=None, overline_Q=None, eps=1e-8, use_x_start_logits=True):
        """spatial_diffusion_discrete.py:193-227 in closed form (module docstring): plain torch, evaluated in fp64 from the fp32
        ``alphas_cumprod`` buffer and returned in the dtype of ``x_start_logits``.  The product path runs da_d3pm_step."""
        if overline_Q is not None:
            raise NotImplementedError("q_posterior_logits: explicit transition tables are not supported (closed form only)")
        K = self.K if K is None else K
        x0 = x_start_logits.double()
        ac = self.alphas_cumprod.double()
        a_t, a_p = ac[t], ac[previous_t.clamp(min=0)]
        r = (a_t / a_p)[:, None]
        fact1 = F.one_hot(x_t, K).double() * r + (1.0 - r) / K
        probs = F.softmax(x0, dim=-1) if use_x_start_logits else x0
        fact2 = a_p[:, None] * probs + ((1.0 - a_p) / K)[:, None]
        out = torch.log(fact1 + eps) + torch.log(fact2 + eps)
        tzero = x0 if use_x_start_logits else torch.log(x0 + 1e-8)
        return torch.where(t[:, None] == 0, tzero, out).to(x_start_logits.dtype)

    @torch.no_grad()
    def p_sample_ddpm(self, x, t, t_index, cond, edge_index, patch_feats, batch, noise=None):
        """spatial_diffusion_discrete.py:282-320.  ``noise`` (extension): the step's [N, K] uniforms, default one ``torch.rand``."""
        logits = self.forward_with_feats(x, t, cond, edge_index, patch_feats=patch_feats, batch=batch)
        if self.classifier_free_prob > 0.0:
            unc = self.forward_with_feats(x, t, cond, edge_index, patch_feats=torch.zeros_like(patch_feats), batch=batch)
            logits = (1 + self.classifier_free_w) * logits - self.classifier_free_w * unc
        if noise is None:
            noise = torch.rand(logits.shape, device=logits.device)
        return self.model.engine(x.device).d3pm_step(self._schedule(), x, logits, t, self.inference_ratio, noise=noise)

    @torch.no_grad()
    def p_sample(self, x, t, t_index, cond, edge_index, sampling_func, patch_feats, batch):
        return sampling_func(x, t, t_index, cond, edge_index, patch_feats, batch)

    @torch.no_grad()
    def p_sample_loop(self, shape, cond, edge_index, batch, patch_feats=None):
        """spatial_diffusion_discrete.py:324-356: one ``torch.randint`` draw for the start, ONE library call for the loop; returns
        the list of per-step index tensors (int64 [N]).  ``patch_feats`` may be passed to bypass the encoder."""
        device = self.device
        index = torch.randint(0, self.K, shape, device=device)
        if patch_feats is None:
            patch_feats = self.visual_features(cond)
        eng = self.model.engine(device)
        plan = self.model._plan_for(eng, edge_index, batch)
        self.model._feat_key = None
        cfg_w = float(self.classifier_free_w) if self.classifier_free_prob > 0.0 else None
        traj, _ = eng.sample_loop_idx(plan, self._schedule(), index, patch_feats, ratio=self.inference_ratio, keep_traj=True,
                                      use_graph=self.use_hip_graph, cfg_w=cfg_w)
        self.model._release_dense_plan_key()
        return list(traj.long().unbind(0))

    # ------------------------------------------------------------------ Lightning hooks
    @torch.no_grad()
    def prediction_step(self, batch, batch_idx):
        return self.p_sample_loop(batch.indexes.shape, batch.patches, batch.edge_index, batch=batch.batch,
                                  patch_feats=getattr(batch, "patch_feats", None))

    def predict_step(self, batch, batch_idx, dataloader_idx=0):
        """The index trajectory (the reference only dumps images here, :146-178)."""
        return self.prediction_step(batch, batch_idx)

    @torch.no_grad()
    def _eval_step(self, batch, batch_idx):
        """validation_step / test_step, spatial_diffusion_discrete.py:358-413: a puzzle counts when every piece has its index.
        Per-graph "all correct" is reduced on the device; one host copy per Batch carries it with the per-piece flags and sizes."""
        pred = self.p_sample_loop(batch.indexes.shape, batch.patches, batch.edge_index, batch=batch.batch,
                                  patch_feats=getattr(batch, "patch_feats", None))[-1]
        gt = batch.indexes.to(pred.device) % self.K
        ok = pred == gt
        dims = batch.patches_dim.to(pred.device).long().reshape(-1, 2)
        G = dims.shape[0]
        wrong = torch.zeros(G, dtype=torch.long, device=pred.device).index_add_(0, batch.batch.to(pred.device), (~ok).long())
        host = torch.cat([wrong == 0, ok, dims.flatten()]).cpu()
        correct, piece_ok, dims = host[:G].bool(), host[G:G + ok.numel()].float(), host[G + ok.numel():].reshape(G, 2).tolist()
        if hasattr(self, "metrics"):
            def upd(name, val):
                if name in self.metrics:
                    self.metrics[name].update(val)
            upd("overall__piece_acc", piece_ok)
            for i in range(G):
                key = f"{tuple(dims[i])}"
                upd(f"{key}_nImages", 1)
                upd("overall_nImages", 1)
                upd(f"{key}_acc", int(correct[i]))
                upd("overall_acc", int(correct[i]))
        return pred
