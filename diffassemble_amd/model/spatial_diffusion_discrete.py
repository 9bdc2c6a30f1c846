"""Counterpart of puzzle_diff/model/spatial_diffusion_discrete.py: ``GNN_Diffusion`` of the discrete position diffusion (D3PM
with the uniform transition over ``backbones.Eff_GAT_Discrete``), with the reference's constructor, attributes and Lightning
hooks: inference (forward, reverse step, the captured sampling loop with classifier-free guidance, validation / test / predict
steps) and training (``q_sample``, ``p_losses``, ``vb_terms_bpd``, ``training_step``), both on a ROCm device only -- off the
device the training methods raise ``NotImplementedError``, as the project has no CPU path.

* ``forward_with_feats`` -> one ``da_denoiser_forward_idx`` call; under grad ``da_train_forward_idx`` / ``da_train_backward_idx``
* ``p_sample_ddpm``      -> forward (two under guidance) + ``da_d3pm_step``
* ``p_sample_loop``      -> ``da_sample_loop_idx``: every iteration enqueued by one C call, replayed as one hipGraph launch
* ``q_sample``           -> ``da_d3pm_q_sample``: the uniforms are drawn inside the kernel, no [N, K] buffer
* ``p_losses``           -> noising, the denoiser's training forward, and ``da_d3pm_loss``: the loss and its gradient with respect
                            to the logits in one call (variational bound, label-smoothed cross entropy, or their hybrid)

Differences from the reference, on purpose:
* no ``Q_onestep`` / ``Q_onestep_transpose`` / ``overline_Q`` buffers ([steps, K, K] fp32 each: 1.9 GB at K = 900, steps = 600).
  For the uniform kernel ``overline_Q[t] = a_t I + (1 - a_t) / K 11^T`` with ``a_t = alphas_cumprod[t]`` and
  ``overline_Q[t] overline_Q[p]^-1 = r I + (1 - r) / K 11^T`` with ``r = a_t / a_p``: the reverse step needs two scalars per
  node.  A reference checkpoint that carries the three tables loads: the keys are dropped;
* the closed form is evaluated instead of fp32 matrix products and ``torch.linalg.inv`` (the reference's inverse
  loses digits at steps = 600; the closed form is the exact one);
* the Gumbel uniforms of the captured loop come from a counter-based generator inside the step kernel (seeded from torch's
  generator once per loop), not from one ``torch.rand`` call per step: the draws differ from the reference's stream;
* ``validation_step`` dumps no images, and ``training_step`` runs no ``batch_idx == 0`` sampling-and-image dump;
* training: the noising uniforms come from the same counter-based generator (its training domain), seeded from torch's generator
  once per ``p_losses`` call; the reference's unused ``noise`` argument of ``p_losses`` carries injected [N, K] uniforms, and the
  extensions ``cfg_rand`` ([G] uniforms of the classifier-free mask) and ``patch_feats`` (encoder bypass) exist for parity runs;
* K comes from the module: the reference's ``one_hot(x_start)`` infers it from the data and fails on a Batch that lacks index
  K - 1; here such a Batch trains like any other;
* with ``classifier_free_prob == 0`` no mask is drawn (the reference draws ``rand(G) > 0``, which drops a puzzle's features with
  probability 2^-24);
* the ``+1e-6`` that ``categorical_kl_logits`` adds to both logit vectors cancels inside the softmaxes and is not reproduced.
"""
import torch
import torch.nn.functional as F

from . import backbones
from . import spatial_diffusion as sd

_Q_TABLES = ("Q_onestep", "Q_onestep_transpose", "overline_Q")
_NOT_BUILT = "discrete training is not built yet"
_OFF_DEVICE = _NOT_BUILT + " off the device: it runs on ROCm tensors only (diffassemble_amd has no CPU path)"
_LOSS_TYPES = ("vb", "cross_entropy", "hybrid")


def _require_device(message, *tensors):
    """The training methods' guard: every argument must be a tensor on a ROCm device."""
    if not tensors or not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise NotImplementedError(message)


class _D3pmLoss(torch.autograd.Function):
    """The discrete p_losses' loss with its gradient with respect to the logits computed in the SAME call (da_d3pm_loss), like
    ``spatial_diffusion._FusedLoss``: backward is one scaling by the upstream gradient.  Returns (total, {total, vb, ce})."""

    @staticmethod
    def forward(ctx, logits, sched, x_start, x_t, t, kind, lambda_loss):
        from ..engine import d3pm_loss
        loss, d_logits, _ = d3pm_loss(sched, logits, x_start, x_t, t, kind, lambda_loss)
        ctx.save_for_backward(d_logits)
        parts = loss.clone()
        ctx.mark_non_differentiable(parts)
        return loss[0].clone(), parts

    @staticmethod
    def backward(ctx, g, _g_parts):
        (d_logits,) = ctx.saved_tensors
        return d_logits * g, None, None, None, None, None, None


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
                                                output_channels=self.output_channels, use_hip_encoder=self.use_hip_encoder)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a reference checkpoint carries the three [steps, K, K] transition tables; this module has their closed form instead
        for k in _Q_TABLES:
            state_dict.pop(prefix + k, None)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ------------------------------------------------------------------ training side (ROCm device only)
    def _train_seed_tensor(self, device):
        """The persistent {seed, offset} pair the noising kernel reads, refilled by one draw from torch's generator per call (what
        ``DenoiserEngine.seed_tensor`` does for the sampling loop)."""
        s = getattr(self, "_train_seed", None)
        if s is None or s.device != device:
            s = self._train_seed = torch.zeros(2, dtype=torch.int64, device=device)
        s.random_()
        return s

    def _draw_t(self, batch):
        """training_step's timesteps: one draw per puzzle, gathered to the pieces ([N] int64)."""
        batch_size = batch.batch.max().item() + 1
        t = torch.randint(0, self.steps, (batch_size,), device=self.device).long()
        return torch.gather(t, 0, batch.batch)

    def _cfg_mask(self, patch_feats, batch, cfg_rand=None):
        """p_losses' classifier-free mask: the features of the puzzles whose uniform is <= ``classifier_free_prob`` are zeroed;
        ``cfg_rand`` [G] given or drawn (not drawn at all with ``classifier_free_prob == 0``)."""
        if cfg_rand is None and not self.classifier_free_prob > 0.0:
            return patch_feats
        if cfg_rand is None:
            cfg_rand = torch.rand(int(batch.max()) + 1, device=batch.device)
        keep = cfg_rand.to(batch.device)[batch] > self.classifier_free_prob
        return keep[:, None] * patch_feats

    def training_step(self, batch=None, batch_idx=0):
        """spatial_diffusion_discrete.py:93-141 without the ``batch_idx == 0`` sampling-and-image dump."""
        if batch is None or not hasattr(batch, "batch"):
            raise NotImplementedError(_OFF_DEVICE)
        _require_device(_OFF_DEVICE, batch.batch, batch.indexes)
        loss = self.p_losses(batch.indexes % self.K, self._draw_t(batch), loss_type=self.loss_type, cond=batch.patches,
                             edge_index=batch.edge_index, batch=batch.batch, patch_feats=getattr(batch, "patch_feats", None))
        self.log("loss", loss)
        return loss

    def q_sample(self, x_start=None, t=None, overline_Q=None, eps=1e-9, noise=None):
        """spatial_diffusion_discrete.py:181-191 in closed form (da_d3pm_q_sample): ``x_start`` [N] indices (or the reference's one-hot
        [N, K]), ``t`` [N] -> x_t [N] int64.  ``noise`` (extension): the [N, K] uniforms; default: drawn inside the kernel."""
        _require_device(_OFF_DEVICE, x_start, t)
        if overline_Q is not None or eps != 1e-9:
            raise NotImplementedError("q_sample: explicit transition tables / another eps are not supported (closed form only)")
        if x_start.dim() == 2:
            x_start = x_start.argmax(-1)
        from ..engine import d3pm_q_sample
        seed = None if noise is not None else self._train_seed_tensor(x_start.device)
        return d3pm_q_sample(self._schedule(), x_start, t, self.K, noise=noise, seed=seed)

    def vb_terms_bpd(self, pred_x_start_logits=None, model_logits=None, x_start=None, x_t=None, t=None, K=None, overline_Q=None):
        """spatial_diffusion_discrete.py:416-472 (da_d3pm_loss, kind vb): mean over the pieces of KL(q(x_{t-1} | x_t, x_0) ||
        p(x_{t-1} | x_t)) / ln 2, the decoder NLL where t == 0; differentiable with respect to ``pred_x_start_logits``.
        ``model_logits`` is accepted for the reference's signature and not read: the kernel forms the model posterior from the
        predicted logits itself (q_posterior_logits at previous_t = t - 1)."""
        _require_device(_OFF_DEVICE, pred_x_start_logits, x_start, x_t, t)
        if overline_Q is not None or (K is not None and K != self.K):
            raise NotImplementedError("vb_terms_bpd: explicit transition tables / another K are not supported (closed form only)")
        return _D3pmLoss.apply(pred_x_start_logits, self._schedule(), x_start, x_t, t, "vb", float(self.lambda_loss))[0]

    def p_losses(self, x_start=None, t=None, noise=None, loss_type="l1", cond=None, edge_index=None, batch=None, cfg_rand=None,
                 patch_feats=None):
        """spatial_diffusion_discrete.py:229-273.  ``x_start`` [N] position indices, ``t`` [N].  ``noise`` (unused by the reference):
        the [N, K] uniforms of the noising for parity runs, default in-kernel draws; ``cfg_rand`` (extension): the [G] uniforms of
        the classifier-free mask; ``patch_feats`` (extension) bypasses the piece encoder.  The three parts {total, vb, ce} of the
        last call stay in ``self.last_loss_parts`` (a [3] device tensor)."""
        _require_device(_OFF_DEVICE, x_start, t)
        if loss_type not in _LOSS_TYPES:
            raise Exception("Loss not implemented %s", loss_type)
        _require_device(_OFF_DEVICE, edge_index, batch)
        x_noisy = self.q_sample(x_start, t, noise=noise)
        if patch_feats is None:
            patch_feats = self.visual_features(cond)
        patch_feats = self._cfg_mask(patch_feats, batch, cfg_rand)
        prediction = self.forward_with_feats(x_noisy, t, cond, edge_index, patch_feats=patch_feats, batch=batch)
        loss, parts = _D3pmLoss.apply(prediction, self._schedule(), x_start, x_noisy, t, loss_type, float(self.lambda_loss))
        self.last_loss_parts = parts
        return loss

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
        self._score(batch, pred == batch.indexes.to(pred.device) % self.K)
        return pred

    def _score(self, batch, ok):
        """``_eval_step``'s bookkeeping from the per-piece flags ``ok`` [N] (device): the per-graph "all correct" reduction, the
        single host copy, and the metric updates."""
        dev = ok.device
        dims = batch.patches_dim.to(dev).long().reshape(-1, 2)
        G = dims.shape[0]
        wrong = torch.zeros(G, dtype=torch.long, device=dev).index_add_(0, batch.batch.to(dev), (~ok).long())
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
