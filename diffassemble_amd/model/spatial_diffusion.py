"""Counterpart of puzzle_diff/model/spatial_diffusion.py: ``GNN_Diffusion`` with the same
constructor kwargs, mutable attributes, state-dict keys (``betas`` ... ``posterior_variance``,
``model.*``) and Lightning hooks, with the per-timestep denoiser and the
sampling loop running in the HIP library:

* ``forward_with_feats``  -> one ``da_denoiser_forward`` call
* ``p_sample_ddim/ddpm``  -> forward + ``da_ddim_step`` / ``da_ddpm_step``
* ``p_sample_loop``       -> ``da_sample_loop``: all T iterations enqueued by one C call and
                            replayed as ONE hipGraph launch (no per-step host syncs; the
                            reference's ``(prev_timestep >= 0).all()`` branches, :535,560, are
                            resolved on the host per iteration index at capture time).

Differences from the reference, on purpose:
* attention weights are returned per step only when ``self.return_attentions`` is True
  (the reference keeps T x 4 x [E, 8] floats that no caller reads; ~10 GB at 900 pieces);
* ``sampling="DDPM"`` works in ``p_sample_loop`` (the reference raises ``ValueError: too
  many values to unpack``, :504-510 vs :663; tests/golden pins that failure mode).
"""
import enum
import os
from functools import partial
from typing import Any

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .. import _lib
from ..engine import Schedule
from ._lightning_compat import LightningModule, MeanMetric, SumMetric
from .backbones import Eff_GAT


class ModelMeanType(enum.Enum):
    """spatial_diffusion.py:58-66 (same members and values, so pickled hparams load)."""
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelScheduler(enum.Enum):
    """spatial_diffusion.py:69-73."""
    LINEAR = enum.auto()
    COSINE = enum.auto()
    COSINE_DISCRETE = enum.auto()


def cosine_discrete_beta_schedule(timesteps, s=0.08):
    steps = timesteps + 1
    t = torch.linspace(0, timesteps, steps)
    ac = lambda t: torch.cos(((t / timesteps) + s) / (1 + s) + np.pi / 2)  # noqa: E731
    betas = 1 - ac(t + 1) / ac(t)
    return torch.clip(betas, 0.0001, 0.9999)


def cosine_beta_schedule(timesteps, s=0.08):
    steps = timesteps + 1
    x = torch.linspace(0, timesteps, steps)
    ac = torch.cos(((x / timesteps) + s) / (1 + s) * np.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0.0001, 0.9999)


def linear_beta_schedule(timesteps):
    return torch.linspace(0.0001, 0.02, timesteps)


def extract(a, t, x_shape=None):
    return a.gather(-1, t)[:, None]


def greedy_cost_assignment(pos1: torch.Tensor, pos2: torch.Tensor) -> torch.Tensor:
    """Same result as the reference's TorchScript loop (spatial_diffusion.py:179-216: repeatedly
    take the globally smallest remaining distance, retire its row and column) without the
    per-assignment ``.item()`` syncs.  ROCm tensors: the device kernel; CPU tensors: one
    stable sort of all pairs, then a single pass (host glue for tests).  int64 [min(n, m), 3]."""
    if pos1.is_cuda:                                   # one launch, no host round trips (da_greedy_assign)
        from ..engine import greedy_assign
        return greedy_assign(pos1, pos2)[: min(pos1.shape[0], pos2.shape[0])]
    dist = torch.norm(pos1[:, None] - pos2, dim=2)
    n, m = dist.shape
    # the reference's dist[mask].min() returns the FIRST minimum in row-major order: stable sort
    order = torch.sort(dist.flatten(), stable=True)[1].cpu().numpy()
    dist_c = dist.flatten().cpu()
    row_used, col_used = np.zeros(n, bool), np.zeros(m, bool)
    out = []
    for f in order:
        i, j = divmod(int(f), m)
        if row_used[i] or col_used[j]:
            continue
        row_used[i] = col_used[j] = True
        out.append((i, j, int(dist_c[f])))          # assignments tensor is int64: value truncated
        if len(out) == min(n, m):
            break
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 3)


_LOSS_KIND = {"l1": 0, "l2": 1, "huber": 2}


def _glue_on_device(*tensors):
    """The training-side glue kernels take contiguous fp32 (poses) / int64 (timesteps) tensors on a ROCm device; anything else keeps torch."""
    return all(t.is_cuda and t.dtype in (torch.float32, torch.int64) for t in tensors)


class _FusedLoss(torch.autograd.Function):
    """F.l1_loss / F.mse_loss / F.smooth_l1_loss(target, prediction) (mean reduction) of p_losses, spatial_diffusion.py:470-480, with the gradient
    with respect to the prediction computed in the SAME launch (da_loss_grad): backward is one scaling by the upstream gradient."""

    @staticmethod
    def forward(ctx, prediction, target, kind):
        from .. import _lib
        p, t = prediction.detach().contiguous(), target.detach().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        d_pred = torch.empty_like(p)
        _lib.check(_lib.lib().da_loss_grad(int(kind), p.numel(), _lib.ptr(t), _lib.ptr(p), _lib.ptr(loss), _lib.ptr(d_pred), _lib.stream_ptr(p.device)))
        ctx.save_for_backward(d_pred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_pred,) = ctx.saved_tensors
        return d_pred * g, None, None


class GNN_Diffusion(LightningModule):
    def __init__(self, steps=600, inference_ratio=1, sampling="DDPM", learning_rate=1e-4,
                 save_and_sample_every=1000, bb=None, classifier_free_prob=0, classifier_free_w=0,
                 noise_weight=0.0, rotation=False, model_mean_type: ModelMeanType = ModelMeanType.EPSILON,
                 input_channels=2, output_channels=2, scheduler: ModelScheduler = ModelScheduler.LINEAR,
                 visual_pretrained: bool = True, freeze_backbone: bool = True, backbone: str = "efficientnet_b0",
                 n_layers: int = 4, architecture: str = "transformer", virt_nodes: int = 4,
                 all_equivariant=False, use_hip_encoder=False, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.use_hip_encoder = use_hip_encoder      # backbone="efficientnet_b0": the in-tree HIP encoder instead of timm's (Eff_GAT)
        self.visual_pretrained = visual_pretrained
        self.free_backbone = freeze_backbone
        self.model_mean_type = model_mean_type
        self.learning_rate = learning_rate
        self.save_and_sample_every = save_and_sample_every
        self.classifier_free_prob = classifier_free_prob
        self.classifier_free_w = classifier_free_w
        self.noise_weight = noise_weight
        self.rotation = rotation
        self.virt_nodes = virt_nodes
        self.all_equivariant = all_equivariant
        self.save_eval_images = False
        self.return_attentions = False      # see module docstring
        self.use_hip_graph = True
        self.sampling = sampling
        if sampling == "DDPM":
            self.inference_ratio = inference_ratio
            self.p_sample = partial(self.p_sample, sampling_func=self.p_sample_ddpm)
            self.eta = 1
        elif sampling == "DDIM":
            self.inference_ratio = inference_ratio
            self.p_sample = partial(self.p_sample, sampling_func=self.p_sample_ddim)
            self.eta = 0
        betas = {ModelScheduler.LINEAR: linear_beta_schedule, ModelScheduler.COSINE: cosine_beta_schedule,
                 ModelScheduler.COSINE_DISCRETE: cosine_discrete_beta_schedule}[scheduler](timesteps=steps)
        # buffers: same op order as spatial_diffusion.py:282-321 so fp32 values are bit-identical
        self.register_buffer("betas", betas)
        alphas = 1.0 - self.betas
        self.register_buffer("alphas", alphas)
        alphas_cumprod = torch.cumprod(self.alphas, axis=0)
        self.register_buffer("alphas_cumprod", alphas_cumprod)
        self.register_buffer("alphas_cumprod_prev", F.pad(self.alphas_cumprod[:-1], (1, 0), value=1.0))
        self.register_buffer("sqrt_recip_alphas", torch.sqrt(1.0 / self.alphas))
        self.register_buffer("sqrt_alphas_cumprod", torch.sqrt(self.alphas_cumprod))
        self.register_buffer("sqrt_recip_alphas_cumprod",
                             torch.from_numpy(np.sqrt((1.0 / self.alphas_cumprod).numpy())))
        self.register_buffer("sqrt_recipm1_alphas_cumprod",
                             torch.from_numpy(np.sqrt((1.0 / self.alphas_cumprod - 1).numpy())))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - self.alphas_cumprod))
        self.register_buffer("posterior_variance",
                             self.betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod))
        self.steps = steps
        self.input_channels = input_channels
        self.output_channels = output_channels
        self.backbone = backbone
        self.n_layers = n_layers
        self.architecture = architecture
        self.init_backbone()
        self.save_hyperparameters()

    def init_backbone(self):
        """spatial_diffusion.py:334-357."""
        extra = 2 if self.rotation else 0
        kw = dict(steps=self.steps, input_channels=self.input_channels + extra,
                  output_channels=self.output_channels + extra, model=self.backbone,
                  architecture=self.architecture, n_layers=self.n_layers, virt_nodes=self.virt_nodes,
                  use_hip_encoder=self.use_hip_encoder)
        if self.rotation:
            self.model = Eff_GAT(all_equivariant=self.all_equivariant, **kw)
        else:
            self.model = Eff_GAT(visual_pretrained=self.visual_pretrained, freeze_backbone=self.free_backbone, **kw)

    def initialize_torchmetrics(self, n_patches):
        metrics = {}
        for i in n_patches:
            metrics[f"{i}_acc"] = MeanMetric()
            metrics[f"{i}__piece_acc"] = MeanMetric()
            metrics[f"{i}_nImages"] = SumMetric()
        metrics["overall_acc"] = MeanMetric()
        metrics["overall__piece_acc"] = MeanMetric()
        metrics["overall_nImages"] = SumMetric()
        self.metrics = nn.ModuleDict(metrics)

    # ------------------------------------------------------------------ operators
    def _mean_type(self):
        return _lib.MEAN_START_X if self.model_mean_type == ModelMeanType.START_X else _lib.MEAN_EPSILON

    def _schedule(self):
        key = (self.betas.data_ptr(), str(self.betas.device), self.steps)
        if getattr(self, "_sched_key", None) != key:
            self._sched = Schedule({k: getattr(self, k) for k in Schedule.KEYS}, self.betas.device)
            self._sched_key = key
        return self._sched

    def forward(self, xy_pos, time, patch_rgb, edge_index, batch) -> Any:
        return self.model(xy_pos, time, patch_rgb, edge_index, batch)

    def forward_with_feats(self, xy_pos: Tensor, time: Tensor, patch_rgb: Tensor, edge_index: Tensor,
                           patch_feats: Tensor, batch, return_attentions=False) -> Any:
        """spatial_diffusion.py:393-408."""
        self.model.return_attentions = bool(return_attentions)
        out, attentions = self.model.forward_with_feats(xy_pos, time, patch_rgb, edge_index, patch_feats, batch)
        if return_attentions:
            return out, attentions
        return out

    def visual_features(self, patch_rgb):
        return self.model.visual_features(patch_rgb)

    def q_sample(self, x_start, t, noise=None):
        """spatial_diffusion.py:421-430 (training-side elementwise glue)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        if _glue_on_device(x_start, noise, t) and x_start.dim() == 2 and t.shape[0] == x_start.shape[0] and not x_start.requires_grad:
            # one library launch instead of two gathers, two broadcasts, two products and a sum (bit-identical: da_q_sample)
            from .. import _lib
            out = torch.empty_like(x_start)
            _lib.check(_lib.lib().da_q_sample(int(self.sqrt_alphas_cumprod.numel()), x_start.shape[0], x_start.shape[1],
                                              _lib.ptr(self.sqrt_alphas_cumprod), _lib.ptr(self.sqrt_one_minus_alphas_cumprod),
                                              _lib.ptr(x_start.contiguous()), _lib.ptr(noise.contiguous()), _lib.ptr(t.contiguous()),
                                              _lib.ptr(out), _lib.stream_ptr(x_start.device)))
            return out
        return (extract(self.sqrt_alphas_cumprod, t) * x_start
                + extract(self.sqrt_one_minus_alphas_cumprod, t) * noise)

    def p_losses(self, x_start, t, noise=None, loss_type="l1", cond=None, edge_index=None, batch=None,
                 patch_feats=None):
        """spatial_diffusion.py:432-483.  The denoiser forward AND backward run in the HIP library
        (da_train_forward / da_train_backward through ``DenoiserTrainFn``); the loss on [N, c] stays in
        torch, like the reference.  ``patch_feats`` (extension) bypasses the piece encoder."""
        if noise is None:
            noise = torch.randn_like(x_start)
        x_noisy = self.q_sample(x_start=x_start, t=t, noise=noise)
        if self.steps == 1:
            x_noisy = torch.zeros_like(x_noisy)
        if patch_feats is None:
            patch_feats = self.visual_features(cond)
        prediction = self.forward_with_feats(x_noisy, t, cond, edge_index, patch_feats=patch_feats, batch=batch,
                                             return_attentions=False)
        target = {ModelMeanType.START_X: x_start, ModelMeanType.EPSILON: noise}[self.model_mean_type]
        if loss_type in _LOSS_KIND and _glue_on_device(target, prediction) and not target.requires_grad and target.shape == prediction.shape:
            return _FusedLoss.apply(prediction, target, _LOSS_KIND[loss_type])          # loss + its gradient in one launch (da_loss_grad)
        if loss_type == "l1":
            return F.l1_loss(target, prediction)
        if loss_type == "l2":
            return F.mse_loss(target, prediction)
        if loss_type == "huber":
            return F.smooth_l1_loss(target, prediction)
        raise NotImplementedError()

    @torch.no_grad()
    def p_sample_ddpm(self, x, t, t_index, cond, edge_index, patch_feats, batch):
        """spatial_diffusion.py:485-510 (returns a bare tensor, like the reference)."""
        out = self.forward_with_feats(x, t, cond, edge_index, patch_feats=patch_feats, batch=batch)
        noise = None if t_index == 0 else torch.randn_like(x)
        return self.model.engine(x.device).ddpm_step(self._schedule(), x, out, t, noise)

    @torch.no_grad()
    def p_sample_ddim(self, x, t, t_index, cond, edge_index, patch_feats, batch):
        """spatial_diffusion.py:548-627."""
        want_att = self.return_attentions
        r = self.forward_with_feats(x, t, cond, edge_index, patch_feats=patch_feats, batch=batch,
                                    return_attentions=want_att)
        model_output, attentions = r if want_att else (r, None)
        if self.classifier_free_prob > 0.0:
            unc = self.forward_with_feats(x, t, cond, edge_index, patch_feats=torch.zeros_like(patch_feats),
                                          batch=batch)
            model_output = (1 + self.classifier_free_w) * model_output - self.classifier_free_w * unc
        noise = torch.randn_like(x) if self.eta > 0 else None
        prev = self.model.engine(x.device).ddim_step(self._schedule(), x, model_output, t, self.inference_ratio,
                                                     self._mean_type(), float(self.eta), noise)
        return prev, attentions

    @torch.no_grad()
    def p_sample_loop(self, shape, cond, edge_index, batch, patch_feats=None, expander=None):
        """spatial_diffusion.py:635-676.  ``patch_feats`` may be passed to bypass the encoder; ``expander=(perms, degree)``
        (extension): the graphs are Exphander graphs given by their permutations -- planned in closed form on
        the device, ``edge_index`` may then be None on the hipGraph fast path."""
        device = self.device
        img = torch.randn(shape, device=device) * self.noise_weight
        if patch_feats is None:
            patch_feats = self.visual_features(cond)
        its = list(reversed(range(0, self.steps, self.inference_ratio)))
        # one C call (a hipGraph replay) for every sampler of the reference: DDIM (eta >= 0), DDPM, with or without
        # classifier-free guidance; only a request for the attention weights needs the per-step path below
        if not self.return_attentions:
            from .. import _lib
            eng = self.model.engine(device)
            plan = self.model._plan_for(eng, edge_index, batch, expander)
            self.model._feat_key = None
            cfg_w = float(self.classifier_free_w) if self.classifier_free_prob > 0.0 and self.sampling == "DDIM" else None
            traj = None
            # the captured loop's unconditional pass rides on the hoisted mlp.0 share (zero features = the bias), which exists on
            # the MFMA path only (da_denoiser_flags bit 3): without it (DA_DISABLE_MFMA=1) guidance takes the per-step path below,
            # which runs the second pass through forward_with_feats on zero features
            if cfg_w is None or (int(eng.flags) & 8):
                try:
                    traj, _ = eng.sample_loop(plan, self._schedule(), img, patch_feats, ratio=self.inference_ratio,
                                              mean_type=self._mean_type(), keep_trajectory=True,
                                              use_graph=self.use_hip_graph, sampler=self.sampling, eta=float(self.eta), cfg_w=cfg_w)
                except _lib.DaError as e:
                    # second line of defence behind flag bit 3 (which mirrors launch_gemm_mfma's shape conditions): only the
                    # library's own "hoisted path not available" refusal falls back to the per-step guidance path
                    if cfg_w is None or "unconditional pass" not in str(e):
                        raise
                    traj = None
            if traj is not None:
                self.model._release_dense_plan_key()          # do not pin this Batch's edge list until the next one is planned
                return list(traj.clone().unbind(0)), [None] * len(its)
        imgs, attentions = [], []
        b = shape[0]
        for i in its:
            t = torch.full((b,), i, device=device, dtype=torch.long)
            if self.sampling == "DDPM":
                img, atts = self.p_sample_ddpm(img, t, i, cond, edge_index, patch_feats, batch), None
            else:
                img, atts = self.p_sample_ddim(img, t, i, cond, edge_index, patch_feats, batch)
            attentions.append(atts)
            imgs.append(img)
        return imgs, attentions

    @torch.no_grad()
    def p_sample(self, x, t, t_index, cond, edge_index, sampling_func, patch_feats, batch):
        return sampling_func(x, t, t_index, cond, edge_index, patch_feats, batch)

    @torch.no_grad()
    def sample(self, image_size, batch_size=16, channels=3, cond=None, edge_index=None, batch=None):
        return self.p_sample_loop(shape=(batch_size, channels, image_size, image_size), cond=cond,
                                  edge_index=edge_index, batch=batch)

    # ------------------------------------------------------------------ Lightning hooks (callers)
    def configure_optimizers(self):
        """spatial_diffusion.py:701-705: Adafactor with transformers' defaults.  On a ROCm device the denoiser's update
        runs as one library call over the training engine's flat buffers (``FusedAdafactor`` -> da_adafactor_step); with
        a piece encoder attached its parameters take a second library call (``HybridAdafactor`` -> ``FusedAdafactorND`` -> da_adafactor_nd_step).  Set the class / instance
        attribute ``fused_optimizer = False`` for transformers' own implementation throughout."""
        fused = bool(getattr(self, "fused_optimizer", True))
        if fused and self.device.type == "cuda" and getattr(self.model, "visual_backbone", None) is None:
            from ..train import FusedAdafactor
            return FusedAdafactor(self.parameters(), self.model.train_engine(self.device))
        if fused and self.device.type == "cuda":
            # trainable piece encoder attached: fused update for the denoiser's flat buffer, FusedAdafactorND (same rule, by pointer) for the rest
            from ..train import HybridAdafactor
            return HybridAdafactor(self.parameters(), self.model.train_engine(self.device))
        from transformers.optimization import Adafactor
        return Adafactor(self.parameters())

    def sync_gradients(self):
        """Data-parallel gradient exchange of the denoiser: one fused all-reduce of the training
        engine's flat gradient buffer over RCCL/xGMI.  Lightning calls it through ``on_before_optimizer_step``
        (once per optimizer step, after gradient accumulation); hand-written loops call it between
        ``loss.backward()`` and ``optimizer.step()`` (``FusedAdafactor.step`` does it by itself)."""
        te = getattr(self.model, "_train_engine", None)
        if te is not None:
            te.sync_gradients()
        enc = getattr(self.model, "visual_backbone", None)
        if enc is not None and getattr(enc, "_train_engine", None) is not None:
            # the encoder's HIP backward also writes param.grad directly: one more flat all-reduce (11 M values)
            from ..sharding import allreduce_gradients
            import torch.distributed as dist
            multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
            if multi and enc._train_engine.grads_attached():
                allreduce_gradients(enc._train_engine.flat_grad, average=True)      # the gradients ARE views of this buffer
                return
            grads = [p.grad for p in enc.parameters() if p.grad is not None]
            if grads and multi:
                flat = torch.cat([g.reshape(-1) for g in grads])
                allreduce_gradients(flat, average=True)
                off = 0
                for g in grads:
                    g.copy_(flat[off:off + g.numel()].view_as(g))
                    off += g.numel()

    def on_before_optimizer_step(self, optimizer=None, *args, **kwargs):
        """The reference relies on ``pl.Trainer(strategy="ddp")`` (train_script.py:215-218) to average
        gradients.  The HIP backward writes ``param.grad`` directly (DenoiserTrainFn returns no autograd
        gradients), so a DDP wrapper's reducer hooks never fire for these parameters: with one process per
        GPU and ``torch.distributed`` initialised (Lightning's DDP strategy does both; its wrapper leaves
        parameters it saw no gradient for untouched under ``find_unused_parameters=True``, the "ddp" default
        of the Lightning versions the reference pins) the exchange happens HERE, as one all-reduce."""
        self.sync_gradients()

    def training_step(self, batch, batch_idx):
        """spatial_diffusion.py:707-766 (image dumps omitted)."""
        batch_size = batch.batch.max().item() + 1
        t = torch.randint(0, self.steps, (batch_size,), device=self.device).long()
        new_t = torch.gather(t, 0, batch.batch)
        loss = self.p_losses(batch.x, new_t, loss_type="huber", cond=batch.patches,
                             edge_index=batch.edge_index, batch=batch.batch)
        self.log("loss", loss)
        return loss

    @torch.no_grad()
    def prediction_step(self, batch, batch_idx):
        return self.p_sample_loop(batch.x.shape, batch.patches, batch.edge_index, batch=batch.batch,
                                  expander=self._expander_of(batch))

    @staticmethod
    def _expander_of(batch):
        """(perms [G, n], degree) when the dataset attached the Exphander permutations to the Batch
        (``expander_perm`` [G * n] as PyG collates a per-sample [n] attribute, ``expander_degree``), else None."""
        perm = getattr(batch, "expander_perm", None)
        if perm is None:
            return None
        G = int(batch.batch.max()) + 1
        deg = getattr(batch, "expander_degree")
        deg = int(deg[0]) if torch.is_tensor(deg) else int(deg)
        return perm.view(G, -1), deg

    def predict_step(self, batch, batch_idx, dataloader_idx=0):
        return self.prediction_step(batch, batch_idx)

    @torch.no_grad()
    def _eval_step(self, batch, batch_idx):
        """validation_step / test_step, spatial_diffusion.py:775-903,915-: sampling loop, greedy
        assignment of predicted positions to the grid, puzzle / piece accuracy.  The whole Batch is scored by one
        ``score2d.batch_scores`` call (da_score2d); the metrics are updated from its one host copy.  With
        ``save_eval_images`` (:957-971) every step of the loop is then rendered for every puzzle (da_render2d) and
        handed to ``save_eval_frame``; off, the default, nothing of that runs."""
        imgs, _ = self.p_sample_loop(batch.x.shape, batch.patches, batch.edge_index, batch=batch.batch,
                                     patch_feats=getattr(batch, "patch_feats", None), expander=self._expander_of(batch))
        img = imgs[-1]
        from ..score2d import batch_scores
        piece_ok, correct, sizes = batch_scores(img, batch.x, batch.patches_dim, batch=batch.batch, rotation=bool(self.rotation),
                                                return_sizes=True)
        if hasattr(self, "metrics"):
            piece_ok, correct, sizes = piece_ok.float(), correct.tolist(), sizes.tolist()
            lo = 0
            for i, (flags, rows, cols) in enumerate(sizes):
                key = f"{(rows, cols)}"
                piece_accuracy = piece_ok[lo:lo + flags]
                lo += flags
                for name, val in ((f"{key}_acc", float(correct[i])), (f"{key}__piece_acc", piece_accuracy),
                                  (f"{key}_nImages", 1), ("overall_acc", float(correct[i])),
                                  ("overall__piece_acc", piece_accuracy), ("overall_nImages", 1)):
                    if name in self.metrics:
                        self.metrics[name].update(val)
        if self.save_eval_images:
            self._save_eval_frames(batch, imgs)
        return img

    # ------------------------------------------------------------------ pictures (spatial_diffusion.py:957-971, 1204-1234)
    eval_image_dir = "results/test"       # where the default save_eval_frame writes
    eval_image_max_bytes = 1 << 30        # frame buffer of one render_frames call of _eval_step

    def create_image_from_patches(self, patches, pos, n_patches=(4, 4), i=0, rotations=None):
        """spatial_diffusion.py:1204-1234 with the reference's signature: the pieces of ONE puzzle pasted where ``pos`` puts
        them (and turned by ``rotations`` = (cos, sin) rows), as a ``PIL.Image`` in mode RGBA.  The frame is made by
        ``render2d.batch_frames`` (one da_render2d launch on a ROCm device), bit-equal to the reference's PIL compositing."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("create_image_from_patches returns a PIL.Image and PIL is not installed; "
                              "diffassemble_amd.render2d.batch_frames gives the same pixels as a uint8 tensor without PIL") from e
        from ..render2d import batch_frames
        poses = pos[:, :2] if rotations is None else torch.cat((pos[:, :2], rotations[:, :2].to(pos.device)), 1)
        frame = batch_frames(patches, poses.to(patches.device), [[int(n_patches[0]), int(n_patches[1])]], rotation=rotations is not None)[0][0]
        return Image.fromarray(frame.cpu().numpy())

    def render_frames(self, batch, imgs, steps=None, max_bytes=None):
        """The pictures of a Batch along the sampling loop: ``frames[k][g]`` = uint8 [32 * rows_g, 32 * cols_g, 4] on the device
        for the selected ``steps`` of ``imgs`` (the list ``p_sample_loop`` returns, or one [N, c] pose tensor) and every puzzle g
        (``render2d.batch_frames``: one launch for all of them)."""
        from ..render2d import MAX_BYTES, batch_frames
        return batch_frames(batch.patches, imgs, batch.patches_dim, batch=batch.batch, rotation=bool(self.rotation), steps=steps,
                            max_bytes=MAX_BYTES if max_bytes is None else max_bytes)

    def save_eval_frame(self, frame, ind_name, step):
        """Receives every frame ``_eval_step`` renders when ``save_eval_images`` is set: ``frame`` uint8 [H, W, 4] on the device,
        ``ind_name`` the puzzle's ``ind_name`` in the Batch (its index in the Batch when the dataset attached none), ``step`` the
        index of the loop step.  Default: ``<eval_image_dir>/{ind_name:03d}_{step:03d}.png`` through PIL.  Override or assign
        another callable to keep the frames elsewhere."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("save_eval_images writes PNG files through PIL, which is not installed; "
                              "assign save_eval_frame to take the frames of render2d.batch_frames without PIL") from e
        os.makedirs(self.eval_image_dir, exist_ok=True)
        Image.fromarray(frame.cpu().numpy()).save(os.path.join(self.eval_image_dir, f"{int(ind_name):03d}_{int(step):03d}.png"))

    def _save_eval_frames(self, batch, imgs):
        """Every step of the loop for every puzzle, rendered in chunks of steps whose frames fit ``eval_image_max_bytes``."""
        dims = torch.as_tensor(batch.patches_dim).reshape(-1, 2).tolist()
        names = getattr(batch, "ind_name", None)
        names = list(range(len(dims))) if names is None else [int(v) for v in torch.as_tensor(names).reshape(-1).tolist()]
        per_step = sum(4 * 32 * r * 32 * c for r, c in dims)
        chunk = max(1, int(self.eval_image_max_bytes) // per_step)
        for lo in range(0, len(imgs), chunk):
            picked = list(range(lo, min(lo + chunk, len(imgs))))
            frames = self.render_frames(batch, imgs, steps=picked, max_bytes=max(int(self.eval_image_max_bytes), per_step))
            for k, step in enumerate(picked):
                for g, frame in enumerate(frames[k]):
                    self.save_eval_frame(frame, names[g], step)

    def validation_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def validation_epoch_end(self, outputs) -> None:
        """spatial_diffusion.py:903 logs the Metric objects, which Lightning computes AND resets at epoch
        end; logging plain values, the reset is done here so every epoch reports its own accuracy."""
        if hasattr(self, "metrics"):
            self.log_dict({k: m.compute() for k, m in self.metrics.items()})
            for m in self.metrics.values():
                m.reset()

    def test_epoch_end(self, outputs) -> None:
        return self.validation_epoch_end(outputs)
