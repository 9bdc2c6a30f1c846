"""Counterpart of puzzle_diff/model/spatial_diffusion_3d_test_double_diffusion.py (the SE(3)
``GNN_Diffusion`` that train_3d.py:19 imports): R^3 Gaussian diffusion on translations, SO(3)
diffusion on rotations (quaternion wxyz | translation per fragment).  On the hot path:
``forward_with_feats`` (:369-382), ``p_sample_ddim`` (:595-663) and ``p_sample_loop``
(:688-731) run in the HIP library, and so does the training step of train_3d.py's configuration
(START_X, ``vn_dgcnn``, ``loss_type="all"``): ``p_losses`` (:410-572) = SE(3) noising in one launch
(da_q_sample_se3) -> VN-DGCNN encoder -> denoiser forward and backward (da_train_forward / da_train_backward,
``DenoiserTrainFn``; no torch autograd through the denoiser) -> the assembly losses (da_loss3d_*), then
``training_step`` (:792-807) and the fused Adafactor of ``configure_optimizers``.  ``use_6dof=True`` (train_3d.py
--use_6dof_rot) is the 13-channel model: pose rows [quaternion | translation | a1 | a2], nine Gaussian channels in the noising
(da_q_sample_se3_6d) and in the DDIM step, and the rotation the loss and the evaluation read is the Gram-Schmidt quaternion of
(a1, a2) (da_rot6d_to_pose and its backward, ``Rot6dToPoseFn``).  ``loss_type="split"``, ``use_vn_dgcnn_equiv_inv_mp``,
metrics dumps and mesh export stay out of scope."""
from functools import partial
from typing import Any

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from .. import _lib
from ..engine import Schedule
from .. import metrics3d
from ._lightning_compat import LightningModule, MeanMetric
from .backbones import Eff_GAT_3d
from .spatial_diffusion import (ModelMeanType, ModelScheduler, cosine_beta_schedule,  # noqa: F401
                                cosine_discrete_beta_schedule, extract, linear_beta_schedule)


def extract_rot(a, t, x_shape):
    b, *_ = t.shape
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


def _metric_was_updated(m):
    """True when a MeanMetric has seen at least one update since its last reset -- for torchmetrics' class
    (``update_called`` / ``_update_count``) and for the stand-in of this package (``count``) alike."""
    for attr in ("update_called", "_update_called"):
        v = getattr(m, attr, None)
        if isinstance(v, bool):
            return v
    v = getattr(m, "_update_count", None)
    if v is not None:
        return int(v) > 0
    return float(getattr(m, "count", 0)) > 0


def rot6d_to_pose(pred):
    """prediction [P, >= 13] (columns 4:7 the translation, 7:13 = a1 | a2) -> pose7 [P, 7] = [Gram-Schmidt quaternion | translation]
    (:480-490, :826-845) in one launch (da_rot6d_to_pose); no gradient -- ``Rot6dToPoseFn`` is the differentiable form."""
    if pred.device.type != "cuda":
        raise _lib.DaError("rot6d_to_pose: the tensor must live on the ROCm device (diffassemble_amd has no CPU / eager fallback)")
    if pred.dim() != 2 or pred.shape[1] < 13:
        raise ValueError(f"rot6d_to_pose: prediction rows are 13 wide (got {tuple(pred.shape)})")
    x = pred.detach().to(torch.float32)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < 13):
        x = x.contiguous()
    ld = x.stride(0) if x.shape[0] > 1 else 13
    out = torch.empty((x.shape[0], 7), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().da_rot6d_to_pose(x.shape[0], _lib.ptr(x), ld, _lib.ptr(out), _lib.stream_ptr(x.device)))
    return out


class Rot6dToPoseFn(torch.autograd.Function):
    """``rot6d_to_pose`` under autograd: the backward is da_rot6d_to_pose_backward (closed form; columns 0:4 of the prediction -- the
    head's own quaternion -- get zeros, as in the reference, whose loss never reads them)."""

    @staticmethod
    def forward(ctx, pred):
        x = pred.detach().to(torch.float32).contiguous()
        ctx.save_for_backward(x)
        return rot6d_to_pose(x)

    @staticmethod
    def backward(ctx, d_pose):
        (x,) = ctx.saved_tensors
        g = d_pose.detach().to(torch.float32).contiguous()
        d_pred = torch.empty((x.shape[0], 13), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().da_rot6d_to_pose_backward(x.shape[0], _lib.ptr(x), x.shape[1], _lib.ptr(g), _lib.ptr(d_pred),
                                                            _lib.stream_ptr(x.device)))
        return d_pred


class GNN_Diffusion(LightningModule):
    def __init__(self, steps=600, inference_ratio=1, sampling="DDPM", learning_rate=1e-4,
                 save_and_sample_every=1000, classifier_free_prob=0, classifier_free_w=0, noise_weight=0.0,
                 model_mean_type: ModelMeanType = ModelMeanType.EPSILON, input_channels=7, output_channels=7,
                 scheduler: ModelScheduler = ModelScheduler.LINEAR, visual_pretrained: bool = True,
                 freeze_backbone: bool = True, n_layers: int = 4, loss_type="all", backbone="vnn",
                 max_epochs=200, use_vn_dgcnn_equiv_inv_mp: bool = False, max_num_part: int = 20,
                 use_6dof: bool = False, architecture="transformer", *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.loss_type = loss_type
        self.visual_pretrained = visual_pretrained
        self.free_backbone = freeze_backbone
        self.model_mean_type = model_mean_type
        self.learning_rate = learning_rate
        self.save_and_sample_every = save_and_sample_every
        self.classifier_free_prob = classifier_free_prob
        self.classifier_free_w = classifier_free_w
        self.noise_weight = noise_weight
        self.backbone = backbone
        self.max_epochs = max_epochs
        self.use_vn_dgcnn_equiv_inv_mp = use_vn_dgcnn_equiv_inv_mp
        self.max_num_part = max_num_part
        self.use_6dof = use_6dof
        self.save_eval_images = False
        self.return_attentions = False
        self.use_hip_graph = True
        if sampling == "DDIM":          # the reference binds a sampler only for DDIM (:269-275)
            self.inference_ratio = inference_ratio
            self.p_sample = partial(self.p_sample, sampling_func=self.p_sample_ddim)
            self.eta = 0
        betas = {ModelScheduler.LINEAR: linear_beta_schedule, ModelScheduler.COSINE: cosine_beta_schedule,
                 ModelScheduler.COSINE_DISCRETE: cosine_discrete_beta_schedule}[scheduler](timesteps=steps)
        self.register_buffer("betas", betas)
        alphas = 1.0 - self.betas
        self.register_buffer("alphas", alphas)
        self.register_buffer("alphas_cumprod", torch.cumprod(self.alphas, axis=0))
        self.register_buffer("alphas_cumprod_prev", F.pad(self.alphas_cumprod[:-1], (1, 0), value=1.0))
        self.register_buffer("sqrt_recip_alphas", torch.sqrt(1.0 / self.alphas))
        self.register_buffer("identity", torch.eye(3))
        self.register_buffer("sqrt_alphas_cumprod", torch.sqrt(self.alphas_cumprod))
        self.register_buffer("sqrt_recip_alphas_cumprod",
                             torch.from_numpy(np.sqrt((1.0 / self.alphas_cumprod).numpy())))
        self.register_buffer("sqrt_recipm1_alphas_cumprod",
                             torch.from_numpy(np.sqrt((1.0 / self.alphas_cumprod - 1).numpy())))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - self.alphas_cumprod))
        self.register_buffer("posterior_variance",
                             self.betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod))
        self.steps = steps
        self.input_channels = 13 if use_6dof else input_channels       # 4 + 3 + 6: quaternion | translation | a1 | a2 (:326-327)
        self.architecture = architecture
        self.n_layers = n_layers
        self.init_backbone()
        self.save_hyperparameters()

    def init_backbone(self):
        self.model = Eff_GAT_3d(steps=self.steps, input_channels=self.input_channels, t_channels=9 if self.use_6dof else 3,
                                n_layers=self.n_layers,
                                architecture=self.architecture, backbone=self.backbone,
                                freeze_backbone=self.free_backbone,
                                use_vn_dgcnn_equiv_inv_mp=self.use_vn_dgcnn_equiv_inv_mp)

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

    def forward_with_feats(self, xy_pos: Tensor, time: Tensor, edge_index: Tensor, pcd_feats: Tensor, batch,
                           return_attentions=False) -> Any:
        """...double_diffusion.py:369-382 (always returns the pair, like the reference)."""
        self.model.return_attentions = bool(return_attentions)
        return self.model.forward_with_feats(xy_pos, time, edge_index, pcd_feats, batch)

    def pcd_features(self, pcd):
        return self.model.pcd_features(pcd)

    def q_sample_tr(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        return (extract(self.sqrt_alphas_cumprod, t) * x_start
                + extract(self.sqrt_one_minus_alphas_cumprod, t) * noise)

    @torch.no_grad()
    def p_sample_ddim(self, x, t, t_index, edge_index, pcd_feats, batch):
        """...double_diffusion.py:595-663."""
        model_output, attentions = self.forward_with_feats(x, t, edge_index, pcd_feats, batch,
                                                           return_attentions=self.return_attentions)
        prev = self.model.engine(x.device).ddim_step(self._schedule(), x, model_output, t, self.inference_ratio,
                                                     self._mean_type())
        return prev, attentions

    @torch.no_grad()
    def p_sample_loop(self, shape, cond, edge_index, batch, pcd_feats=None):
        """...double_diffusion.py:688-731: identity rotations + randn * noise_weight translations (use_6dof: all nine Gaussian
        channels, and every trajectory entry is [P, 13])."""
        device = self.device
        b = shape[0]
        tr = torch.randn((b, 9 if self.use_6dof else 3), device=device) * self.noise_weight
        quat = torch.zeros((b, 4), device=device)
        quat[:, 0] = 1.0                              # matrix_to_quaternion(eye(3))
        img = torch.cat([quat, tr], dim=1)
        if pcd_feats is None:
            pcd_feats = self.pcd_features(cond)
        its = list(reversed(range(0, self.steps, self.inference_ratio)))
        if not self.return_attentions:
            eng = self.model.engine(device)
            plan = self.model._plan_for(eng, edge_index, batch)
            self.model._feat_key = None
            traj, _ = eng.sample_loop(plan, self._schedule(), img, pcd_feats, ratio=self.inference_ratio,
                                      mean_type=self._mean_type(), keep_trajectory=True,
                                      use_graph=self.use_hip_graph)
            self.model._release_dense_plan_key()          # do not pin this Batch's edge list until the next one is planned
            return list(traj.clone().unbind(0)), [None] * len(its)
        imgs, attentions = [], []
        for i in its:
            img, atts = self.p_sample(img, torch.full((b,), i, device=device, dtype=torch.long), i,
                                      edge_index=edge_index, pcd_feats=pcd_feats, batch=batch)
            attentions.append(atts)
            imgs.append(img)
        return imgs, attentions

    @torch.no_grad()
    def p_sample(self, x, t, t_index, edge_index, sampling_func, pcd_feats, batch):
        return sampling_func(x, t, t_index, edge_index, pcd_feats, batch)

    def pose_losses(self, prediction, target, cond, n_batch, valids, loss_type="all"):
        """The loss of ...double_diffusion.py:462-572 behind the noising and the forward: prediction / target [P, 7] (quaternion
        wxyz | translation), cond [P, N, 3] the fragments -> the weighted ``loss_dict`` (diffassemble_amd/losses3d.py; HIP
        forward and backward, the gradient reaches ``prediction``).  The seam a later ``p_losses`` calls.  ``valids`` must
        mark exactly P slots; that is not checked on the device (no host synchronisation), see ``assembly_losses``."""
        from .. import losses3d
        return losses3d.assembly_losses(prediction, target, cond, n_batch, valids, n_parts=self.max_num_part, loss_type=loss_type)

    def q_sample_se3(self, x_start, t, noise=None):
        """The noising of p_losses (:421-441) as ONE launch (da_q_sample_se3): Gaussian ``q_sample`` on the translation,
        ``so3_scale(R0, sqrt_alphas_cumprod[t]) @ IGSO(3) draw`` on the rotation, back to a quaternion.  ``noise`` =
        ``(noise_tr [P, 3], axes [P, 3], unif [P])``; drawn here in the reference's order when None (randn for the
        translation, randn for the axes, rand for the uniforms), so a seeded run replays the reference's stream.
        ``use_6dof`` (:424-431, da_q_sample_se3_6d): ``noise_tr`` is [P, 9] -- the Gaussian part is [translation | R0[:, 0] |
        R0[:, 1]], the first two columns of the clean rotation matrix -- and the result is [P, 13]; ``x_start`` stays [P, 7]."""
        nt = 9 if self.use_6dof else 3
        P = x_start.shape[0]
        dev = x_start.device
        if dev.type != "cuda":
            raise _lib.DaError("q_sample_se3: the tensors must live on the ROCm device (diffassemble_amd has no CPU / eager fallback)")
        if noise is None:
            noise = (torch.randn(P, nt, device=dev), torch.randn(P, 3, device=dev), torch.rand(P, device=dev))
        noise_tr, axes, unif = (n.detach().to(dev, torch.float32).contiguous() for n in noise)
        if noise_tr.shape != (P, nt) or axes.shape != (P, 3) or unif.shape != (P,) or x_start.shape != (P, 7) or t.shape != (P,):
            raise ValueError(f"q_sample_se3: x_start [P, 7], t [P], noise = (noise_tr [P, {nt}], axes [P, 3], unif [P])")
        sch = self._schedule()
        x0 = x_start.detach().to(torch.float32).contiguous()
        tt = t.detach().to(dev, torch.int64).contiguous()
        sac = self.sqrt_alphas_cumprod.to(torch.float32).contiguous()
        out = torch.empty((P, 4 + nt), dtype=torch.float32, device=dev)
        q_sample = _lib.lib().da_q_sample_se3_6d if self.use_6dof else _lib.lib().da_q_sample_se3
        with torch.cuda.device(dev):
            _lib.check(q_sample(self.steps, P, _lib.ptr(sac), _lib.ptr(sch.t["sqrt_one_minus_alphas_cumprod"]), _lib.ptr(sch.igso3_trap()),
                                _lib.ptr(x0), _lib.ptr(tt), _lib.ptr(noise_tr), _lib.ptr(axes), _lib.ptr(unif), _lib.ptr(out),
                                _lib.stream_ptr(dev)))
        return out

    def p_losses(self, x_start, t, noise=None, loss_type="l1", cond=None, edge_index=None, batch=None, n_batch=None,
                 valids=None, pcd_feats=None):
        """...double_diffusion.py:410-572 -> the ``loss_dict`` of ``loss_type="all"``.  Noising, encoder, denoiser forward +
        backward and the losses all run in the HIP library; torch autograd only links them (``DenoiserTrainFn``, ``_Loss3d``,
        the encoder's own Function).  ``noise`` = ``(noise_tr, axes, unif)`` (see ``q_sample_se3``); ``pcd_feats`` (extension,
        like 2D's ``patch_feats``) bypasses the encoder."""
        if loss_type != "all":             # the reference raises at :570 ("split" cannot run there: trans_l2_loss without valids)
            raise NotImplementedError(f"loss_type={loss_type!r}: the 3D model trains with loss_type='all' (train_3d.py)")
        if self.model_mean_type != ModelMeanType.START_X:
            raise NotImplementedError(
                "ModelMeanType.EPSILON: the reference's own 3D p_losses cannot run it -- its target is `noise`, which is None on "
                "that path (:458-461), and the loss fails with a TypeError; train with ModelMeanType.START_X (train_3d.py)")
        x_noisy = self.q_sample_se3(x_start, t, noise)
        if self.steps == 1:
            x_noisy = torch.zeros_like(x_noisy)
        if pcd_feats is None:
            pcd_feats = self.model.pcd_features_train(cond)
        prediction, _ = self.forward_with_feats(x_noisy, t, edge_index, pcd_feats=pcd_feats, batch=batch, return_attentions=False)
        if self.use_6dof:        # the loss reads the translation and the Gram-Schmidt rotation of (a1, a2); the head's quaternion carries none (:480-490)
            prediction = Rot6dToPoseFn.apply(prediction)
        return self.pose_losses(prediction, x_start, cond, n_batch, valids, loss_type=loss_type)

    def training_step(self, batch, batch_idx):
        """...double_diffusion.py:792-807 (the batch_idx == 0 sampling dump omitted, as the 2D step omits its image dumps)."""
        batch_size = batch.batch.max().item() + 1
        t = torch.randint(0, self.steps, (batch_size,), device=self.device).long()
        new_t = torch.gather(t, 0, batch.batch)
        loss_dict = self.p_losses(batch.x, new_t, loss_type=self.loss_type, cond=batch.pcds, edge_index=batch.edge_index,
                                  batch=batch.batch, n_batch=len(batch.data_id), valids=batch.valids,
                                  pcd_feats=getattr(batch, "pcd_feats", None))
        loss = sum(loss_dict.values())
        for k, v in loss_dict.items():
            self.log(k, v)
        self.log("loss", loss)
        return loss

    # ------------------------------------------------------------------ Lightning hooks (inference callers)
    def initialize_torchmetrics(self, categories):
        """...double_diffusion.py:347-364: four MeanMetrics per category + their averages."""
        import torch.nn as nn
        metrics = {}
        for i in categories:
            for k in ("rmse_t", "rmse_r", "gd_r", "part_acc"):
                metrics[f"{k}_{i}"] = MeanMetric()
        self.metrics = nn.ModuleDict(metrics)
        self.avg_metrics = nn.ModuleDict({f"{k}_AVG": MeanMetric() for k in ("rmse_t", "rmse_r", "gd_r", "part_acc")})

    @torch.no_grad()
    def _eval_step(self, batch, batch_idx):
        """validation_step / test_step (:895-960, :1036-1080): one sampling loop for the whole Batch, then the four pose
        metrics of every object against the ground-truth poses in ``batch.x`` (wandb / mesh dumps omitted): one
        ``metrics3d.batch_metrics`` call (``da_metrics3d``) and one [G, 4] copy to the host per Batch.  Returns
        the final poses [P, 7] (use_6dof: read out of the 13-wide rows by da_rot6d_to_pose)."""
        sampled_pos, _ = self.p_sample_loop(batch.x.shape, batch.pcds, batch.edge_index, batch=batch.batch,
                                            pcd_feats=getattr(batch, "pcd_feats", None))
        final_pos = sampled_pos[-1]
        if self.use_6dof:        # [P, 13] -> [Gram-Schmidt quaternion | translation] (:826-845, :914-960)
            final_pos = rot6d_to_pose(final_pos)
        pcds = getattr(batch, "pcds", None)
        cats = getattr(batch, "category", None)
        if cats is not None:                   # the object count is known on the host: ptr without reading the device
            ptr = torch.searchsorted(batch.batch, torch.arange(len(cats) + 1, device=batch.batch.device)).to(torch.int32)
            vals = metrics3d.batch_metrics(pcds, final_pos, batch.x, ptr=ptr).cpu()
        else:
            vals = metrics3d.batch_metrics(pcds, final_pos, batch.x, batch=batch.batch).cpu()
        if hasattr(self, "metrics"):
            names = ("rmse_t", "rmse_r", "gd_r") + (("part_acc",) if pcds is not None else ())
            for i, row in enumerate(vals.tolist()):
                cat = batch.category[i]
                for k, v in zip(names, row):
                    if f"{k}_{cat}" in self.metrics:
                        self.metrics[f"{k}_{cat}"].update(v)
        # (the step only UPDATES the per-category metrics; they are computed, logged and reset once per epoch in
        # validation_epoch_end -- computing them here would log a batch-weighted mean of running means and, under DDP,
        # trigger one metric sync per category per step)
        return final_pos

    def validation_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    @torch.no_grad()
    def prediction_step(self, batch, batch_idx):
        return self.p_sample_loop(batch.x.shape, batch.pcds, batch.edge_index, batch=batch.batch,
                                  pcd_feats=getattr(batch, "pcd_feats", None))

    def predict_step(self, batch, batch_idx, dataloader_idx=0):
        return self.prediction_step(batch, batch_idx)

    def validation_epoch_end(self, outputs) -> None:
        """:1015-1031: every per-category metric feeds the matching *_AVG metric; the per-category metrics are reset
        (Lightning does that for logged Metric objects at epoch end)."""
        if not hasattr(self, "metrics"):
            return
        seen = {}
        for k in ("rmse_t", "rmse_r", "gd_r", "part_acc"):
            for name, m in self.metrics.items():
                if name.startswith(k + "_") and _metric_was_updated(m):        # categories without a sample stay out of the averages
                    seen[name] = m.compute()
                    self.avg_metrics[f"{k}_AVG"].update(float(seen[name]))
        self.log_dict({**seen, **{k: m.compute() for k, m in self.avg_metrics.items() if _metric_was_updated(m)}})
        for m in list(self.metrics.values()) + list(self.avg_metrics.values()):
            m.reset()

    def test_epoch_end(self, outputs) -> None:
        return self.validation_epoch_end(outputs)

    def configure_optimizers(self):
        """Adafactor with transformers' defaults, as the 2D module: on a ROCm device one library call over the training engine's
        flat buffers (``FusedAdafactor``) when the encoder is frozen or absent, ``HybridAdafactor`` (a second call,
        ``FusedAdafactorND``, for the encoder's tensors) with a trainable encoder attached; ``fused_optimizer = False`` (class /
        instance attribute) = transformers' own implementation throughout."""
        fused = bool(getattr(self, "fused_optimizer", True))
        if fused and self.device.type == "cuda":
            enc = getattr(self.model, "pcd_backbone", None)
            te = self.model.train_engine(self.device)
            if enc is None or self.model.freeze_backbone or not any(p.requires_grad for p in enc.parameters()):
                from ..train import FusedAdafactor
                mine = {id(p) for p in te.params}
                return FusedAdafactor([p for p in self.parameters() if id(p) in mine], te)
            from ..train import HybridAdafactor
            return HybridAdafactor(self.parameters(), te)
        from transformers.optimization import Adafactor
        return Adafactor(self.parameters())
