"""Counterpart of puzzle_diff/model/spatial_diffusion_discrete_rot.py: ``GNN_Diffusion`` of the discrete position + rotation
diffusion (two D3PM processes with the uniform transition, K positions and ``rot_K = 4`` quarter turns, over
``backbones.Eff_GAT_Discrete_ROT``), with the reference's constructor, attributes and Lightning hooks.  Inference only: forward,
reverse step, the captured sampling loop, validation / test / predict steps, on a ROCm device.

* ``forward_with_feats`` -> one ``da_denoiser_forward_rot`` call -> (logits [N, K], rot_logits [N, 4])
* ``p_sample_ddpm``      -> forward + ``da_d3pm_rot_step`` -> the reference's triple (index, rot_0, rot_prev_t)
* ``p_sample_loop``      -> ``da_sample_loop_rot``: every iteration enqueued by one C call, replayed as one hipGraph launch

The reference rotates the crops by the accumulated rotation and re-encodes them inside the loop (:353, :373).  ``rot_acc`` takes
four values per piece, so here the loop reads FOUR feature images per Batch, ``patch_feats`` [4, N, 1088] (image r: the crops
rotated by -r quarter turns), and selects each piece's row per step on the device.

Differences from the reference, on purpose (besides those of ``spatial_diffusion_discrete``):
* no ``overline_Q_rot`` buffer: the closed form serves both processes; a reference checkpoint that carries it loads;
* the reference backbone's ``forward_with_feats`` raises as shipped; this module computes what it computes once the
  ``(x, attentions)`` pair of ``Transformer_GNN`` is unpacked;
* no classifier-free branch at inference (the reference has none either), no image dumps;
* ``p_losses`` / ``training_step`` raise ``NotImplementedError``: the two-head training path is not built.
"""
import torch

from . import backbones
from . import spatial_diffusion_discrete as sdd

_Q_TABLES = sdd._Q_TABLES + ("overline_Q_rot",)
_NOT_BUILT = "discrete-rotation training is not built yet"


class GNN_Diffusion(sdd.GNN_Diffusion):
    def __init__(self, only_rotation=False, cold_diffusion=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.rot_K = 4
        self.only_rotation = only_rotation
        self.cold_diffusion = cold_diffusion
        self.losses_keys = ["rot_loss"] if only_rotation else ["rot_loss", "x_loss"]

    def init_backbone(self):
        self.model = backbones.Eff_GAT_Discrete_ROT(steps=self.steps, input_channels=self.input_channels,
                                                    output_channels=self.output_channels)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.pop(prefix + "overline_Q_rot", None)           # (the parent drops its own three tables)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ------------------------------------------------------------------ training side: not built
    def training_step(self, batch=None, batch_idx=0):
        raise NotImplementedError(_NOT_BUILT)

    def p_losses(self, *args, **kwargs):
        raise NotImplementedError(_NOT_BUILT)

    # ------------------------------------------------------------------ reverse process
    def forward_with_feats(self, xy_pos, time, patch_rgb, edge_index, patch_feats, rot, batch, rot_acc=None):
        """spatial_diffusion_discrete_rot.py:147-159.  ``rot_acc`` (extension): per-piece feature image for ``patch_feats`` [4, N, 1088]."""
        return self.model.forward_with_feats(xy_pos, rot, time, patch_rgb, edge_index, patch_feats, batch, rot_acc=rot_acc)

    def _feats4(self, cond, patch_feats):
        """The loop's [4, N, 1088] table: given, or encoded from the four rotated crops where the encoder exists."""
        if patch_feats is None:
            return self.model.visual_features4(cond)
        return patch_feats

    @torch.no_grad()
    def p_sample_ddpm(self, x, rot, t, t_index, cond, edge_index, patch_feats, batch, rot_acc=None, noise=None, noise_rot=None):
        """spatial_diffusion_discrete_rot.py:288-330 -> (x_sample, argmax(rot logits), rot_sample).  ``noise`` [N, K] / ``noise_rot``
        [N, 4] (extensions): the step's uniforms, default one ``torch.rand`` each, in the reference's order."""
        logits, rot_logits = self.forward_with_feats(x, t, cond, edge_index, patch_feats, rot, batch, rot_acc=rot_acc)
        if noise is None:
            noise = torch.rand(logits.shape, device=logits.device)
        if noise_rot is None:
            noise_rot = torch.rand(rot_logits.shape, device=logits.device)
        return self.model.engine(x.device).d3pm_rot_step(self._schedule(), x, rot, logits, rot_logits, t, self.inference_ratio,
                                                         noise_x=noise, noise_rot=noise_rot)

    @torch.no_grad()
    def p_sample(self, x, rot, t, t_index, cond, edge_index, sampling_func, patch_feats, batch):
        return sampling_func(x, rot, t, t_index, cond, edge_index, patch_feats, batch)

    @torch.no_grad()
    def p_sample_loop(self, shape, cond, edge_index, batch, x_start=None, patch_feats=None):
        """spatial_diffusion_discrete_rot.py:334-375: two ``torch.randint`` draws for the start, ONE library call for the loop; returns
        the list of per-step ``(index, rot_acc)`` pairs (int64 [N] each).  ``patch_feats`` [4, N, 1088] bypasses the encoder."""
        device = self.device
        index = torch.randint(0, self.K, shape, device=device)
        rot = torch.randint(0, self.rot_K, shape, device=device)
        if self.only_rotation and x_start is None:
            raise ValueError("only_rotation: p_sample_loop needs x_start (every step starts from the given indices)")
        feats4 = self._feats4(cond, patch_feats)
        eng = self.model.engine(device)
        plan = self.model._plan_for(eng, edge_index, batch)
        self.model._feat_key = None
        tx, ta, _, _ = eng.sample_loop_rot(plan, self._schedule(), index, rot, feats4, ratio=self.inference_ratio, keep_traj=True,
                                           use_graph=self.use_hip_graph, cold=self.cold_diffusion,
                                           x_fixed=x_start if self.only_rotation else None)
        self.model._release_dense_plan_key()
        return list(zip(tx.long().unbind(0), ta.long().unbind(0)))

    # ------------------------------------------------------------------ Lightning hooks
    def _loop_of(self, batch):
        return self.p_sample_loop(batch.indexes.shape, batch.patches, batch.edge_index, batch=batch.batch,
                                  x_start=batch.indexes.to(self.device) % self.K, patch_feats=getattr(batch, "patch_feats", None))

    @torch.no_grad()
    def prediction_step(self, batch, batch_idx):
        return self._loop_of(batch)

    def predict_step(self, batch, batch_idx, dataloader_idx=0):
        """The (index, rot_acc) trajectory (the reference also dumps images here, :380-446)."""
        return self.prediction_step(batch, batch_idx)

    @torch.no_grad()
    def _eval_step(self, batch, batch_idx):
        """validation_step / test_step, spatial_diffusion_discrete_rot.py:448-526: a puzzle counts when every piece has its index AND
        its rotation; under ``only_rotation`` the rotations alone decide.  Reduced on the device, one host copy per Batch."""
        pred, pred_rot = self._loop_of(batch)[-1]
        dev = pred.device
        ok_rot = (pred_rot % self.rot_K) == (batch.rot_index.to(dev) % self.rot_K)
        ok = ok_rot if self.only_rotation else (pred == batch.indexes.to(dev) % self.K) & ok_rot
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
        return pred, pred_rot
