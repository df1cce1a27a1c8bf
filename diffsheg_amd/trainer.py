"""Harness boundary: ``generate_batch`` and the arbitrary-length
window chain of ``test_arbitrary_len`` / ``test_custom_aud``
(/root/reference/trainers/ddpm_show_trainer.py:163-198, :801-819, :864-906; BEAT twin
ddpm_beat_trainer.py:185-220, :932-1039), plus the sharding of independent chains over ranks
(the reference shards test videos with a DistributedSampler, ddpm_show_trainer.py:743-750).

The validation loop's tail (ddpm_show_trainer.py:440-583: FGD encoder, MSE / PCK / diversity meters) is ``validate_batch`` /
``validation_summary`` on top of :mod:`diffsheg_amd.metrics`.  The eval-mode forward of the training objective (``forward(eval_mode=True)``
:135-181 with the arithmetic of ``backward_G`` :222-260) is ``denoising_losses``, its per-level curve ``loss_profile``.  The BEAT results tail (ddpm_beat_trainer.py:1044-1060: gesture channels
from standardised axis-angle to the standardised Euler degrees the reference saves and scores) is the ``pose_rep="euler"`` keyword of
the sampling entry points, on :func:`diffsheg_amd.glue.axis_angle_to_euler`.  Training, BVH/JSON writers, HuBERT extraction and
checkpoint saving are out of scope.
"""
from __future__ import annotations

import numbers
import os

import argparse
from typing import Dict, List, Optional, Sequence

import torch

from .config import DiffSHEGConfig
from .diffusion import (GaussianDiffusion, ModelMeanType, ModelVarType, SpacedDiffusion, create_named_schedule_sampler,
                        get_named_beta_schedule, space_timesteps)
from .model import UniDiffuser, normalize_guidance_scale, normalize_modality


def sampler_namespace(cfg: DiffSHEGConfig, **over) -> argparse.Namespace:
    """The `opt` attributes the sampler reads (gaussian_diffusion.py / scheduler.py)."""
    ns = argparse.Namespace(jump_length=cfg.jump_length, jump_n_sample=cfg.jump_n_sample, overlap_len=cfg.overlap_len,
                            addBlend=cfg.add_blend, no_resample=cfg.no_resample, no_repaint=cfg.no_repaint,
                            timestep_respacing=cfg.timestep_respacing, unidiffuser=cfg.unidiffuser, same_overlap_noisy=False,
                            fix_head_var=False, ddim=True, n_poses=cfg.n_poses, net_dim_pose=cfg.net_dim_pose,
                            PE="pe_sinu", diffusion_steps=cfg.diffusion_steps, fix_very_first=False,
                            dataset_name="talkshow" if cfg.dataset == "show" else "beat")
    for k, v in over.items():
        setattr(ns, k, v)
    return ns


_M64 = (1 << 64) - 1


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def window_seed(seed: int, window: int) -> int:
    """Philox key of window ``window`` of a chain sampled with base seed ``seed``: a 64-bit hash of the pair, so that
    neighbouring (seed, window) pairs share no stream (``seed + window`` collides for (s, w + 1) and (s + 1, w))."""
    return _splitmix64(_splitmix64(int(seed) & _M64) ^ ((int(window) + 1) * 0xD1342543DE82EF95 & _M64))


def level_seed(seed: int, timestep: int) -> int:
    """Philox seed of the noise :meth:`DDPMTrainer.loss_profile` draws at the ORIGINAL timestep ``timestep``: a hash of the pair alone, so
    a level's noise does not depend on which other levels are profiled, nor on the spacing the level belongs to."""
    return _splitmix64(_splitmix64(int(seed) & _M64) ^ ((int(timestep) + 1) * 0xA0761D6478BD642F & _M64))


def get_windows(x, size: int, step: int):
    """ddpm_show_trainer.py:801-819 — tensors or dicts of tensors; the tail window may be shorter."""
    if isinstance(x, dict):
        per_key = {k: get_windows(v, size, step) for k, v in x.items()}
        n = len(next(iter(per_key.values())))
        return [{k: per_key[k][i] for k in per_key} for i in range(n)]
    seq_len = x.shape[1]
    if seq_len <= size:
        return [x]
    win_num = (seq_len - (size - step)) / float(step)
    out = [x[:, m * step: m * step + size, ...] for m in range(int(win_num))]
    if win_num - int(win_num) != 0:
        out.append(x[:, int(win_num) * step:, ...])
    return out


def window_lengths(n_frames: int, size: int, step: int) -> List[int]:
    """Frame counts of the windows :func:`get_windows` cuts a stream of ``n_frames`` frames into (window ``i`` starts at
    ``i * step``): full windows, then the stream's own shorter tail."""
    if n_frames <= size:
        return [n_frames]
    win_num = (n_frames - (size - step)) / float(step)
    out = [size] * int(win_num)
    if win_num - int(win_num) != 0:
        out.append(n_frames - int(win_num) * step)
    return out


# bf16 batches of 7 and more clips need windows of at least this many frames (UniDiffuser.set_condition: FiLM rows staged per token block).
# A ragged window batch whose rows are all short tails is padded up to it; the rows keep their lengths.
MIN_PAD_FRAMES, MIN_PAD_BATCH = 11, 7


def ragged_window_plan(chain_frames: Sequence[int], size: int, step: int) -> List[dict]:
    """Window batches of chains of different lengths sampled together.  Chain ``b`` gets exactly the windows
    :func:`get_windows` gives a stream of ``chain_frames[b]`` frames; batch ``i`` of the plan holds window ``i`` of every chain that
    has one: ``{"rows": chain indices, "start": i * step, "lengths": frames of each row's window, "frames": padded frame count}``.
    ``frames`` is the longest row, or :data:`MIN_PAD_FRAMES` when :data:`MIN_PAD_BATCH` or more rows are all shorter than that."""
    per = [window_lengths(int(n), size, step) for n in chain_frames]
    plan = []
    for i in range(max(len(w) for w in per)):
        rows = [b for b, w in enumerate(per) if i < len(w)]
        lens = [per[b][i] for b in rows]
        pad = max(lens)
        if len(rows) >= MIN_PAD_BATCH and pad < MIN_PAD_FRAMES:
            pad = MIN_PAD_FRAMES
        plan.append({"rows": rows, "start": i * step, "lengths": lens, "frames": pad})
    return plan


def synchronised_window_plan(stream_frames: Sequence[int], n_poses: int, overlap_len: int) -> dict:
    """Every window of every stream as one row of ONE batch (synchronised window batches).  Stream ``s`` of
    ``stream_frames[s]`` frames gets exactly the windows of :func:`window_lengths` (size ``n_poses``, stride ``n_poses - overlap_len``);
    the rows are stream-major.  Returns ``{"stream": stream of each row, "window": its index in the stream, "left": the row of the previous
    window of the same stream or -1, "start": its first stream frame, "lengths": its frame count, "frames": the padded frame count of the
    batch, "ranges": one ``(first row, one past the last row)`` per stream}``.  ``frames`` follows :func:`ragged_window_plan`'s rule.
    Refuses ``overlap_len < 1`` (windows that share nothing are independent clips: ``generate_batch``) and ``2 * overlap_len > n_poses``
    (a window would share frames with its two neighbours at once)."""
    n_poses, L = int(n_poses), int(overlap_len)
    if L < 1:
        raise ValueError(f"synchronised windows need overlap_len >= 1, got {L}: windows that share no frame are independent clips (generate_batch)")
    if 2 * L > n_poses:
        raise ValueError(f"synchronised windows need 2 * overlap_len <= n_poses, got overlap_len = {L}, n_poses = {n_poses}")
    if len(stream_frames) == 0 or any(int(n) < 1 for n in stream_frames):
        raise ValueError(f"synchronised windows need at least one stream, of at least one frame each, got {list(stream_frames)}")
    step = n_poses - L
    plan = {"stream": [], "window": [], "left": [], "start": [], "lengths": [], "ranges": []}
    for s, n in enumerate(stream_frames):
        first = len(plan["stream"])
        for i, w in enumerate(window_lengths(int(n), n_poses, step)):
            plan["left"].append(len(plan["stream"]) - 1 if i > 0 else -1)
            plan["stream"].append(s); plan["window"].append(i); plan["start"].append(i * step); plan["lengths"].append(w)
        plan["ranges"].append((first, len(plan["stream"])))
    pad = max(plan["lengths"])
    if len(plan["stream"]) >= MIN_PAD_BATCH and pad < MIN_PAD_FRAMES:
        pad = MIN_PAD_FRAMES
    plan["frames"] = pad
    return plan


def stitch_synchronised(windows, plan: dict, overlap_len: int) -> List[torch.Tensor]:
    """The streams of a synchronised window batch ``windows [rows, T, ...]``: the chain's keep rule — the first
    ``length - overlap_len`` frames of every window but a stream's last, and the whole last window.  One tensor per stream."""
    L = int(overlap_len)
    out = []
    for lo, hi in plan["ranges"]:
        out.append(torch.cat([windows[r, :plan["lengths"][r] - (L if r < hi - 1 else 0)] for r in range(lo, hi)], 0))
    return out


class DDPMTrainer:
    """Sampling half of DDPMTrainer_show / DDPMTrainer_beat (ddpm_show_trainer.py:40-90)."""

    def __init__(self, args, encoder: UniDiffuser, eval_model=None):
        self.opt = args
        self.encoder = encoder
        self.device = encoder.device
        self.diffusion_steps = int(getattr(args, "diffusion_steps", 1000))
        betas = get_named_beta_schedule("linear", self.diffusion_steps)
        kw = dict(opt=args, betas=betas, model_mean_type=ModelMeanType.EPSILON,
                  model_var_type=ModelVarType.FIXED_SMALL, loss_type=None)
        self.diffusion = GaussianDiffusion(**kw)
        self._diffusion_kw = kw
        self.sampler = create_named_schedule_sampler("uniform", self.diffusion)      # ddpm_show_trainer.py:83
        # the reference hard-codes 'ddim25' here (ddpm_show_trainer.py:73, ddpm_beat_trainer.py:76): the defaults of the three options
        self.set_sampling(getattr(args, "sampling_steps", 25), getattr(args, "sampling_spacing", "ddim"), getattr(args, "solver", "ddim"))
        # validation (ddpm_show_trainer.py:440-583): eval_model = a metrics.HalfEmbeddingNet, or None for no FGD (--no_fgd)
        self.eval_model = eval_model
        self.pose_stats = None
        self.skeleton = None
        self.reset_validation()

    def set_sampling(self, steps: int = 25, spacing="ddim", solver: str = "ddim") -> None:
        """The sampling configuration of every DDIM path of this trainer (``generate_batch``, ``sample_arbitrary_len`` also with
        ``lengths=``, ``sample_inbetween``, ``sample_variations``, ``restyle``, the sharded chains and :class:`streaming.StreamPool`, which
        all sample through ``diffusion_ddim_val``): rebuilds that object.  ``steps`` evaluations of a plain clip; ``spacing="ddim"`` the
        reference's stride ('ddimK'), ``"logsnr"`` timesteps uniform in log-SNR ('logsnrK', :func:`diffusion.space_timesteps`), or an
        explicit list of original timesteps (its length must be ``steps``); ``solver="ddim" | "dpm2m"`` (``ddim_sample_loop``).  The
        defaults are the reference's hard-coded 'ddim25' with the DDIM step.  ``level=`` / ``strength=`` of the editing entries count in
        the current ``steps``.  Raises before anything changes: an unknown spacing / solver, a list of another length, ``dpm2m`` with
        ``opt.same_overlap_noisy``."""
        steps = int(steps)
        if solver not in ("ddim", "dpm2m"):
            raise ValueError(f'solver must be "ddim" or "dpm2m", got {solver!r}')
        if solver == "dpm2m" and bool(getattr(self.opt, "same_overlap_noisy", False)):
            raise NotImplementedError("the dpm2m solver does not keep the saved noisy tails of same_overlap_noisy")
        if isinstance(spacing, str):
            if spacing not in ("ddim", "logsnr"):
                raise ValueError(f'spacing must be "ddim", "logsnr" or a list of timesteps, got {spacing!r}')
            use = space_timesteps(self.diffusion_steps, f"{spacing}{steps}")
        else:
            use = set(int(t) for t in spacing)
            if len(use) != steps or len(use) != len(list(spacing)):
                raise ValueError(f"an explicit spacing needs {steps} distinct timesteps, got {len(list(spacing))}")
        self.diffusion_ddim_val = SpacedDiffusion(use_timesteps=use, solver=solver, rescale_timesteps=False, **self._diffusion_kw)
        self.sampling = (steps, spacing if isinstance(spacing, str) else sorted(use), solver)

    # ---- BEAT results tail: gesture channels as the reference's standardised Euler angles (ddpm_beat_trainer.py:1044-1060) ----
    def set_pose_stats(self, stats) -> None:
        """The dataset's pose statistics (a :class:`diffsheg_amd.glue.PoseStats`, or ``None`` to drop them), placed on this trainer's
        device.  Needed by ``pose_rep="euler"`` and :meth:`from_euler`; they change nothing else."""
        from .glue import PoseStats
        if stats is not None and not isinstance(stats, PoseStats):
            raise ValueError(f"set_pose_stats takes a glue.PoseStats, got {type(stats).__name__}")
        self.pose_stats = stats.to(self.device) if stats is not None else None

    def _euler_requested(self, pose_rep: str) -> bool:
        """``pose_rep`` of the sampling entry points: ``"axis_angle"`` (default) is the sampler's own representation, untouched."""
        if pose_rep == "axis_angle":
            return False
        if pose_rep != "euler":
            raise ValueError(f'pose_rep must be "axis_angle" or "euler", got {pose_rep!r}')
        if getattr(self.opt, "dataset_name", "talkshow") == "talkshow":
            raise ValueError('pose_rep="euler" is the BEAT results tail: SHOW results are SMPL-X parameters (glue.inv_standardize)')
        if not getattr(self.opt, "axis_angle", True):
            raise ValueError('pose_rep="euler" needs opt.axis_angle: without it the gesture channels already are Euler angles')
        if getattr(self, "pose_stats", None) is None:
            raise ValueError('pose_rep="euler" needs the pose statistics: call set_pose_stats first')
        return True

    def _gesture_split(self) -> int:
        return int(getattr(self.opt, "split_pos", self.encoder.cfg.split_pos))

    def _to_euler(self, motion: torch.Tensor, lengths=None) -> torch.Tensor:
        from .glue import axis_angle_to_euler
        return axis_angle_to_euler(motion, self.pose_stats, split_pos=self._gesture_split(), lengths=lengths)

    def from_euler(self, pose: torch.Tensor, lengths=None) -> torch.Tensor:
        """The inverse helper for ``motions``, ``head`` and ``tail``: ``[..., C]`` frames whose gesture channels are standardised Euler
        degrees (what ``pose_rep="euler"`` returns, or BVH poses normalised with the Euler statistics) -> the sampler's standardised
        axis-angle gesture channels (datasets/beat.py:376-401), expression channels unchanged; on the device.  ``lengths`` as for
        :func:`diffsheg_amd.glue.euler_to_axis_angle`."""
        from .glue import euler_to_axis_angle
        self._euler_requested("euler")
        return euler_to_axis_angle(pose.to(self.device), self.pose_stats, split_pos=self._gesture_split(), lengths=lengths)

    # ---- joint positions of a sampled result: forward kinematics on the device ----
    def set_skeleton(self, skeleton) -> None:
        """The skeleton of :meth:`joint_positions` / ``return_positions=True`` (a :class:`diffsheg_amd.glue.Skeleton`, or ``None`` to
        drop it), uploaded once to this trainer's device.  Needs :meth:`set_pose_stats` first; changes nothing else."""
        from .glue import Skeleton
        if skeleton is None:
            self.skeleton = None
            return
        if not isinstance(skeleton, Skeleton):
            raise ValueError(f"set_skeleton takes a glue.Skeleton, got {type(skeleton).__name__}")
        if getattr(self, "pose_stats", None) is None:
            raise ValueError("set_skeleton needs the pose statistics: call set_pose_stats first")
        if 3 * skeleton.channels != self._gesture_split() or self.pose_stats.channels != self._gesture_split():
            raise ValueError(f"set_skeleton: the skeleton drives {skeleton.channels} joints and the statistics have {self.pose_stats.channels} "
                             f"entries, the gesture channels are {self._gesture_split()}")
        skeleton.to(self.device)
        self.skeleton = skeleton

    def _positions_requested(self, return_positions) -> bool:
        """``return_positions`` of the sampling entry points: the default returns at once; otherwise the refusals of ``pose_rep="euler"``."""
        if not return_positions:
            return False
        if getattr(self.opt, "dataset_name", "talkshow") == "talkshow":
            raise ValueError("return_positions is built for BEAT: SHOW results are SMPL-X parameters, not joint rotations of a skeleton")
        if not getattr(self.opt, "axis_angle", True):
            raise ValueError("return_positions needs opt.axis_angle: the positions are computed from the sampler's axis-angle channels")
        if getattr(self, "pose_stats", None) is None:
            raise ValueError("return_positions needs the pose statistics: call set_pose_stats first")
        if getattr(self, "skeleton", None) is None:
            raise ValueError("return_positions needs a skeleton: call set_skeleton first")
        return True

    def joint_positions(self, result: torch.Tensor, lengths=None) -> torch.Tensor:
        """World-space joint positions ``[..., J, 3]`` of a sampled result ``[..., C]`` in the sampler's representation (standardised
        axis-angle gesture channels), on the device: :func:`diffsheg_amd.glue.joint_positions` with this trainer's skeleton and
        statistics.  ``lengths``: one frame count per clip; padded frames give zeros."""
        from .glue import joint_positions
        self._positions_requested(True)
        return joint_positions(result.to(self.device), self.skeleton, self.pose_stats, split_pos=self._gesture_split(), lengths=lengths)

    def generate_batch(self, audio_emb, p_id, dim_pose, add_cond={}, inpaint_dict=None, cond_scale=None, lengths=None,
                       pose_rep: str = "axis_angle", modality="both", expression=None, guidance=None, cfg_schedule=None,
                       return_positions: bool = False, **sampler_kw):
        """ddpm_show_trainer.py:163-198.  ``sampler_kw`` (noise_source= / seed=) is this build's
        noise-injection hook; the reference draws from the global torch RNG.  ``cond_scale`` (a float, or one value per batch
        row) overrides ``opt.cond_scale`` for this batch.  ``lengths`` (one frame count per row, ``1 .. T``): clips of different
        lengths padded to ``T`` frames — row ``b`` is sampled as its first ``lengths[b]`` frames alone, the padded frames of the
        result are 0 (the reference always passes ``cur_len = T``, which is the default).  ``pose_rep="euler"`` (BEAT): the gesture
        channels of the returned sample are the reference's standardised Euler degrees, the expression channels are untouched and
        padded frames stay 0; the default returns the sampler's result as it is, with no extra launch.  ``modality`` /
        ``expression`` (:meth:`UniDiffuser.set_condition`): ``"expression"`` samples the face alone (gesture columns of the result 0),
        ``"gesture"`` samples gestures for the given expression track ``[B, T, expression_dim]`` (expression columns = the track);
        ``inpaint_dict`` is honoured on the active columns only.  ``row_seeds=`` (in ``sampler_kw``, with ``row_keys=``): one Philox key
        per row in place of ``seed=`` — rows at different windows of their chains in one batch (:mod:`diffsheg_amd.streaming`).
        ``guidance`` (a :class:`diffsheg_amd.glue.MotionGuidance` built for ``[B, T, dim_pose]``): soft keyframes and velocity /
        acceleration damping, fused into every denoise step; with ``lengths`` the stencils end at each clip's own last frame.
        ``cfg_schedule`` (a :class:`diffsheg_amd.glue.CFGSchedule`): the weight of the classifier-free guidance per model timestep and
        encoder, and the std rescale of the guided eps, for this batch (default: the encoder's sticky ``set_guidance_schedule``).
        ``return_positions=True`` (BEAT, after :meth:`set_pose_stats` and :meth:`set_skeleton`): returns ``(result, positions)``, the
        result being the very tensor of the call without it and ``positions [B, T, J, 3]`` its joints in world space
        (:meth:`joint_positions`; always from the axis-angle result, also with ``pose_rep="euler"``; padded frames 0)."""
        euler = self._euler_requested(pose_rep)
        positions = self._positions_requested(return_positions)
        if cond_scale is not None:
            sampler_kw["cond_scale"] = cond_scale
        if cfg_schedule is not None:
            sampler_kw["cfg_schedule"] = cfg_schedule
        if guidance is not None:
            sampler_kw["cond_fn"] = guidance
        audio_emb = audio_emb.to(self.device)
        B, T = len(audio_emb), audio_emb.shape[1]
        if lengths is None:
            cur_len = torch.full((B,), T, dtype=torch.long)          # (host tensor: the loops read its values, a device tensor would cost a sync)
        else:
            cur_len = torch.tensor([int(v) for v in lengths], dtype=torch.long)
        model_kwargs = {"audio_emb": audio_emb, "length": cur_len, "person_id": p_id, "add_cond": add_cond,
                        "y": inpaint_dict, "pe_type": getattr(self.opt, "PE", "pe_sinu")}
        if (expression is not None or modality not in (None, "both", 0)) and normalize_modality(
                modality, expression, B, T, self.encoder.cfg.expression_dim, self.encoder.cfg.unidiffuser,
                bool(getattr(self.opt, "same_overlap_noisy", False))) != 0:
            model_kwargs["modality"], model_kwargs["expression"] = modality, expression
        if getattr(self.opt, "ddim", True):
            out = self.diffusion_ddim_val.ddim_sample_loop(self.encoder, (B, T, dim_pose), clip_denoised=False,
                                                           progress=True, model_kwargs=model_kwargs, **sampler_kw)
        else:
            out = self.diffusion.p_sample_loop(self.encoder, (B, T, dim_pose), clip_denoised=False, progress=True,
                                               model_kwargs=model_kwargs, **sampler_kw)
        if not euler and not positions:
            return out
        pos = self.joint_positions(out["sample"] if isinstance(out, dict) else out, lengths) if positions else None
        if euler:
            if isinstance(out, dict):           # (same_overlap_noisy: the saved noisy tail stays in the sampler's representation)
                out = dict(out, sample=self._to_euler(out["sample"], lengths))
            else:
                out = self._to_euler(out, lengths)
        return (out, pos) if positions else out

    # ---- validation loop tail: FGD encoder + MSE / PCK / diversity (ddpm_show_trainer.py:440-583) -----------------------
    def reset_validation(self) -> None:
        """Fresh meters (the reference creates them at the top of every validation pass)."""
        self._val_batches: List[dict] = []

    def load_fid_net(self, path: str, map_location="cpu"):
        """ddpm_show_trainer.py:294-306: the FGD autoencoder from ``checkpoint['model_state']`` or ``['state_dict']``, with or without
        a ``module.`` prefix, as ``self.eval_model`` (a :class:`diffsheg_amd.metrics.HalfEmbeddingNet` on this trainer's device)."""
        from .metrics import HalfEmbeddingNet
        checkpoint = torch.load(path, map_location=map_location)
        state_dict = checkpoint["model_state"] if "model_state" in checkpoint else checkpoint["state_dict"]
        self.eval_model = HalfEmbeddingNet(self.opt, state_dict, device=self.device)
        return self.eval_model

    @property
    def pck_joint_dim(self) -> int:
        """Trailing "joint" axis of the PCK: SHOW views the tensors as [B, T, C, 1], BEAT as [B, T, C / 3, 3]."""
        return 1 if getattr(self.opt, "dataset_name", "talkshow") == "talkshow" else 3

    def validate_batch(self, audio_emb, motions, p_id, add_cond={}, lengths=None, **sampler_kw) -> torch.Tensor:
        """One iteration of the reference's validation loop behind the data loader (ddpm_show_trainer.py:493-550): the reference's
        ``inpaint_dict`` (with ``opt.overlap_len > 0`` the first ``overlap_len`` frames are pinned to ``motions``), ``generate_batch``,
        both sides through ``eval_model`` (first ``n_poses`` frames; skipped when it is ``None``), MSE / PCK / diversity.  Everything
        stays on the device and nothing synchronises: the batch's few numbers and its latents are fetched by
        :meth:`validation_summary`.  Returns the samples ``[B, T, C]`` — bit-identical to ``generate_batch`` alone with the same
        arguments.  ``sampler_kw`` as for :meth:`generate_batch` (``seed=``, ``noise_source=``, ``cond_scale=``, ...)."""
        from .metrics import batch_metrics
        if normalize_modality(sampler_kw.get("modality", "both"), None) != 0:
            raise ValueError("validate_batch scores both modalities: MSE / PCK / diversity and the FGD encoder are defined on all channels")
        if lengths is not None:
            raise ValueError("validate_batch takes full clips only: the FGD encoder is defined for n_poses frames, and MSE / PCK / "
                             "diversity of padded frames would be meaningless (score ragged batches clip by clip)")
        opt = self.opt
        C_, L = int(opt.net_dim_pose), int(opt.overlap_len)
        motions = motions.to(device=self.device, dtype=torch.float32)
        if motions.shape[0] < 2:
            raise ValueError("validate_batch needs at least two clips: the reference's diversity divides by B_div (B_div - 1)")
        if self.eval_model is not None and motions.shape[1] < self.eval_model.n_poses:
            raise ValueError(f"clips have {motions.shape[1]} frames, the FGD encoder needs n_poses = {self.eval_model.n_poses}")
        inpaint_dict = {}
        if L > 0:
            mask = torch.zeros_like(motions, dtype=torch.bool)
            mask[..., :L, :] = True
            inpaint_dict = {"gt": motions, "outpainting_mask": mask, "outpainting_mask_any": True}
        outputs = self.generate_batch(audio_emb, p_id, C_, add_cond, inpaint_dict, **sampler_kw)
        if isinstance(outputs, dict):
            outputs = outputs["sample"]
        rec = batch_metrics(outputs, motions, self.pck_joint_dim)
        if self.eval_model is not None:
            rec["latent_out"] = self.eval_model(outputs)
            rec["latent_ori"] = self.eval_model(motions)
        self._val_batches.append(rec)
        return outputs

    def validation_summary(self, group=None) -> Dict[str, float]:
        """End of a validation pass (ddpm_show_trainer.py:552-571): one device-to-host copy of every batch's few numbers (and the
        latents), the meters, the Frechet distance of all latents of this rank, and — in an initialised process group — the
        reference's ``all_reduce`` of every meter (FGD is computed per rank and averaged through its meter, as there).  Returns
        ``{"MSE", "PCK", "Diversity"}`` and, with an ``eval_model``, ``"FGD"``; the meters stay readable as ``self.val_meters``."""
        import torch.distributed as dist
        from .metrics import AverageMeter, frechet_distance
        if not self._val_batches:
            raise ValueError("validation_summary: no validate_batch call since the last reset_validation")
        meters = {k: AverageMeter(k) for k in ("diversity", "pck", "mse", "fgd")}
        # one small tensor per batch: [mse, pck, diversity per group ...], gathered in a single copy
        flat = torch.cat([torch.cat([r["mse"].reshape(1), r["pck"].reshape(1), r["diversity"]]) for r in self._val_batches]).cpu().tolist()
        pos = 0
        for r in self._val_batches:
            n_groups = int(r["diversity"].numel())
            mse_val, pck_val = flat[pos], flat[pos + 1]
            for d in flat[pos + 2:pos + 2 + n_groups]:
                meters["diversity"].update(d, r["b_div"])
            meters["mse"].update(mse_val, r["batch"])
            meters["pck"].update(pck_val, r["batch"])
            pos += 2 + n_groups
        has_fgd = "latent_out" in self._val_batches[0]
        if has_fgd:
            lat_out = torch.cat([r["latent_out"] for r in self._val_batches]).cpu().numpy()
            lat_ori = torch.cat([r["latent_ori"] for r in self._val_batches]).cpu().numpy()
            meters["fgd"].update(frechet_distance(lat_out, lat_ori))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            for k, m in meters.items():
                if k != "fgd" or has_fgd:
                    m.all_reduce(group)
        self.val_meters = meters
        out = {"MSE": meters["mse"].avg, "PCK": meters["pck"].avg, "Diversity": meters["diversity"].avg}
        if has_fgd:
            out["FGD"] = meters["fgd"].avg
        return out

    # ---- the eval-mode forward of the training objective (ddpm_beat_trainer.py:135-181, :222-260) -----------------------------
    def _loss_kwargs(self, audio_emb, motions, p_id, add_cond, lengths):
        audio_emb = audio_emb.to(self.device)
        B, T = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        if getattr(self.opt, "use_single_style", False):                 # ddpm_beat_trainer.py:137-139
            p_id = torch.zeros_like(p_id)
            p_id[:, :1] = 1
        cur_len = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.tensor([int(v) for v in lengths], dtype=torch.long)
        x0 = motions.to(device=self.device, dtype=torch.float32)
        return x0, {"audio_emb": audio_emb, "length": cur_len, "person_id": p_id, "add_cond": add_cond, "y": None,
                    "pe_type": getattr(self.opt, "PE", "pe_sinu")}

    def denoising_losses(self, audio_emb, motions, p_id, add_cond={}, t=None, noise=None, seed=None, lengths=None, cond_scale=None,
                         row_keys=None) -> Dict[str, torch.Tensor]:
        """The reference's ``forward(batch, eval_mode=True)`` followed by the arithmetic of ``backward_G`` (ddpm_beat_trainer.py:135-181,
        :222-260; the SHOW trainer's are the same code), without the backward pass: "how well does the model predict the noise on this
        take".  ``motions [B, T, C]`` standardised; ``t`` an int or one timestep of the full process per row, ``None`` draws them from the
        uniform sampler (seeded by ``seed``; numpy's global state without one, as the reference); ``noise`` given or drawn from the Philox
        streams (``seed``; a ragged batch draws per row: ``row_keys``, by default the row numbers); ``lengths`` one frame count per row;
        ``cond_scale`` as for :meth:`generate_batch`.  Returns ``loss_model_pred`` (x 1000), ``loss_vel_rec`` (x 100), ``loss_x0_rec``
        (x 100, Huber at beta 0.1) and ``final_loss`` as 0-d fp64 device tensors, plus ``row_terms [B, 7]`` and ``frame_mse [B, T]``
        (:meth:`GaussianDiffusion.training_losses`).  Two quirks of the reference are kept: ``final_loss`` adds the UNSCALED velocity term
        (:247), and ``opt.expr_weight`` has no effect (:231 overwrites the weighted form).  The velocity and Huber terms are always
        included (``add_vel_loss`` past ``vel_loss_start``).  A batch without a single frame pair is refused.  No synchronisation."""
        if max([int(v) for v in lengths] if lengths is not None else [int(motions.shape[1])]) < 2:
            raise ValueError("denoising_losses: no row has two frames, loss_vel_rec has no frame pair to average over")
        x0, kw = self._loss_kwargs(audio_emb, motions, p_id, add_cond, lengths)
        B = int(x0.shape[0])
        if t is None:
            import numpy as np
            rng = None if seed is None else np.random.RandomState(_splitmix64(int(seed) & _M64) & 0xFFFFFFFF)
            t, _ = self.sampler.sample(B, "cpu", rng)                 # (host values: the tables are read on the host)
        if lengths is not None and noise is None and row_keys is None:
            row_keys = list(range(B))
        out = self.diffusion.training_losses(self.encoder, x0, t, kw, noise, seed=seed, row_keys=row_keys if noise is None else None,
                                             cond_scale=cond_scale)
        return dict(out["scalars"], row_terms=out["row_terms"], frame_mse=out["frame_mse"])

    def loss_profile(self, audio_emb, motions, p_id, add_cond={}, levels=None, seed: int = 0, cond_scale=None, full: bool = False):
        """The per-level curves of the reference's ``calc_bpd_loop`` (gaussian_diffusion.py:1446-1501): ``mse`` (eps) and ``xstart_mse`` per clip
        at every level, without the ``vb`` term — its decoder likelihood (``discretized_gaussian_log_likelihood``) assumes data in 1/255
        image bins, which standardised motion is not.  ``levels``: indices into ``diffusion_ddim_val``'s levels (default: all of them, 25
        unless :meth:`set_sampling` changed it), or with ``full=True`` timesteps of the full process.  The condition is set once; then one
        evaluation per level with one timestep for the whole batch (the regime where the embedding Linears run on the distinct speakers
        only).  The noise of a level comes from :func:`level_seed` ``(seed, original timestep)``: a level's result does not depend on which
        other levels are asked for.  Nothing synchronises inside.  Returns ``{"levels", "mse" [L, B], "xstart_mse" [L, B],
        "loss_model_pred" [L]}``, fp64 on the device."""
        diff = self.diffusion if full else self.diffusion_ddim_val
        levels = list(range(diff.num_timesteps)) if levels is None else [int(v) for v in levels]
        if not levels or any(v < 0 or v >= diff.num_timesteps for v in levels):
            raise ValueError(f"levels must be indices in 0 .. {diff.num_timesteps - 1}, got {levels}")
        x0, kw = self._loss_kwargs(audio_emb, motions, p_id, add_cond, None)
        mse, xmse, lmp = [], [], []
        for k in levels:
            out = diff.training_losses(self.encoder, x0, k, kw, seed=level_seed(seed, diff.timestep_map[k]), cond_scale=cond_scale)
            rows = out["row_terms"]
            mse.append(out["mse"])
            xmse.append(rows[:, 2] / rows[:, 5])
            lmp.append(out["scalars"]["loss_model_pred"])
        return {"levels": levels, "mse": torch.stack(mse), "xstart_mse": torch.stack(xmse), "loss_model_pred": torch.stack(lmp)}

    # ---- H2: arbitrary-length chain ---------------------------------------------------------
    def sample_arbitrary_len(self, audio_emb: torch.Tensor, p_id: torch.Tensor, add_cond: Dict[str, torch.Tensor],
                             noise_source_for_window=None, seed: Optional[int] = None,
                             motions: Optional[torch.Tensor] = None, row_keys: Optional[Sequence[int]] = None,
                             cond_scale=None, lengths: Optional[Sequence[int]] = None, pose_rep: str = "axis_angle",
                             modality="both", expression=None, guidance=None, cfg_schedule=None, return_positions: bool = False):
        """The per-video body of test_arbitrary_len (ddpm_show_trainer.py:864-906): windows of n_poses
        with stride n_poses-overlap_len; window k>0 out-paints from the last overlap_len frames of
        window k-1 (sequential chain).  Output stays on the device (the reference copies every window
        to the host).  ``opt.fix_very_first`` (ddpm_show_trainer.py:885-888): window 0 is out-painted too, from the
        LAST overlap_len frames of the first ground-truth window of ``motions`` (standardised, [B, N, C]) — the
        reference's indexing, kept as is.  Batch rows are independent chains of equal length.  ``cond_scale`` (a float, or one
        value per chain) is the guidance scale of every window of the chains (default: ``opt.cond_scale``).

        ``lengths`` (one frame count per chain): chains of DIFFERENT lengths — ``audio_emb`` / ``add_cond`` / ``motions`` are
        ``[B, N_max, ...]``, chain ``b`` is their first ``lengths[b]`` frames (what lies behind is never read into a valid frame).
        Every chain is sampled exactly as alone: its own window list (:func:`ragged_window_plan`), its next window out-painted from
        ITS last ``overlap_len`` valid frames, with ``row_keys`` its own noise.  Returns a LIST of ``[lengths[b], C]`` tensors
        (not a padded tensor); ``opt.same_overlap_noisy`` is refused.

        ``pose_rep="euler"`` (BEAT, after :meth:`set_pose_stats`): the chain is sampled as always and the gesture channels of the
        finished result (of every result of the list form) are converted to the reference's standardised Euler degrees.

        ``modality`` / ``expression``: one modality alone for every window of the chains (:meth:`generate_batch`).  The track of
        ``"gesture"`` is ``[B, N, E]``, ``[N, E]`` (one track for every chain) or, with ``lengths``, a list of ``[lengths[b], E]``
        tensors; it is cut into windows exactly like the audio.  The overlap hand-off, ``fix_very_first`` and the out-painting mask
        act on the active columns only; ``opt.same_overlap_noisy`` is refused.

        ``guidance`` (a :class:`diffsheg_amd.glue.MotionGuidance`; chains of equal length only): its ``target`` / ``weight`` are
        stream-long ``[B, N, C]`` and cut into windows like the audio, ``vel`` / ``acc`` / ``space`` / ``level_scale`` are shared by every
        window.  The stencils are per window: smoothness is NOT enforced across a window boundary (the out-painted overlap carries the
        previous window's frames).  With ``lengths`` (the ragged chain) it raises ``NotImplementedError``.

        ``cfg_schedule`` (a :class:`diffsheg_amd.glue.CFGSchedule`): the guidance schedule of every window, in both forms.

        ``return_positions=True`` (BEAT, after :meth:`set_pose_stats` and :meth:`set_skeleton`): returns ``(result, positions)`` — the
        result of the call without it, and the world-space joints ``[B, N, J, 3]`` of the finished stream (with ``lengths`` a list of
        ``[lengths[b], J, 3]`` tensors from one launch), always computed from the axis-angle result."""
        if guidance is not None and lengths is not None:
            raise NotImplementedError("guidance in the ragged chain (lengths=) is not built")
        euler = self._euler_requested(pose_rep)
        positions = self._positions_requested(return_positions)
        expression = self._chain_track(modality, expression, int(audio_emb.shape[0]), int(audio_emb.shape[1]), lengths)
        if guidance is not None:
            N = int(audio_emb.shape[1])
            for name in ("target", "weight"):
                v = getattr(guidance, name)
                if v is not None and (v.dim() != 3 or int(v.shape[0]) != int(audio_emb.shape[0]) or int(v.shape[1]) != N):
                    raise ValueError(f"guidance: {name} must be stream-long [B, N, C] = [{int(audio_emb.shape[0])}, {N}, C], got {tuple(v.shape)}")
        if lengths is not None:
            outs = self._sample_arbitrary_len_ragged(audio_emb, p_id, add_cond, [int(v) for v in lengths], noise_source_for_window, seed,
                                                     motions, row_keys, cond_scale, modality, expression, cfg_schedule)
            res = [self._to_euler(o) for o in outs] if euler else outs
            if not positions:
                return res
            pos = self.joint_positions(torch.cat(outs, 0))
            return res, list(torch.split(pos, [int(o.shape[0]) for o in outs], 0))
        opt = self.opt
        n_poses, L, C = int(opt.n_poses), int(opt.overlap_len), int(opt.net_dim_pose)
        step = n_poses - L
        audio_list = get_windows(audio_emb, n_poses, step)
        expr_list = get_windows(expression, n_poses, step) if expression is not None else [None] * len(audio_list)
        cond_list = get_windows(add_cond, n_poses, step) if add_cond not in (None, {}) else [{}] * len(audio_list)
        fix_first = bool(getattr(opt, "fix_very_first", False)) and L > 0
        if fix_first and motions is None:
            raise ValueError("fix_very_first needs the ground-truth motions of the clip")
        motion_list = get_windows(motions.to(self.device), n_poses, step) if fix_first else None
        guide_list = [None] * len(audio_list)
        if guidance is not None:
            if guidance.target is None:
                guide_list = [guidance] * len(audio_list)
            else:
                guide_list = [guidance.with_terms(y.contiguous(), w.contiguous()) for y, w in
                              zip(get_windows(guidance.target, n_poses, step), get_windows(guidance.weight, n_poses, step))]
        outs: List[torch.Tensor] = []
        outputs = None
        son = bool(getattr(opt, "same_overlap_noisy", False))     # ddpm_beat_trainer.py:1006,1022-1028
        previous_noisy_tail = None
        for ii, (a, cnd, ex) in enumerate(zip(audio_list, cond_list, expr_list)):
            inpaint_dict = {"clip_idx": ii} if son else {}
            if L > 0:
                B, T = a.shape[0], a.shape[1]
                inpaint_dict["gt"] = torch.zeros(B, T, C, device=self.device)
                inpaint_dict["outpainting_mask"] = torch.zeros(B, T, C, dtype=torch.bool, device=self.device)
                inpaint_dict["outpainting_mask_any"] = ii > 0 or fix_first     # what `True in mask` would say, without the sync
                if ii == 0 and fix_first:
                    inpaint_dict["outpainting_mask"][..., :L, :] = True
                    inpaint_dict["gt"][:, :L, ...] = motion_list[0][:, -L:, ...]
                elif ii > 0:
                    inpaint_dict["outpainting_mask"][..., :L, :] = True
                    inpaint_dict["gt"][:, :L, ...] = outputs[:, -L:, ...]
                    if son:
                        inpaint_dict["previous_noisy_tail"] = previous_noisy_tail
            kw = {}
            if noise_source_for_window is not None:
                kw["noise_source"] = noise_source_for_window(ii)
            elif seed is not None:
                kw["seed"] = window_seed(seed, ii)
            if row_keys is not None:
                kw["row_keys"] = row_keys          # Philox: one stream per (window, chain): key = hash(seed, window), counter high words = chain id
            if cond_scale is not None:
                kw["cond_scale"] = cond_scale
            if ex is not None or modality not in (None, "both", 0):
                kw["modality"], kw["expression"] = modality, ex
            if guide_list[ii] is not None:
                kw["guidance"] = guide_list[ii]
            if cfg_schedule is not None:
                kw["cfg_schedule"] = cfg_schedule
            outputs = self.generate_batch(a, p_id, C, cnd, inpaint_dict, **kw)
            if son:
                previous_noisy_tail, outputs = outputs["saved_noisy_tail"], outputs["sample"]
            outs.append(outputs if ii == len(audio_list) - 1 else outputs[:, :step])
        full = torch.cat(outs, dim=1)
        res = self._to_euler(full) if euler else full
        return (res, self.joint_positions(full)) if positions else res


    def _chain_track(self, modality, expression, B: int, N: int, lengths) -> Optional[torch.Tensor]:
        """The ``expression`` argument of the chain entry points -> ``None`` (no gesture-only run) or the padded track ``[B, N, E]``."""
        if expression is None and modality in (None, "both", 0):
            return None                                  # the joint run: nothing to validate, nothing changes
        E = self.encoder.cfg.expression_dim
        if isinstance(expression, (list, tuple)):
            if len(expression) != B or lengths is None or any(tuple(t.shape) != (int(n), E) for t, n in zip(expression, lengths)):
                raise ValueError(f"expression as a list needs lengths= and one [lengths[b], {E}] tensor per chain")
            pad = expression[0].new_zeros(B, N, E)
            for b, t in enumerate(expression):
                pad[b, :t.shape[0]] = t
            expression = pad
        elif isinstance(expression, torch.Tensor) and expression.dim() == 2:
            expression = expression.unsqueeze(0).expand(B, -1, -1)
        if normalize_modality(modality, expression, B, N, E, self.encoder.cfg.unidiffuser,
                              bool(getattr(self.opt, "same_overlap_noisy", False))) != 2:
            return None
        return expression

    def _sample_arbitrary_len_ragged(self, audio_emb, p_id, add_cond, lengths: List[int], noise_source_for_window, seed, motions,
                                     row_keys, cond_scale, modality="both", expression=None, cfg_schedule=None) -> List[torch.Tensor]:
        opt = self.opt
        n_poses, L, C = int(opt.n_poses), int(opt.overlap_len), int(opt.net_dim_pose)
        step = n_poses - L
        B, N_max = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        if len(lengths) != B or any(n < 1 or n > N_max for n in lengths):
            raise ValueError(f"lengths needs one frame count in 1 .. {N_max} per chain ({B}), got {lengths}")
        if bool(getattr(opt, "same_overlap_noisy", False)):
            raise NotImplementedError("same_overlap_noisy with per-chain lengths: the saved noisy tails address the padded window")
        add_cond = add_cond or {}
        fix_first = bool(getattr(opt, "fix_very_first", False)) and L > 0
        if fix_first and motions is None:
            raise ValueError("fix_very_first needs the ground-truth motions of the clip")
        if fix_first and min(lengths) < L:
            raise ValueError(f"fix_very_first pins overlap_len = {L} frames of every chain's first window: chains need at least that many frames, got {lengths}")
        pid = p_id if p_id.dim() == 2 else p_id.unsqueeze(0)
        if pid.shape[0] == 1:
            pid = pid.expand(B, -1)
        gs = normalize_guidance_scale(cond_scale)              # None / one value / one per chain
        if gs is not None and len(gs) not in (1, B):
            raise ValueError(f"cond_scale needs one value or one per chain ({B}), got {len(gs)}")

        def cut(t: torch.Tensor, rows: List[int], start: int, frames: int) -> torch.Tensor:
            w = t[rows, start:start + frames]
            if w.shape[1] < frames:                      # (a batch of short tails padded beyond the longest stream)
                w = torch.cat([w, w.new_zeros((w.shape[0], frames - w.shape[1]) + tuple(w.shape[2:]))], 1)
            return w

        pieces: List[List[torch.Tensor]] = [[] for _ in range(B)]
        tails: List[Optional[torch.Tensor]] = [None] * B       # chain -> its last overlap_len valid frames so far
        plan = ragged_window_plan(lengths, n_poses, step)
        n_win = [len(window_lengths(n, n_poses, step)) for n in lengths]
        for ii, wb in enumerate(plan):
            rows, lens, T = wb["rows"], wb["lengths"], wb["frames"]
            a = cut(audio_emb, rows, wb["start"], T)
            cnd = {k: cut(v, rows, wb["start"], T) for k, v in add_cond.items()}
            inpaint_dict = {}
            if L > 0:
                gt = torch.zeros(len(rows), T, C, device=self.device)
                mask = torch.zeros(len(rows), T, C, dtype=torch.bool, device=self.device)
                inpaint_dict["outpainting_mask_any"] = ii > 0 or fix_first
                if ii == 0 and fix_first:
                    mask[:, :L] = True
                    for r, b in enumerate(rows):         # (the reference's indexing: the LAST overlap_len frames of the chain's first window)
                        gt[r, :L] = motions[b, lens[r] - L:lens[r]].to(self.device)
                elif ii > 0:
                    mask[:, :L] = True
                    gt[:, :L] = torch.stack([tails[b] for b in rows], 0)
                inpaint_dict["gt"], inpaint_dict["outpainting_mask"] = gt, mask
            kw = {}
            if noise_source_for_window is not None:
                kw["noise_source"] = noise_source_for_window(ii)
            elif seed is not None:
                kw["seed"] = window_seed(seed, ii)
            if row_keys is not None:
                kw["row_keys"] = [row_keys[b] for b in rows]
            if gs is not None:
                kw["cond_scale"] = gs[0] if len(gs) == 1 else [gs[b] for b in rows]
            if any(n != T for n in lens):
                kw["lengths"] = lens
            if cfg_schedule is not None:
                kw["cfg_schedule"] = cfg_schedule
            if expression is not None or modality not in (None, "both", 0):
                kw["modality"] = modality
                kw["expression"] = cut(expression, rows, wb["start"], T).contiguous() if expression is not None else None
            out = self.generate_batch(a, pid[rows], C, cnd, inpaint_dict, **kw)
            for r, b in enumerate(rows):
                n = lens[r]
                if L > 0:
                    tails[b] = out[r, n - L:n]
                pieces[b].append(out[r, :n] if ii == n_win[b] - 1 else out[r, :step])
        return [torch.cat(p, 0) for p in pieces]

    # ---- long streams as ONE batch: synchronised windows ---------------------
    def sample_arbitrary_len_synchronised(self, audio_emb: torch.Tensor, p_id: torch.Tensor, add_cond: Dict[str, torch.Tensor], seed: int,
                                          row_keys: Optional[Sequence[int]] = None, lengths: Optional[Sequence[int]] = None,
                                          cond_scale=None, cfg_schedule=None, guidance=None, modality="both", expression=None,
                                          pose_rep: str = "axis_angle", return_windows: bool = False):
        """Long streams without a window chain: every window of every stream (:func:`synchronised_window_plan`) is one row of ONE batch,
        all rows run the plain sampling loop together, and behind every denoise step the ``overlap_len`` frames two neighbouring windows
        share are reconciled by the ``addBlend`` cross-fade (``ddim_sample_loop(sync_left=)``), so both carry the same values there.
        Nothing is sequential across windows and there is no seam to repair; the result is NOT the reference's out-painting chain.

        ``audio_emb`` / ``add_cond`` are streams ``[S, N, ...]``; with ``lengths`` stream ``s`` is their first ``lengths[s]`` frames and
        the result is a list of ``[lengths[s], C]`` tensors (as in :meth:`sample_arbitrary_len`), else ``[S, N, C]``.  ``p_id`` and
        ``cond_scale`` (a float, or one per stream) are per stream.  Noise: every stream frame owns ONE value — ``z [S, N, C]`` from the
        per-row Philox streams (key ``seed``, counter high words ``row_keys``, default the stream numbers; draw 0) is cut into windows like
        the audio, so windows that overlap start from the same noise, and a stream's noise depends on ``(seed, its key, its length)``
        alone; ``N * C`` and every ``lengths[s] * C`` must be multiples of 4.  ``guidance`` (a :class:`diffsheg_amd.glue.MotionGuidance`):
        ``target`` / ``weight`` are stream-long ``[S, N, C]`` and cut like the audio, in both forms; the stencils are per window.
        ``cfg_schedule``, ``modality`` / ``expression`` (the track ``[S, N, E]``, ``[N, E]`` or with ``lengths`` a list) and ``pose_rep``
        as in the chain; :meth:`set_sampling` (steps, spacing, ``solver="dpm2m"``) applies.  ``return_windows=True``: also the raw
        ``[rows, T, C]`` batch (the sampler's representation) and the plan.

        Refused before any device call: ``opt.ddim`` off (the DDPM loop draws per-window noise at every step), ``opt.fix_very_first``
        (a mask), ``opt.same_overlap_noisy``; there is no ``noise_source``: a stack of per-window draws is what the scheme excludes."""
        opt = self.opt
        if not getattr(opt, "ddim", True):
            raise NotImplementedError("synchronised windows need the DDIM loop (opt.ddim): the DDPM loop draws per-window noise at every step")
        if bool(getattr(opt, "fix_very_first", False)):
            raise NotImplementedError("synchronised windows take no mask: opt.fix_very_first out-paints the first window")
        if bool(getattr(opt, "same_overlap_noisy", False)):
            raise NotImplementedError("synchronised windows with opt.same_overlap_noisy: nothing is handed from window to window")
        euler = self._euler_requested(pose_rep)
        n_poses, L, C = int(opt.n_poses), int(opt.overlap_len), int(opt.net_dim_pose)
        S, N = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        if lengths is not None:
            lengths = [int(v) for v in lengths]
            if len(lengths) != S or any(n < 1 or n > N for n in lengths):
                raise ValueError(f"lengths needs one frame count in 1 .. {N} per stream ({S}), got {lengths}")
        plan = synchronised_window_plan(lengths if lengths is not None else [N] * S, n_poses, L)
        if (N * C) % 4 or any((n * C) % 4 for n in (lengths or [])):
            raise ValueError("synchronised windows: frames * channels of every stream must be a multiple of 4 (per-row Philox streams)")
        keys = list(range(S)) if row_keys is None else [int(k) for k in row_keys]
        if len(keys) != S:
            raise ValueError(f"row_keys needs one key per stream ({S}), got {len(keys)}")
        gs = normalize_guidance_scale(cond_scale)              # None / one value / one per stream
        if gs is not None and len(gs) not in (1, S):
            raise ValueError(f"cond_scale needs one value or one per stream ({S}), got {len(gs)}")
        expression = self._chain_track(modality, expression, S, N, lengths)
        if guidance is not None:
            for name in ("target", "weight"):
                v = getattr(guidance, name)
                if v is not None and (v.dim() != 3 or int(v.shape[0]) != S or int(v.shape[1]) != N):
                    raise ValueError(f"guidance: {name} must be stream-long [S, N, C] = [{S}, {N}, C], got {tuple(v.shape)}")
        T, rows, step = plan["frames"], len(plan["stream"]), n_poses - L

        def cut(t: torch.Tensor) -> torch.Tensor:
            """``[S, N, ...]`` -> the plan's rows ``[rows, T, ...]``, zero behind every row's length."""
            if lengths is None:                          # equal streams: window i of every stream at once, then stream-major
                wins = [torch.cat([w, w.new_zeros((S, T - w.shape[1]) + tuple(w.shape[2:]))], 1) if w.shape[1] < T else w
                        for w in get_windows(t, n_poses, step)]
                return torch.stack(wins, 1).reshape((rows, T) + tuple(t.shape[2:])).contiguous()
            dev = t.device
            frame = torch.tensor(plan["start"], device=dev)[:, None] + torch.arange(T, device=dev)[None]
            valid = torch.arange(T, device=dev)[None] < torch.tensor(plan["lengths"], device=dev)[:, None]
            w = t[torch.tensor(plan["stream"], device=dev)[:, None], frame.clamp_(max=N - 1)]
            return w * valid.reshape(valid.shape + (1,) * (t.dim() - 2)).to(w.dtype)

        audio_emb = audio_emb.to(self.device)
        a = cut(audio_emb)
        cnd = {k: cut(v.to(self.device)) for k, v in (add_cond or {}).items()}
        pid = p_id if p_id.dim() == 2 else p_id.unsqueeze(0)
        if pid.shape[0] == 1:
            pid = pid.expand(S, -1)
        pid = pid[plan["stream"]]
        dd = self.diffusion_ddim_val
        z = dd.draw_noise(S, N, C, self.device, int(seed), keys, None, lengths)
        # (seed: the loop's own draws are unused at eta = 0; given so that the call does not advance the default-seed counter)
        kw = {"noise": cut(z), "sync_left": plan["left"], "sync_len": L, "seed": int(seed)}
        ragged = any(n != T for n in plan["lengths"])
        if ragged:
            kw["lengths"] = plan["lengths"]
        if gs is not None:
            kw["cond_scale"] = gs[0] if len(gs) == 1 else [gs[s] for s in plan["stream"]]
        if cfg_schedule is not None:
            kw["cfg_schedule"] = cfg_schedule
        if expression is not None or modality not in (None, "both", 0):
            kw["modality"] = modality
            kw["expression"] = cut(expression.to(self.device)) if expression is not None else None
        if guidance is not None:
            kw["guidance"] = guidance if guidance.target is None else guidance.with_terms(cut(guidance.target), cut(guidance.weight))
        windows = self.generate_batch(a, pid, C, cnd, {}, **kw)
        streams = stitch_synchronised(windows, plan, L)
        if lengths is not None:
            out = [self._to_euler(s) for s in streams] if euler else streams
        else:
            out = torch.stack(streams, 0)
            out = self._to_euler(out) if euler else out
        return (out, windows, plan) if return_windows else out

    # ---- a speech signal in, motion out -------------------------------------------------------
    def sample_custom_audio(self, wave16k, p_id: torch.Tensor, frontend, **kw):
        """``test_custom_aud`` (ddpm_show_trainer.py:944-1100) for a 16 kHz signal: ``frontend.features(wave16k)`` (an
        :class:`diffsheg_amd.audio.AudioFrontEnd`: mel ``[N, 128]`` and HuBERT ``[N, 1024]`` on the device) followed by
        :meth:`sample_arbitrary_len`; ``kw`` (``seed=``, ``pose_rep=``, ``modality=``, ``cond_scale=`` ...) passes through.  A list of
        signals is sampled as chains of different lengths (the ``lengths=`` form: a list of results).  The reference's ``.wav`` branch
        hands HuBERT the 22 050 Hz signal of ``librosa.load`` as if it were 16 kHz; this call takes a 16 kHz signal, the ``.npy``
        branch and what the model was trained on."""
        if isinstance(wave16k, (list, tuple)):
            mel, hub, lengths = frontend.features_batch(wave16k)
            return self.sample_arbitrary_len(mel, p_id, {"pretrain_aud_feat": hub}, lengths=lengths, **kw)
        mel, hub = frontend.features(wave16k)
        return self.sample_arbitrary_len(mel[None], p_id, {"pretrain_aud_feat": hub[None]}, **kw)

    # ---- motion in-betweening: one window pinned at both ends ---------------------------------
    def sample_inbetween(self, audio_emb: torch.Tensor, p_id: torch.Tensor, add_cond: Dict[str, torch.Tensor],
                         head: torch.Tensor, tail: torch.Tensor, *, tail_blend: bool = True, seed: Optional[int] = None,
                         row_keys: Optional[Sequence[int]] = None, noise_source=None, cond_scale=None, modality="both",
                         expression=None, guidance=None) -> torch.Tensor:
        """"Here are two clips and the audio between them, fill the gap": ``audio_emb [B, T, 128]`` (+ ``add_cond``) conditions one
        window, whose first ``L = opt.overlap_len`` frames are pinned to ``head`` and whose last ``L`` to ``tail`` (both ``[B, L, C]``,
        standardised motion; ``2 L < T``); the frames in between are sampled.  This is the reference's own out-painting loop
        (``ddim_sample_loop`` on a mask, gaussian_diffusion.py:1034-1056, RePaint schedule :1106-1159; ``jump_length``,
        ``jump_n_sample``, ``no_resample``, ``no_repaint`` act as in a chained window) on a mask that is True at both ends.
        With ``tail_blend=False`` it is exactly that loop: generated motion is cross-faded into the pinned frames on the head side
        only (``addBlend``).  ``tail_blend=True`` (default) adds the mirrored fade on the last ``L`` frames.  Needs ``opt.ddim``
        (mask-present DDPM is not built).  Returns the window ``[B, T, C]`` on the device; no host sync.  ``modality`` /
        ``expression`` ``[B, T, E]`` as for :meth:`generate_batch`: the pinned frames act on the active columns only.  ``guidance``
        (:class:`diffsheg_amd.glue.MotionGuidance` for ``[B, T, C]``) steers the frames in between; the pinned frames stay pinned."""
        opt = self.opt
        L, C = int(opt.overlap_len), int(opt.net_dim_pose)
        if not getattr(opt, "ddim", True):
            raise NotImplementedError("sample_inbetween needs opt.ddim (mask-present DDPM sampling is not built)")
        B, T = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        if L <= 0 or 2 * L >= T:
            raise ValueError(f"sample_inbetween needs 0 < 2 * overlap_len < T (overlap_len = {L}, T = {T})")
        if tuple(head.shape) != (B, L, C) or tuple(tail.shape) != (B, L, C):
            raise ValueError(f"head / tail must be [B, overlap_len, C] = {(B, L, C)}, got {tuple(head.shape)} / {tuple(tail.shape)}")
        gt = torch.zeros(B, T, C, device=self.device)
        gt[:, :L] = head.to(self.device)
        gt[:, T - L:] = tail.to(self.device)
        mask = torch.zeros(B, T, C, dtype=torch.bool, device=self.device)
        mask[:, :L] = True
        mask[:, T - L:] = True
        kw = {"tail_blend": bool(tail_blend)}
        for k, v in (("seed", seed), ("row_keys", row_keys), ("noise_source", noise_source), ("cond_scale", cond_scale), ("guidance", guidance)):
            if v is not None:
                kw[k] = v
        if expression is not None or modality not in (None, "both", 0):
            kw["modality"], kw["expression"] = modality, expression
        out = self.generate_batch(audio_emb, p_id, C, add_cond, {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}, **kw)
        return out["sample"] if isinstance(out, dict) else out

    # ---- editing an existing take: variations close to it, re-rolled regions, another speaker's style ------------------------
    @staticmethod
    def strength_to_level(strength: float, respacing: int = 25) -> int:
        """``strength`` in ``(0, 1]`` -> start level ``K = max(1, round(strength * respacing))`` (Python's ``round``: halves go to the
        even neighbour).  1 is the whole schedule, i.e. nothing of the input survives but its kept elements."""
        s = float(strength)
        if not 0.0 < s <= 1.0:
            raise ValueError(f"strength must be in (0, 1], got {strength}")
        return max(1, int(round(s * int(respacing))))

    def _edit_level(self, level, strength) -> int:
        R = self.diffusion_ddim_val.num_timesteps
        if (level is None) == (strength is None):
            raise ValueError("give level= (1 .. respacing) or strength= (0 .. 1], one of the two")
        K = int(level) if level is not None else self.strength_to_level(strength, R)
        if not 1 <= K <= R:
            raise ValueError(f"level must be in 1 .. {R}, got {level}")
        if not getattr(self.opt, "ddim", True):
            raise NotImplementedError("editing needs opt.ddim (restarts of the DDPM loop are not built)")
        return K

    def sample_variations(self, motions: torch.Tensor, audio_emb: torch.Tensor, p_id: torch.Tensor, add_cond: Dict[str, torch.Tensor], *,
                          level: Optional[int] = None, strength: Optional[float] = None, keep: Optional[torch.Tensor] = None,
                          seed: Optional[int] = None, row_keys: Optional[Sequence[int]] = None, row_seeds: Optional[Sequence[int]] = None,
                          cond_scale=None, lengths=None, modality="both", expression=None, pose_rep: str = "axis_angle",
                          guidance=None, cfg_schedule=None) -> torch.Tensor:
        """Variations of an existing motion ``motions [B, T, C]`` (standardised, the sampler's representation): it is noised to spaced
        level ``K - 1`` (``q_sample`` with the loop's draw 0) and denoised from there with the DDIM loop, in one native call.  ``level=K``
        (``1 .. respacing``) or ``strength=s`` (``K = max(1, round(s * respacing))``): small K stays close to the input, K = respacing
        keeps nothing of it.  Two seeds give two variations; ``row_keys`` / ``row_seeds`` / ``lengths`` / ``modality`` / ``expression``
        / ``cond_scale`` / ``cfg_schedule`` / ``pose_rep`` as for :meth:`generate_batch` (the gains are indexed by the original timestep, so a
        restart reads the same table as the whole loop).

        ``keep`` (bool, broadcastable to ``[B, T, C]``, True = leave as it is; :func:`diffsheg_amd.glue.edit_region` builds one): the
        RePaint path — ``gt = motions``, ``mask = keep``, the jump schedule walked from ``t_T = K`` — with ``addBlend`` off (the
        reference's fade would rewrite kept frames ``[:overlap_len]``).  Kept elements of the result are the input bit for bit: the
        last step blends ``1 * gt + 0 * n``.  ``opt.fix_head_var`` is refused (q_sample would keep the head channels un-noised).
        ``guidance`` (:class:`diffsheg_amd.glue.MotionGuidance`) steers the re-sampled elements softly; kept elements stay bit for bit."""
        if getattr(self.opt, "fix_head_var", False):
            raise NotImplementedError("sample_variations with opt.fix_head_var is not built")
        K = self._edit_level(level, strength)
        if bool(getattr(self.opt, "same_overlap_noisy", False)):
            raise NotImplementedError("sample_variations with same_overlap_noisy: the saved noisy tails describe whole schedules")
        audio_emb = audio_emb.to(self.device)
        B, T, C = int(audio_emb.shape[0]), int(audio_emb.shape[1]), int(self.opt.net_dim_pose)
        if tuple(motions.shape) != (B, T, C):
            raise ValueError(f"motions must be [B, T, C] = {(B, T, C)}, got {tuple(motions.shape)}")
        x0 = motions.to(device=self.device, dtype=torch.float32)
        kw = {"start_level": K, "x_start": x0}
        inpaint = {}
        if keep is not None:
            if keep.dtype != torch.bool:
                raise ValueError(f"keep must be a bool mask, got {keep.dtype}")
            try:
                mask = keep.to(self.device).expand(B, T, C)
            except RuntimeError as e:
                raise ValueError(f"keep {tuple(keep.shape)} does not broadcast to {(B, T, C)}") from e
            inpaint = {"gt": x0, "outpainting_mask": mask}
            kw["add_blend"] = False
        for k, v in (("seed", seed), ("row_keys", row_keys), ("row_seeds", row_seeds), ("cond_scale", cond_scale), ("guidance", guidance),
                     ("cfg_schedule", cfg_schedule)):
            if v is not None:
                kw[k] = v
        return self.generate_batch(audio_emb, p_id, C, add_cond, inpaint, lengths=lengths, pose_rep=pose_rep, modality=modality,
                                   expression=expression, **kw)

    def restyle(self, motions: torch.Tensor, audio_emb: torch.Tensor, p_id_from: torch.Tensor, p_id_to: torch.Tensor,
                add_cond: Dict[str, torch.Tensor], *, level: int, cond_scale=None, guidance=None) -> torch.Tensor:
        """"Same performance, other speaker's style": ``motions [B, T, C]`` is inverted to spaced level ``K = level`` with the DDIM
        reverse ODE under the source speaker ``p_id_from`` (``ddim_reverse_sample`` at levels ``0 .. K-1``, gaussian_diffusion.py:1068-1104)
        and decoded under the target speaker ``p_id_to`` with ``ddim_sample_loop(start_level=K, noise=inverted)`` at ``eta = 0``.

        Index convention (the reference's, and guided-diffusion's): the reverse step at level ``k`` moves x from ``alphas_cumprod[k]`` to
        ``alphas_cumprod_next[k] = alphas_cumprod[k + 1]``, so the reverse loop ENDS at ``alphas_cumprod[K]``; the forward step at level
        ``k`` reads x as being at ``alphas_cumprod[k]``, so decoding ``K`` steps STARTS at ``alphas_cumprod[K - 1]``.  The pairing is off
        by one level on purpose — it is the one guided-diffusion's own encode / decode loops use — and it is not an exact inverse, even
        under one speaker.  Deterministic: no draws on either side.  ``guidance`` is not built here (the reverse ODE takes none):
        ``NotImplementedError``."""
        if guidance is not None:
            raise NotImplementedError("guidance in restyle is not built: the DDIM reverse ODE takes no guidance")
        K = self._edit_level(level, None)
        audio_emb = audio_emb.to(self.device)
        B, T, C = int(audio_emb.shape[0]), int(audio_emb.shape[1]), int(self.opt.net_dim_pose)
        if tuple(motions.shape) != (B, T, C):
            raise ValueError(f"motions must be [B, T, C] = {(B, T, C)}, got {tuple(motions.shape)}")
        model_kwargs = {"audio_emb": audio_emb, "length": None, "person_id": p_id_from, "add_cond": add_cond, "y": {},
                        "pe_type": getattr(self.opt, "PE", "pe_sinu")}
        inv = self.diffusion_ddim_val.ddim_reverse_sample_loop(self.encoder, motions.to(self.device), K, model_kwargs=model_kwargs,
                                                               cond_scale=cond_scale)
        kw = {"start_level": K, "noise": inv, "seed": 0}
        if cond_scale is not None:
            kw["cond_scale"] = cond_scale
        out = self.generate_batch(audio_emb, p_id_to, C, add_cond, {}, **kw)
        return out["sample"] if isinstance(out, dict) else out

    def sample_arbitrary_len_sharded(self, *args, **kw) -> Optional[torch.Tensor]:
        """Long stream -> independent chains over the ranks -> gather on rank 0 -> optionally the seams between the chains
        re-sampled as in-betweening windows (module-level function below)."""
        return sample_arbitrary_len_sharded(self, *args, **kw)


# ---- multi-GPU: independent chains / batch rows sharded over ranks -----------------
def shard_range(n_items: int, rank: int, world: int) -> range:
    """Contiguous, balanced split of ``n_items`` independent units; no data-path collective is needed
    because no tensor couples two batch rows / two chains anywhere on the path."""
    base, extra = divmod(n_items, world)
    lo = rank * base + min(rank, extra)
    return range(lo, lo + base + (1 if rank < extra else 0))


def split_segments(n_frames: int, n_segments: int, n_poses: int, overlap_len: int) -> List[range]:
    """Cut a long feature stream into ``n_segments`` contiguous, independently-chained segments whose
    lengths are whole numbers of window strides where possible.  Each segment starts with an un-masked
    window, exactly like separate test videos: the chains themselves do not out-paint across the seams
    (``sample_arbitrary_len_sharded(seam_repair=True)`` closes them afterwards, :func:`seam_windows`)."""
    step = n_poses - overlap_len
    n_strides = max(1, (n_frames - overlap_len) // step) if n_frames > n_poses else 1
    n_segments = max(1, min(n_segments, n_strides))
    segs, start = [], 0
    for i in range(n_segments):
        strides = n_strides // n_segments + (1 if i < n_strides % n_segments else 0)
        end = n_frames if i == n_segments - 1 else start + strides * step
        segs.append(range(start, end))
        start = end
    return segs


# Philox key of the seam windows: window_seed(seed, SEAM_WINDOW).  Chains use window indices 0, 1, 2, ... (one per n_poses - overlap_len
# frames of a segment), so no chain of a stream shorter than 2^40 strides can reach this index.
SEAM_WINDOW = 1 << 40


def seam_windows(segs: Sequence[range], n_poses: int) -> List[range]:
    """Seam ``s`` is the boundary ``p = segs[s + 1].start`` between segments ``s`` and ``s + 1``; its window is the ``n_poses`` frames
    ``[p - n_poses // 2, p - n_poses // 2 + n_poses)``: first ``overlap_len`` frames from the left chain, last from the right."""
    return [range(sg.start - n_poses // 2, sg.start - n_poses // 2 + n_poses) for sg in segs[1:]]


def _seam_windows_fit(segs: Sequence[range], n_poses: int) -> bool:
    wins = seam_windows(segs, n_poses)
    if not wins:
        return True
    return wins[0].start >= segs[0].start and wins[-1].stop <= segs[-1].stop and all(a.stop <= b.start for a, b in zip(wins[:-1], wins[1:]))


def split_segments_for_repair(n_frames: int, n_segments: int, n_poses: int, overlap_len: int) -> List[range]:
    """:func:`split_segments`, with the segment count lowered until the seam windows are pairwise disjoint and inside the stream
    (always true when every segment has at least ``n_poses`` frames; a one-stride segment has ``n_poses - overlap_len``).  The
    result of :func:`split_segments` is returned unchanged whenever its seam windows already fit."""
    while True:
        segs = split_segments(n_frames, n_segments, n_poses, overlap_len)
        if _seam_windows_fit(segs, n_poses):
            return segs
        n_segments = len(segs) - 1


def _repair_seams(trainer: "DDPMTrainer", stream: torch.Tensor, offset: int, seams: Sequence[int], segs: Sequence[range],
                  audio_emb: torch.Tensor, add_cond: Dict[str, torch.Tensor], pid: torch.Tensor, seed: int, max_rows: int,
                  cond_scale, tail_blend: bool, modality="both", expression: Optional[torch.Tensor] = None) -> None:
    """Re-sample the windows of the seams ``seams`` (global indices) in place in ``stream [n, C]``, which holds frames
    ``[offset, offset + n)`` of the whole stream: one batched in-betweening window per ``max_rows`` seams (row = seam), conditioning
    and pinned frames gathered with one index tensor, result scattered back with the same one.  Key = (seed, SEAM_WINDOW), counter
    high words = global seam index: a seam's noise does not depend on the rank or the batch it is sampled in."""
    if not seams:
        return
    opt = trainer.opt
    n_poses, L = int(opt.n_poses), int(opt.overlap_len)
    wins = seam_windows(segs, n_poses)
    dev = stream.device
    key = window_seed(seed, SEAM_WINDOW)
    for c0 in range(0, len(seams), max_rows):
        chunk = list(seams[c0:c0 + max_rows])
        idx = torch.tensor([wins[s].start for s in chunk], device=dev).unsqueeze(1) + torch.arange(n_poses, device=dev).unsqueeze(0)
        a = audio_emb[0][idx.to(audio_emb.device)]                           # (conditioning may still live on the host: it is moved per window)
        cnd = {k: v[0][idx.to(v.device)] for k, v in add_cond.items()}
        loc = idx - offset
        win = stream[loc]                                                   # [rows, n_poses, C]
        ex = expression[0][idx.to(expression.device)].contiguous() if expression is not None else None
        out = trainer.sample_inbetween(a, pid[:1].expand(len(chunk), -1), cnd, win[:, :L], win[:, n_poses - L:], tail_blend=tail_blend,
                                       seed=key, row_keys=chunk, cond_scale=cond_scale,
                                       **({} if modality in (None, "both", 0) else {"modality": modality, "expression": ex}))
        stream.index_copy_(0, loc.reshape(-1), out.reshape(-1, out.shape[-1]).to(stream.dtype))


def _collectives_active(group=None) -> bool:
    """True when the per-rank code paths (broadcast / shard / gather) must run: more than one rank, or — DSH_FORCE_COLLECTIVES=1 —
    an initialised group of ONE rank.  The latter exists so that the RCCL calls (broadcast, gather on device buffers) execute on a
    single-GPU test box instead of short-circuiting at world size 1 (tests/test_gpu_sharded.py)."""
    import torch.distributed as dist
    if not dist.is_initialized():
        return False
    return dist.get_world_size(group) > 1 or os.environ.get("DSH_FORCE_COLLECTIVES") == "1"


def broadcast_stream(t: Optional[torch.Tensor], device, src: int = 0, group=None) -> torch.Tensor:
    """rank ``src`` -> all: one conditioning tensor (mel [1,N,128] / HuBERT [1,N,1024]; 41 MB for 5 min of audio)."""
    import torch.distributed as dist
    if not _collectives_active(group):
        return t
    rank = dist.get_rank(group)
    meta = torch.zeros(8, dtype=torch.long, device=device)
    if rank == src:
        meta[0] = t.dim()
        meta[1:1 + t.dim()] = torch.tensor(t.shape, device=device)
    dist.broadcast(meta, src, group=group)
    shape = [int(v) for v in meta[1:1 + int(meta[0])]]
    buf = t.to(device=device, dtype=torch.float32).contiguous() if rank == src else torch.empty(shape, device=device)
    dist.broadcast(buf, src, group=group)
    return buf


def sample_arbitrary_len_sharded(trainer: "DDPMTrainer", audio_emb: Optional[torch.Tensor], p_id: torch.Tensor,
                                 add_cond: Optional[Dict[str, torch.Tensor]], n_segments: int, seed: int = 0, group=None,
                                 inputs_on_rank0_only: bool = False, max_chains_per_batch: int = 64,
                                 cond_scale: Optional[float] = None, seam_repair: bool = False,
                                 seam_tail_blend: bool = True, ragged: bool = False,
                                 pose_rep: str = "axis_angle", modality="both",
                                 expression: Optional[torch.Tensor] = None, guidance=None) -> Optional[torch.Tensor]:
    """BASELINE config 4: one long feature stream ``[1, N, ...]`` sampled on all ranks of ``group``.

    Windows of ONE chain are sequential (window k needs the final sample of window k-1 at every denoising step,
    ddpm_show_trainer.py:891-893), so the stream is cut into ``n_segments`` independent chains
    (:func:`split_segments`; every chain starts from an un-masked window, exactly like separate test videos, which is how the
    reference itself parallelises: DistributedSampler over videos, one chain per rank, ddpm_show_trainer.py:743-750,924-931).
    By default the returned stream therefore has a motion discontinuity at every segment boundary; ``seam_repair=True`` closes
    them (below).
    Each rank owns a contiguous run of segments (:func:`shard_range`), samples equally long ones together as a batched
    chain (batch row = chain), and rank 0 gathers the frames (RCCL gather, 8.4 MB for 9000 frames).  There is no other
    collective on the data path.  Noise: on-device Philox, key = hash(seed, window index), counter high words = segment id, so every chain is
    sampled identically whatever the world size or batching.  ``cond_scale``: one guidance scale for the whole stream (default:
    ``opt.cond_scale``).  Returns ``[1, N, C]`` on rank 0, ``None`` elsewhere.

    ``seam_repair=True`` (needs ``opt.ddim``, ``0 < 2 * overlap_len < n_poses``): after the chains, the ``n_poses`` frames around
    every segment boundary (:func:`seam_windows`) are re-sampled as an in-betweening window (:meth:`DDPMTrainer.sample_inbetween`):
    first ``overlap_len`` frames pinned to the left chain's output, last ``overlap_len`` to the right chain's, the frames in between
    drawn from the stream's own conditioning of that window, the whole window written back.  ``seam_tail_blend`` is that call's
    ``tail_blend``.  All seams of a rank are ONE batched window (chunked by ``max_chains_per_batch``).  Seam windows have to be
    pairwise disjoint and inside the stream; the segment count is lowered until they are (:func:`split_segments_for_repair`: only
    when some segment is shorter than ``n_poses`` frames, e.g. ``(9000, 256)`` or ``(400, 8)`` for SHOW), so the chains of a
    repaired stream may differ from the default mode's for such counts.  A seam whose two segments live on the same rank is
    repaired there before the gather (no new collective); the ``world - 1`` seams between ranks are repaired on rank 0 after it.
    Noise: key = hash(seed, :data:`SEAM_WINDOW`), counter high words = global seam index; windows are disjoint, so the repaired
    stream is the same whatever the world size, the rank that ran a seam, or the batching.  Frames outside the seam windows are
    those of the default mode, bit for bit.

    ``ragged=True``: a rank's chains are sampled together whatever their lengths (``sample_arbitrary_len(lengths=...)``, chunked by
    ``max_chains_per_batch``) instead of one chain batch per distinct length after another — the number of sequential windows is that
    of the longest chain, not the sum over the distinct lengths.  Every chain is still the chain sampled alone with its id as row key;
    the seam repair runs behind the chains as before.  Default ``False``: the grouping by length, bit for bit.

    ``pose_rep="euler"`` (BEAT, after ``trainer.set_pose_stats``): chains, gather and seam repair run in the sampler's axis-angle
    representation as always; rank 0 converts the gesture channels of the finished stream to the reference's standardised Euler degrees.

    ``modality`` / ``expression``: one modality alone for the chains and the seam repair (:meth:`DDPMTrainer.sample_arbitrary_len`).  The
    track of ``"gesture"`` is ``[1, N, E]`` (or ``[N, E]``); with ``inputs_on_rank0_only`` it is broadcast with the audio.

    ``guidance`` (:class:`diffsheg_amd.glue.MotionGuidance`) is not built for the sharded path: ``NotImplementedError``.
    """
    if guidance is not None:
        raise NotImplementedError("guidance in the sharded long-audio path is not built (use sample_arbitrary_len on chains of equal length)")
    euler = trainer._euler_requested(pose_rep)
    if cond_scale is not None and not isinstance(cond_scale, numbers.Real):
        raise ValueError("sample_arbitrary_len_sharded takes one scalar cond_scale for its stream")
    import torch.distributed as dist
    opt = trainer.opt
    n_poses, L, C = int(opt.n_poses), int(opt.overlap_len), int(opt.net_dim_pose)
    dev = trainer.device
    ddp = _collectives_active(group)
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if ddp else (0, 1)
    add_cond = add_cond or {}
    if inputs_on_rank0_only and ddp:
        keys = [sorted(add_cond.keys()) if rank == 0 else None]
        dist.broadcast_object_list(keys, 0, group=group)
        audio_emb = broadcast_stream(audio_emb, dev, 0, group)
        add_cond = {k: broadcast_stream(add_cond[k] if rank == 0 else None, dev, 0, group) for k in keys[0]}
        has_track = [expression is not None if rank == 0 else None]
        dist.broadcast_object_list(has_track, 0, group=group)
        if has_track[0]:
            expression = broadcast_stream((expression if expression.dim() == 3 else expression.unsqueeze(0)) if rank == 0 else None, dev, 0, group)
    if audio_emb.shape[0] != 1:
        raise ValueError("sample_arbitrary_len_sharded takes ONE stream [1, N, ...]; batch several streams by calling it per stream")
    N = int(audio_emb.shape[1])
    expression = trainer._chain_track(modality, expression, 1, N, None)          # None, or [1, N, E]
    mkw = {} if modality in (None, "both", 0) else {"modality": modality}
    if seam_repair:
        if not getattr(opt, "ddim", True) or L <= 0 or 2 * L >= n_poses:
            raise ValueError("seam_repair needs opt.ddim and 0 < 2 * overlap_len < n_poses")
        segs = split_segments_for_repair(N, n_segments, n_poses, L)
    else:
        segs = split_segments(N, n_segments, n_poses, L)
    mine = shard_range(len(segs), rank, world)
    pid = p_id if p_id.dim() == 2 else p_id.unsqueeze(0)
    by_len: Dict[int, List[int]] = {}
    for si in mine:
        by_len.setdefault(len(segs[si]), []).append(si)
    local: Dict[int, torch.Tensor] = {}
    if ragged:
        ids = list(mine)
        for c0 in range(0, len(ids), max_chains_per_batch):
            chunk = ids[c0:c0 + max_chains_per_batch]
            lens = [len(segs[i]) for i in chunk]

            def stack(v: torch.Tensor) -> torch.Tensor:          # [chains, longest, ...], zero padded behind every chain
                out = v.new_zeros((len(chunk), max(lens)) + tuple(v.shape[2:]))
                for j, i in enumerate(chunk):
                    out[j, :lens[j]] = v[0, segs[i].start:segs[i].stop]
                return out
            outs = trainer.sample_arbitrary_len(stack(audio_emb), pid[:1].expand(len(chunk), -1), {k: stack(v) for k, v in add_cond.items()},
                                                seed=seed, row_keys=chunk, cond_scale=cond_scale, lengths=lens,
                                                **(dict(mkw, expression=stack(expression)) if expression is not None else mkw))
            for j, i in enumerate(chunk):
                local[i] = outs[j]
    for ids in ([] if ragged else by_len.values()):
        for c0 in range(0, len(ids), max_chains_per_batch):
            chunk = ids[c0:c0 + max_chains_per_batch]
            a = torch.cat([audio_emb[:, segs[i].start:segs[i].stop] for i in chunk], 0)
            cnd = {k: torch.cat([v[:, segs[i].start:segs[i].stop] for i in chunk], 0) for k, v in add_cond.items()}
            ex = torch.cat([expression[:, segs[i].start:segs[i].stop] for i in chunk], 0) if expression is not None else None
            out = trainer.sample_arbitrary_len(a, pid[:1].expand(len(chunk), -1), cnd, seed=seed, row_keys=chunk, cond_scale=cond_scale,
                                               **(dict(mkw, expression=ex) if ex is not None else mkw))
            for j, i in enumerate(chunk):
                local[i] = out[j]
    loc = torch.cat([local[i] for i in mine], 0) if len(mine) else torch.zeros(0, C, device=dev)
    if seam_repair and len(mine) > 1:
        # seams inside this rank's run of segments (seam s lies between segments s and s + 1)
        _repair_seams(trainer, loc, segs[mine[0]].start, list(mine)[:-1], segs, audio_emb, add_cond, pid, seed, max_chains_per_batch,
                      cond_scale, seam_tail_blend, modality, expression)
    sizes = [sum(len(segs[i]) for i in shard_range(len(segs), r, world)) for r in range(world)]
    parts = gather_outputs(loc, sizes, group)
    if parts is None:
        return None
    full = torch.cat(parts, 0)
    if seam_repair and world > 1:
        # seams between two ranks' runs: one more batch, on rank 0
        last = [shard_range(len(segs), r, world) for r in range(world)]
        between = [r[-1] for r in last if len(r) and r[-1] < len(segs) - 1]
        _repair_seams(trainer, full, 0, between, segs, audio_emb, add_cond, pid, seed, max_chains_per_batch, cond_scale, seam_tail_blend,
                      modality, expression)
    full = full.unsqueeze(0)
    return trainer._to_euler(full) if euler else full


def gather_outputs(local: torch.Tensor, world_sizes: Sequence[int], group=None) -> Optional[List[torch.Tensor]]:
    """all ranks -> rank 0 gather of per-rank outputs with differing leading dims (RCCL / gloo)."""
    import torch.distributed as dist
    if not _collectives_active(group):
        return [local]
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    mx = max(world_sizes)
    mx = max(mx, 1)
    # (a gloo group gathers through the host: single-GPU test boxes that oversubscribe one device cannot use RCCL)
    via = local.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    pad = torch.zeros((mx,) + tuple(local.shape[1:]), dtype=local.dtype, device=via)
    pad[: local.shape[0]] = local
    bufs = [torch.empty_like(pad) for _ in range(world)] if rank == 0 else None
    dist.gather(pad, bufs, dst=0, group=group)
    if rank != 0:
        return None
    return [b[:n].to(local.device) for b, n in zip(bufs, world_sizes)]
