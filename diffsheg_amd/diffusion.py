"""Host-side mirror of the reference sampler interface (boundary 2).

Same class / function names and call signatures as /root/reference/models/gaussian_diffusion.py
(``GaussianDiffusion.p_sample_loop`` :776, ``ddim_sample_loop`` :1106) and models/respace.py
(``space_timesteps`` :7, ``SpacedDiffusion`` :60); the loops themselves run natively in
libdiffsheg_hip.so (csrc/sampler.hip) with no host syncs per step.

Differences a caller can observe, all loud:
  * the model must be a :class:`diffsheg_amd.model.UniDiffuser` (epsilon prediction, FIXED_SMALL var);
  * ``denoised_fn`` / ``cond_fn`` / ``pre_seq`` / ``transl_req`` raise NotImplementedError (``same_overlap_noisy``, ``eta != 0`` and ``fix_head_var`` are built: the
    saved noisy tails live in the native context, eta adds one draw per DDIM step, fix_head_var is a no-op of
    the reference's own sampling code — see ``_run``);
  * Gaussian noise comes from ``noise_source`` (any object with ``randn(shape) -> Tensor``, consumed in
    the reference's draw order — this is how parity tests inject identical noise) or, if None, from the
    on-device Philox generator seeded by ``seed`` / ``torch.initial_seed()``; ``row_keys`` (one integer per
    batch row) additionally gives every row its own Philox stream, so that a chain draws the same noise in
    whatever batch / on whatever rank it is sampled (the sharded long-audio path); ``row_seeds`` (with ``row_keys``, one integer
    per batch row) gives every row its own Philox key in place of ``seed``, so rows of one batch may stand at different windows of
    their chains (``dsh_run_spec.row_seeds``; :class:`diffsheg_amd.streaming.StreamPool`);
  * the guidance scale is ``opt.cond_scale`` as in the reference (ignored for weights without ``classifier_free``), or the
    loops' ``cond_scale=`` keyword (a float, or one value per batch row), which wins over ``opt``; either holds for the call only;
    ``cfg_schedule=`` (a glue.CFGSchedule: the weight of the guidance per timestep and encoder, std rescale) likewise holds for the call;
  * ``model_kwargs['length']`` with an entry ``< T`` makes the batch ragged (``UniDiffuser.set_condition(lengths=)``): every row is
    sampled as the clip alone at its length (with ``row_keys``: from the same noise), padded frames of the result are exactly 0;
  * ``model_kwargs['modality']`` (``"expression"`` / ``"gesture"``, the latter with ``model_kwargs['expression']`` = the given track) samples
    one encoder's channels alone (``UniDiffuser.set_condition(modality=)``): the other columns of the result are 0 / the given track;
  * ``ddim_sample_loop(..., tail_blend=True)`` mirrors the ``addBlend`` cross-fade onto the last ``overlap_len`` frames, for a mask
    that pins both ends of a window (``DDPMTrainer.sample_inbetween``, seam repair); off by default;
  * editing an existing motion: ``q_sample`` (gaussian_diffusion.py:417-462) runs on the device, from given noise or the Philox streams;
    ``ddim_sample_loop(..., start_level=K)`` starts at spaced level ``K - 1`` from ``noise=`` (x at that level) or ``x_start=`` (a clean
    motion, noised in the loop with draw 0); ``ddim_reverse_sample`` / ``ddim_reverse_sample_loop`` are the DDIM reverse ODE (:1068-1104);
  * ``ddim_sample_loop(..., sync_left=, sync_len=)``: synchronised window batches — the rows are windows of long streams and the frames two
    neighbouring windows share are reconciled behind every denoise step (``dsh_run_spec.sync_left``); off by default;
  * few-step sampling: ``space_timesteps`` also takes the reference's section counts and ``'logsnrK'`` (K timesteps uniform in log-SNR),
    ``SpacedDiffusion`` any non-empty subset of the timesteps (a subset that is no 'ddimK' stride travels as a list,
    ``dsh_run_spec.timesteps``), and ``ddim_sample_loop(..., solver="dpm2m")`` runs the second-order DPM-Solver++(2M) update where a
    denoise step follows the denoise step one level above it (``dsh_run_spec.solver``); the default is the reference's loop;
  * the eval-mode forward losses: ``training_losses`` (gaussian_diffusion.py:1319-1426, epsilon / MSE branch) noises ``x_start``, evaluates the
    model once and reduces the loss terms on the device (``dsh_op_denoise_losses``); ``target_vel`` / ``pred_vel`` are not materialised, ``loss_type``
    KL / RESCALED_KL, a single modality and ``pre_seq`` are refused; ``UniformSampler`` / ``create_named_schedule_sampler`` (:21-76) draw timesteps.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import enum
import numbers
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .model import UniDiffuser, normalize_guidance_scale, normalize_lengths, normalize_modality

_TABLES = ["betas", "alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next", "sqrt_recip_alphas_cumprod",
           "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
           "posterior_mean_coef1", "posterior_mean_coef2"]


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self in (LossType.KL, LossType.RESCALED_KL)


class UniformSampler:
    """gaussian_diffusion.py:35-76: every timestep of ``diffusion`` with the same probability, all weights 1.  Host-side."""

    def __init__(self, diffusion):
        self.diffusion = diffusion
        self._weights = np.ones([diffusion.num_timesteps])

    def weights(self):
        return self._weights

    def sample(self, batch_size: int, device, generator=None):
        """``(timesteps, weights)`` for a batch (:52-67): int64 indices in ``0 .. num_timesteps - 1`` and float32 weights, on ``device``.
        ``generator``: a ``numpy.random.Generator`` / ``RandomState`` (two samplers given equally seeded generators draw the same
        timesteps), or ``None`` for numpy's global state, which is what the reference draws from."""
        w = self.weights()
        p = w / np.sum(w)
        rng = np.random if generator is None else generator
        indices_np = rng.choice(len(p), size=(int(batch_size),), p=p)
        indices = torch.from_numpy(np.asarray(indices_np, dtype=np.int64)).to(device)
        weights = torch.from_numpy(1 / (len(p) * p[indices_np])).float().to(device)
        return indices, weights


def create_named_schedule_sampler(name: str, diffusion):
    """gaussian_diffusion.py:21-32; only "uniform" is built (the loss-aware resampler belongs to a training run)."""
    if name == "uniform":
        return UniformSampler(diffusion)
    raise NotImplementedError(f"unknown schedule sampler: {name}")


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    """A small host tensor to the device without blocking the host: through pinned memory, asynchronously on the current stream."""
    return t.pin_memory().to(device, non_blocking=True)


def denoise_losses(eps, noise, x_t, x0, c1, c2, split: int, lens_dev=None, huber_beta: float = 0.1, want_x0_pred: bool = True,
                   want_frame_mse: bool = True) -> dict:
    """``dsh_op_denoise_losses`` on the current stream: ``eps`` / ``noise`` / ``x_t`` / ``x0`` ``[B, T, C]`` and ``c1`` / ``c2`` ``[B]``, contiguous
    fp32 on one GPU; ``lens_dev`` an int32 device tensor ``[B]`` or ``None``.  Returns ``{"scalars" [4] fp64 (loss_model_pred, loss_vel_rec,
    loss_x0_rec, final_loss), "counts" [3] fp64 (valid frames, frame pairs, elements), "row_terms" [B, LOSS_COLS] fp64, "pred_x0", "frame_mse"}``
    (the last two ``None`` when not asked for); views of one result buffer.  Two launches, no synchronisation."""
    if not eps.is_cuda:
        raise _lib.DshError("denoise_losses runs on the GPU (no CPU fallback)")
    B, T, Cc = (int(v) for v in eps.shape)
    for name, v in (("eps", eps), ("noise", noise), ("x_t", x_t), ("x0", x0)):
        if tuple(v.shape) != (B, T, Cc) or v.dtype != torch.float32 or not v.is_contiguous() or v.device != eps.device:
            raise ValueError(f"denoise_losses: {name} must be a contiguous fp32 [B, T, C] = {(B, T, Cc)} tensor on {eps.device}")
    for name, v in (("c1", c1), ("c2", c2)):
        if tuple(v.shape) != (B,) or v.dtype != torch.float32 or not v.is_contiguous() or v.device != eps.device:
            raise ValueError(f"denoise_losses: {name} must be a contiguous fp32 [B] tensor on {eps.device}")
    if lens_dev is not None and (tuple(lens_dev.shape) != (B,) or lens_dev.dtype != torch.int32 or lens_dev.device != eps.device):
        raise ValueError("denoise_losses: lens_dev must be an int32 [B] tensor on the tensors' device")
    L = _lib.lib()
    dev = eps.device
    nbytes = _lib.check(int(L.dsh_denoise_losses_result_bytes(B, T)), "dsh_denoise_losses_result_bytes")
    res = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    x0p = torch.empty_like(eps) if want_x0_pred else None
    fm = torch.empty(B, T, dtype=torch.float32, device=dev) if want_frame_mse else None
    with torch.cuda.device(dev):
        rc = L.dsh_op_denoise_losses(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), eps.data_ptr(), noise.data_ptr(), x_t.data_ptr(),
                                     x0.data_ptr(), c1.data_ptr(), c2.data_ptr(), None if lens_dev is None else lens_dev.data_ptr(), B, T, Cc,
                                     int(split), float(huber_beta), None if x0p is None else x0p.data_ptr(),
                                     None if fm is None else fm.data_ptr(), res.data_ptr())
    _lib.check(rc, "dsh_op_denoise_losses")
    H, K = _lib.LOSS_HEADER, _lib.LOSS_COLS
    return {"scalars": res[:4], "counts": res[4:7], "row_terms": res[H:H + B * K].view(B, K), "pred_x0": x0p, "frame_mse": fm}


LOSS_SCALARS = ("loss_model_pred", "loss_vel_rec", "loss_x0_rec", "final_loss")


def get_named_beta_schedule(schedule_name: str, num_diffusion_timesteps: int) -> np.ndarray:
    """gaussian_diffusion.py:234-251 — only 'linear' is on the path."""
    if schedule_name != "linear":
        raise NotImplementedError(f"unknown beta schedule: {schedule_name}")
    return diffusion_table(num_diffusion_timesteps, 0, "betas")


def diffusion_table(steps: int, respacing: int, name: str) -> np.ndarray:
    buf = (C.c_double * max(steps, 1))()
    n = _lib.check(_lib.lib().dsh_diffusion_table(steps, respacing, name.encode(), buf, steps), "dsh_diffusion_table")
    return np.array(buf[:n], dtype=np.float64)


def _int_array(values):
    vals = [int(v) for v in values]
    return (C.c_int32 * max(len(vals), 1))(*vals), len(vals)


def diffusion_table_subset(steps: int, kept, name: str) -> np.ndarray:
    """The table ``name`` of the process respaced to the original timesteps ``kept`` (ascending)."""
    arr, n = _int_array(kept)
    buf = (C.c_double * max(n, 1))()
    m = _lib.check(_lib.lib().dsh_diffusion_table_subset(steps, arr, n, name.encode(), buf, n), "dsh_diffusion_table_subset")
    return np.array(buf[:m], dtype=np.float64)


def solver_coeffs(steps: int, kept, k: int):
    """``(A, Bc, G)`` of the dpm2m solver at spaced level ``k`` of the subset ``kept``, fp64 (dsh_solver_coeffs)."""
    arr, n = _int_array(kept)
    out = (C.c_double * 3)()
    _lib.check(_lib.lib().dsh_solver_coeffs(steps, arr, n, int(k), out), "dsh_solver_coeffs")
    return tuple(out)


def masked_start_level(steps: int, kept) -> int:
    """``t_T`` of an out-painting run on the subset ``kept``: 0 for a 'ddimK' stride (the reference's 15 / int(0.6 K)), else one past the
    first level at or below the noise level where the reference starts a masked ddim25 window (dsh_masked_start_level)."""
    arr, n = _int_array(kept)
    return _lib.check(_lib.lib().dsh_masked_start_level(steps, arr, n), "dsh_masked_start_level")


def logsnr_timesteps(num_timesteps: int, k: int) -> List[int]:
    """``k`` timesteps placed uniformly in log-SNR: lambda(t) = log(ac_t / (1 - ac_t)) / 2 from the fp64 base table, the grid
    ``linspace(lambda(n - 1), lambda(0), k)``, and for every grid point the timestep nearest in lambda (ties: the lower one)."""
    if k < 1:
        raise ValueError(f"cannot place {k} timesteps")
    ac = diffusion_table(num_timesteps, 0, "alphas_cumprod")
    lam = 0.5 * np.log(ac / (1.0 - ac))
    grid = np.linspace(lam[-1], lam[0], k)
    kept = sorted(int(np.argmin(np.abs(lam - g))) for g in grid)       # (argmin returns the first, i.e. lowest, index of a tie)
    if len(set(kept)) != k:
        raise ValueError(f"cannot place {k} distinct timesteps uniformly in log-SNR on {num_timesteps} steps ({len(set(kept))} distinct)")
    return kept


def space_timesteps(num_timesteps: int, section_counts) -> set:
    """respace.py:7-57: ``'ddimK'`` (the DDIM stride), section counts (``"a,b,c"`` or a list: that many evenly spaced steps from each of
    the equal portions of the process), and — not in the reference — ``'logsnrK'`` (:func:`logsnr_timesteps`)."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            k = int(section_counts[len("ddim"):])
            buf = (C.c_int32 * num_timesteps)()
            n = _lib.check(_lib.lib().dsh_timestep_map(num_timesteps, k, buf, num_timesteps), "dsh_timestep_map")
            return set(buf[:n])
        if section_counts.startswith("logsnr"):
            return set(logsnr_timesteps(num_timesteps, int(section_counts[len("logsnr"):])))
        section_counts = [int(v) for v in section_counts.split(",")]
    counts = [int(v) for v in section_counts]
    size_per, extra = divmod(num_timesteps, len(counts))
    start, steps = 0, []
    for i, count in enumerate(counts):
        size = size_per + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        steps += [start + round(j_stride) for j_stride in _accumulate(stride, count)]
        start += size
    return set(steps)


def _accumulate(stride, count):
    """0, stride, stride + stride, ...: the running float sum the reference rounds (not j * stride)."""
    cur = 0.0
    for _ in range(count):
        yield cur
        cur += stride


def get_schedule_jump_cjm_ddim(time_respacing: int = 25, jump_length: int = 1, jump_n_sample: int = 1) -> List[int]:
    """scheduler.py:178-208."""
    buf = (C.c_int32 * 4096)()
    n = _lib.check(_lib.lib().dsh_jump_schedule(time_respacing, jump_length, jump_n_sample, buf, 4096), "dsh_jump_schedule")
    return list(buf[:n])


class _SavedTails:
    """Opaque stand-in for the reference's ``saved_noisy_tail`` dict: the tensors stay in the native context."""

    def __init__(self, model):
        self.model = model


class GaussianDiffusion:
    """Full-chain sampler handle (ancestral DDPM): mirrors gaussian_diffusion.py:300-390."""

    _respacing = 0
    _kept = None          # SpacedDiffusion on a subset that is no 'ddimK' stride: the sorted original timesteps
    solver = "ddim"       # the update rule ddim_sample_loop uses when its solver= keyword is not given

    def __init__(self, *, opt, betas=None, model_mean_type=ModelMeanType.EPSILON,
                 model_var_type=ModelVarType.FIXED_SMALL, loss_type=None, rescale_timesteps=False,
                 num_timesteps: Optional[int] = None):
        if model_mean_type not in (ModelMeanType.EPSILON, "epsilon"):
            raise NotImplementedError("only epsilon prediction is built (trainers use model_mean_type='epsilon')")
        if model_var_type not in (ModelVarType.FIXED_SMALL,):
            raise NotImplementedError("only FIXED_SMALL variance is built")
        if rescale_timesteps:
            raise NotImplementedError("rescale_timesteps=True is not on the path")
        self.opt = opt
        self.model_mean_type, self.model_var_type, self.loss_type = model_mean_type, model_var_type, loss_type
        self.rescale_timesteps = False
        n = int(num_timesteps if num_timesteps is not None else (len(betas) if betas is not None else 1000))
        if betas is not None:
            ref = diffusion_table(n, 0, "betas")
            if not np.allclose(np.asarray(betas, dtype=np.float64), ref, rtol=0, atol=1e-15):
                raise NotImplementedError("only the 'linear' beta schedule is built")
        self.original_num_steps = n
        self._load_tables()

    def _load_tables(self):
        for name in _TABLES:
            setattr(self, name, diffusion_table(self.original_num_steps, self._respacing, name))
        self.num_timesteps = len(self.betas)
        self.timestep_map = list(range(self.num_timesteps))

    # ---- helpers --------------------------------------------------------------------------
    def _opts(self, kind: int, clip_denoised: bool, noise_mode: int, seed: int, clip_idx: int = 0, eta: float = 0.0,
              add_blend=None) -> _lib.SamplerOptsC:
        o = self.opt
        if add_blend is None:
            add_blend = getattr(o, "addBlend", getattr(o, "add_blend", True))
        return _lib.SamplerOptsC(kind, self.original_num_steps, max(self._respacing, 1),
                                 int(getattr(o, "jump_length", 3)), int(getattr(o, "jump_n_sample", 5)),
                                 int(getattr(o, "overlap_len", 0)), int(bool(add_blend)),
                                 int(bool(getattr(o, "no_resample", False))), int(bool(getattr(o, "no_repaint", False))),
                                 int(bool(clip_denoised)), noise_mode, seed & 0xFFFFFFFFFFFFFFFF,
                                 int(bool(getattr(o, "same_overlap_noisy", False))), int(clip_idx), float(eta))

    def _guidance(self, model, cond_scale, B: int):
        """Guidance scale of one call (transformer.py:537, :586): the keyword wins over opt.cond_scale; without classifier-free weights the
        reference never reads opt.cond_scale, and an explicit scale other than 1 is an error.  None: the model's own setting stays."""
        gs = normalize_guidance_scale(cond_scale)
        if gs is None:
            gs = normalize_guidance_scale(getattr(self.opt, "cond_scale", None))
            if not model.cfg.classifier_free:
                gs = None
        elif not model.cfg.classifier_free:
            if any(v != 1.0 for v in gs):
                raise ValueError(f"cond_scale={list(gs)}: the weights are not classifier-free (no null_cond_emb), only 1 is possible")
            gs = None
        if gs is not None and len(gs) not in (1, B):
            raise ValueError(f"cond_scale needs one value or one per batch row ({B}), got {len(gs)}")
        return gs

    @staticmethod
    def _condition(model, model_kwargs, shape, lens, son: bool) -> None:
        """One modality alone (model_kwargs['modality'] / ['expression'], UniDiffuser.set_condition) is refused like the rest, before
        conditioning; then the context is conditioned (if it is not already) and the sample shape checked against it."""
        B, T, Cc = shape
        modality, expression = model_kwargs.get("modality", "both"), model_kwargs.get("expression")
        normalize_modality(modality, expression, B, T, model.cfg.expression_dim, model.cfg.unidiffuser, son)
        model._maybe_set_condition(model_kwargs["audio_emb"], model_kwargs["person_id"], model_kwargs.get("add_cond"), lens, modality, expression)
        if (B, T) != (model.batch, model.frames) or Cc != model.cfg.net_dim_pose:
            raise ValueError(f"shape {tuple(shape)} does not match the conditioning")

    @staticmethod
    @contextlib.contextmanager
    def _native(model, gs, sched=None):
        """The native calls of one loop: on the model's device and stream, under the call's guidance scale and guidance schedule (the two
        things that are sticky in the context — they also govern plain evaluations: the model's own settings come back afterwards).
        ``sched``: the call's ``cfg_schedule=`` (None: the model's own setting stays)."""
        prev_gs, prev_sched = model.guidance_scale, model.guidance_schedule
        set_gs = gs is not None and gs != prev_gs
        set_sched = sched is not None and sched != prev_sched
        if set_sched:
            model.set_guidance_schedule(sched)
        try:
            if set_gs:
                model.set_guidance_scale(gs)
            cur = model._enter()
            try:
                yield
            finally:
                model._exit(cur)
                if set_gs:
                    model.set_guidance_scale(prev_gs)
        finally:
            if set_sched:
                model.set_guidance_schedule(prev_sched)

    @staticmethod
    def _check_guide_shapes(guidance, shape) -> None:
        """A guidance built for another sample shape is refused with the other argument checks, before anything is conditioned."""
        B, T, Cc = shape
        for name in ("target", "weight", "vel", "acc"):
            v = getattr(guidance, name)
            want = (B, T, Cc) if name in ("target", "weight") else (Cc,)
            if v is not None and tuple(v.shape) != want:
                raise ValueError(f"guidance: {name} {tuple(v.shape)} does not match the sample shape: expected {want}")

    def _guide_fields(self, guidance, shape, dev):
        """The guide_* fields of a run's dsh_run_spec for a glue.MotionGuidance (or None): ``(tensors to keep alive, run_spec keywords)``.
        The tensors go to the model's device as they are built; shapes are refused here with the sample's shape in the message, the rest
        (level count, space, the reverse loop) by the library's check_run."""
        if guidance is None:
            return None, {}
        B, T, Cc = shape
        self._check_guide_shapes(guidance, shape)
        held = {name: getattr(guidance, name).to(device=dev, dtype=torch.float32).contiguous()
                for name in ("target", "weight", "vel", "acc") if getattr(guidance, name) is not None}
        kw = {f"guide_{n}": v.data_ptr() for n, v in held.items()}
        kw.update(guidance=1, guide_space=_lib.GUIDE_SPACES[guidance.space], guide_batch=B, guide_frames=T, guide_channels=Cc,
                  guide_scale=guidance.level_scale or ())
        return held, kw

    def _run(self, kind, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta=0.0,
             noise_source=None, seed=None, return_trace=False, row_keys=None, cond_scale=None, tail_blend=False,
             row_seeds=None, start_level=None, x_start=None, add_blend=None, solver=None, cfg_schedule=None, sync_left=None,
             sync_len=None):
        if not isinstance(model, UniDiffuser):
            raise TypeError("model must be a diffsheg_amd.model.UniDiffuser (no generic-callable / CPU fallback)")
        model.check_guidance_schedule(cfg_schedule)        # (refused here, before anything is conditioned or set in the native context)
        # the update rule of the DDIM loops: refused here, before anything is conditioned or set in the native context
        if solver is None:
            solver = self.solver if kind == 0 else "ddim"
        if solver not in ("ddim", "dpm2m"):
            raise ValueError(f'solver must be "ddim" or "dpm2m", got {solver!r}')
        if solver == "dpm2m":
            if kind != 0:
                raise TypeError("solver is an argument of the DDIM loops only")
            if eta != 0.0:
                raise ValueError("the dpm2m solver is deterministic: eta must be 0")
            if bool(getattr(self.opt, "same_overlap_noisy", False)):
                raise NotImplementedError("the dpm2m solver does not keep the saved noisy tails of same_overlap_noisy")
        # cond_fn: the closed family of glue.MotionGuidance runs fused into the step kernels; an arbitrary callable would put a host round
        # trip and an autograd graph into every step
        from .glue import MotionGuidance
        if denoised_fn is not None or (cond_fn is not None and not isinstance(cond_fn, MotionGuidance)):
            raise NotImplementedError("denoised_fn / cond_fn are not on the accelerated path (cond_fn: only a glue.MotionGuidance is)")
        if eta != 0.0 and kind != 0:
            raise TypeError("eta is an argument of the DDIM loops only")
        if model_kwargs is None or model_kwargs.get("y", None) is None:
            # the reference dereferences model_kwargs['y'].keys() (gaussian_diffusion.py:810,1126)
            raise AttributeError("'NoneType' object has no attribute 'keys' (model_kwargs['y'] must be a dict)")
        y = model_kwargs["y"]
        # options of the reference's `opt` namespace that change results and are not built: refuse, never ignore
        # opt.fix_head_var (gaussian_diffusion.py:444,759): q_sample (training / pre_seq only) zeroes the noise of the head channels;
        # in p_sample the mask it edits is [B, 1, 1], so `nonzero_mask[..., 90:] = 0` selects nothing, and ddim_sample never reads
        # the switch — sampling is bit-identical with it on (checked against the imported reference: tests/golden/make_golden.py
        # gen_eta_fhv, fixture ddpm50_fhv_show.npz).  What remains of it on this path is the reference's own refusal of other datasets.
        if getattr(self.opt, "fix_head_var", False) and kind == 1 and getattr(self.opt, "dataset_name", None) not in ("freeform_all", "talkshow"):
            raise NotImplementedError("fix_head_var: dataset_name must be 'freeform_all' or 'talkshow' (gaussian_diffusion.py:760-766)")
        son = bool(getattr(self.opt, "same_overlap_noisy", False))
        if son and kind != 0:
            raise NotImplementedError("same_overlap_noisy only exists in the DDIM loop (gaussian_diffusion.py:1040-1060)")
        tail_blend = bool(tail_blend)
        if tail_blend and kind != 0:
            raise TypeError("tail_blend is an argument of the DDIM loops only")
        if tail_blend and son:
            raise NotImplementedError("tail_blend with same_overlap_noisy: the saved noisy tails describe a window chain, not a window "
                                      "pinned at both ends")
        # restart from a level (an edit of an existing motion): DDIM loops only, x enters at spaced level K - 1
        K = 0
        if start_level is not None or x_start is not None:
            if kind != 0:
                raise TypeError("start_level / x_start are arguments of the DDIM loops only")
            if noise is not None and x_start is not None:
                raise ValueError("give noise= (x at level start_level - 1) or x_start= (a clean motion), not both")
            if start_level is not None:
                K = int(start_level)
                if not 1 <= K <= self._respacing:
                    raise ValueError(f"start_level must be in 1 .. {self._respacing}, got {start_level}")
                if noise is None and x_start is None:
                    raise ValueError("start_level needs noise= (x at level start_level - 1) or x_start= (a clean motion)")
                if son:
                    raise NotImplementedError("start_level with same_overlap_noisy: the saved noisy tails describe whole schedules")
                if tail_blend:
                    raise NotImplementedError("start_level with tail_blend is not built")
        clip_idx = int(y.get("clip_idx", 0)) if son else 0
        B, T, Cc = (int(s) for s in shape)
        # synchronised window batches (dsh_run_spec.sync_left): whatever would put per-window noise into the shared frames is refused here,
        # before anything is conditioned; the geometry (injective, inside every row's length) is check_run's, against the condition's lengths
        if (sync_left is None) != (sync_len is None):
            raise ValueError("sync_left and sync_len go together")
        if sync_left is not None:
            sync_left = [int(v) for v in sync_left]
            if kind != 0:
                raise TypeError("sync_left is an argument of the DDIM loops only (the DDPM loop draws per-window noise at every step)")
            if eta != 0.0:
                raise ValueError("synchronised windows are deterministic: eta must be 0")
            if son or tail_blend or K:
                raise NotImplementedError("synchronised windows cannot be combined with same_overlap_noisy, tail_blend or start_level")
            if noise_source is not None or noise is None or x_start is not None:
                raise ValueError("synchronised windows need noise= (x_T with ONE noise value per stream frame) and take no noise_source / x_start")
            if "outpainting_mask" in y and bool(y.get("outpainting_mask_any", True)):
                raise NotImplementedError("synchronised windows take no mask (the RePaint schedule's undo steps draw per-window noise)")
            if len(sync_left) != B or int(sync_len) < 1:
                raise ValueError(f"sync_left needs one entry per batch row ({B}) and sync_len >= 1, got {len(sync_left)} entries, sync_len = {sync_len}")
        if cond_fn is not None:
            self._check_guide_shapes(cond_fn, (B, T, Cc))
        if tail_blend and 2 * int(getattr(self.opt, "overlap_len", 0)) > T:
            raise ValueError(f"tail_blend: the head and the tail fade overlap (2 * overlap_len = {2 * int(self.opt.overlap_len)} > {T} frames)")
        gs = self._guidance(model, cond_scale, B)
        dev = model.device
        # clips of different lengths in one padded batch (model_kwargs['length'] with an entry < T): both options below address the last
        # overlap_len frames of the PADDED window, which a short clip does not reach — refused before anything is conditioned
        lens = normalize_lengths(model_kwargs.get("length"), B, T)
        if lens is not None and (son or tail_blend):
            raise NotImplementedError("per-clip lengths cannot be combined with same_overlap_noisy or tail_blend")
        if lens is not None and row_keys is not None and noise_source is None and any((v * Cc) % 4 for v in lens):
            raise ValueError("row_keys on a ragged batch: length * channels must be a multiple of 4 for every clip")
        self._condition(model, model_kwargs, (B, T, Cc), lens, son)
        gt = mask = None
        masked = False
        if "outpainting_mask" in y:
            mask = y["outpainting_mask"].to(device=dev)
            # the reference's `True in mask` costs one host sync per window; a harness that built the mask itself says what
            # it holds (key "outpainting_mask_any", set by trainer.sample_arbitrary_len) and no sync is needed
            hint = y.get("outpainting_mask_any", None)
            masked = bool(hint) if hint is not None else bool(mask.any().item())
            if masked:
                if kind == 1:
                    raise NotImplementedError("mask-present DDPM sampling (hard-wired 250-step schedule) is excluded")
                # the kernels index mask / gt as dense [B,T,C]: broadcast what the reference would broadcast, reject the rest
                try:
                    mask = mask.expand(B, T, Cc).to(torch.uint8).contiguous()
                    gt = y["gt"].to(device=dev, dtype=torch.float32).expand(B, T, Cc).contiguous()
                except RuntimeError as e:
                    raise ValueError(f"outpainting_mask {tuple(y['outpainting_mask'].shape)} / gt {tuple(y['gt'].shape)} "
                                     f"do not broadcast to the sample shape {(B, T, Cc)}") from e
        init = 2 if x_start is not None else int(noise is not None)      # dsh_sample: 0 x_T is drawn, 1 x is given, 2 x holds x0
        given = x_start if x_start is not None else noise
        if given is not None and tuple(given.shape) != (B, T, Cc):
            raise ValueError(f"{'x_start' if init == 2 else 'noise'} {tuple(given.shape)} does not match the sample shape {(B, T, Cc)}")
        x = given.to(device=dev, dtype=torch.float32).contiguous().clone() if init else torch.empty(B, T, Cc, device=dev)
        mode = 0 if noise_source is not None else 1
        if seed is None:
            seed = int(torch.initial_seed()) + GaussianDiffusion._calls
            GaussianDiffusion._calls += 1
        opts = self._opts(kind, clip_denoised, mode, int(seed), clip_idx, eta, add_blend)
        lib = _lib.lib()
        if row_keys is not None and len(row_keys) != B:
            raise ValueError(f"row_keys needs one key per batch row ({B}), got {len(row_keys)}")
        if row_seeds is not None and (row_keys is None or len(row_seeds) != B):
            raise ValueError(f"row_seeds needs row_keys and one seed per batch row ({B})")
        # the whole call in one dsh_run_spec: nothing is set in, or left behind in, the native context.  Philox noise only: per-row generator
        # keys (a chain's global id) and per-row seeds
        keyed = row_keys is not None and noise_source is None
        guide, guide_kw = self._guide_fields(cond_fn, (B, T, Cc), dev)
        spec = _lib.run_spec(timesteps=self._kept if (self._kept and kind == 0) else (), row_keys=row_keys if keyed else (),
                             row_seeds=row_seeds if (keyed and row_seeds is not None) else (), init=init, masked=int(masked), start_level=K,
                             tail_blend=int(tail_blend), solver=int(solver == "dpm2m"), x=x.data_ptr(),
                             sync_left=sync_left or (), sync_len=int(sync_len or 0),
                             gt=None if gt is None else gt.data_ptr(), mask=mask.data_ptr() if masked else None, **guide_kw)
        n_draws, n_steps = C.c_int64(), C.c_int64()
        _lib.check(lib.dsh_sample_count(C.byref(opts), C.byref(spec), C.byref(n_draws), C.byref(n_steps)), "dsh_sample_count")
        stack = trace = None
        if noise_source is not None:
            stack = torch.empty(n_draws.value, B * T * Cc, device=dev)
            for i in range(n_draws.value):
                stack[i].copy_(noise_source.randn((B, T, Cc)).reshape(-1), non_blocking=False)
            spec.noise_stack, spec.n_draws = stack.data_ptr(), n_draws.value
        if return_trace:
            trace = torch.empty(n_steps.value, B, T, Cc, device=dev)
            spec.trace = trace.data_ptr()
        with self._native(model, gs, cfg_schedule):
            _lib.check(lib.dsh_sample_run(model._h, C.byref(opts), C.byref(spec)), "dsh_sample_run")
        self._keep = (gt, mask, stack, guide)   # consumed asynchronously on the stream
        if son:
            # gaussian_diffusion.py:1155-1157: the loop returns the dict of the last step plus the saved tails.  The tails live
            # in the native context (one slot per spaced level, overwritten step by step exactly like the reference's dict,
            # which IS the object the next window receives as y['previous_noisy_tail']); the handle only documents that.
            out = {"sample": x, "saved_noisy_tail": _SavedTails(model)}
            return (out, trace) if return_trace else out
        return (x, trace) if return_trace else x

    _calls = 0

    # ---- boundary 2 ------------------------------------------------------------------------
    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, pre_seq=None, transl_req=None, progress=False, **kw):
        """gaussian_diffusion.py:776-841 (plain ancestral loop over all timesteps)."""
        if pre_seq is not None or transl_req is not None:
            raise NotImplementedError("pre_seq / transl_req are not on the accelerated path")
        if self._respacing:
            raise NotImplementedError("p_sample_loop on a SpacedDiffusion is not used by the harness")
        return self._run(1, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, **kw)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, **kw):
        """gaussian_diffusion.py:1106-1159 (dispatches to the harmonize schedule when a mask is set).  ``tail_blend=True`` (keyword,
        not in the reference) adds the mirrored cross-fade on the last ``overlap_len`` frames, for masks that pin both ends of the
        window (dsh_run_spec.tail_blend); the default is the reference's loop.

        ``start_level=K`` (keyword, ``1 .. K .. respacing``): the loop starts at spaced level ``K - 1`` instead of the top — levels
        ``K-1 .. 0``, or with a mask the RePaint jump schedule walked from ``t_T = K``.  ``noise=`` then is x AT level ``K - 1``;
        ``x_start=`` is a clean motion, noised to that level inside the loop with draw 0 (the draw x_T takes in a run from noise, so
        ``row_keys`` / ``row_seeds`` / ragged lengths address it alike) — one or the other.

        ``solver="ddim" | "dpm2m"`` (keyword; default: this object's ``solver`` attribute, ``"ddim"``): ``"dpm2m"`` makes every denoise step
        that directly follows the denoise step one level above it — and is not the last — the second-order DPM-Solver++(2M) update
        (dsh_run_spec.solver); all other steps, the draws and the noise addressing are the DDIM loop's.  Needs ``eta == 0`` and no
        ``same_overlap_noisy``.  Meant for few steps on a ``'logsnrK'`` subset (:func:`space_timesteps`).

        ``cond_fn``: a :class:`diffsheg_amd.glue.MotionGuidance` (soft keyframes, velocity / acceleration damping) — every denoise step is
        the guided form of its kernel (``condition_score``, gaussian_diffusion.py:660-682; ``p_sample_loop``: ``condition_mean``,
        :645-658), under both solvers, with masks, ``eta`` and ragged lengths; no draw is added.  Any other callable, and
        ``denoised_fn``, stay refused.

        ``cfg_schedule`` (keyword, also on ``p_sample_loop``): a :class:`diffsheg_amd.glue.CFGSchedule` — the guidance weight per model
        timestep and encoder, and the std rescale of the guided eps — for this call, handled as ``cond_scale=`` is: the model's sticky
        schedule (``UniDiffuser.set_guidance_schedule``) comes back afterwards, also when the call raises.

        ``sync_left`` / ``sync_len`` (keywords, together; not in the reference): synchronised window batches.  The rows are windows of
        long streams; row ``b`` shares its first ``sync_len`` frames with the last ``sync_len`` valid frames of row ``sync_left[b]``
        (``-1``: none), and behind every denoise step both copies take the ``addBlend`` cross-fade of the two
        (``dsh_run_spec.sync_left``, ``dsh_op_window_sync``).  ``noise=`` must be x_T cut from ONE noise value per stream frame
        (:meth:`DDPMTrainer.sample_arbitrary_len_synchronised` builds all of it).  Refused with ``eta != 0``, a mask, ``noise_source``,
        ``start_level`` / ``x_start``, ``tail_blend`` and ``opt.same_overlap_noisy``."""
        if not self._respacing:
            raise NotImplementedError("ddim_sample_loop needs a SpacedDiffusion('ddimK') (trainers use 'ddim25')")
        return self._run(0, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta=eta, **kw)


    # ---- editing an existing motion -----------------------------------------------------------
    def _fixed_from(self) -> int:
        """opt.fix_head_var in q_sample (gaussian_diffusion.py:443-456): the head channels keep x_start; -1 without the switch."""
        if not getattr(self.opt, "fix_head_var", False):
            return -1
        name = getattr(self.opt, "dataset_name", None)
        if name == "freeform_all":
            return 24
        if name == "talkshow":
            return 90
        raise NotImplementedError("fix_head_var: dataset_name must be 'freeform_all' or 'talkshow' (gaussian_diffusion.py:444-455)")

    def q_sample_coefficients(self, t, B: int):
        """(sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]) per row as fp32 host tensors: the fp64 square roots of the table
        rounded once, like the reference's tables through ``_extract_into_tensor``."""
        ts = [int(t)] * B if isinstance(t, numbers.Integral) else [int(v) for v in (t.tolist() if isinstance(t, torch.Tensor) else t)]
        if len(ts) != B or any(v < 0 or v >= self.num_timesteps for v in ts):
            raise ValueError(f"t needs one index in 0 .. {self.num_timesteps - 1} (or one per batch row, {B}), got {ts}")
        ac = self.alphas_cumprod[np.asarray(ts, dtype=np.int64)]
        return (torch.from_numpy(np.sqrt(ac).astype(np.float32)), torch.from_numpy(np.sqrt(1.0 - ac).astype(np.float32)))

    def q_sample(self, x_start, t, noise=None, *, seed=None, row_keys=None, row_seeds=None, lengths=None, _coef_dev=None):
        """gaussian_diffusion.py:417-462 on the device: ``sqrt(ac[t]) x_start + sqrt(1 - ac[t]) noise``, ``x_start [B, T, C]`` on a GPU,
        ``t`` an int or one index of THIS diffusion's (spaced) tables per row.  ``noise`` given: used as it is.  Otherwise it is drawn in
        the same pass from the Philox streams a sampling loop with the same ``seed`` / ``row_keys`` / ``row_seeds`` / ``lengths`` takes its
        draw 0 from.  ``lengths`` (one frame count per row): padded frames of the result are 0.  ``opt.fix_head_var`` keeps the head
        channels of ``x_start`` (24 / 90 and up for the reference's two datasets), as the reference does."""
        if not isinstance(x_start, torch.Tensor) or x_start.dim() != 3:
            raise ValueError("q_sample takes x_start [B, T, C]")
        fixed_from = self._fixed_from()
        if not x_start.is_cuda:
            raise _lib.DshError("q_sample runs on the GPU (no CPU fallback)")
        B, T, Cc = (int(v) for v in x_start.shape)
        if _coef_dev is None:
            a, s = self.q_sample_coefficients(t, B)
        if noise is not None and tuple(noise.shape) != (B, T, Cc):
            raise ValueError(f"noise {tuple(noise.shape)} does not match x_start {(B, T, Cc)}")
        lens = normalize_lengths(lengths, B, T) if lengths is not None else None
        if row_keys is not None and len(row_keys) != B:
            raise ValueError(f"row_keys needs one key per batch row ({B}), got {len(row_keys)}")
        if row_seeds is not None and (row_keys is None or len(row_seeds) != B):
            raise ValueError(f"row_seeds needs row_keys and one seed per batch row ({B})")
        if noise is None and row_keys is None and lens is not None:
            raise ValueError("lengths with Philox noise need row_keys (a ragged row draws from its own stream)")
        if noise is None and row_keys is not None and ((T * Cc) % 4 or any((v * Cc) % 4 for v in (lens or []))):
            raise ValueError("row_keys: frames * channels (and length * channels of every row) must be a multiple of 4")
        dev = x_start.device
        x0 = x_start.to(torch.float32).contiguous()
        out = torch.empty_like(x0)
        nz = None if noise is None else noise.to(device=dev, dtype=torch.float32).contiguous()
        a_d, s_d = _coef_dev if _coef_dev is not None else (a.to(dev), s.to(dev))      # (training_losses hands in the device copies it made)
        if seed is None and noise is None:
            seed = int(torch.initial_seed()) + GaussianDiffusion._calls
            GaussianDiffusion._calls += 1
        M = 0xFFFFFFFFFFFFFFFF
        karr = None if (row_keys is None or noise is not None) else (C.c_uint64 * B)(*[int(k) & M for k in row_keys])
        sd = None
        if karr is not None and row_seeds is not None:
            sd = torch.tensor([(int(k) & M) - (1 << 64) if (int(k) & M) >> 63 else int(k) & M for k in row_seeds], dtype=torch.int64).to(dev)
        larr = None if lens is None else (C.c_int32 * B)(*lens)
        with torch.cuda.device(dev):
            rc = _lib.lib().dsh_op_q_sample(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), out.data_ptr(), x0.data_ptr(),
                                            None if nz is None else nz.data_ptr(), a_d.data_ptr(), s_d.data_ptr(), B, T, Cc, 0, 0, fixed_from,
                                            int(seed or 0) & M, 0, karr, None if sd is None else sd.data_ptr(), larr, 0)
        _lib.check(rc, "dsh_op_q_sample")
        return out

    # ---- the eval-mode forward losses ----------------------------------------------------------
    def _row_values(self, table: np.ndarray, ts: List[int], B: int, dev, dtype=torch.float32) -> torch.Tensor:
        """``table[t_b]`` per row on the device, rounded once to ``dtype`` like the reference's ``_extract_into_tensor``.  One timestep for
        the whole batch is a fill launch; different ones go through pinned memory.  Neither blocks the host."""
        vals = np.asarray(table)[np.asarray(ts, dtype=np.int64)]
        if len(set(ts)) == 1:
            return torch.full((B,), vals[0].item(), dtype=dtype, device=dev)
        return _upload(torch.from_numpy(np.ascontiguousarray(vals)).to(dtype), dev)

    def draw_noise(self, B: int, T: int, Cc: int, dev, seed: int, row_keys=None, row_seeds=None, lens=None) -> torch.Tensor:
        """The noise ``q_sample(x_start, t, seed=, row_keys=, row_seeds=, lengths=)`` would draw inside its pass, as a tensor: the values of
        ``dsh_op_philox_randn`` at offset 0, or with ``row_keys`` those of the row ops at draw 0 (which wait for the stream once: they
        upload the keys).  Padded frames of a ragged row are 0."""
        M = 0xFFFFFFFFFFFFFFFF
        lib = _lib.lib()
        buf = torch.empty(B, T, Cc, device=dev) if lens is None else torch.zeros(B, T, Cc, device=dev)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if row_keys is None:
                rc = lib.dsh_op_philox_randn(stream, buf.data_ptr(), B * T * Cc, int(seed) & M, 0)
                what = "dsh_op_philox_randn"
            else:
                karr = (C.c_uint64 * B)(*[int(k) & M for k in row_keys])
                sd = None
                if row_seeds is not None:
                    sd = _upload(torch.tensor([(int(k) & M) - (1 << 64) if (int(k) & M) >> 63 else int(k) & M for k in row_seeds],
                                              dtype=torch.int64), dev)
                larr = None if lens is None else (C.c_int32 * B)(*lens)
                rc = lib.dsh_op_philox_randn_rows_ragged_seeded(stream, buf.data_ptr(), B, T * Cc, int(seed) & M, 0, karr, larr, 0, Cc,
                                                                None if sd is None else sd.data_ptr())
                what = "dsh_op_philox_randn_rows_ragged_seeded"
        _lib.check(rc, what)
        return buf

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, *, seed=None, row_keys=None, row_seeds=None, cond_scale=None,
                        cfg_schedule=None):
        """gaussian_diffusion.py:1319-1426, epsilon / MSE branch, in the reference's eval mode (no conditioning dropout, no gradient):
        ``x_t = q_sample(x_start, t, noise)``, one evaluation ``eps = model(x_t, timestep_map[t], ...)``, and the loss terms reduced on the
        device (``dsh_op_denoise_losses``).  ``x_start [B, T, C]`` on the GPU; ``t`` an int or one index per row into THIS diffusion's
        tables.  ``noise`` given: used as it is; else drawn from the Philox streams ``q_sample(..., seed=, row_keys=, row_seeds=)`` draws from,
        into a buffer (the same bits).  ``model_kwargs`` as for the sampling loops (``audio_emb``, ``person_id``, ``add_cond``, ``length``,
        ``pe_type``; ``y`` is accepted and unused: the reference's masking at :1394-1400 is commented out); ``length`` entries ``< T`` make
        the batch ragged under q_sample's rules (Philox noise then needs ``row_keys``): row ``b`` is scored as the clip alone at its
        length.  ``cond_scale`` as for the loops: with a scale other than 1 the guided eps is scored (transformer.py:537, :585),
        ``cond_scale=1.0`` scores the conditional model.  ``cfg_schedule`` (a :class:`diffsheg_amd.glue.CFGSchedule`) as for the loops: the
        guided eps under that schedule at each row's timestep, for this call.

        Returns the reference's keys where they cost nothing — ``"mse" [B]`` (``mean_flat`` of ``(noise - eps)^2`` over the row's own
        frames, fp64), ``"target"`` (the noise), ``"pred"`` (eps), ``"target_x0"`` (``x_start`` itself), ``"pred_x0"`` — plus ``"x_t"``,
        ``"row_terms" [B, 7]`` fp64 (include/diffsheg_hip.h), ``"frame_mse" [B, T]`` and ``"scalars"``: 0-d fp64 device tensors
        ``loss_model_pred`` / ``loss_vel_rec`` / ``loss_x0_rec`` / ``final_loss`` in backward_G's formulas (``loss_vel_rec`` and
        ``final_loss`` are left out when no row has two frames).  ``target_vel`` / ``pred_vel`` are not materialised: the velocity loss is
        row term 3.  Nothing synchronises (but the row ops behind ``row_keys``) and nothing is copied to the host."""
        # ---- refusals: before any device call ----
        if not isinstance(model, UniDiffuser):
            raise TypeError("model must be a diffsheg_amd.model.UniDiffuser (no generic-callable / CPU fallback)")
        model.check_guidance_schedule(cfg_schedule)
        lt = self.loss_type
        if (isinstance(lt, LossType) and lt.is_vb()) or (isinstance(lt, str) and lt.lower() in ("kl", "rescaled_kl")):
            raise NotImplementedError(f"loss_type {lt}: the variational-bound losses are not built (FIXED_SMALL variance: only the MSE branch)")
        if lt is not None and not isinstance(lt, LossType) and not (isinstance(lt, str) and lt.lower() in ("mse", "rescaled_mse")):
            raise NotImplementedError(f"unknown loss_type {lt!r}")
        model_kwargs = dict(model_kwargs or {})
        if model_kwargs.get("pre_seq") is not None:
            raise NotImplementedError("pre_seq is not on the accelerated path")
        if not isinstance(x_start, torch.Tensor) or x_start.dim() != 3:
            raise ValueError("training_losses takes x_start [B, T, C]")
        B, T, Cc = (int(v) for v in x_start.shape)
        if normalize_modality(model_kwargs.get("modality", "both"), model_kwargs.get("expression"), B, T, model.cfg.expression_dim,
                              model.cfg.unidiffuser) != 0:
            raise NotImplementedError("training_losses scores both modalities: the objective is defined on all channels")
        if not x_start.is_cuda:
            raise _lib.DshError("training_losses runs on the GPU (no CPU fallback)")
        ts = [int(t)] * B if isinstance(t, numbers.Integral) else [int(v) for v in (t.tolist() if isinstance(t, torch.Tensor) else t)]
        if len(ts) != B or any(v < 0 or v >= self.num_timesteps for v in ts):
            raise ValueError(f"t needs one index in 0 .. {self.num_timesteps - 1} (or one per batch row, {B}), got {ts}")
        if noise is not None and tuple(noise.shape) != (B, T, Cc):
            raise ValueError(f"noise {tuple(noise.shape)} does not match x_start {(B, T, Cc)}")
        lens = normalize_lengths(model_kwargs.get("length"), B, T)
        if row_keys is not None and len(row_keys) != B:
            raise ValueError(f"row_keys needs one key per batch row ({B}), got {len(row_keys)}")
        if row_seeds is not None and (row_keys is None or len(row_seeds) != B):
            raise ValueError(f"row_seeds needs row_keys and one seed per batch row ({B})")
        if noise is None and row_keys is None and lens is not None:
            raise ValueError("lengths with Philox noise need row_keys (a ragged row draws from its own stream)")
        if noise is None and row_keys is not None and ((T * Cc) % 4 or any((v * Cc) % 4 for v in (lens or []))):
            raise ValueError("row_keys: frames * channels (and length * channels of every row) must be a multiple of 4")
        split = int(getattr(self.opt, "split_pos", model.cfg.split_pos))
        beta = float(getattr(self.opt, "huber_beta", 0.1))
        if not 0 < split < Cc:
            raise ValueError(f"split_pos = {split} must lie inside (0, {Cc})")
        gs = self._guidance(model, cond_scale, B)
        # ---- device work ----
        dev = model.device
        x0 = x_start.to(device=dev, dtype=torch.float32).contiguous()
        if noise is None:
            if seed is None:
                seed = int(torch.initial_seed()) + GaussianDiffusion._calls
                GaussianDiffusion._calls += 1
            nz = self.draw_noise(B, T, Cc, dev, seed, row_keys, row_seeds, lens)
        else:
            nz = noise.to(device=dev, dtype=torch.float32).contiguous()
        a_d = self._row_values(np.sqrt(self.alphas_cumprod), ts, B, dev)
        s_d = self._row_values(np.sqrt(1.0 - self.alphas_cumprod), ts, B, dev)
        x_t = self.q_sample(x0, ts, noise=nz, lengths=lens, _coef_dev=(a_d, s_d))
        c1 = self._row_values(self.sqrt_recip_alphas_cumprod, ts, B, dev)
        c2 = self._row_values(self.sqrt_recipm1_alphas_cumprod, ts, B, dev)
        t_model = self._row_values(np.asarray(self.timestep_map, dtype=np.int64), ts, B, dev, torch.int64)
        with self._native(model, gs, cfg_schedule):
            eps = model(x_t, t_model, sqrt_alphas=[c1, c2], audio_emb=model_kwargs.get("audio_emb"), length=model_kwargs.get("length"),
                        person_id=model_kwargs.get("person_id"), add_cond=model_kwargs.get("add_cond"),
                        pe_type=model_kwargs.get("pe_type", "pe_sinu"), y=model_kwargs.get("y"))
        lens_dev = None if lens is None else _upload(torch.tensor(lens, dtype=torch.int32), dev)
        r = denoise_losses(eps, nz, x_t, x0, c1, c2, split, lens_dev, beta)
        rows = r["row_terms"]
        out = {"mse": (rows[:, 0] + rows[:, 1]) / rows[:, 5], "target": nz, "pred": eps, "target_x0": x_start, "pred_x0": r["pred_x0"],
               "x_t": x_t, "row_terms": rows, "frame_mse": r["frame_mse"], "counts": r["counts"]}
        has_pair = max(lens or [T]) > 1
        out["scalars"] = {k: r["scalars"][i] for i, k in enumerate(LOSS_SCALARS) if has_pair or k in ("loss_model_pred", "loss_x0_rec")}
        return out

    def _invert(self, model, x, from_level, to_level, clip_denoised, denoised_fn, model_kwargs, eta, return_trace, cond_scale=None):
        if not isinstance(model, UniDiffuser):
            raise TypeError("model must be a diffsheg_amd.model.UniDiffuser (no generic-callable / CPU fallback)")
        if not self._respacing:
            raise NotImplementedError("the DDIM reverse ODE needs a SpacedDiffusion('ddimK') (trainers use 'ddim25')")
        if denoised_fn is not None:
            raise NotImplementedError("denoised_fn is not on the accelerated path")
        if eta != 0.0:
            raise ValueError("Reverse ODE only for deterministic path (eta must be 0, gaussian_diffusion.py:1081)")
        if model_kwargs is None or model_kwargs.get("y", None) is None:
            raise AttributeError("'NoneType' object has no attribute 'keys' (model_kwargs['y'] must be a dict)")
        y = model_kwargs["y"]
        if "outpainting_mask" in y and bool(y.get("outpainting_mask_any", True)):
            raise NotImplementedError("the reverse ODE takes no mask (ddim_reverse_sample has no RePaint branch)")
        if bool(getattr(self.opt, "same_overlap_noisy", False)):
            raise NotImplementedError("same_overlap_noisy does not apply to the reverse ODE")
        from_level, to_level = int(from_level), int(to_level)
        if not 0 <= from_level < to_level <= self._respacing:
            raise ValueError(f"the reverse ODE needs 0 <= from_level < to_level <= {self._respacing}, got {from_level}, {to_level}")
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("the reverse ODE takes x [B, T, C]")
        B, T, Cc = (int(v) for v in x.shape)
        gs = self._guidance(model, cond_scale, B)
        self._condition(model, model_kwargs, (B, T, Cc), normalize_lengths(model_kwargs.get("length"), B, T), False)
        dev = model.device
        out = x.to(device=dev, dtype=torch.float32).contiguous().clone()
        opts = self._opts(0, clip_denoised, 1, 0, 0, 0.0)
        # (no draws: the reverse loop reads neither the noise fields nor row keys)
        lib = _lib.lib()
        spec = _lib.run_spec(timesteps=self._kept or (), invert_from=from_level, invert_to=to_level, x=out.data_ptr())
        n_steps = C.c_int64()
        _lib.check(lib.dsh_sample_count(C.byref(opts), C.byref(spec), None, C.byref(n_steps)), "dsh_sample_count")
        trace = torch.empty(n_steps.value, B, T, Cc, device=dev) if return_trace else None
        spec.trace = None if trace is None else trace.data_ptr()
        with self._native(model, gs):
            _lib.check(lib.dsh_sample_run(model._h, C.byref(opts), C.byref(spec)), "dsh_sample_run")
        return (out, trace) if return_trace else out

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0, cond_scale=None):
        """gaussian_diffusion.py:1068-1104: one step of the DDIM reverse ODE, x at spaced level ``t`` (an int, or a tensor whose entries
        are all equal) -> level ``t + 1``.  Returns ``{"sample": x}``; ``pred_xstart`` stays on the device side and is not returned."""
        if isinstance(t, torch.Tensor):
            ts = set(int(v) for v in t.reshape(-1).tolist())
            if len(ts) != 1:
                raise NotImplementedError("one level per call: per-row levels need per-row schedules")
            t = ts.pop()
        return {"sample": self._invert(model, x, int(t), int(t) + 1, clip_denoised, denoised_fn, model_kwargs, eta, False, cond_scale)}

    def ddim_reverse_sample_loop(self, model, x, to_level, model_kwargs=None, return_trace=False, clip_denoised=False, eta=0.0,
                                 cond_scale=None):
        """DDIM inversion: ``x [B, T, C]`` (a clean motion) carried through ``ddim_reverse_sample`` at the spaced levels
        ``0 .. to_level - 1``, natively and in one call (dsh_sample_run with invert_to).  No draws.  The result stands at ``alphas_cumprod[to_level]``;
        ``ddim_sample_loop(start_level=K, noise=...)`` enters at ``alphas_cumprod[K - 1]`` (the guided-diffusion pairing of the two
        loops: close to, not exactly, an inverse).  ``return_trace``: also the state after every step ``[to_level, B, T, C]``."""
        return self._invert(model, x, 0, to_level, clip_denoised, None, model_kwargs, eta, return_trace, cond_scale)


class SpacedDiffusion(GaussianDiffusion):
    """respace.py:60-110: tables rebuilt from the kept cumulative alphas; the model sees ORIGINAL timesteps."""

    def __init__(self, use_timesteps, solver: str = "ddim", **kwargs):
        """``use_timesteps``: any non-empty subset of ``range(n)``.  A 'ddimK' stride takes the stride's own native route; any other subset
        travels as a list (dsh_run_spec.timesteps).  ``solver``: the default update rule of ``ddim_sample_loop``."""
        self.use_timesteps = set(int(t) for t in use_timesteps)
        n = len(kwargs["betas"]) if kwargs.get("betas") is not None else int(kwargs.get("num_timesteps", 1000))
        k = len(self.use_timesteps)
        if k == 0 or min(self.use_timesteps) < 0 or max(self.use_timesteps) >= n:
            raise ValueError(f"use_timesteps must be a non-empty subset of range({n})")
        if solver not in ("ddim", "dpm2m"):
            raise ValueError(f'solver must be "ddim" or "dpm2m", got {solver!r}')
        try:
            strided = self.use_timesteps == space_timesteps(n, f"ddim{k}")
        except _lib.DshError:                     # (no integer stride gives k steps)
            strided = False
        self._kept = None if strided else sorted(self.use_timesteps)
        self._respacing = k
        self.solver = solver
        super().__init__(**kwargs)

    def _load_tables(self):
        if self._kept is None:
            super()._load_tables()
        else:
            for name in _TABLES:
                setattr(self, name, diffusion_table_subset(self.original_num_steps, self._kept, name))
            self.num_timesteps = len(self.betas)
        self.timestep_map = sorted(self.use_timesteps)
