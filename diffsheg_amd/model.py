"""Host-side mirror of the reference denoiser interface (boundary 1).

``UniDiffuser`` here is *not* an nn.Module: it is a thin handle on a ``dsh_ctx`` of
libdiffsheg_hip.so that keeps the reference's call signature

    model(x, timesteps, sqrt_alphas, audio_emb, length, person_id, add_cond={}, pe_type=..., y=None)

(/root/reference/models/transformer.py:728) so ``GaussianDiffusion.p_mean_variance`` style callers
(``model(x, ts, **model_kwargs)``, gaussian_diffusion.py:536) work unchanged.  PyTorch is used only
for device memory and the stream handle.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .config import DiffSHEGConfig
from .weights import strip_ddp_prefix, validate_state_dict

# "bf16x3": the fp32 path with its large Linears as three bf16 MFMAs per product (precision 2 of the C header); bit-identical to "fp32" at or below
# the few-row threshold (512 token rows), so a single clip gains nothing
_PRECISION = {"fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "bf16x3": 2}


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev_f32(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def normalize_guidance_scale(scale) -> Optional[Tuple[float, ...]]:
    """Guidance-scale argument -> ``None`` (the config's ``cond_scale``) or a tuple of float32-representable values: one value for the
    whole batch (a float, a 0-d tensor / array) or one per batch row (a sequence, a 1-D tensor / array).  Raises ``ValueError`` on an
    empty or multi-dimensional argument and on a non-finite value."""
    if scale is None:
        return None
    if isinstance(scale, torch.Tensor):
        scale = scale.detach().to("cpu", torch.float64)
        vals = [float(scale)] if scale.dim() == 0 else (scale.tolist() if scale.dim() == 1 else None)
    elif isinstance(scale, numbers.Real):
        vals = [float(scale)]
    elif hasattr(scale, "ndim") and getattr(scale, "ndim") == 0:        # numpy scalar / 0-d array
        vals = [float(scale)]
    else:
        try:
            vals = [float(v) for v in scale]
        except (TypeError, ValueError) as e:
            raise ValueError(f"cond_scale must be a float or a sequence of floats, got {type(scale).__name__}") from e
    if vals is None:
        raise ValueError("cond_scale must be a scalar or one value per batch row (1-D)")
    if not vals:
        raise ValueError("cond_scale: empty sequence")
    vals = torch.tensor(vals, dtype=torch.float64).to(torch.float32).tolist()      # (what the kernels will read)
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"cond_scale must be finite (in float32), got {vals}")
    return tuple(vals)


def normalize_lengths(length, batch: int, frames: int) -> Optional[Tuple[int, ...]]:
    """Per-clip frame counts of a padded batch ``[batch, frames, ...]`` -> ``None`` (every clip is ``frames`` long: also what ``None``
    and the reference's ``cur_len = T`` tensors mean) or a tuple of ``batch`` ints in ``1 .. frames`` with at least one entry
    ``< frames``.  Raises ``ValueError`` on a wrong count or a length outside that range.  (The values are read on the host: a device
    tensor costs one sync per call.)"""
    if length is None:
        return None
    if isinstance(length, torch.Tensor):
        length = length.detach().to("cpu").reshape(-1).tolist()
    vals = [int(v) for v in length]
    if len(vals) != batch:
        raise ValueError(f"length needs one entry per batch row ({batch}), got {len(vals)}")
    if any(v < 1 or v > frames for v in vals):
        raise ValueError(f"length: every clip needs 1 .. {frames} frames (the padded frame count), got {vals}")
    return None if all(v == frames for v in vals) else tuple(vals)


MODALITIES = {"both": 0, "expression": 1, "gesture": 2}      # the numbers of dsh_set_modality (include/diffsheg_hip.h)


def normalize_modality(modality="both", expression=None, batch: Optional[int] = None, frames: Optional[int] = None,
                       expression_dim: Optional[int] = None, unidiffuser: bool = True, same_overlap_noisy: bool = False) -> int:
    """``modality`` / ``expression`` arguments -> 0 (both), 1 (expression) or 2 (gesture).  ``modality`` is one of the names of
    :data:`MODALITIES`, its number, or ``None`` (both).  Raises ``ValueError`` on an unknown value; on a partial modality for the
    single-``MotionTransformer`` model (``unidiffuser=False``) or together with ``same_overlap_noisy`` (the saved noisy tails describe
    all channels); on ``"gesture"`` without an ``expression`` track or with one that is not a floating-point ``[batch, frames,
    expression_dim]`` tensor (each dimension checked where given); and on a track given with any other modality."""
    if modality is None:
        m = 0
    elif isinstance(modality, str):
        if modality not in MODALITIES:
            raise ValueError(f"modality must be one of {sorted(MODALITIES)}, got {modality!r}")
        m = MODALITIES[modality]
    elif isinstance(modality, numbers.Integral) and not isinstance(modality, bool):
        m = int(modality)
        if m not in MODALITIES.values():
            raise ValueError(f"modality must be 0 (both), 1 (expression) or 2 (gesture), got {m}")
    else:
        raise ValueError(f"modality must be one of {sorted(MODALITIES)}, got {modality!r}")
    if m != 0 and not unidiffuser:
        raise ValueError("a partial modality needs the UniDiffuser: a single MotionTransformer has no separate expression / gesture encoders")
    if m != 0 and same_overlap_noisy:
        raise ValueError("same_overlap_noisy with a partial modality: the saved noisy tails describe all channels")
    if m != 2:
        if expression is not None:
            raise ValueError('an expression track is only read with modality="gesture"')
        return m
    if expression is None:
        raise ValueError('modality="gesture" needs the expression track: expression=[B, T, expression_dim]')
    if not isinstance(expression, torch.Tensor) or not torch.is_floating_point(expression) or expression.dim() != 3:
        raise ValueError("expression must be a floating-point tensor [B, T, expression_dim]")
    want = (batch, frames, expression_dim)
    if any(w is not None and int(w) != int(g) for w, g in zip(want, expression.shape)):
        raise ValueError(f"expression must be [B, T, expression_dim] = {want}, got {tuple(expression.shape)}")
    return m


class UniDiffuser:
    """MI355X UniDiffuser: ``encoder_aud`` + ``encoder_exp`` + ``encoder_ges`` behind one C handle."""
    _UNIDIFFUSER = True

    def __init__(self, cfg: DiffSHEGConfig, state_dict: Dict[str, torch.Tensor], device="cuda:0",
                 precision: str = "fp32"):
        if not torch.cuda.is_available():
            raise _lib.DshError("no GPU visible: diffsheg_amd has no CPU fallback (the CPU oracle lives in oracle/ "
                                "and is test infrastructure only)")
        if precision not in _PRECISION:
            raise ValueError(f"precision must be one of {sorted(_PRECISION)}")
        self.cfg = cfg
        self.device = torch.device(device)
        self.precision = precision
        self._lib = _lib.lib()
        torch.cuda.set_device(self.device)
        self._stream = torch.cuda.current_stream(self.device)
        mc = _lib.ModelConfigC(cfg.dim_pose, cfg.expression_dim, cfg.style_dim, int(cfg.classifier_free),
                               float(cfg.cond_scale), cfg.latent_dim, cfg.ff_size, cfg.num_layers, cfg.num_heads,
                               cfg.audio_dim, cfg.aud_latent_dim, cfg.hubert_dim, cfg.hubert_enc_dim,
                               _PRECISION[precision], int(not cfg.unidiffuser), int(cfg.diffusion_steps))
        if cfg.unidiffuser != self._UNIDIFFUSER:
            raise ValueError(f"{type(self).__name__} needs a config with unidiffuser={self._UNIDIFFUSER} (runner.py:33-57 picks the class by opt.unidiffuser)")
        h = C.c_void_p()
        _lib.check(self._lib.dsh_create(C.byref(mc), C.c_void_p(self._stream.cuda_stream), C.byref(h)), "dsh_create")
        self._h = h
        self._cond_key = None
        self._cond_keep = None
        self.lengths = None                    # per-clip frame counts of a ragged condition (set_condition(lengths=))
        self.modality = 0                      # 0 both / 1 expression / 2 gesture: part of the condition (set_condition(modality=))
        self._guidance = None                  # set_guidance_scale(): None = the config's cond_scale
        self._schedule = None                  # set_guidance_schedule(): None = no schedule
        self._dummy = torch.zeros(1, device=self.device)
        self.load_state_dict(state_dict)

    # ---- weights ---------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        sd = strip_ddp_prefix(state_dict)
        validate_state_dict(self.cfg, sd)
        for name, t in sd.items():
            if not torch.is_floating_point(t):
                continue                      # num_batches_tracked
            a = t.detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * a.dim())(*a.shape)
            _lib.check(self._lib.dsh_load_tensor(self._h, name.encode(), C.c_void_p(a.data_ptr()), shape, a.dim()),
                       f"dsh_load_tensor({name})")
        _lib.check(self._lib.dsh_finalize_weights(self._h), "dsh_finalize_weights")

    @property
    def weight_bytes(self) -> int:
        return int(self._lib.dsh_weight_bytes(self._h))

    # ---- nn.Module look-alikes used by the reference sampler/harness ---------------------------
    def parameters(self) -> Iterator[torch.Tensor]:
        yield self._dummy                     # `next(model.parameters()).device` (gaussian_diffusion.py:1181)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stream ordering ---------------------------------------------------------------------
    def _enter(self) -> "torch.cuda.Stream":
        """The context is bound to the stream that was current at construction.  When the caller now works under
        another torch stream, order the context stream after it (and, in :meth:`_exit`, the caller's stream after the
        context's work), so inputs are complete before the native kernels read them and outputs / freed temporaries
        are not touched early.  A context built on the NULL stream runs on a private *blocking* stream, which the NULL
        stream orders implicitly, so waiting on / for ``torch.cuda.default_stream()`` is sufficient there as well."""
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
        return cur

    def _exit(self, cur: "torch.cuda.Stream") -> None:
        if cur != self._stream:
            cur.wait_stream(self._stream)

    # ---- conditioning ------------------------------------------------------------------------
    def set_condition(self, audio_emb: torch.Tensor, person_id: torch.Tensor, hubert: torch.Tensor, lengths=None, modality="both",
                      expression: Optional[torch.Tensor] = None) -> None:
        """Upload the step-invariant conditioning and run hubert_encoder / pid_embed once.  ``lengths`` (one frame count per clip,
        ``1 .. T``): the batch is ragged — clip ``b`` is the first ``lengths[b]`` frames of its padded row, and those frames of every
        following evaluation / sampling loop are what the clip gives alone at that length, whatever the padded frames of any input
        hold (``dsh_set_condition_ragged``).  ``None`` or all equal to ``T``: every clip is full, the path it always was.

        ``modality`` (``"both"`` / ``"expression"`` / ``"gesture"``, part of the condition): one encoder alone (``dsh_set_modality``).
        ``"expression"`` launches no gesture-encoder kernel: the expression columns of every result are the joint run's, the gesture
        columns 0.  ``"gesture"`` needs ``expression`` ``[B, T, expression_dim]`` (standardised, the clean track), which the gesture
        encoder reads at every step in place of the expression encoder's estimate; the expression encoder is not launched, the
        expression columns of an evaluation are 0 and those of a sampled result are the track itself.  Tensors keep their full
        width; the inactive columns of ``x``, ``gt``, the mask and the noise are never read."""
        B, T = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        lens = normalize_lengths(lengths, B, T)
        mod = normalize_modality(modality, expression, B, T, self.cfg.expression_dim, self.cfg.unidiffuser)
        if person_id.dim() == 1:                                   # transformer.py:502-503
            person_id = person_id.unsqueeze(0)
        if person_id.shape[0] != B:
            if person_id.shape[0] != 1:
                raise ValueError("person_id batch does not match audio_emb")
            person_id = person_id.expand(B, -1)
        if tuple(audio_emb.shape) != (B, T, self.cfg.audio_dim):
            raise ValueError(f"audio_emb must be [B,T,{self.cfg.audio_dim}], got {tuple(audio_emb.shape)}")
        if tuple(hubert.shape) != (B, T, self.cfg.hubert_dim):
            raise ValueError(f"pretrain_aud_feat must be [B,T,{self.cfg.hubert_dim}], got {tuple(hubert.shape)}")
        if person_id.shape[1] != self.cfg.style_dim:
            raise ValueError(f"person_id must be [B,{self.cfg.style_dim}]")
        a, p, hb = (_dev_f32(t, self.device) for t in (audio_emb, person_id, hubert))
        ex = _dev_f32(expression, self.device) if mod == 2 else None
        cur = self._enter()
        try:
            if lens is None:
                _lib.check(self._lib.dsh_set_condition(self._h, B, T, a.data_ptr(), p.data_ptr(), hb.data_ptr()),
                           "dsh_set_condition")
            else:
                _lib.check(self._lib.dsh_set_condition_ragged(self._h, B, T, (C.c_int32 * B)(*lens), a.data_ptr(), p.data_ptr(),
                                                              hb.data_ptr()), "dsh_set_condition_ragged")
            self.modality = 0                  # (a new condition is a joint one)
            if mod != 0:
                _lib.check(self._lib.dsh_set_modality(self._h, mod, _ptr(ex)), "dsh_set_modality")
                self.modality = mod
        finally:
            self._exit(cur)                    # (also when the call is refused: the caller's stream stays ordered after the context's)
        self._cond_keep = (a, p, hb, ex)       # (the library copies them in stream order; kept for the allocator's sake)
        self.batch, self.frames = B, T
        self.lengths = lens                    # None: every clip is full

    def _maybe_set_condition(self, audio_emb, person_id, add_cond, length=None, modality="both", expression=None) -> None:
        if "pretrain_aud_feat" not in (add_cond or {}):
            raise ValueError("add_cond['pretrain_aud_feat'] (HuBERT features) is required (addHubert=True)")
        hub = add_cond["pretrain_aud_feat"]
        # Identity + in-place-version check on the caller's tensor objects.  The objects themselves are
        # kept alive in the key: a freed tensor's address can be handed to a new tensor of the same shape,
        # so data_ptr alone would alias stale conditioning.
        B, T = int(audio_emb.shape[0]), int(audio_emb.shape[1])
        mod = normalize_modality(modality, expression, B, T, self.cfg.expression_dim, self.cfg.unidiffuser)
        # (the modality and the given track are part of the condition: the track by identity and version like the others)
        src = (audio_emb, person_id, hub) + ((expression,) if mod == 2 else ())
        vers = tuple(t._version for t in src)
        # (the lengths are part of the condition; compared by value: callers build a fresh `length` tensor per call)
        lens = normalize_lengths(length, int(audio_emb.shape[0]), int(audio_emb.shape[1]))
        if (self._cond_key is None or len(self._cond_key[0]) != len(src) or any(a is not b for a, b in zip(self._cond_key[0], src))
                or self._cond_key[1] != vers or self._cond_key[2] != lens or self._cond_key[3] != mod):
            self._cond_key = None              # (a refused call below leaves the native condition as it was, whatever it is now)
            self.set_condition(audio_emb, person_id, hub, lens, mod, expression if mod == 2 else None)
            self._cond_key = (src, vers, lens, mod)

    # ---- classifier-free guidance ---------------------------------------------------------------
    def set_guidance_scale(self, scale=None) -> None:
        """Guidance scale of every following evaluation and sampling loop (sticky, like the reference's ``opt.cond_scale``, which
        transformer.py:537 / :586 read on every forward): a float for the whole batch, a sequence / 1-D tensor of one value per batch
        row, or ``None`` for the config's ``cond_scale``.  Per-row values must match the batch of the next call.  Weights without
        ``classifier_free`` take only 1."""
        vals = normalize_guidance_scale(scale)
        if vals is not None and not self.cfg.classifier_free and any(v != 1.0 for v in vals):
            raise ValueError(f"cond_scale={list(vals)}: the weights are not classifier-free (no null_cond_emb), only 1 is possible")
        n = 0 if vals is None else len(vals)
        arr = (C.c_float * max(n, 1))(*(vals or (1.0,)))
        cur = self._enter()
        try:
            _lib.check(self._lib.dsh_set_guidance_scale(self._h, arr, n), "dsh_set_guidance_scale")
        finally:
            self._exit(cur)
        self._guidance = vals

    @property
    def guidance_scale(self) -> Optional[Tuple[float, ...]]:
        """The current setting: ``None`` (the config's ``cond_scale``) or the tuple given to :meth:`set_guidance_scale`."""
        return self._guidance

    def check_guidance_schedule(self, sched) -> None:
        """What :meth:`set_guidance_schedule` refuses, without touching the context (the loops ask before they condition anything)."""
        from .glue import CFGSchedule
        if sched is None:
            return
        if not isinstance(sched, CFGSchedule):
            raise ValueError(f"a guidance schedule is a glue.CFGSchedule (or None), got {type(sched).__name__}")
        if sched.steps != int(self.cfg.diffusion_steps):
            raise ValueError(f"CFGSchedule(steps={sched.steps}): the model has {self.cfg.diffusion_steps} diffusion steps (one gain per original timestep)")
        if not self.cfg.classifier_free and not sched.trivial:
            raise ValueError("CFGSchedule: the weights are not classifier-free (no null_cond_emb), there is no guidance to schedule")
        if not self.cfg.unidiffuser and not sched.same_for_both:
            raise ValueError("CFGSchedule: a single MotionTransformer has one encoder: expression and gesture gains (and rescale) must be equal")

    def set_guidance_schedule(self, sched=None) -> None:
        """Guidance schedule of every following evaluation and sampling loop (sticky, like :meth:`set_guidance_scale`): a
        :class:`diffsheg_amd.glue.CFGSchedule` — gains per original timestep and encoder, std rescale — or ``None`` for none, which puts
        every evaluation back on the launches it issues without one (``dsh_set_guidance_schedule``)."""
        self.check_guidance_schedule(sched)
        cur = self._enter()
        try:
            if sched is None:
                _lib.check(self._lib.dsh_set_guidance_schedule(self._h, None, None, 0, 0.0, 0.0), "dsh_set_guidance_schedule")
            else:
                fp = C.POINTER(C.c_float)
                e, g = np.ascontiguousarray(sched.expression, dtype=np.float32), np.ascontiguousarray(sched.gesture, dtype=np.float32)
                _lib.check(self._lib.dsh_set_guidance_schedule(self._h, e.ctypes.data_as(fp), g.ctypes.data_as(fp), sched.steps,
                                                               sched.rescale[0], sched.rescale[1]), "dsh_set_guidance_schedule")
        finally:
            self._exit(cur)
        self._schedule = sched

    @property
    def guidance_schedule(self):
        """The current setting: ``None`` or the :class:`~diffsheg_amd.glue.CFGSchedule` given to :meth:`set_guidance_schedule`."""
        return self._schedule

    # ---- boundary 1 -----------------------------------------------------------------------------
    def __call__(self, x, timesteps, sqrt_alphas=None, audio_emb=None, length=None, person_id=None, add_cond=None,
                 pe_type="pe_sinu", y=None, modality="both", expression=None) -> torch.Tensor:
        return self.forward(x, timesteps, sqrt_alphas, audio_emb, length, person_id, add_cond, pe_type, y, modality, expression)

    def forward(self, x, timesteps, sqrt_alphas, audio_emb, length, person_id, add_cond=None, pe_type="pe_sinu",
                y=None, modality="both", expression=None) -> torch.Tensor:
        if pe_type not in ("pe_sinu",):
            raise NotImplementedError(f"pe_type={pe_type!r}: only the default 'pe_sinu' path is built")
        if sqrt_alphas is None or len(sqrt_alphas) != 2:
            raise ValueError("sqrt_alphas=[sqrt_recip_alphas_cumprod_t, sqrt_recipm1_alphas_cumprod_t] is required")
        self._maybe_set_condition(audio_emb, person_id, add_cond, length, modality, expression)
        B, T, Cc = x.shape
        if (B, T) != (self.batch, self.frames) or Cc != self.cfg.net_dim_pose:
            raise ValueError(f"x shape {tuple(x.shape)} does not match conditioning ({self.batch},{self.frames},{self.cfg.net_dim_pose})")
        xd = _dev_f32(x, self.device)
        td = timesteps.to(device=self.device, dtype=torch.int64).contiguous()
        c1 = _dev_f32(sqrt_alphas[0].reshape(B, -1)[:, 0], self.device)
        c2 = _dev_f32(sqrt_alphas[1].reshape(B, -1)[:, 0], self.device)
        out = torch.empty_like(xd)
        cur = self._enter()
        try:
            _lib.check(self._lib.dsh_eval(self._h, xd.data_ptr(), td.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                          out.data_ptr()), "dsh_eval")
        finally:
            self._exit(cur)
        return out

    # ---- introspection -----------------------------------------------------------------------------
    def eval_flops(self) -> float:
        return float(self._lib.dsh_eval_flops(self._h))

    def debug_tap(self, what: str) -> torch.Tensor:
        w = {"aud_feat": self.cfg.audio_dim, "expr_x0": self.cfg.expression_dim}[what]
        out = torch.empty(self.batch, self.frames, w, device=self.device)
        _lib.check(self._lib.dsh_debug_copy(self._h, what.encode(), out.data_ptr()), "dsh_debug_copy")
        return out


class MotionTransformer(UniDiffuser):
    """The model ``runner.py:46-57`` builds when ``opt.unidiffuser`` is False (``model_base='transformer_encoder'``): ONE
    motion transformer over all ``net_dim_pose`` channels.  Same native context (``single_transformer = 1``), state-dict keys
    without the ``encoder_*`` prefix, and the reference's call signature (transformer.py:496)

        model(x, timesteps, audio_emb, length, person_id, add_cond={}, pe_type=..., y=None, block=None)

    — no ``sqrt_alphas`` (gaussian_diffusion.py:527-536 only passes them for the UniDiffuser)."""
    _UNIDIFFUSER = False

    def __call__(self, x, timesteps, audio_emb=None, length=None, person_id=None, add_cond=None, pe_type="pe_sinu", y=None,
                 block=None, sqrt_alphas=None) -> torch.Tensor:
        return self.forward(x, timesteps, audio_emb, length, person_id, add_cond, pe_type, y, block)

    def forward(self, x, timesteps, audio_emb, length, person_id, add_cond=None, pe_type="pe_sinu", y=None, block=None) -> torch.Tensor:
        one = torch.ones(x.shape[0], device=self.device)
        return UniDiffuser.forward(self, x, timesteps, [one, one], audio_emb, length, person_id, add_cond, pe_type, y)

    def debug_tap(self, what: str) -> torch.Tensor:
        raise NotImplementedError("aud_feat / expr_x0 taps exist only in the UniDiffuser model")
