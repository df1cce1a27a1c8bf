"""Live sessions: gestures and expressions for audio that is still arriving.

The long-audio entry points of :mod:`diffsheg_amd.trainer` need the whole feature stream up front and keep every chain of a batch at
the same window index.  A live caller (an avatar server, a call) has audio in pieces and sessions that start and end at different
times.  :class:`StreamPool` holds such chains open between calls and samples the windows that are due at one moment TOGETHER, whatever
their window indices:

* the noise of window ``k`` of a chain is Philox key ``window_seed(seed, k)``, counter high words = the chain's key.  With per-row keys
  AND per-row seeds (``dsh_sample_set_row_seeds``) every row of a batch draws exactly what it draws alone, so a session's stream is the
  chain ``DDPMTrainer.sample_arbitrary_len(audio, ..., seed=seed, row_keys=[key])`` gives for the audio fed so far — bit for bit for a
  session sampled alone, to batch-vs-alone round-off inside a batch;
* the state a chain carries from window to window — its last ``overlap_len`` frames — lives in a device-resident slot table
  ``tails[capacity, overlap_len, C]``; two kernels (``dsh_op_chain_handoff`` / ``dsh_op_chain_save_tail``) turn it into the next
  window's inpaint dictionary and refresh it, so nothing of a session leaves the device between calls.

The window rule is that of :func:`diffsheg_amd.trainer.get_windows` on the audio fed so far (:class:`StreamWindows`, pure Python).
Chained windows all run the same jump schedule, so sessions that are due together stay in lockstep inside a call; first windows run the
plain schedule and are a batch of their own (mixing the two in one call needs per-row schedules and is not built).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .model import normalize_guidance_scale
from .trainer import MIN_PAD_BATCH, MIN_PAD_FRAMES, DDPMTrainer, window_seed


class StreamWindows:
    """Window / cursor bookkeeping of ONE live chain (no tensors): which windows of ``n_poses`` frames, ``step_len = n_poses -
    overlap_len`` apart, a stream fed in pieces gives — exactly those :func:`diffsheg_amd.trainer.get_windows` cuts the whole stream into.

    A chain with cursor ``c`` is *due* when ``c + n_poses`` frames have been fed: its window is ``[c, c + n_poses)``, it emits the
    window's first ``step_len`` frames (the offline keep rule for every window but the last) and the cursor moves on by ``step_len``.
    :meth:`close_plan` says what the end of the stream still owes, from the ``m`` frames fed beyond the cursor."""

    def __init__(self, n_poses: int, overlap_len: int):
        n_poses, overlap_len = int(n_poses), int(overlap_len)
        if not 1 <= overlap_len < n_poses:
            raise ValueError(f"a window chain needs 1 <= overlap_len < n_poses, got overlap_len = {overlap_len}, n_poses = {n_poses}")
        self.n_poses, self.overlap_len, self.step_len = n_poses, overlap_len, n_poses - overlap_len
        self.fed = 0            # frames fed so far
        self.cursor = 0         # first frame of the next window
        self.windows = 0        # windows taken so far = index of the next window

    @property
    def pending(self) -> int:
        """Frames fed beyond the cursor."""
        return self.fed - self.cursor

    def feed(self, n: int) -> None:
        if int(n) < 1:
            raise ValueError(f"feed needs at least one frame, got {n}")
        self.fed += int(n)

    def due(self) -> bool:
        return self.fed >= self.cursor + self.n_poses

    def take(self) -> Tuple[int, int, int]:
        """The due window as ``(start, length, frames emitted)``; moves the cursor."""
        if not self.due():
            raise ValueError(f"no window is due: {self.pending} frames beyond the cursor, a window needs {self.n_poses}")
        start = self.cursor
        self.cursor += self.step_len
        self.windows += 1
        return start, self.n_poses, self.step_len

    def close_plan(self) -> Tuple[str, int, int, int]:
        """What closing the stream now still owes, as ``(kind, start, length, frames emitted)``; changes nothing.  With ``m`` frames
        fed beyond the cursor (every due window taken first):

        * ``"empty"``: nothing was fed — nothing is owed;
        * ``"flush"``: ``m == overlap_len`` behind at least one window — that window was the stream's last, and the offline path keeps
          all of it: the held-back last ``overlap_len`` frames of it are emitted, no window is sampled;
        * ``"tail"``: ``m > overlap_len`` behind at least one window — a chained tail window of ``m`` frames, emitted whole;
        * ``"short"``: no window yet and ``overlap_len < m < n_poses`` — one plain window of the stream's length, emitted whole;
        * no window yet and ``0 < m <= overlap_len``: ``ValueError`` — a window has to be longer than ``overlap_len`` frames (the
          chain's hand-off pins its first ``overlap_len`` frames; the reference's chain cannot express ``T <= overlap_len``)."""
        if self.due():
            raise ValueError("windows are still due: take them before closing")
        m, L = self.pending, self.overlap_len
        if self.windows == 0:
            if m == 0:
                return "empty", 0, 0, 0
            if m <= L:
                raise ValueError(f"a stream of {m} frames cannot be closed: a window needs more than overlap_len = {L} frames "
                                 f"(feed at least {L + 1 - m} more)")
            return "short", 0, m, m
        if m == L:
            return "flush", self.cursor, L, L
        return "tail", self.cursor, m, m


def _dev_i32(vals: Sequence[int], device) -> torch.Tensor:
    return torch.tensor(list(vals), dtype=torch.int32).to(device)


def _stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def chain_handoff(tails: torch.Tensor, slots: Sequence[int], frames: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``dsh_op_chain_handoff``: the inpaint dictionary's ``gt [R, frames, C]`` (first ``L`` frames = ``tails[slots[r]]``, the rest 0)
    and ``outpainting_mask [R, frames, C]`` uint8 (1 on the first ``L`` frames) of a chained window batch, from the slot table
    ``tails [S, L, C]`` (fp32, device, contiguous), in one launch on the current stream.  Refuses (``DshError``) ``L >= frames`` and a
    slot outside the table."""
    if not (tails.is_cuda and tails.dtype == torch.float32 and tails.dim() == 3 and tails.is_contiguous()):
        raise ValueError("tails must be a contiguous fp32 device tensor [S, L, C]")
    S, L, Cc = (int(v) for v in tails.shape)
    R = len(slots)
    gt = torch.empty(R, int(frames), Cc, device=tails.device)
    mask = torch.empty(R, int(frames), Cc, dtype=torch.uint8, device=tails.device)
    idx = _dev_i32(slots, tails.device)
    with torch.cuda.device(tails.device):
        _lib.check(_lib.lib().dsh_op_chain_handoff(_stream_ptr(tails.device), tails.data_ptr(), S, (C.c_int32 * max(R, 1))(*slots), idx.data_ptr(),
                                                   R, int(frames), L, Cc, gt.data_ptr(), mask.data_ptr()), "dsh_op_chain_handoff")
    return gt, mask


def chain_save_tail(x: torch.Tensor, slots: Sequence[int], tails: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> None:
    """``dsh_op_chain_save_tail``: ``tails[slots[r]] = x[r, n_r - L : n_r]`` with ``n_r = lengths[r]`` (default: all of ``x``'s frames), in
    one launch on the current stream.  ``x [R, T, C]`` fp32 device contiguous.  Refuses ``L >= T``, a length outside ``L .. T``, a slot
    outside the table and a slot named twice."""
    if not (tails.is_cuda and tails.dtype == torch.float32 and tails.dim() == 3 and tails.is_contiguous()):
        raise ValueError("tails must be a contiguous fp32 device tensor [S, L, C]")
    S, L, Cc = (int(v) for v in tails.shape)
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous() and int(x.shape[2]) == Cc and int(x.shape[0]) == len(slots)):
        raise ValueError(f"x must be a contiguous fp32 device tensor [{len(slots)}, T, {Cc}]")
    R, T = int(x.shape[0]), int(x.shape[1])
    idx = _dev_i32(slots, x.device)
    lens_h = lens_d = None
    if lengths is not None:
        if len(lengths) != R:
            raise ValueError(f"lengths needs one entry per row ({R})")
        lens_h, lens_d = (C.c_int32 * max(R, 1))(*[int(v) for v in lengths]), _dev_i32(lengths, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dsh_op_chain_save_tail(_stream_ptr(x.device), x.data_ptr(), lens_h, None if lens_d is None else lens_d.data_ptr(),
                                                     (C.c_int32 * max(R, 1))(*slots), idx.data_ptr(), R, T, L, Cc, tails.data_ptr(), S),
                   "dsh_op_chain_save_tail")


class _Session:
    __slots__ = ("slot", "key", "p_id", "cond_scale", "win", "audio", "cond", "base", "rows_alloc")

    def __init__(self, slot, key, p_id, cond_scale, win):
        self.slot, self.key, self.p_id, self.cond_scale, self.win = slot, key, p_id, cond_scale, win
        self.audio: Optional[torch.Tensor] = None          # frames [base, fed) of the mel features ...
        self.cond: Dict[str, torch.Tensor] = {}            # ... and of every add_cond entry
        self.base = 0
        self.rows_alloc = 0                                # frames the buffers' storage holds (>= their own length after a trim)


class StreamPool:
    """A fixed number of live window chains on one model, batched by what is due::

        pool = StreamPool(trainer, capacity, seed)
        sid = pool.open(p_id, key=None, cond_scale=None)
        pool.feed(sid, audio_emb[n, 128], add_cond={"pretrain_aud_feat": hubert[n, 1024]})      # any n >= 1, device or host
        out = pool.step()                    # {sid: Tensor[step_len, C]} for every session that was due
        rest = pool.close(sid)               # Tensor[frames, C]: what the stream's end still owes

    ``trainer`` is a :class:`DDPMTrainer` with ``opt.ddim`` and ``opt.overlap_len >= 1``; ``opt.fix_very_first`` and
    ``opt.same_overlap_noisy`` are refused, and so are noise stacks and a partial modality (the pool draws Philox noise and samples both
    modalities).  ``key`` is the chain id of the session's noise (default: a counter); a session's stream equals
    ``trainer.sample_arbitrary_len(audio[None], p_id, add_cond, seed=seed, row_keys=[key], cond_scale=cond_scale)[0]`` on everything fed.

    :meth:`step` advances every due session by ONE window with at most two sampler calls: one batched plain window for the sessions at
    window 0, one batched chained window (hand-off kernel -> ``generate_batch`` -> save-tail kernel) for all others, whatever their
    window indices.  A session fed more than one stride of audio is due again: call ``step`` until it returns ``{}``.  Consumed audio is
    dropped, so a session that is not due holds fewer than ``n_poses`` frames of features.

    :meth:`close` first takes the windows that are still due, then settles the end of the stream (:meth:`StreamWindows.close_plan`): a
    tail window (or the one short window of a stream that never reached ``n_poses`` frames) is sampled AT ONCE, in the closing call.
    :meth:`close_many` closes several sessions together and batches their tail windows into one chained call (``lengths=`` when they
    differ) and their short windows into one plain call; ``close(sid)`` is ``close_many([sid])[sid]``.  A refused close (fewer than
    ``overlap_len + 1`` frames in all) raises before anything changes: the session stays open and can be fed.
    """

    def __init__(self, trainer: DDPMTrainer, capacity: int, seed: int):
        opt = trainer.opt
        if not getattr(opt, "ddim", True):
            raise ValueError("StreamPool needs opt.ddim (mask-present DDPM sampling is not built)")
        if bool(getattr(opt, "fix_very_first", False)):
            raise ValueError("StreamPool refuses opt.fix_very_first: a live session has no ground-truth first window")
        if bool(getattr(opt, "same_overlap_noisy", False)):
            raise ValueError("StreamPool refuses opt.same_overlap_noisy: the saved noisy tails live in the context, one batch shape at a time")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be at least 1, got {capacity}")
        self.trainer = trainer
        self.n_poses, self.overlap_len, self.channels = int(opt.n_poses), int(opt.overlap_len), int(opt.net_dim_pose)
        StreamWindows(self.n_poses, self.overlap_len)                     # (raises on overlap_len < 1 or >= n_poses)
        self.step_len = self.n_poses - self.overlap_len
        self.capacity, self.seed = int(capacity), int(seed)
        self.device = trainer.device
        # slot s: the last overlap_len frames (standardised, fp32) of the window its session sampled last
        self.tails = torch.zeros(self.capacity, self.overlap_len, self.channels, device=self.device)
        self._free: List[int] = list(range(self.capacity - 1, -1, -1))
        self._sessions: Dict[int, _Session] = {}
        self._next_sid = 0

    # ---- sessions ---------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self._sessions)

    def _get(self, sid: int) -> _Session:
        try:
            return self._sessions[sid]
        except KeyError:
            raise KeyError(f"no open session {sid!r}") from None

    def open(self, p_id: torch.Tensor, key: Optional[int] = None, cond_scale: Optional[float] = None) -> int:
        """A new session for speaker ``p_id`` (one-hot ``[style_dim]`` or ``[1, style_dim]``); returns its id.  Raises ``RuntimeError``
        when all ``capacity`` slots are taken (a closed session's slot is reused)."""
        cfg = self.trainer.encoder.cfg
        p = p_id.reshape(-1).to(device=self.device, dtype=torch.float32)
        if p.numel() != cfg.style_dim:
            raise ValueError(f"p_id must hold {cfg.style_dim} entries, got {tuple(p_id.shape)}")
        gs = normalize_guidance_scale(cond_scale)
        if gs is not None:
            if len(gs) != 1:
                raise ValueError("a session takes one cond_scale")
            if not cfg.classifier_free and gs[0] != 1.0:
                raise ValueError(f"cond_scale={gs[0]}: the weights are not classifier-free (no null_cond_emb), only 1 is possible")
        if not self._free:
            raise RuntimeError(f"the pool is full: {self.capacity} sessions are open")
        sid = self._next_sid
        self._next_sid += 1
        self._sessions[sid] = _Session(self._free.pop(), sid if key is None else int(key), p, None if gs is None else gs[0],
                                       StreamWindows(self.n_poses, self.overlap_len))
        return sid

    def feed(self, sid: int, audio_emb: torch.Tensor, add_cond: Optional[Dict[str, torch.Tensor]] = None, **refused) -> None:
        """``n >= 1`` more frames of features: mel ``[n, audio_dim]`` and every ``add_cond`` entry ``[n, ...]`` (``pretrain_aud_feat`` is
        required), on the host or the device."""
        self._refuse(refused)
        s = self._get(sid)
        cfg = self.trainer.encoder.cfg
        add_cond = add_cond or {}
        if "pretrain_aud_feat" not in add_cond:
            raise ValueError("add_cond['pretrain_aud_feat'] (HuBERT features) is required (addHubert=True)")
        n = int(audio_emb.shape[0]) if audio_emb.dim() == 2 else -1
        if n < 1 or int(audio_emb.shape[1]) != cfg.audio_dim:
            raise ValueError(f"audio_emb must be [n, {cfg.audio_dim}] with n >= 1, got {tuple(audio_emb.shape)}")
        if s.audio is not None and set(add_cond) != set(s.cond):
            raise ValueError(f"add_cond keys changed inside a session: {sorted(add_cond)} after {sorted(s.cond)}")
        for k, v in add_cond.items():
            if v.dim() < 2 or int(v.shape[0]) != n:
                raise ValueError(f"add_cond[{k!r}] must be [{n}, ...], got {tuple(v.shape)}")

        def grow(old: Optional[torch.Tensor], new: torch.Tensor) -> torch.Tensor:
            new = new.to(device=self.device, dtype=torch.float32)
            return new.contiguous() if old is None or old.shape[0] == 0 else torch.cat([old, new], 0)      # (fresh storage: trimmed frames go)
        s.audio = grow(s.audio, audio_emb)
        s.cond = {k: grow(s.cond.get(k), v) for k, v in add_cond.items()}
        s.rows_alloc = int(s.audio.shape[0])
        s.win.feed(n)

    # ---- sampling ---------------------------------------------------------------------------------------------------------------
    def _trim(self, s: _Session) -> None:
        """Drop the features in front of the cursor (views; copied out of a storage that holds a window and a stride or more)."""
        drop = s.win.cursor - s.base
        if drop <= 0:
            return
        copy = s.rows_alloc >= self.n_poses + self.step_len
        s.audio = s.audio[drop:].clone() if copy else s.audio[drop:]
        s.cond = {k: (v[drop:].clone() if copy else v[drop:]) for k, v in s.cond.items()}
        s.base = s.win.cursor
        if copy:
            s.rows_alloc = int(s.audio.shape[0])

    def _sample(self, rows: List[Tuple[_Session, int, int]], chained: bool) -> torch.Tensor:
        """One sampler call: ``rows`` = (session, window start, window length), all plain (window 0) or all chained.  Returns the
        window batch ``[R, T, C]``; rows shorter than ``T`` are zero behind their length."""
        lens = [n for _, _, n in rows]
        T = max(lens)
        if len(rows) >= MIN_PAD_BATCH and T < MIN_PAD_FRAMES:            # (trainer.ragged_window_plan: a batch of short tails is padded)
            T = MIN_PAD_FRAMES

        def cut(pick) -> torch.Tensor:
            parts = []
            for s, start, n in rows:
                w = pick(s)[start - s.base:start - s.base + n]
                if n < T:
                    w = torch.cat([w, w.new_zeros((T - n,) + tuple(w.shape[1:]))], 0)
                parts.append(w)
            return torch.stack(parts, 0)
        a = cut(lambda s: s.audio)
        cnd = {k: cut(lambda s, k=k: s.cond[k]) for k in rows[0][0].cond}
        pid = torch.stack([s.p_id for s, _, _ in rows], 0)
        # Philox: key = hash(pool seed, the row's OWN window index), counter high words = the session's chain id
        kw = {"seed": self.seed, "row_keys": [s.key for s, _, _ in rows],
              "row_seeds": [window_seed(self.seed, s.win.windows) for s, _, _ in rows]}
        scales = [s.cond_scale for s, _, _ in rows]
        if any(v is not None for v in scales):
            default = float(getattr(self.trainer.opt, "cond_scale", self.trainer.encoder.cfg.cond_scale))
            kw["cond_scale"] = [default if v is None else v for v in scales]
        if any(n != T for n in lens):
            kw["lengths"] = lens
        inpaint = {}
        if chained:
            gt, mask = chain_handoff(self.tails, [s.slot for s, _, _ in rows], T)
            inpaint = {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}      # (said, not looked up: no host sync)
        return self.trainer.generate_batch(a, pid, self.channels, cnd, inpaint, **kw)

    def _advance(self, sessions: List[Tuple[int, _Session]]) -> Dict[int, torch.Tensor]:
        """One full window for each of the given (due) sessions: at most one plain and one chained call.  Un-converted frames."""
        out: Dict[int, torch.Tensor] = {}
        groups = [[(sid, s) for sid, s in sessions if (s.win.windows > 0) == chained] for chained in (False, True)]
        for chained, group in enumerate(groups):
            if not group:
                continue
            x = self._sample([(s, s.win.cursor, self.n_poses) for _, s in group], bool(chained))
            chain_save_tail(x, [s.slot for _, s in group], self.tails)
            for r, (sid, s) in enumerate(group):
                s.win.take()
                self._trim(s)
                out[sid] = x[r, :self.step_len]
        return out

    def _finish(self, pieces: Dict[int, List[torch.Tensor]], pose_rep: str, return_positions: bool = False):
        """Per-session frame lists -> one tensor each, gesture channels converted when asked (one launch for all of them).  With
        ``return_positions`` also ``{sid: Tensor[frames, J, 3]}``, the joints of the same frames from their axis-angle form (one launch)."""
        euler = self.trainer._euler_requested(pose_rep)
        positions = self.trainer._positions_requested(return_positions)
        cat = {sid: (torch.cat(p, 0) if len(p) != 1 else p[0]) if p else torch.zeros(0, self.channels, device=self.device) for sid, p in pieces.items()}
        joints = None
        if positions:
            sizes = [int(t.shape[0]) for t in cat.values()]
            joints = dict(zip(cat, torch.split(self.trainer.joint_positions(torch.cat(list(cat.values()), 0)), sizes, 0)))
        if euler and any(int(t.shape[0]) for t in cat.values()):
            sids = [sid for sid, t in cat.items() if int(t.shape[0])]
            conv = self.trainer._to_euler(torch.cat([cat[sid] for sid in sids], 0))
            pos = 0
            for sid in sids:
                n = int(cat[sid].shape[0])
                cat[sid] = conv[pos:pos + n]
                pos += n
        return (cat, joints) if positions else cat

    @staticmethod
    def _refuse(kw) -> None:
        if kw.get("guidance") is not None:
            raise NotImplementedError("guidance in live sessions (StreamPool) is not built")
        if kw:
            raise ValueError(f"StreamPool does not take {sorted(kw)}: it draws Philox noise from its own seed (no noise_source stacks) and "
                             "samples both modalities (a partial modality is not served)")

    def step(self, pose_rep: str = "axis_angle", return_positions: bool = False, **refused):
        """Advance every due session by one window; ``{sid: Tensor[step_len, C]}`` (on the device, no host synchronisation), ``{}`` when
        none was due.  ``pose_rep="euler"`` (BEAT, after ``trainer.set_pose_stats``): the emitted frames' gesture channels as the
        reference's standardised Euler degrees; the chain itself stays in the sampler's representation.  ``return_positions=True``
        (after ``trainer.set_skeleton``): ``(frames, positions)`` with ``positions = {sid: Tensor[step_len, J, 3]}``, the world-space
        joints of the emitted frames (from their axis-angle form, whatever ``pose_rep`` says); ``({}, {})`` when none was due."""
        self._refuse(refused)
        self.trainer._euler_requested(pose_rep)
        self.trainer._positions_requested(return_positions)
        due = [(sid, s) for sid, s in self._sessions.items() if s.win.due()]
        if not due:
            return ({}, {}) if return_positions else {}
        return self._finish({sid: [t] for sid, t in self._advance(due).items()}, pose_rep, return_positions)

    def close(self, sid: int, pose_rep: str = "axis_angle", return_positions: bool = False, **refused):
        """End session ``sid``: ``Tensor[frames, C]``, everything its stream still owes (possibly ``[0, C]``).  Frees its slot.
        ``return_positions=True``: ``(frames, Tensor[frames, J, 3])``."""
        out = self.close_many([sid], pose_rep, return_positions, **refused)
        return (out[0][sid], out[1][sid]) if return_positions else out[sid]

    def close_many(self, sids: Sequence[int], pose_rep: str = "axis_angle", return_positions: bool = False, **refused):
        """End several sessions in one call: their tail windows share one chained sampler call, their short windows one plain call.
        ``return_positions=True``: ``(frames, positions)``, two dicts by session."""
        self._refuse(refused)
        self.trainer._euler_requested(pose_rep)
        self.trainer._positions_requested(return_positions)
        sids = list(dict.fromkeys(sids))
        sessions = [(sid, self._get(sid)) for sid in sids]
        for _, s in sessions:                                  # refusals first: nothing has changed when one raises
            if not s.win.due():
                s.win.close_plan()
        pieces: Dict[int, List[torch.Tensor]] = {sid: [] for sid in sids}
        while True:
            due = [(sid, s) for sid, s in sessions if s.win.due()]
            if not due:
                break
            for sid, t in self._advance(due).items():
                pieces[sid].append(t)
        plans = {sid: s.win.close_plan() for sid, s in sessions}
        for kind, chained in (("short", False), ("tail", True)):
            group = [(sid, s) for sid, s in sessions if plans[sid][0] == kind]
            if group:
                x = self._sample([(s, plans[sid][1], plans[sid][2]) for sid, s in group], chained)
                for r, (sid, _) in enumerate(group):
                    pieces[sid].append(x[r, :plans[sid][2]])
        for sid, s in sessions:
            if plans[sid][0] == "flush":
                pieces[sid].append(self.tails[s.slot].clone())      # (the slot is about to be reused)
        out = self._finish(pieces, pose_rep, return_positions)
        for sid, s in sessions:
            self._free.append(s.slot)
            del self._sessions[sid]
        return out
