"""dsh_op_denoise_losses on a real MI355X against the float64 reference of tests/losses_ref.py, on random tensors at the shapes where the kernel
can break: one frame (no pair), two frames, frame counts that are no multiple of the 8-frame chunk, more than one chunk, C = 232 / 192 with the
split at 129 / 141 (neither a multiple of 4: 16-byte vectors straddle the split, rows and chunks start at any 4-byte offset), C = 5 (below a
wave, the scalar copy), and a ragged batch.  c1 / c2 are the full process's coefficients at t = 0, 500, 999 — at 999 c1 ~ 158 and
x0_pred = c1 x_t - c2 eps cancels.

Tolerances: none is fixed in advance.  A term's gate is MARGIN x the error the SAME formula shows when torch evaluates it in float32 on the CPU
(losses_ref.row_terms_f32: what the reference itself would compute) against float64 on the same inputs, with a floor of 8 float32 ulp of the term
(the kernel's differences are float32 operations like torch's; only its squares and sums are float64, so it cannot be expected to beat float32
round-off of the differences, and where torch's own error happens to cancel the floor keeps the gate meaningful).  The exact properties — the
bits of x0_pred, run-to-run, row independence, padded frames, counts, optional outputs — are compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import losses_ref as LR  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.diffusion import denoise_losses, diffusion_table  # noqa: E402

DEV = "cuda:0"
MARGIN = 4.0
ULP_FLOOR = 8
BETA = LR.HUBER_BETA
T_LEVELS = (0, 500, 999)

#        B  T   C    split  lens
CASES = [(1, 1, 232, 129, None),
         (2, 2, 192, 141, None),
         (3, 11, 232, 129, None),
         (5, 34, 192, 141, None),
         (2, 88, 232, 129, None),
         (3, 7, 5, 2, None),
         (3, 11, 232, 129, (1, 5, 11))]
IDS = ["1x1x232", "2x2x192", "3x11x232", "5x34x192", "2x88x232", "3x7x5", "ragged_1_5_11"]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _tables():
    ac = diffusion_table(1000, 0, "alphas_cumprod")
    return (np.sqrt(ac).astype(np.float32), np.sqrt(1.0 - ac).astype(np.float32),
            diffusion_table(1000, 0, "sqrt_recip_alphas_cumprod").astype(np.float32),
            diffusion_table(1000, 0, "sqrt_recipm1_alphas_cumprod").astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs (CPU fp32) and both references of case i, computed once and shared by the tests."""
    B, T, Cc, split, lens = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    x0, noise = torch.randn(B, T, Cc, generator=g), torch.randn(B, T, Cc, generator=g)
    eps = noise + 0.7 * torch.randn(B, T, Cc, generator=g)                   # a model that is roughly right
    sa, s1, r, rm1 = _tables()
    ts = [T_LEVELS[b % 3] for b in range(B)]
    a, s = torch.from_numpy(sa[ts]), torch.from_numpy(s1[ts])
    x_t = a.view(B, 1, 1) * x0 + s.view(B, 1, 1) * noise
    c1, c2 = torch.from_numpy(r[ts]), torch.from_numpy(rm1[ts])
    t = {"eps": eps, "noise": noise, "x_t": x_t, "x0": x0, "c1": c1, "c2": c2}
    t["f64"] = LR.row_terms_f64(eps, noise, x_t, x0, c1, c2, split, BETA, lens)
    t["f32"] = LR.row_terms_f32(eps, noise, x_t, x0, c1, c2, split, BETA, lens)
    t["frame_mse"] = LR.frame_mse_f64(eps, noise, lens)
    return t


def run(t, split, lens=None, rows=None, x0_pred=True, frame_mse=True, poison=False):
    """The op on (the rows `rows` of) the tensors of a case; poison: frames behind a row's length hold NaN in all four tensors."""
    sel = (lambda v: v) if rows is None else (lambda v: v[list(rows)])
    d = {k: sel(t[k]).contiguous().clone() for k in ("eps", "noise", "x_t", "x0", "c1", "c2")}
    lens = None if lens is None else [lens[b] for b in (rows if rows is not None else range(len(lens)))]
    if poison:
        for k in ("eps", "noise", "x_t", "x0"):
            for b, n in enumerate(lens):
                d[k][b, n:] = float("nan")
    d = {k: v.to(DEV) for k, v in d.items()}
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(DEV)
    r = denoise_losses(d["eps"], d["noise"], d["x_t"], d["x0"], d["c1"], d["c2"], split, ld, BETA, x0_pred, frame_mse)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in r.items()}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_row_terms_and_scalars_match_the_float64_reference(i):
    B, T, Cc, split, lens = CASES[i]
    t = case(i)
    r = run(t, split, lens)
    rows = r["row_terms"].numpy()
    assert np.array_equal(rows[:, 5:], t["f64"][:, 5:])                         # element and pair counts: exact
    worst = 0.0
    for j, name in enumerate(("eps gesture", "eps expression", "x0", "velocity", "huber")):
        want, f32 = t["f64"][:, j], t["f32"][:, j]
        err, err32 = np.abs(rows[:, j] - want), np.abs(f32 - want)
        gate = np.maximum(MARGIN * err32, ULP_FLOOR * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
        ratio = float((err / np.maximum(err32, np.finfo(np.float64).tiny)).max()) if err32.max() > 0 else 0.0
        worst = max(worst, float((err / np.maximum(gate, np.finfo(np.float64).tiny)).max()) if want.any() else 0.0)
        print(f"[losses op {IDS[i]}] {name}: |gpu - f64| max {err.max():.3e} (rel {float((err / np.maximum(np.abs(want), 1e-300)).max()):.2e}), "
              f"|torch fp32 - f64| max {err32.max():.3e}, ratio {ratio:.3f}")
        assert (err <= gate).all(), (name, err, gate)
    print(f"[losses op {IDS[i]}] worst error / gate = {worst:.3f}")
    # the batch scalars are the reference's formulas on the row terms the kernel itself produced: float64 round-off only
    sc = r["scalars"].numpy()
    want = LR.scalars_f64(rows, Cc, BETA)
    pairs = rows[:, 6].sum()
    assert np.array_equal(r["counts"].numpy(), [rows[:, 5].sum() / Cc, pairs, rows[:, 5].sum()])
    for k, name in enumerate(LR.SCALARS):
        if pairs == 0 and name in ("loss_vel_rec", "final_loss"):
            continue
        assert abs(sc[k] - want[name]) <= 1e-13 * abs(want[name]), (name, sc[k], want[name])
    if pairs == 0:                                                              # no pair: 0, not NaN (the Python callers refuse such a batch)
        assert sc[1] == 0.0 and sc[3] == sc[0] + sc[2]
    fm = r["frame_mse"].double().numpy()
    assert np.abs(fm - t["frame_mse"]).max() <= 2.0 ** -23 * np.abs(t["frame_mse"]).max()     # one float32 rounding of a float64 mean
    if lens is not None:
        for b, n in enumerate(lens):
            assert not fm[b, n:].any() and not r["pred_x0"][b, n:].any()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_x0_pred_has_the_bits_of_the_ddim_step(i):
    B, T, Cc, split, lens = CASES[i]
    t = case(i)
    got = run(t, split, lens)["pred_x0"]
    lib = _lib.lib()
    for b in range(B):
        n = T if lens is None else lens[b]
        x = t["x_t"][b:b + 1, :n].contiguous().to(DEV)
        e = t["eps"][b:b + 1, :n].contiguous().to(DEV)
        x0_out = torch.empty_like(x)
        _lib.check(lib.dsh_op_ddim_step_full(None, _p(x), _p(e), _p(x0_out), None, None, None, None, None, None, 1, n, Cc, float(t["c1"][b]),
                                             float(t["c2"][b]), 1.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0), "dsh_op_ddim_step_full")
        torch.cuda.synchronize()
        assert torch.equal(got[b:b + 1, :n], x0_out.cpu()), (b, int((got[b:b + 1, :n] != x0_out.cpu()).sum()))


@pytest.mark.parametrize("i", [2, 3, 4, 5, 6], ids=[IDS[k] for k in (2, 3, 4, 5, 6)])
def test_bits_do_not_depend_on_run_batch_position_padding_or_outputs(i):
    B, T, Cc, split, lens = CASES[i]
    t = case(i)
    r1, r2 = run(t, split, lens), run(t, split, lens)
    for k in ("scalars", "row_terms", "pred_x0", "frame_mse"):
        assert torch.equal(r1[k], r2[k]), k                                     # two runs
    # a row alone, and at another position of another batch (an odd C moves its byte offset to another alignment mod 16)
    for b in range(B):
        alone = run(t, split, lens, rows=[b])
        assert torch.equal(alone["row_terms"][0], r1["row_terms"][b]), b
        assert torch.equal(alone["pred_x0"][0], r1["pred_x0"][b]) and torch.equal(alone["frame_mse"][0], r1["frame_mse"][b])
    order = list(range(B))[::-1] + [0]
    moved = run(t, split, lens, rows=order)
    for pos, b in enumerate(order):
        assert torch.equal(moved["row_terms"][pos], r1["row_terms"][b]), (pos, b)
    # optional outputs off: the rest is unchanged
    bare = run(t, split, lens, x0_pred=False, frame_mse=False)
    assert bare["pred_x0"] is None and bare["frame_mse"] is None
    assert torch.equal(bare["row_terms"], r1["row_terms"]) and torch.equal(bare["scalars"], r1["scalars"])
    if lens is not None:
        # padded frames poisoned with NaN change nothing; a ragged row has the bits of the row alone at its own length
        p = run(t, split, lens, poison=True)
        for k in ("scalars", "row_terms", "pred_x0", "frame_mse"):
            assert torch.equal(p[k], r1[k]), k
        for b, n in enumerate(lens):
            cut = {k: (v[b:b + 1, :n] if v.dim() == 3 else v[b:b + 1]) for k, v in t.items() if k in ("eps", "noise", "x_t", "x0", "c1", "c2")}
            assert torch.equal(run(cut, split)["row_terms"][0], r1["row_terms"][b]), b


def test_tensors_at_any_4_byte_offset():
    """Base pointers that are 4-byte but not 16-byte aligned, each tensor at another offset: the vector copy starts each tile at its own
    first 16-byte boundary; the LDS image, and with it every bit of the result, is the same."""
    i = 4
    B, T, Cc, split, _ = CASES[i]
    t = case(i)
    want = run(t, split)
    n = B * T * Cc
    bufs, ptrs = [], []
    for off, k in enumerate(("eps", "noise", "x_t", "x0")):                     # offsets of 0, 1, 2, 3 floats
        buf = torch.zeros(n + 4, device=DEV)
        buf[off:off + n] = t[k].reshape(-1).to(DEV)
        bufs.append(buf)
        ptrs.append(C.c_void_p(buf.data_ptr() + 4 * off))
    c1, c2 = t["c1"].to(DEV), t["c2"].to(DEV)
    L = _lib.lib()
    res = torch.empty(int(L.dsh_denoise_losses_result_bytes(B, T)) // 8, dtype=torch.float64, device=DEV)
    x0p = torch.zeros(n + 4, device=DEV)
    _lib.check(L.dsh_op_denoise_losses(None, *ptrs, _p(c1), _p(c2), None, B, T, Cc, split, BETA, C.c_void_p(x0p.data_ptr() + 4), None, _p(res)),
               "dsh_op_denoise_losses")
    torch.cuda.synchronize()
    H, K = _lib.LOSS_HEADER, _lib.LOSS_COLS
    assert torch.equal(res[H:H + B * K].view(B, K).cpu(), want["row_terms"]) and torch.equal(res[:4].cpu(), want["scalars"])
    assert torch.equal(x0p[1:1 + n].view(B, T, Cc).cpu(), want["pred_x0"]) and float(x0p[0]) == 0.0 and not x0p[1 + n:].any()


def test_refused_arguments():
    L = _lib.lib()
    x = torch.zeros(2, 4, 8, device=DEV)
    c = torch.ones(2, device=DEV)
    res = torch.empty(int(L.dsh_denoise_losses_result_bytes(2, 4)) // 8, dtype=torch.float64, device=DEV)

    def call(eps=x, B=2, T=4, Cc=8, split=3, beta=0.1, result=res, x0p=None):
        return L.dsh_op_denoise_losses(None, _p(eps), _p(x), _p(x), _p(x), _p(c), _p(c), None, B, T, Cc, split, beta, x0p, None,
                                       result if isinstance(result, C.c_void_p) else _p(result))
    assert call() == 0
    for kw, word in ((dict(eps=None), b"null"), (dict(result=None), b"null"), (dict(B=0), b"positive"), (dict(T=-1), b"positive"),
                     (dict(split=0), b"split"), (dict(split=8), b"split"), (dict(beta=0.0), b"huber_beta"), (dict(Cc=449, split=3), b"448"),
                     (dict(x0p=C.c_void_p(x.data_ptr() + 2)), b"aligned"), (dict(result=C.c_void_p(res.data_ptr() + 4)), b"aligned")):
        assert call(**kw) == -1 and word in L.dsh_last_error(), kw
    torch.cuda.synchronize()
    with pytest.raises(_lib.DshError):
        denoise_losses(x.cpu(), x.cpu(), x.cpu(), x.cpu(), c.cpu(), c.cpu(), 3)
