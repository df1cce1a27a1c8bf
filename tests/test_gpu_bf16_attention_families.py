"""Every bf16 attention kernel of attention.hip, and the fp32 instantiations of its VALU templates, against the gates of bf16_gates.py on
hostile input families (bf16_gates.ATTN_FAMILIES: an outlier V column, V x 1e-3, a saturated time-softmax, a saturated channel softmax, K
equal on all frames) at the smallest shapes at which each form changes behaviour (bf16_gates.ATTN_FORMS):

  tiled MFMA       dsh_op_linear_attention_ragged(dtype 1, variant 0), D 512, hd 64, T 11 / 33 / 88 / 96   k^, A, q^ rounded to bf16
  row-major MFMA   (1, 1), the same shapes                                                                the same rounding points
  pre-loaded VALU  (1, 1) and (0, 0), D 128, hd 16, T 11 / 34 / 96                                        fp32 up to the store
  loop VALU        (1, 1) and (0, 0), hd 16 and hd 64, T 97 / 120                                         fp32 up to the store

Reference: bf16_gates.attn_chain in float64 with the form's rounding points.  Gate, every element of every valid row: half a bf16 ulp of
the store (bf16 storage) + MARGIN x max |fp32 chain - fp64 chain| on the same operands (attn_gate); nothing is a fraction of the output
range and nothing comes from a kernel output.  The MFMA forms add attn_flip_slack, a term computed from the fp64 operands and the documented
accuracy of v_exp_f32 and of the fp32 sums: an exact k^, q^ or A that lies within that error of a bf16 rounding tie may round to its other
neighbour in the kernel, which moves the outputs it feeds by one ulp of the operand times their weight (zero for every other output).  On
an MI355X the two MFMA kernels rounded such operands differently from the fp64 chain - and from each other - in 9 of the 48 dense cases
(figures in the docstring of bf16_gates.py).  Each form runs dense (3 clips), ragged (lengths attn_lens(T), plain and CFG-doubled, K and
V rows behind each length filled with NaN and +-inf) and with every length equal to T, which must be the no-lengths launch bit for bit.
The tiled kernel's `rev` argument (clips walked in descending order) is reached through dsh_op_linear_attention_tiled and must not change
a bit; that entry also lays a dense batch out as the two CFG halves (2 + 1 clips) with the block-aligned gap between them.

Not reached: the fp32 hd 64 pre-loaded instantiations (TM = 48 / 96).  fp32 at hd 64 and <= 96 frames takes the MFMA kernel unless
DSH_ATTN_F32_MFMA=0, and switches.h latches that switch at the first read in the process.

Every test prints a [bf16 gate] line: the worst element over its allowance."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_gates as G  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402

DEV = "cuda:0"
ROWS = [pytest.param(*r, id=f"{r[0]}-D{r[1]}-hd{r[2]}-T{r[3]}") for r in G.ATTN_ROWS]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _launch(form, qkv, hd, lens=None):
    """dsh_op_linear_attention_ragged on qkv [nb, T, 3 D] (CPU, bf16 values) in the form's storage type; the output on the CPU"""
    dtype, variant = G.ATTN_FORMS[form][:2]
    st = torch.bfloat16 if dtype else torch.float32
    nb, T, D3 = qkv.shape
    qd = qkv.to(st).to(DEV).contiguous()
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = torch.full((nb, T, D3 // 3), float("nan"), device=DEV, dtype=st)
    _lib.check(_lib.lib().dsh_op_linear_attention_ragged(None, dtype, variant, _p(qd), nb, T, D3 // 3, hd, _p(out), _p(ld), 0 if lens is None else len(lens), None))
    torch.cuda.synchronize()
    return out.cpu()


def _poison(qkv, lens):
    """K and V rows behind each clip's length: NaN and +-inf, alternating with the clip (as test_attention_kernels_exclude_padded_frames)"""
    D = qkv.shape[2] // 3
    bad = qkv.clone()
    for b in range(qkv.shape[0]):
        n = lens[b % len(lens)]
        bad[b, n:, D:2 * D] = float("nan") if b % 2 else float("inf")
        bad[b, n:, 2 * D:] = float("-inf") if b % 2 else float("nan")
    return bad


def _gate_and_report(out, qkv, form, family, hd, lens, mode):
    nb, T, D3 = qkv.shape
    ref, cal, flips = G.attn_gate(qkv, hd, G.ATTN_FORMS[form][2], lens)
    what = f"attention {form} {family} D {D3 // 3} hd {hd} T {T} nb {nb} {mode}"
    unit = "0.5 ulp + " if out.dtype == torch.bfloat16 else ""
    tail = f" + flips); without the flip allowance {G.attn_ratio(out, ref, cal, T, lens):.3f}" if torch.is_tensor(flips) else ")"
    print(f"[bf16 gate] {what}: worst |out - ref| / ({unit}{G.MARGIN:g} x calibration {cal:.3e}{tail} = {G.attn_ratio(out, ref, cal, T, lens, flips):.3f}")
    G.attn_check(out, ref, cal, T, lens, what, extra=flips)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("form,D,hd,T", ROWS)
def test_dense(form, D, hd, T, family):
    qkv = G.attn_inputs(G.ATTN_NB, T, family, D, hd)
    _gate_and_report(_launch(form, qkv, hd), qkv, form, family, hd, None, "dense")


@pytest.mark.parametrize("doubled", [False, True])
@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("form,D,hd,T", ROWS)
def test_ragged(form, D, hd, T, family, doubled):
    """Valid rows against the chain evaluated on each clip's own frames, at the tight gate; padded query rows finite."""
    lens = G.attn_lens(T)
    qkv = G.attn_inputs(len(lens) * (2 if doubled else 1), T, family, D, hd)
    out = _launch(form, _poison(qkv, lens), hd, lens)
    assert torch.isfinite(out).all(), "a padded K / V value reached an output"
    _gate_and_report(out, qkv, form, family, hd, lens, "ragged, CFG-doubled" if doubled else "ragged")


@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("form,D,hd,T", ROWS)
def test_every_length_equal_to_T_is_the_plain_launch(form, D, hd, T, family):
    qkv = G.attn_inputs(G.ATTN_NB, T, family, D, hd)
    plain, full = _launch(form, qkv, hd), _launch(form, qkv, hd, [T] * G.ATTN_NB)
    assert torch.isfinite(plain).all()
    assert _same_bits(plain, full), float((plain.float() - full.float()).abs().max())


# ---- the tiled kernel's rev argument and its two-halves layout ---------------------------------------------------------------------------
def _tiled(qkv, n_half, lens, rev):
    nb, T, D3 = qkv.shape
    qd = qkv.to(DEV).contiguous()
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = torch.full((nb, T, D3 // 3), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.lib().dsh_op_linear_attention_tiled(None, _p(qd), nb, n_half, T, D3 // 3, _p(out), _p(ld), 0 if lens is None else len(lens), rev))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("nb", [3, 6])
@pytest.mark.parametrize("T", [34, 88])
def test_tiled_rev_changes_no_bit(T, nb, family, ragged):
    """rev = 1 against rev = 0, bit for bit, and rev = 0 at the tight gate: 3 clips (dense: halves of 2 and 1) and 6 (two halves of 3 that
    share the lengths one frame, T - 1 and a block edge)."""
    lens = [1, T - 1, 24] if ragged else None
    qkv = G.attn_inputs(nb, T, family)
    n_half = 3 if (ragged or nb == 6) else 2
    src = _poison(qkv, lens) if ragged else qkv
    fwd, bwd = _tiled(src, n_half, lens, 0), _tiled(src, n_half, lens, 1)
    assert torch.isfinite(fwd).all() and torch.isfinite(bwd).all()
    assert _same_bits(fwd, bwd), float((fwd.float() - bwd.float()).abs().max())
    _gate_and_report(fwd, qkv, "tiled", family, 64, lens, f"halves {n_half} + {nb - n_half}, {'ragged' if ragged else 'dense'}")


def test_tiled_entry_refuses_what_the_kernel_cannot_index():
    q = torch.zeros(3, 8, 3 * 64, device=DEV, dtype=torch.bfloat16)
    y = torch.zeros(3, 8, 64, device=DEV, dtype=torch.bfloat16)
    ld = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    L = _lib.lib()
    assert L.dsh_op_linear_attention_tiled(None, _p(q), 3, 4, 8, 64, _p(y), None, 0, 0) != 0          # more clips in the first half than in the batch
    assert L.dsh_op_linear_attention_tiled(None, _p(q), 3, 2, 8, 64, _p(y), _p(ld), 2, 0) != 0        # lengths: nb is neither n_lens nor twice that
    assert L.dsh_op_linear_attention_tiled(None, _p(q), 3, 2, 97, 64, _p(y), None, 0, 0) != 0         # more than 96 frames
    assert L.dsh_op_linear_attention_tiled(None, _p(q), 3, 2, 8, 64, _p(y), None, 0, 2) != 0          # rev is 0 or 1
