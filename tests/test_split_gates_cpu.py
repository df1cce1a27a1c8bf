"""Precision "bf16x3" without a GPU: the new precision value is known to the Python layer and the C header, the torch emulation of the
split-bf16 loop (split_gates.emul) passes the gate derived from its arithmetic on every input family, and three subtly wrong loops are
rejected - each by the gate the arithmetic says can see it (split_gates.py, module docstring):

  dropped a_lo w_hi   breaks the 2^-16 order (the term is 2^-8 |a w|): the DERIVED gate rejects it on every family.
  truncated lo        stays inside the order (a remainder of 2 x 2^-16 in place of 2^-16, random in sign: a factor ~sqrt(K) inside the worst
                      case of three aligned remainders), so the derived gate accepts it everywhere - as it must: the arithmetic calls it
                      harmless at that gate.  The PINNING gate (distance from the emulation, fp32 allowance alone) rejects it wherever the
                      fp32 chain is itself more exact than 2^-16 of the products.  It is not where the fp32 chain's own distance from fp64
                      is larger than the mutant's: the whole-row offsets of PRO 1 / PRO 2 (the fold's x W' - mean c cancellation, the
                      moments of offset rows) and PRO 0 on the low-variance rows (an O(1) bias and residual: the fp32 store is the error).
  unshifted PRO 1     rows at offset -200: 2.1e-3 from fp64 against 2.1e-5 shifted.  The pinning gate rejects it at K = 512 and 960; the
                      derived gate at K = 512 (allowance 2.0e-3: 3 x 3.9e-4 for the fp32 fold's own cancellation at this offset + the
                      worst-case split term 8.4e-4).  At K = 960 the derived allowance is 2.6e-3 (3 x 4.7e-4 + 1.2e-3) and the mutant
                      passes it: the figures are printed, the pinning gate is the one that holds there.
"""
import os
import re

import pytest
import torch

import f32_gates as G
import split_gates as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(pro, fam, K) for pro in (0, 1, 2) for K in (512, 960) for fam in S.FAMILIES]
_cache = {}


def _case(pro, fam, K):
    if (pro, fam, K) not in _cache:
        _cache[(pro, fam, K)] = S.family_case(pro, fam, K)
    return _cache[(pro, fam, K)]


# ---- 1. the precision is known ------------------------------------------------------------------------------------------------------------
def test_precision_value_is_known_to_python_and_the_header():
    from diffsheg_amd import _lib, model
    assert model._PRECISION["bf16x3"] == 2
    hdr = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    assert re.search(r"_PRECISION_BF16X3\s*=\s*2\b", hdr)
    assert int(re.search(r"#define DSH_LAUNCH_COUNT_ENTRIES (\d+)", hdr).group(1)) == 22
    assert len(_lib.LAUNCH_FAMILIES) == 22 and _lib.LAUNCH_FAMILIES[20] == "gemm_f32_split" and _lib.LAUNCH_FAMILIES[21] == "gemm_f32_split_128" and _lib.LAUNCH_FAMILIES[12] == "gemm_f32_pro"
    assert "dsh_op_gemm_f32_pro_ex" in hdr


def test_model_rejects_an_unknown_precision_by_name():
    from diffsheg_amd import model
    assert sorted(set(model._PRECISION.values())) == [0, 1, 2]
    assert "bf16x2" not in model._PRECISION


# ---- 2. the emulation passes the derived gate ------------------------------------------------------------------------------------------------
def test_split_pieces_are_rne_and_the_remainder_is_2_to_the_minus_16():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(5)) * 37.0
    hi, lo = S.split(x)
    assert torch.equal(hi, x.bfloat16().float()) and torch.equal(lo, (x - hi).bfloat16().float())
    assert float(((x - hi).abs() / x.abs()).max()) <= 2.0 ** -8
    assert float(((x.double() - hi.double() - lo.double()).abs() / x.double().abs()).max()) <= 2.0 ** -16
    ints = torch.arange(-128, 129).float()
    assert torch.equal(S.split(ints)[1], torch.zeros_like(ints))                # up to 8 significant bits: no lo piece


@pytest.mark.parametrize("pro,fam,K", CASES)
def test_emulation_passes_the_derived_gate(pro, fam, K):
    t = _case(pro, fam, K)
    out = S.emul(t).float()
    r = S.check(t, out)
    err, _, cal, sp = S.figures(t, out)
    print(f"[{t['name']}] |emul - fp64| {err:.2e} = {r:.3f} of the gate (fp32 calibration {cal:.2e}, largest split term {sp:.2e})")
    assert r <= 1.0
    assert S.check_emul(t, out) <= 1.0                                          # (its own fp32 rounding: far inside the fp32 allowance)
    # the split term is the issue's expression: 3 x 2^-16 x (rstd) sum |a| |W| (x the Lipschitz constant of the activation)
    if pro == 0:
        want = 3 * 2.0 ** -16 * (t["X"].double().abs() @ t["W"].double().abs().T)
        assert torch.allclose(S.split_term(t), want, rtol=1e-12, atol=0)


def test_shift_buys_two_orders_of_magnitude_at_offset_minus_200():
    t = _case(1, "off-200", 512)
    ref = G.ref64(t)
    shifted = float((S.emul(t) - ref).abs().max())
    unshifted = float((S.emul(t, shifted=False) - ref).abs().max())
    fp32 = float((G.chain(t).double() - ref).abs().max())
    print(f"[off-200 K=512] shifted {shifted:.2e}, unshifted {unshifted:.2e}, fp32 loop {fp32:.2e}")
    assert shifted < 1e-4 and unshifted > 20 * shifted and shifted < fp32


# ---- 3. mutants -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pro,fam,K", CASES)
def test_dropped_term_is_rejected_by_the_derived_gate(pro, fam, K):
    t = _case(pro, fam, K)
    out = S.emul(t, drop_alo=True).float()
    assert S.rejected(S.check, t, out), f"a loop without a_lo w_hi passes the derived gate of {t['name']}"
    assert S.rejected(S.check_emul, t, out)


# where the fp32 chain's own distance from fp64 is above the truncation's (module docstring): the pinning gate cannot see it there
TRUNC_HIDDEN = {(0, "lowvar"), (1, "off+50"), (1, "off-200"), (2, "off+50"), (2, "off-200")}


@pytest.mark.parametrize("pro,fam,K", CASES)
def test_truncated_lo_is_rejected_where_fp32_is_finer_than_the_split(pro, fam, K):
    t = _case(pro, fam, K)
    out = S.emul(t, trunc_lo=True).float()
    # inside the worst case of three aligned 2^-16 remainders: harmless at the derived gate, on every family
    assert S.check(t, out) <= 1.0
    ref, _, cal = G.gate(t)
    dist = float((out.double() - S.emul(t))[:t["M"]].abs().max())
    print(f"[{t['name']}] truncated lo: {dist:.2e} from the emulation, fp32 calibration {cal:.2e}")
    if (pro, fam) in TRUNC_HIDDEN:
        assert dist <= G.MARGIN * cal, "the fp32 chain is coarser than the mutant here: that is why the pinning gate accepts it"
    else:
        assert S.rejected(S.check_emul, t, out), f"a loop with truncated lo pieces passes the pinning gate of {t['name']}"


# ---- 3b. the model's own Linear forms, K = 2 048 and 3 072 included (split_gates.MODEL_LINEARS) ------------------------------------------------
# (the FiLM table's 16 384 columns are left to the GPU test: the same K = 2 048 as aud_film here, and its column-sampled calibration is
# checked below on a narrower twin)
LARGE_K = ("conv1", "aud_time_embed.2", "pid_embed.2", "aud_film")
CPU_MODEL = [n for n in S.MODEL_LINEARS if n != "film"]


@pytest.mark.parametrize("name", CPU_MODEL)
def test_model_linear_forms_emulation_inside_both_gates_and_dropped_term_rejected(name):
    """M = 513: the emulation of every form the model launches sits inside the derived and the pinning gate, and a loop without a_lo w_hi is
    rejected by both - at K = 2 048 and 3 072 as at the grid's K (the dropped term is 2^-8 of the products against an allowance of 3 x 2^-16
    of their absolute sum: both grow alike with K)."""
    t = S.model_case(name, 513)
    out = S.emul(t).float()
    r, re_ = S.check(t, out), S.check_emul(t, out)
    err, _, cal, sp = S.figures(t, out)
    mut = S.emul(t, drop_alo=True).float()
    merr = float((mut.double() - G.gate(t)[0])[:t["M"]].abs().max())
    print(f"[{t['name']} K={t['K']}] |emul - fp64| {err:.2e} = {r:.3f} of the derived gate, {re_:.3f} of the pinning gate (fp32 calibration {cal:.2e}, largest split term "
          f"{sp:.2e}); dropped a_lo w_hi: {merr:.2e} from fp64")
    assert r <= 1.0 and re_ <= 1.0
    assert S.rejected(S.check, t, mut), f"a loop without a_lo w_hi passes the derived gate of {t['name']}"
    assert S.rejected(S.check_emul, t, mut), f"a loop without a_lo w_hi passes the pinning gate of {t['name']}"


def test_large_k_rows_are_in_the_table():
    ks = {n: S.model_case(n, 513)["K"] for n in LARGE_K}
    assert ks == {"conv1": 3072, "aud_time_embed.2": 2048, "pid_embed.2": 2048, "aud_film": 2048}
    film = S.model_case("film", 513)
    assert (film["N"], film["K"]) == (16384, 2048) and len(film["cal_cols"]) == 1024


def test_column_sampled_calibration_never_widens_the_gate():
    """f32_gates.gate with cal_cols (used for the FiLM table's N): the allowance over a sample of the columns is at most the allowance over all."""
    whole = G.pro0_inputs(513, 2048, 512, act=1, res=False)
    part = dict(G.pro0_inputs(513, 2048, 512, act=1, res=False), cal_cols=torch.arange(0, 2048, 4))
    (_, a, ca), (_, b, cb) = G.gate(whole), G.gate(part)
    print(f"[cal_cols] calibration over all 2 048 columns {ca:.3e}, over every fourth {cb:.3e}")
    assert cb <= ca and float(b.max()) <= float(a.max()) and cb > 0.5 * ca
    out = S.emul(part).float()
    assert S.check(part, out) <= 1.0 and S.check_emul(part, out) <= 1.0


@pytest.mark.parametrize("K", [512, 960])
def test_unshifted_pro1_is_rejected_at_offset_minus_200(K):
    t = _case(1, "off-200", K)
    out = S.emul(t, shifted=False).float()
    ref, allow, cal = G.gate(t)
    err = float((out.double() - ref).abs().max())
    print(f"[{t['name']}] unshifted: {err:.2e} from fp64; fp32 allowance {float(allow.max()):.2e}, largest split term {float(S.split_term(t).max()):.2e}")
    assert S.rejected(S.check_emul, t, out), "an unshifted PRO 1 passes the pinning gate on rows at offset -200"
    if K == 512:
        assert S.rejected(S.check, t, out), "an unshifted PRO 1 passes the derived gate on rows at offset -200"


@pytest.mark.parametrize("fam", ["plain", "lowvar", "out300", "out-1e4"])
def test_unshifted_pro1_is_harmless_without_a_row_offset(fam):
    """Rows whose mean is of the size of their spread: the shift moves every element by less than the spread, the split error is unchanged
    in order, and the derived gate accepts the unshifted loop - the arithmetic says it is harmless there."""
    t = _case(1, fam, 512)
    assert S.check(t, S.emul(t, shifted=False).float()) <= 1.0
