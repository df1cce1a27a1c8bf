"""The gates of bf16_gates.py, tested without a GPU on the operands of the op tests at their smallest shapes:
(a) a faithful emulation of each kernel (the fp32 chain with the documented rounding points, K accumulated in natural and in reversed
    order, round-to-nearest bf16 store) passes the new gate;
(b) eight subtly wrong kernels (mutants of the fp64 reference) are all rejected by it;
(c) the gate each op test had before is evaluated on the same mutants, and its verdict is pinned in OLD_GATE_ACCEPTS below.

Verdicts of the previous gates on these operands (300 rows, T = 64, 3 clips), maximum error of the mutant beside the gate it met:
  1. one k-term dropped in every row          1024 -> 512: rejected (0.41 > 0.17)   pro 2: rejected (0.36 > 0.16)
                                              FFN Linear3: rejected (max 0.30 > 0.20, rms 0.023 > 0.020) - the worst of 150 k elements
                                              meets a large |x_k w_k|; the typical element is off by 0.04 and would pass
  2. two 16-wide K fragments of one tile swapped              rejected              FFN Linear3: rejected
  3. neighbouring clip's FiLM row on the last frame of a clip pro 2: rejected       FFN: rejected
  4. bf16 store truncated instead of rounded                  ACCEPTED
  5. bias left out of one 32-column tile                      rejected              FFN: rejected
  6. lo plane of the hi / lo residual dropped (fp32 output)   rejected (the fp32 gate of pro 0 was 1e-3 of range)
  7. LayerNorm divisor 1024 instead of 999 (pro 3)            ACCEPTED
  8. time-softmax over T - 1 frames                           rejected;  over one padded frame of a ragged clip: rejected
     (logits of std 2: the time-softmax is peaked, one frame more or less moves y by O(1))
The new gates reject all of them: half an ulp of the store plus 4e-3 (accumulation bound, K = 1024), 3 x the calibration + 2.7e-3 for one operand flip
(LN + FiLM + SiLU prologue: the CPU chain itself has no flip in these 300 rows) or 3 x the calibrated 5.6e-3 (FFN), in place of 0.16 .. 0.20.
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_gates as G

OLD_GATE_ACCEPTS = {
    "tl0/kterm": False, "tl0/fragswap": False, "tl0/truncate": True, "tl0/bias_tile": False,
    "tl2/kterm": False, "tl2/film_neighbour": False, "tl0res/lo_dropped": False, "tl3/ln_divisor": True,
    "ffn/kterm": False, "ffn/fragswap": False, "ffn/film_neighbour": False, "ffn/bias_tile": False,
    "attn/t_minus_1": False, "attn/padded_frame": False,
}

MV, T, NB = 300, 64, 3


def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _record(name, old_accepts):
    assert old_accepts == OLD_GATE_ACCEPTS[name], f"{name}: the previous gate {'accepts' if old_accepts else 'rejects'} this mutant; update the table"


def _drop_last_k(W):
    W = W.clone(); W[:, -1] = 0
    return W


def _swap_fragments(W, tile=2):
    """K fragments 3 and 4 (16 features each) exchanged in the 32 output features of one tile."""
    W = W.clone()
    r = slice(32 * tile, 32 * tile + 32)
    a, b = W[r, 48:64].clone(), W[r, 64:80].clone()
    W[r, 48:64], W[r, 64:80] = b, a
    return W


def _neighbour_rows(Mv, frames, nb):
    rows = torch.arange(Mv)
    clip = (rows // frames) % nb
    return torch.where(rows % frames == frames - 1, (clip + 1) % nb, clip)


# ---- token-per-lane Linear, pro 0 (1024 -> 512, bf16 out) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tl0():
    t = G.tl_inputs(1024, 512, 0, False, MV, T, NB)
    ref = G.tl_chain(t, MV, T, NB, 0, 0, torch.float64)
    slack = G.accum_bound(t["X"][:MV], t["W"], 1024)
    return t, ref, slack


def _old_tl_ct(out, ref):
    return float((out.double() - ref).abs().max()) < 2e-2 * max(1.0, float(ref.abs().max()))


def _old_tl_cf(out, ref, pro):
    return float((out.double() - ref).abs().max()) < 2e-2 * max(1.0, float(ref.abs().max())) * (1 if pro else 1e-3 / 2e-2) + 1e-4


@pytest.mark.parametrize("reverse", [False, True])
def test_tl_linear_emulation_passes(tl0, reverse):
    t, ref, slack = tl0
    out = G.tl_chain(t, MV, T, NB, 0, 0, torch.float32, reverse=reverse).bfloat16()
    assert G.assert_rounded(out, ref, slack) <= 1.0


@pytest.mark.parametrize("mutant", ["kterm", "fragswap", "truncate", "bias_tile"])
def test_tl_linear_mutants_are_rejected(tl0, mutant):
    t, ref, slack = tl0
    m = dict(t)
    if mutant == "kterm":
        m["W"] = _drop_last_k(t["W"])
    elif mutant == "fragswap":
        m["W"] = _swap_fragments(t["W"])
    elif mutant == "bias_tile":
        m["b"] = t["b"].clone(); m["b"][64:96] = 0
    y = G.tl_chain(m, MV, T, NB, 0, 0, torch.float64)
    out = G.truncate_bf16(y) if mutant == "truncate" else y.bfloat16()
    assert _rejected(G.assert_rounded, out, ref, slack, frames=T, nb=NB)
    _record("tl0/" + mutant, _old_tl_ct(out, ref))


def test_worst_element_report_names_tile_clip_and_frame(tl0):
    t, ref, slack = tl0
    out = ref.bfloat16().clone()
    out[133, 70] += 1.0
    with pytest.raises(AssertionError, match=r"row 133 col 70 \(row % 32 = 5, col % 32 = 6, clip 2, frame 5\)"):
        G.assert_rounded(out, ref, slack, frames=T, nb=NB)
    out[133, 70] = float("nan")
    with pytest.raises(AssertionError, match="row 133 col 70"):
        G.assert_rounded(out, ref, slack, frames=T, nb=NB)


# ---- hi / lo residual (1024 -> 512 + R, fp32 out) -------------------------------------------------------------------------------------------
def test_dropped_lo_plane_is_rejected_and_exact_planes_pass():
    t = G.tl_inputs(1024, 512, 0, True, MV, T, NB)
    ref = G.tl_chain(t, MV, T, NB, 0, 0, torch.float64)
    slack = G.accum_bound(t["X"][:MV], t["W"], 1024) + G.hilo_slack(t["R"][:MV], ref)
    # faithful: R split into planes (2^-17 relative), the fp32 result split again
    R = t["R"][:MV]
    hi = R.bfloat16().float(); lo = (R - hi).bfloat16().float()
    for reverse in (False, True):
        y = G.tl_chain(dict(t, R=None), MV, T, NB, 0, 0, torch.float32, reverse=reverse) + hi + lo
        yh = y.bfloat16().float(); yl = (y - yh).bfloat16().float()
        assert G.assert_close_f32(yh + yl, ref, slack) <= 1.0
        assert G.assert_rounded(yh.bfloat16(), ref, slack) <= 1.0
    mut = G.tl_chain(dict(t, R=None), MV, T, NB, 0, 0, torch.float64) + hi.double()
    assert _rejected(G.assert_close_f32, mut.float(), ref, slack, frames=T, nb=NB)
    _record("tl0res/lo_dropped", _old_tl_cf(mut.float(), ref, 0))


# ---- LN + FiLM + SiLU prologue (pro 2, 512 -> 512 + R, fp32 + bf16 out) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def tl2():
    t = G.tl_inputs(512, 512, 2, True, MV, T, NB)
    ref = G.tl_chain(t, MV, T, NB, 2, 0, torch.float64)
    slack, _ = G.prologue_slack(t, MV, T, NB, 2, 0, ref)
    return t, ref, slack


@pytest.mark.parametrize("reverse", [False, True])
def test_film_prologue_emulation_passes(tl2, reverse):
    t, ref, slack = tl2
    y = G.tl_chain(t, MV, T, NB, 2, 0, torch.float32, reverse=reverse)
    assert G.assert_close_f32(y, ref, slack) <= 1.0
    assert G.assert_rounded(y.bfloat16(), ref, slack) <= 1.0


@pytest.mark.parametrize("mutant", ["kterm", "film_neighbour"])
def test_film_prologue_mutants_are_rejected(tl2, mutant):
    t, ref, slack = tl2
    if mutant == "kterm":
        y = G.tl_chain(dict(t, W=_drop_last_k(t["W"])), MV, T, NB, 2, 0, torch.float64)
    else:
        y = G.tl_chain(t, MV, T, NB, 2, 0, torch.float64, film_rows=_neighbour_rows(MV, T, NB))
    assert _rejected(G.assert_close_f32, y.float(), ref, slack, frames=T, nb=NB)
    assert _rejected(G.assert_rounded, y.bfloat16(), ref, slack, frames=T, nb=NB)
    _record("tl2/" + mutant, _old_tl_cf(y.float(), ref, 2) and _old_tl_ct(y.bfloat16(), ref))


# ---- folded concat-LayerNorm (pro 3, 999 real columns of 1024, SiLU) ------------------------------------------------------------------------
def _pro3_inputs():
    K, N, kreal = 1024, 1024, 999
    t = G.tl_inputs(K, N, 3, False, MV, T, NB)
    t["X"][:, kreal:] = 0; t["W"][:, kreal:] = 0; t["gam"][kreal:] = 0; t["bet"][kreal:] = 0
    return t, kreal


def test_folded_layernorm_emulation_passes_and_wrong_divisor_is_rejected():
    t, kreal = _pro3_inputs()
    pre, slack, ref = G.tl_folded(t, MV, 3, 1, kreal)
    slack = G.SILU_LIP * slack + G.silu_hw(ref)
    # the fold is an identity up to the rounding of W' = bf16(gamma W): the unfolded fp64 LayerNorm agrees to ~1e-2, not to the gate
    unfolded = F.silu(F.layer_norm(t["X"][:MV, :kreal].double(), (kreal,), t["gam"][:kreal].double(), t["bet"][:kreal].double(), 1e-5)
                      @ t["W"][:, :kreal].double().T + t["b"].double())
    assert float((unfolded - ref).abs().max()) < 3e-2
    # faithful: fp32 sums, E[x^2] - mean^2, folded epilogue
    x = t["X"][:MV, :kreal].float()
    Wf = (t["W"].float() * t["gam"].float()).bfloat16().float()[:, :kreal]
    c = Wf.double().sum(1).float()
    d = (t["b"].double() + t["W"].double()[:, :kreal] @ t["bet"].double()[:kreal]).float()
    for reverse in (False, True):
        xs, ws = (x.flip(1), Wf.flip(1)) if reverse else (x, Wf)
        mean = xs.sum(-1, keepdim=True) / kreal
        var = (xs * xs).sum(-1, keepdim=True) / kreal - mean * mean
        y = F.silu(torch.rsqrt(var + 1e-5) * (xs @ ws.T - mean * c) + d)
        assert G.assert_rounded(y.bfloat16(), ref, slack) <= 1.0
    # mutant 7: moments divided by the padded width
    mean = x.double().sum(-1, keepdim=True) / 1024
    var = (x.double() ** 2).sum(-1, keepdim=True) / 1024 - mean * mean
    mut = F.silu(torch.rsqrt(var + 1e-5) * (x.double() @ Wf.double().T - mean * c.double()) + d.double())
    assert _rejected(G.assert_rounded, mut.bfloat16(), ref, slack)
    old = float(((mut.bfloat16().double() - unfolded).abs().max() / unfolded.abs().max())) < 2e-2      # the gate of the large-mean test
    _record("tl3/ln_divisor", old)


# ---- fused FFN -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ffn():
    n_const = 128
    t = G.ffn_inputs(MV, T, NB, n_const)
    ref = G.ffn_chain(t, MV, T, NB, n_const, torch.float64)
    c32 = G.ffn_chain(t, MV, T, NB, n_const, torch.float32, noise=G.gelu_noise((MV, 1024)))
    slack, rms = G.calibrate(c32, ref)
    return t, ref, slack, rms, n_const


def _old_ffn(y, ref):
    scale = max(1.0, float(ref.abs().max()))
    e32 = float((y.float().double() - ref).abs().max()); e16 = float((y.bfloat16().double() - ref).abs().max())
    return e32 < 3e-2 * scale and e16 < 4e-2 * scale and float((y.float().double() - ref).pow(2).mean().sqrt()) < 3e-3 * scale


@pytest.mark.parametrize("reverse", [False, True])
def test_ffn_emulation_passes(ffn, reverse):
    t, ref, slack, rms, n_const = ffn
    y = G.ffn_chain(t, MV, T, NB, n_const, torch.float32, reverse=reverse, noise=G.gelu_noise((MV, 1024), seed=2 + reverse))
    assert G.assert_close_f32(y, ref, slack) <= 1.0
    assert G.assert_rounded(y.bfloat16(), ref, slack) <= 1.0
    assert G.assert_rms(y, ref, rms) <= 1.0
    assert G.assert_rms(y.bfloat16(), ref, rms + G.bf16_rounding_rms(ref)) <= 1.0


@pytest.mark.parametrize("mutant", ["kterm", "fragswap", "film_neighbour", "bias_tile"])
def test_ffn_mutants_are_rejected(ffn, mutant):
    t, ref, slack, rms, n_const = ffn
    kw = {}
    if mutant == "kterm":
        kw["w3"] = _drop_last_k(t["W3"])
    elif mutant == "fragswap":
        kw["w3"] = _swap_fragments(t["W3"])
    elif mutant == "film_neighbour":
        kw["film_rows"] = _neighbour_rows(MV, T, NB)
    else:
        b3 = t["b3"].clone(); b3[64:96] = 0
        kw["b3"] = b3
    y = G.ffn_chain(t, MV, T, NB, n_const, torch.float64, **kw)
    assert _rejected(G.assert_close_f32, y.float(), ref, slack, frames=T, nb=NB)
    assert _rejected(G.assert_rounded, y.bfloat16(), ref, slack, frames=T, nb=NB)
    if mutant == "kterm":          # every row is wrong: the rms gate alone rejects it
        assert _rejected(G.assert_rms, y.float(), ref, rms)
    _record("ffn/" + mutant, _old_ffn(y, ref))


# ---- bf16 linear attention ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn():
    qkv = G.attn_inputs(2, 30)
    ref = G.attn_chain(qkv, torch.float64)
    slack, _ = G.calibrate(G.attn_chain(qkv, torch.float32), ref)
    return qkv, ref, slack


def test_attention_emulation_passes(attn):
    qkv, ref, slack = attn
    y = G.attn_chain(qkv, torch.float32)
    assert G.assert_rounded(y.bfloat16().reshape(-1, 512), ref.reshape(-1, 512), slack) <= 1.0
    # the time-softmax accumulated over the frames in reversed order
    y = G.attn_chain(qkv.flip(1), torch.float32).flip(1)
    assert G.assert_rounded(y.bfloat16().reshape(-1, 512), ref.reshape(-1, 512), slack) <= 1.0


def test_attention_mutants_are_rejected(attn):
    qkv, ref, slack = attn
    nb, Tq, _ = qkv.shape
    old_ref = G.attn_chain(qkv, torch.float64, rounded=False)        # the previous test's reference rounds nothing
    mut = G.attn_chain(qkv, torch.float64, lens=[Tq - 1])
    assert _rejected(G.assert_rounded, mut.bfloat16().reshape(-1, 512), ref.reshape(-1, 512), slack, frames=Tq, nb=nb)
    _record("attn/t_minus_1", float((mut.bfloat16().double() - old_ref).abs().max()) < 2e-2 * max(1.0, float(old_ref.abs().max())))
    # ragged: clips of 21 valid frames; the wrong kernel lets the first padded frame (finite here) into the time-softmax
    lens = [21]
    rref = G.attn_chain(qkv, torch.float64, lens=lens)
    rslack, _ = G.calibrate(G.attn_chain(qkv, torch.float32, lens=lens), rref)
    ok = G.attn_chain(qkv, torch.float32, lens=lens).bfloat16()
    assert G.assert_rounded(ok[:, :21].reshape(-1, 512), rref[:, :21].reshape(-1, 512), rslack) <= 1.0
    mut = G.attn_chain(qkv, torch.float64, lens=[22]).bfloat16()
    assert _rejected(G.assert_rounded, mut[:, :21].reshape(-1, 512), rref[:, :21].reshape(-1, 512), rslack, frames=21, nb=nb)
    rold = G.attn_chain(qkv, torch.float64, lens=lens, rounded=False)
    _record("attn/padded_frame", float((mut[:, :21].double() - rold[:, :21]).abs().max()) < 2e-2 * max(1.0, float(rold.abs().max())))


# ---- every attention kernel form x input family x length of test_gpu_bf16_attention_families.py --------------------------------------------
# (storage dtype, rounding points) decide the chain and the gate: the tiled and the row-major MFMA kernel share theirs
ATTN_CPU_ROWS = sorted({(G.ATTN_FORMS[form][0], G.ATTN_FORMS[form][2], D, hd, T) for form, D, hd, T in G.ATTN_ROWS}, reverse=True)
FRAME_MUTANTS = ("frame_more", "frame_fewer")


def _attn_mutants(qkv, dtype, rounds, hd, lens, doubled, ref):
    """name -> output of a subtly wrong kernel, stored with round-to-nearest in the form's storage type (the truncating store excepted)"""
    st = torch.bfloat16 if dtype else torch.float32
    kw = dict(lens=lens, hd=hd)
    m = {"frame_more": G.attn_chain(qkv, torch.float64, rounded=rounds, frames_delta=1, **kw).to(st),
         "frame_fewer": G.attn_chain(qkv, torch.float64, rounded=rounds, frames_delta=-1, **kw).to(st)}
    if dtype:
        m["truncating_store"] = G.truncate_bf16(ref)
    if rounds:
        m["k_rounded_before_normalisation"] = G.attn_chain(qkv, torch.float64, rounded=("A", "q"), k_round_early=True, **kw).to(st)
    else:
        m["k_rounded_inside"] = G.attn_chain(qkv, torch.float64, rounded=("k",), **kw).to(st)
        m["A_rounded_inside"] = G.attn_chain(qkv, torch.float64, rounded=("A",), **kw).to(st)
    if hd == 16:
        m["channel_softmax_over_64"] = G.attn_chain(qkv, torch.float64, rounded=rounds, q_group=64, **kw).to(st)
    if doubled:
        m["second_half_reads_lens_b"] = G.attn_chain(qkv, torch.float64, rounded=rounds, hd=hd, lens=G.attn_wrong_half_lens(lens)).to(st)
    return m


@pytest.mark.parametrize("mode", ["dense", "ragged", "doubled"])
@pytest.mark.parametrize("dtype,rounds,D,hd,T", ATTN_CPU_ROWS)
def test_attention_family_gates_pass_the_chain_and_reject_the_mutants(dtype, rounds, D, hd, T, mode):
    """On the operands the GPU tests build: the fp64 chain in the form's storage type passes its own gate in every family, every mutant is
    rejected by at least one family, and what each family can NOT see is pinned: a K-softmax saturated on one middle frame is blind to
    which other frames enter (dense batch: ratio <= 1 for both frame-count mutants); the other five families each reject both."""
    lens = None if mode == "dense" else G.attn_lens(T)
    nb = G.ATTN_NB if lens is None else len(lens) * (2 if mode == "doubled" else 1)
    st = torch.bfloat16 if dtype else torch.float32
    seen = {}
    for family in G.ATTN_FAMILIES:
        qkv = G.attn_inputs(nb, T, family, D, hd)
        ref, cal, flips = G.attn_gate(qkv, hd, rounds, lens)
        assert cal > 0
        assert G.attn_check(ref.to(st), ref, cal, T, lens, extra=flips) <= 1.0
        if rounds:          # the fp32 chain with the exponentials taken the kernels' way (exp2 of a rounded x log2e - m log2e): other flips, same gate
            assert G.attn_check(G.attn_chain(qkv, torch.float32, lens=lens, hd=hd, fast_exp=True).bfloat16(), ref, cal, T, lens, extra=flips) <= 1.0
        for name, out in _attn_mutants(qkv, dtype, rounds, hd, lens, mode == "doubled", ref).items():
            ratio = G.attn_ratio(out, ref, cal, T, lens, flips)
            assert (ratio > 1.0) == _rejected(G.attn_check, out, ref, cal, T, lens, extra=flips)
            seen.setdefault(name, set())
            if ratio > 1.0:
                seen[name].add(family)
    for name, fams in seen.items():
        assert fams, f"{name}: no family rejects it at D {D} hd {hd} T {T} ({mode})"
    for name in FRAME_MUTANTS:
        assert seen[name] >= set(G.ATTN_FAMILIES) - {"k_sat"}, (name, seen[name])
        if mode == "dense":
            assert "k_sat" not in seen[name], name


def test_attention_plain_family_is_the_recipe_of_the_op_test():
    g = torch.Generator().manual_seed(34 + 3)
    assert torch.equal(G.attn_inputs(3, 34), (torch.randn(3, 34, 3 * 512, generator=g) * 2).bfloat16())
    assert torch.equal(G.attn_inputs(3, 34, "plain", 512, 64), G.attn_inputs(3, 34))
    x = G.attn_inputs(3, 34, "q_sat", 128, 16).float().view(3, 34, 3, 8, 16)
    assert float(x[:, :, 0, :, 3].min()) > 20 and float(x[:, :, 1:, :, 3].max()) < 12


# ---- fused encoder_aud tail (D = 128) --------------------------------------------------------------------------------------------------------------
AUD_SHAPES = [(300, 88, 4), (44, 11, 4), (290, 34, 9)]
_AUD = {}


def _aud(shape):
    if shape not in _AUD:
        t = G.aud_inputs(*shape)
        _AUD[shape] = (t,) + G.aud_gates(t, *shape)
    return _AUD[shape]


@pytest.mark.parametrize("shape", AUD_SHAPES)
@pytest.mark.parametrize("reverse", [False, True])
def test_aud_tail_emulation_passes(shape, reverse):
    t, ref, slack, rms, cal, st = _aud(shape)
    Mc, T, nb = shape
    y = G.aud_chain(t, Mc, T, nb, torch.float32, reverse=reverse, noise=G.gelu_noise((Mc, 1024), seed=2 + reverse))
    assert G.assert_close_f32(y, ref, slack) <= 1.0
    assert G.assert_rounded(y.bfloat16(), ref, slack) <= 1.0
    assert G.assert_rms(y, ref, rms) <= 1.0
    assert G.assert_rms(y.bfloat16(), ref, rms + G.bf16_rounding_rms(ref)) <= 1.0
    # the gate is a fraction of a percent of the output range (the whole-model test of the aud_feat tap allows 2 %)
    assert float(slack.max()) < 5e-3 * float(ref.max() - ref.min())


@pytest.mark.parametrize("shape", AUD_SHAPES)
@pytest.mark.parametrize("mutant", ["film_neighbour_one_row", "w2_kstep", "film_block1_for_block2", "residual_x", "truncate"])
def test_aud_tail_mutants_are_rejected(shape, mutant):
    t, ref, slack, rms, cal, st = _aud(shape)
    Mc, T, nb = shape
    kw, m = {}, t
    if mutant == "film_neighbour_one_row":          # ONE row (the last frame of clip 0) takes the next clip's FiLM row
        rows = torch.arange(Mc)
        fr = (rows // T) % nb
        fr[T - 1] = 1
        kw["film_rows"] = fr
    elif mutant == "w2_kstep":                      # one 16-wide k step of linear2 (hidden features 336 .. 351) left out
        W2 = t["W2"].clone(); W2[:, 336:352] = 0
        m = dict(t, W2=W2)
    elif mutant == "film_block1_for_block2":
        m = dict(t, film=torch.cat([t["film"][:, :256], t["film"][:, :256]], 1))
    elif mutant == "residual_x":
        kw["final_res"] = "x"
    y = G.aud_chain(m, Mc, T, nb, torch.float64, **kw)
    if mutant == "truncate":
        # one flip of s2 is worth more than an ulp of the output, so no single element gives a truncating store away against the fp64
        # chain, and its rms (ulp / sqrt(3) in place of ulp / sqrt(12)) lands on the rms gate: the store is checked against the kernel's
        # own fp32 output instead, exactly
        G.assert_store_is_rne(y.float().bfloat16(), y.float())
        assert _rejected(G.assert_store_is_rne, G.truncate_bf16(y.float()), y.float())
        return
    assert _rejected(G.assert_close_f32, y.float(), ref, slack, frames=T, nb=nb)
    assert _rejected(G.assert_rounded, y.bfloat16(), ref, slack, frames=T, nb=nb)
    bad = int(((y - ref).abs() > slack).sum())
    assert bad > (100 if mutant == "film_neighbour_one_row" else 1000), bad     # one row of 128 / most of the tensor
    if mutant != "film_neighbour_one_row":          # every row is wrong: the rms gate alone rejects it
        assert _rejected(G.assert_rms, y.float(), ref, rms)


def test_ln_raw_moment_slack_grows_with_the_offset_only():
    """The widening of the large-offset test is nothing at offset 0 beside the calibrated gate and follows mean^2 / var."""
    t, ref, slack, rms, cal, st = _aud((300, 88, 4))
    A2 = (t["g2"] * (1 + t["film"][:, 256:384]))[(torch.arange(300) // 88) % 4]
    w0 = G.ln_raw_moment_slack(st["y2"], A2, t["Ws2"])
    w100 = G.ln_raw_moment_slack(st["y2"] - 100.0, A2, t["Ws2"])
    assert float(w0.max()) < 1e-2 * G.MARGIN * cal
    r = st["y2"].double()
    growth = (1 + (r.mean(-1) - 100) ** 2 / r.var(-1, unbiased=False)) / (1 + r.mean(-1) ** 2 / r.var(-1, unbiased=False))
    assert torch.allclose(w100.max(-1).values / w0.max(-1).values, growth, rtol=1e-2)


# ---- audio_proj ----------------------------------------------------------------------------------------------------------------------------------------
def test_aproj_emulation_passes_and_the_other_encoders_bias_is_rejected():
    t = G.aproj_inputs(129, 2)
    for e in (0, 1):
        ref = G.aproj_ref(t, e)
        slack = G.accum_bound(t["X"], t["W"][e], 256)
        for reverse in (False, True):
            assert G.assert_rounded(G.aproj_ref(t, e, torch.float32, reverse=reverse).bfloat16(), ref, slack) <= 1.0
    ref, slack = G.aproj_ref(t, 1), G.accum_bound(t["X"], t["W"][1], 256)
    assert _rejected(G.assert_rounded, G.aproj_ref(t, 1, bias_of=0).bfloat16(), ref, slack)
    assert _rejected(G.assert_rounded, G.truncate_bf16(ref), ref, slack)


# ---- layer-0 seed --------------------------------------------------------------------------------------------------------------------------------------
JOINT_CASES = [(103, 44, 11), (141, 290, 34)]


@pytest.mark.parametrize("w,Mc,T", JOINT_CASES)
def test_joint_emulation_passes(w, Mc, T):
    t = G.joint_inputs(w, Mc, T, ldx=w + 40, c0=17)
    refs, slacks = G.joint_ref(t, Mc, T), G.joint_slack(t, Mc, T)
    for reverse in (False, True):
        outs = G.joint_ref(t, Mc, T, torch.float32, reverse=reverse, planes=True)
        for o, r, s in zip(outs, refs, slacks):
            assert G.assert_close_f32(o, r, s) <= 1.0
    assert float(slacks[1].max()) < 5e-4          # (2^-17 of a value of a few units and 144 x 2^-23 of ~10 in products)


@pytest.mark.parametrize("w,Mc,T", JOINT_CASES)
@pytest.mark.parametrize("mutant", ["pe_modulus", "null_on_cond", "last_fragment", "lo_dropped"])
def test_joint_mutants_are_rejected(w, Mc, T, mutant):
    t = G.joint_inputs(w, Mc, T, ldx=w + 40, c0=17)
    (rc, rn), (sc, sn) = G.joint_ref(t, Mc, T), G.joint_slack(t, Mc, T)
    if mutant == "pe_modulus":                    # PE row = row % (frames + 1)
        mc, mn = G.joint_ref(t, Mc, T, pe_mod=T + 1)
    elif mutant == "null_on_cond":                # the null constant reaches the conditional half as well
        mc, mn = rn, rn
    elif mutant == "last_fragment":               # columns >= 16 (nf - 1) left out
        mc, mn = G.joint_ref(t, Mc, T, kdrop=16 * ((w + 15) // 16 - 1))
    else:
        mc, mn = rc.bfloat16().double(), rn.bfloat16().double()
    assert _rejected(G.assert_close_f32, mc.float(), rc, sc, frames=T, nb=Mc // T)
    if mutant != "null_on_cond":
        assert _rejected(G.assert_close_f32, mn.float(), rn, sn, frames=T, nb=Mc // T)


# ---- elementary properties -----------------------------------------------------------------------------------------------------------------------
def test_ulp_and_bound_definitions():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 255.0, 256.0, 0.0, 1e-45, -3.0])
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 1.0, 2.0, 2.0 ** -133, 2.0 ** -133, 2.0 ** -6], dtype=torch.float64)
    assert torch.equal(G.ulp_bf16(v), want)
    # the spacing of bf16 around v is ulp_bf16(v)
    x = torch.tensor([1.0, 3.0, 100.0]).bfloat16()
    nxt = (x.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - x.double()), G.ulp_bf16(x))
    X, W = torch.tensor([[1.0, -2.0]]), torch.tensor([[3.0, 4.0], [-1.0, 0.5]])
    assert torch.equal(G.accum_bound(X, W, 2), 2 * 2.0 ** -23 * torch.tensor([[11.0, 2.0]], dtype=torch.float64))
    # half an ulp is accepted, anything more is not; truncation differs from rounding
    ref = torch.tensor([[1.0 + 2.0 ** -8]], dtype=torch.float64)
    G.assert_rounded(torch.tensor([[1.0]]).bfloat16(), ref)
    with pytest.raises(AssertionError):
        G.assert_rounded(torch.tensor([[1.0]]).bfloat16(), ref + 2.0 ** -20)
    assert float(G.truncate_bf16(torch.tensor([1.0 + 3 * 2.0 ** -9]))) == 1.0 and float(torch.tensor([1.0 + 3 * 2.0 ** -9]).bfloat16()) == 1.0 + 2.0 ** -7

