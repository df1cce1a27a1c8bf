"""The gates of metrics_gates.py, shown to bite without a GPU on the operands and cases of test_gpu_conv_gemm.py,
test_gpu_metrics_edges.py and test_gpu_fgd_encoder_edges.py:
(a) faithful emulations pass: the conv in float32 in both K orders and in the K order of the kernel's MFMA steps, the diversity in the
    kernel's order (inner j-sum in float32, the rest in float64), the PCK emulation against a direct restatement of the reference's lines;
(b) subtly wrong kernels are rejected at every case they apply to: six conv mutants, four PCK mutants, four diversity mutants;
(c) the case lists reach the paths they are meant to reach (the launcher's dispatch rules restated here from its comments)."""
import argparse

import numpy as np
import pytest
import torch

import metrics_gates as G

F64 = torch.float64


def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


# ---- conv ---------------------------------------------------------------------------------------------------------------------------------
def _mfma_k_order(Kp):
    """K order of conv_gemm_f32_kernel: K tiles ascending; inside a tile four 8-float chunks; each of the four MFMA steps of a chunk takes
    k = e and k = e + 4 of it (lanes 0 .. 31 / 32 .. 63)"""
    return [kt * 32 + c * 8 + h * 4 + e for kt in range(Kp // 32) for c in range(4) for e in range(4) for h in range(2)]


@pytest.mark.parametrize("name", list(G.CONV_CASES))
def test_conv_emulations_pass_the_gate(name):
    t = G.conv_case(name)
    M = t["M"]
    for rev in (False, True):
        G.conv_check(t, G.conv_chain(t, torch.float32, reverse=rev)[:M])
    # the kernel's own K order (one accumulator per output, the zero-padded K included)
    rows = torch.nn.functional.pad(G.conv_rows(t, torch.float32)[:M], (0, t["Kp"] - t["Kreal"]))
    W = G.conv_w_padded(t)[:, :t["Kp"]]
    perm = _mfma_k_order(t["Kp"])
    out = G._act(G._mm(rows[:, perm], W[:, perm], False) + t["b"], t, G.SLOPE32)
    G.conv_check(t, out)
    print(f"[{name}] kernel-order emulation / calibration = {G.conv_ratio(t, out)}")
    ref, cal = G.conv_gate(t)
    if t["family"] != "ints":
        assert 0 < G.MARGIN * cal < 1e-3 * max(1.0, float(ref.abs().max())), "the gate is inside the path's 1e-3 of range"
    # the launch's X buffer: exactly the floats some window covers are finite
    flat = G.conv_x_flat(t)
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    covered[G.conv_index(t, t["B"], t["x_clip"], t["x_step"], t["Kreal"]).reshape(-1)] = True
    assert torch.equal(torch.isfinite(flat), covered) and not bool(covered[-G.X_TAIL:].any())
    if t["x_clip"] > t["Tin"] * t["Cin"]:
        assert not bool(covered[t["Tin"] * t["Cin"]:t["x_clip"]].any())


@pytest.mark.parametrize("mutant,name", [(m, n) for m in G.CONV_MUTANTS for n in G.CONV_CASES])
def test_conv_mutants_are_rejected(mutant, name):
    t = G.conv_case(name)
    if not G.CONV_MUTANTS[mutant](t):
        assert mutant != "drop_piece"
        return                                       # (does not apply to this shape: nothing it could get wrong)
    assert _rejected(G.conv_check, t, G.conv_mutant(t, mutant).float()), (mutant, name)


def test_conv_mutants_each_apply_somewhere_in_every_family():
    for m, applies in G.CONV_MUTANTS.items():
        fams = {G.conv_case(n)["family"] for n in G.CONV_CASES if applies(G.conv_case(n))}
        assert fams == set(G.CONV_FAMILIES), (m, fams)


def _dispatch(M, N):
    """launch_conv_gemm_f32's rules: (rows per block tile, nt_m, nt_n, blocks launched, padded blocks)"""
    bm = 128 if M >= 2048 else 64
    nt_m, nt_n = -(-M // bm), -(-N // 64)
    grid = -(-nt_m // 8) * 8 * nt_n if nt_m >= 8 else nt_m * nt_n
    return bm, nt_m, nt_n, grid, grid - nt_m * nt_n


def test_conv_cases_reach_every_path():
    want = {448: (64, 7, 2, 14, 0), 449: (64, 8, 2, 16, 0), 513: (64, 9, 2, 32, 14), 2047: (64, 32, 2, 64, 0), 2048: (128, 16, 2, 32, 0),
            2049: (128, 17, 2, 48, 14)}
    for M, d in want.items():
        t = G.conv_case(f"dispatch-M{M}")
        assert t["M"] == M and t["N"] == 68 and t["Kreal"] == 24 and _dispatch(M, 68) == d
    cases = [G.conv_case(n) for n in G.CONV_CASES]
    width = [t for t in cases if t["name"].startswith("width-")]
    geom = [t for t in cases if t["name"].startswith("geom-")]
    assert {(t["N"], t["Kreal"]) for t in width} == {(N, K) for N in G.CONV_N for K in G.CONV_K}
    assert {t["Kp"] for t in width} == {32, 64, 704, 1216}
    for group in (width, geom):
        assert {t["family"] for t in group} == set(G.CONV_FAMILIES)
        assert {t["B"] for t in group} == {1, 3} and {t["leaky"] for t in group} == {0, 1}
        assert {t["x_clip"] > t["Tin"] * t["Cin"] for t in group} == {False, True}
        assert {t["y_clip"] > t["Tout"] * t["N"] for t in group} == {False, True}
    assert {(t["ks"], t["stride"], t["Tout"] == 1) for t in geom} == {(3, 1, False), (4, 2, False), (3, 1, True)}
    assert {t["Tout"] for t in width} == {1, 23, 70} and any(t["M"] > 64 for t in width) and any(t["ldw"] > t["Kp"] for t in width)
    assert any(t["stride"] == 2 and (t["Tin"] - t["ks"]) % 2 for t in geom), "a stride-2 clip whose last frame no window covers"


# ---- PCK ----------------------------------------------------------------------------------------------------------------------------------
def _threshold_stats(n, seed):
    o, m = G.threshold_joints(n, seed)
    s = G.pck_sums(o, m, 3)
    base = G.pck_hits(s)
    d = o.astype(np.float64)
    f64 = np.sqrt((d * d).sum(1)) < 0.5
    return {"below": float((s == G.BELOW_QUARTER).mean()), "at": float((s == np.float32(0.25)).mean()), "above": float((s == G.ABOVE_QUARTER).mean()),
            "contract": float(((G.pck_hits(G.pck_sums(o, m, 3, 1)) != base) | (G.pck_hits(G.pck_sums(o, m, 3, 2)) != base)).mean()),
            "f64": float((f64 != base).mean())}


def test_threshold_family_sits_on_the_threshold():
    st = _threshold_stats(200_000, 1)
    print(f"threshold family, 200 000 joints: {st}")
    assert 0.12 <= st["below"] <= 0.22 and 0.70 <= st["at"] <= 0.82 and 0.03 <= st["above"] <= 0.08
    assert 0.07 <= st["contract"] <= 0.16 and 0.25 <= st["f64"] <= 0.40
    # the 4 096 joints of the GPU test hold hundreds of the two populous kinds and of every mutant's victims
    for seed in (0, 1):
        o, m = G.threshold_joints(4096, seed)
        s = G.pck_sums(o, m, 3)
        assert (s == G.BELOW_QUARTER).sum() >= 400 and (s == np.float32(0.25)).sum() >= 2500 and (s == G.ABOVE_QUARTER).sum() >= 100


@pytest.mark.parametrize("seed", [0, 1])
def test_pck_mutants_change_the_count_on_the_threshold_family(seed):
    o, m = G.threshold_joints(4096, seed)
    base = G.pck_emul(o, m, 3)
    assert base == G.pck_restated(o, m, 3)
    counts = {"contract_1": G.pck_emul(o, m, 3, contract=1), "contract_2": G.pck_emul(o, m, 3, contract=2), "le": G.pck_emul(o, m, 3, le=True),
              "sqrt_high": G.pck_emul(o, m, 3, sqrt_high=True)}
    print(f"threshold family seed {seed}: count {base} of 4096; mutants {counts}")
    for k, v in counts.items():
        assert v != base, k
    assert counts["le"] - base >= 2500 and base - counts["sqrt_high"] >= 400


def test_pck_emulation_equals_the_restated_reference():
    for seed in (0, 1):
        for off in (0.0, 37.25):
            o, m = G.threshold_joints(4096, seed, off)
            assert G.pck_emul(o, m, 3) == G.pck_restated(o, m, 3)
    # the offset form: the float32 subtraction returns multiples of ulp(37.25) = 2^-18, none of them the unrounded direction
    o, m = G.threshold_joints(4096, 0, 37.25)
    v, _ = G.threshold_joints(4096, 0)
    d = o - m
    assert np.all(d * np.float32(2 ** 18) == np.round(d * np.float32(2 ** 18))) and (d != v).mean() > 0.9
    assert G.pck_emul(o, m, 3) != G.pck_emul(v, np.zeros_like(v), 3)
    o, m = G.threshold_scalars(4096)
    base = G.pck_emul(o, m, 1)
    assert base == G.pck_restated(o, m, 1) == int((np.abs(o) < 0.5).sum()) and 0 < base < 4096
    assert G.pck_emul(o, m, 1, le=True) == int((np.abs(o) <= 0.5).sum()) != base
    for shape in G.METRIC_SHAPES:
        for fam in G.METRIC_FAMILIES:
            o, m = G.metric_inputs(*shape, family=fam)
            assert G.pck_emul(o.numpy(), m.numpy(), shape[3]) == G.pck_restated(o.numpy(), m.numpy(), shape[3])


# ---- MSE / diversity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", G.METRIC_FAMILIES)
def test_diversity_in_the_kernels_order_stays_inside_the_derived_gate(shape, family):
    B, T, C, jd, b_div = shape
    o, m = G.metric_inputs(*shape, family=family)
    ref = G.div_ref(o, b_div)
    assert ref.shape == (B // b_div,) and np.all(ref > 0)
    r = G.div_check(G.div_kernel_order(o, b_div), ref, b_div)
    print(f"[{shape} {family}] kernel-order emulation: error / gate = {r:.3f}")
    assert r <= 1.0
    # mutants
    assert _rejected(G.div_check, G.div_kernel_order(o, b_div, divisor=b_div * b_div), ref, b_div)
    if B % b_div:
        assert _rejected(G.div_check, G.div_kernel_order(o, b_div, remainder="merged"), ref, b_div)
    if B % b_div >= 2:
        assert _rejected(G.div_check, G.div_kernel_order(o, b_div, remainder="own"), ref, b_div)
    if (T * C) % 256:
        assert _rejected(G.div_check, G.div_kernel_order(o, b_div, next_clip_cols=True), ref, b_div)
    # MSE: a float64 sum in another order is inside the gate, a float32 accumulation is not (where there is enough to add)
    exact, n, gate = G.mse_ref(o, m)
    d = (o - m).double().reshape(-1)
    assert abs(float((d * d).flip(0).cumsum(0)[-1]) - exact) <= gate * exact
    if n >= 4096:
        assert abs(float((d * d).float().cumsum(0)[-1]) - exact) > gate * exact


def test_metric_shapes_reach_every_path():
    shapes = set(G.METRIC_SHAPES)
    assert any(B % bd for B, T, C, jd, bd in shapes) and any(B // bd >= 2 and B % bd for B, T, C, jd, bd in shapes)
    assert any(T * C < 256 for B, T, C, jd, bd in shapes) and any(T * C == 256 for B, T, C, jd, bd in shapes) and any(T * C == 257 for B, T, C, jd, bd in shapes)
    assert {bd for *_, bd in shapes} >= {2, 64, 65, 128} and 64 * 256 * 4 == 64 * 1024
    assert any(B * T * C // jd > 1024 * 256 for B, T, C, jd, bd in shapes), "the grid-stride loop"
    assert any(B * T * C // jd < 256 for B, T, C, jd, bd in shapes), "fewer joints than one block"
    assert {jd for _, _, _, jd, _ in shapes} == {1, 3}


# ---- encoder --------------------------------------------------------------------------------------------------------------------------------
def test_encoder_gate_from_the_packed_layers_in_float32():
    """packed_forward in float32 with one accumulator per output: close to its float64 form (the calibration is round-off, not a second
    network), not equal to it, and the same in both K orders to within MARGIN."""
    from diffsheg_amd import _lib, metrics
    from diffsheg_amd.weights import make_synthetic_fid_state_dict
    opt = argparse.Namespace(n_poses=64, net_dim_pose=103, vae_length=32)
    sd = make_synthetic_fid_state_dict(opt, 7)
    h = metrics.create_fgd_handle(64, 103, 32)
    try:
        metrics.load_fgd_weights(h, sd)
        layers = metrics.packed_fgd_layers(h)
    finally:
        _lib.lib().dsh_fgd_destroy(h)
    x = torch.randn(G.ENC_CAL_CLIPS, 64, 103, generator=torch.Generator().manual_seed(3))
    ref, cal = G.encoder_gate(layers, x, 64, 103)
    rng = float(ref.max() - ref.min())
    print(f"64 frames / 103 channels / base 32: calibration {cal:.2e} = {cal / rng:.2e} of the latent range")
    assert ref.shape == (G.ENC_CAL_CLIPS, 32) and 0 < G.MARGIN * cal < 1e-5 * rng
