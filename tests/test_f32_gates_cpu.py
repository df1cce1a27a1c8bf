"""The gates of f32_gates.py, tested without a GPU on the operands and cases of the GPU tests:
(a) faithful fp32 emulations of each launch pass the gate at every case: the documented expression with the kernel's one-pass moments
    shifted by the mean of the first K tile (PRO 1, PRO 2), and every chain with its accumulations in reversed order;
(b) eleven subtly wrong kernels are rejected at every case they apply to;
(c) mutant 1 - the row moments shifted by the row's FIRST ELEMENT, which is gemm_f32_pro.hip before the shift was changed - is rejected
    on the outlier-column inputs and ACCEPTED on the plain and whole-row-offset ones: the inputs the tests had before could not see it.
"""
import pytest
import torch
import torch.nn.functional as F

import f32_gates as G

F64 = torch.float64


def _rejected(t, out):
    try:
        G.check(t, out)
    except AssertionError:
        return True
    return False


def _forward(t):
    if t["kind"] == "pro1" or (t["kind"] == "pro2" and not t["stat_groups"]):
        return G.chain(t, moments="tile")
    return G.chain(t)


# ---- (a) emulations -------------------------------------------------------------------------------------------------------------------------
# the grid on the CPU: every N and K at the M on either side of a row tile and of the XCD ordering switch (the GPU tests run all of them)
CPU_CASES = [n for n in G.CASES if "-grid-" not in n or n.split("-")[2].split("x")[0] in ("1", "65", "449")]


@pytest.mark.parametrize("name", CPU_CASES)
def test_emulations_pass_the_gate(name):
    t = G.case(name)
    assert G.check(t, _forward(t)) <= G.MARGIN
    assert G.check(t, G.chain(t, reverse=True)) <= G.MARGIN
    ref, allow, cal = G.gate(t)
    rest = torch.ones(len(allow), dtype=torch.bool)
    rest[t.get("special", [])] = False
    assert float(allow[rest].max()) < 1e-3 * max(1.0, float(ref.abs().max())), (allow.max(), "the gate is inside the path's 1e-3 of range")
    if t["kind"] == "pro0" and t["stats_out"]:
        sref, a_mean, a_m2 = G.stats_gate(t)
        st = G.group_moments(G.pro0_chain(t, torch.float32, reverse=True)).double()
        assert float((st[..., 0] - sref[..., 0]).abs().max()) <= a_mean and float((st[..., 1] - sref[..., 1]).abs().max()) <= a_m2


@pytest.mark.parametrize("sty", [False, True])
@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("T", [1, 2, 33, 64])
def test_attention_emulations_pass_the_gate(T, family, sty):
    t = G.attn_inputs(3, T, family, sty)
    assert G.check(t, G.chain(t)[:3 * T]) <= 1.0
    out = G.attn_chain(t, torch.float32, reverse=True)[:3].reshape(-1, 512)
    assert G.check(t, out) <= G.MARGIN


# ---- (b), (c) mutants -------------------------------------------------------------------------------------------------------------------------
PADDED = [n for n in G.CASES if n.startswith("p1-seg-") and G.CASES[n][1][3] < sum(G.CASES[n][1][2])] + ["p1-fam-plain-947", "p1-fam-off+50-947"]
FAM = lambda fams, kinds=("p1", "p2"): [n for n in G.CASES if "-fam-" in n and n.split("-fam-")[1].rsplit("-", 1)[0] in fams and n[:2] in kinds]
SOME_GRID = ["p0-grid-65x68x32", "p0-grid-449x100x96", "p1-grid-65x68x32", "p1-grid-449x100x1024", "p2-grid-65x68x64", "p2-grid-1x4x512"]

MUTANTS = {
    # 1. moments as one-pass sums shifted by x[:, 0] (fp32, the kernel's grouping): the kernel before the fix
    "shift_x0": (FAM(G.OUTLIER_FAMILIES), lambda t: G.chain(t, moments="x0")),
    # 2. LayerNorm divisor K instead of k_real
    "divisor_K": (PADDED, lambda t: G.chain(t, F64, divisor=t["K"])),
    # 3. the (0 - shift) terms of the zero-padded columns left in the shifted sums
    "pad_correction": (PADDED, lambda t: G.chain(t, F64, moments="tile", pad_fix=False)),
    # 4. eps 1e-6 instead of 1e-5
    "eps_1e-6": (FAM(("lowvar",)), lambda t: G.chain(t, F64, eps=1e-6)),
    # 5. FiLM row of the neighbouring clip on the last frame of every clip
    "film_neighbour": ([n for n in G.CASES if n.startswith("p2-clips-")] + FAM(("plain", "out300"), ("p2",)) + ["side-512"],
                       lambda t: G.chain(t, F64, film_rows=G.neighbour_rows(t))),
    # 6. one K tile dropped (the last one)
    "dropped_tile": (SOME_GRID + ["p1-seg-512_256_128_128-999-act1", "p2-stats-4x256", "p0-act2-res1-alias1"], lambda t: G.chain(t, F64, drop_tile=t["K"] // 32 - 1)),
    # 7. two equal-width concat segments (128 | 128) swapped
    "segments_swapped": (["p1-seg-512_256_128_128-999-act0", "p1-seg-512_256_128_128-999-act1"], lambda t: G.chain(t, F64, swap=(768, 896, 128))),
    # 8. fc (the row sums of the folded weight) taken from the unfolded weight
    "fc_unfolded": ([n for n in G.CASES if n.startswith(("p1-seg-", "p1-fam-plain", "p1-fam-off", "p1-fam-out300"))] + SOME_GRID[2:4],
                    lambda t: G.chain(t, F64, fc=F.pad(t["W"], (0, t["K"] - t["k_real"])).double().sum(1))),
    # 9. stat_gs off by a factor 2 in the combination of the group moments (one group has nothing to combine: G >= 2)
    "stat_gs_x2": ([n for n in G.CASES if n.startswith(("p2-stats-", "side-")) and not n.startswith("p2-stats-1x")], lambda t: G.chain(t, F64, gs_factor=2.0)),
}


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (names, _) in MUTANTS.items() for n in names])
def test_mutants_are_rejected(mutant, name):
    t = G.case(name)
    assert _rejected(t, MUTANTS[mutant][1](t).float()), f"{mutant} passes the gate of {name}"


@pytest.mark.parametrize("name", FAM(("plain", "off+50", "off-200")))
def test_first_element_shift_is_invisible_without_an_outlier_column(name):
    """The whole-row offsets (the cases the tests had before) are absorbed by x[:, 0]: mutant 1 passes the gate there."""
    t = G.case(name)
    assert G.check(t, G.chain(t, moments="x0")) <= G.MARGIN


def test_first_element_shift_costs_orders_of_magnitude_on_rstd():
    """rstd of the two shifts against fp64 on the outlier rows (K = 512, column 0 = 300): x[0] ~1e-4, first-tile mean at round-off."""
    t = G.case("p1-fam-out300-512")
    _, r64 = G.two_pass(t["X"].double())
    err = {s: float((G.onepass_moments(t["Xp"], 512, s)[1].double() / r64 - 1).abs().max()) for s in ("x0", "tile")}
    assert err["x0"] > 1e-5 and err["tile"] < 1e-6, err


@pytest.mark.parametrize("sty", [False, True])
@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("T", [1, 2, 32, 37, 64])
def test_attention_mutants_are_rejected(T, family, sty):
    t = G.attn_inputs(3, T, family, sty)
    # 10. the time-softmax (and A = k^T v) over T + 1 frames (with one frame of k at + 40 every other frame weighs e^-40: the saturated
    #     softmax is one-hot with or without the extra frame, the mutant computes the same function there)
    if family != "k_sat":
        assert _rejected(t, G.attn_chain(t, F64, extra_frame=True)[:3].reshape(-1, 512).float())
    if sty:
        # 11. row moments over one head instead of eight; and the FiLM row of the neighbouring clip
        assert _rejected(t, G.attn_chain(t, F64, moment_heads=1)[:3].reshape(-1, 512).float())
        assert _rejected(t, G.attn_chain(t, F64, film_rows=(torch.arange(G.CAL_CLIPS) + 1) % 3)[:3].reshape(-1, 512).float())


def test_worst_element_report_names_tile_clip_and_frame():
    t = G.case("p2-clips-11x7")
    out = G.chain(t)[:t["M"]].clone()
    out[133, 70] += 1.0
    with pytest.raises(AssertionError, match=r"row 133 col 70 \(row % 32 = 5, col % 32 = 6, clip 5, frame 1\)"):
        G.check(t, out)
    out[133, 70] = float("nan")
    with pytest.raises(AssertionError, match="row 133 col 70"):
        G.check(t, out)
