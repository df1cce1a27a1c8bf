"""The gates of gemm_gates.py, tested without a GPU on the operands and cases of the GPU tests:
(a) three emulated fp32 summation orders - the K-split kernel's, the GEMV's lane-and-butterfly order and two products per accumulation
    step - pass the gate of every fp32 case, and the reversed chain passes every case;
(b) subtly wrong kernels are rejected on every case they apply to (all of them computed in float64, so that nothing but the fault
    separates them from the reference);
(c) the case list is what it says: every case is dispatched to the kernel family it was written for, the integer cases have an exact
    answer in both dtypes, and no allowance exceeds the worst-case bound of an fp32 accumulation.
"""
import pytest
import torch

import gemm_gates as G

RANDOM = [n for n in G.CASES if not G.CASES[n].get("ints")]
INTS = [n for n in G.CASES if G.CASES[n].get("ints")]


def _rejected(t, outs):
    try:
        G.check(t, outs)
    except AssertionError:
        return True
    return False


# ---- (c) the case list ------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_it_names():
    assert 300 <= len(G.CASES) <= 700, len(G.CASES)
    fams = {}
    for n, kw in G.CASES.items():
        fam, pick = G.expected_launch(kw["M"], kw["N"], kw["K"], kw["dtype"])
        assert fam == kw["family"], (n, fam)
        assert pick in (None, 2) or n.startswith("tiled-128rule"), (n, pick)
        fams.setdefault((fam, kw["dtype"]), []).append(kw)
    assert set(fams) == {("gemv", 0), ("gemv", 1), ("ksplit", 0), ("tiled", 0), ("tiled", 1)}
    assert G.expected_launch(300, 8192, 1024, G.BF16) == ("tiled", 0)
    for dt in (G.F32, G.BF16):
        # every M, N and K of the grids survives the thinning
        gv = [kw for kw in fams[("gemv", dt)]]
        assert {kw["M"] for kw in gv} >= set(G.GEMV_M) and {kw["N"] for kw in gv} >= set(G.GEMV_N) and {kw["K"] for kw in gv} >= set(G.GEMV_K[dt]) | {8192}
        tl = [kw for n, kw in G.CASES.items() if n.startswith("tiled-") and kw["dtype"] == dt]
        assert {kw["M"] for kw in tl} >= set(G.TILED_M[dt]) and {kw["N"] for kw in tl} >= set(G.TILED_N)
        assert {kw["K"] // G.KTILE[dt] for kw in tl} >= {1, 2, 3}
        # 7, 8 and 9 row tiles at either tile height (fp32 below 513 rows is tiled under DSH_GEMM_KSPLIT=0 only), and in every setting
        # the row counts on either side of the XCD ordering switch at 8 tiles
        seen = {64: set(), 128: set()}
        for setting, env in G.SETTINGS.items():
            here = set()
            for kw in G.CASES.values():
                fam, pick = G.expected_launch(kw["M"], kw["N"], kw["K"], dt, env)
                if kw["dtype"] == dt and fam == "tiled":
                    here.add(-(-kw["M"] // G.TILE_BM[pick]))
            seen[G.TILE_BM[G.expected_launch(600, 100, 1024, dt, env)[1]]] |= here
            assert min(here) < 8 <= max(here) or (dt == G.F32 and setting not in ("ksplit0", "tile0", "tile2", "variant0")), (dt, setting, sorted(here))
        assert seen[64] >= {7, 8, 9} and seen[128] >= {7, 8, 9}, (dt, seen)
    ks = fams[("ksplit", 0)]
    assert {kw["M"] for kw in ks} >= set(G.KS_M) and {kw["N"] for kw in ks} >= set(G.KS_N) and {kw["K"] for kw in ks} >= set(G.KS_K)
    # the GEMV's limits: at the limit on the GEMV, one K tile further off it; DSH_GEMV=0 takes every case off it
    assert G.expected_launch(4, 16, 8192, 0)[0] == G.expected_launch(16, 16, 2048, 1)[0] == "gemv"
    assert G.expected_launch(4, 16, 8192 + 32, 0)[0] == "ksplit" and G.expected_launch(16, 16, 2048 + 64, 1)[0] == "tiled"
    assert all(G.expected_launch(kw["M"], kw["N"], kw["K"], kw["dtype"], G.SETTINGS["gemv0"])[0] != "gemv" for kw in G.CASES.values())
    assert all(G.expected_launch(kw["M"], kw["N"], kw["K"], kw["dtype"], G.SETTINGS["ksplit0"])[0] != "ksplit" for kw in G.CASES.values())


@pytest.mark.parametrize("name", INTS)
def test_integer_cases_are_exact_in_both_dtypes(name):
    t = G.case(name)
    ref = G.ref64(t)
    assert bool((ref == ref.round()).all()) and float(ref.abs().max()) <= 256, "every result is an integer a bf16 holds"
    assert float(G.accum_bound(t["X"], t["W"], 1).max()) * 2 ** 23 < 2 ** 24, "every partial sum is an integer an fp32 holds"
    assert G.check(t, G.outputs(t, G.chain32(t, reverse=True))) == 0.0
    wrong = ref.clone()
    wrong[t["M"] - 1, t["N"] - 1] += 1
    assert _rejected(t, G.outputs(t, wrong))


# ---- (a) emulations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RANDOM)
def test_emulations_pass_the_gate(name):
    t = G.case(name)
    ref, allow, cal = G.gate(t)
    assert 0 < allow <= float(G.accum_bound(t["X"], t["W"], t["K"]).min()), "the allowance is inside the worst case of an fp32 accumulation"
    assert allow < 1e-4 * max(1.0, float(ref.abs().max()))
    assert G.check(t, G.outputs(t, G.chain32(t, reverse=True))) <= 1.0
    if t["dtype"] == G.F32 and name not in G._BIG:
        for emu in (G.emulate_ksplit, G.emulate_gemv, G.emulate_pairs):
            assert G.check(t, G.outputs(t, emu(t)), f"{name} {emu.__name__}") <= 1.0


def test_emulated_orders_sit_inside_the_calibration():
    """the experiment the gate's docstring quotes: M 256, N 64, K 32 .. 2048, seeded randn operands"""
    for K in (32, 256, 1024, 2048):
        t = G.inputs(256, 64, K, G.F32)
        ref, allow, cal = G.gate(t)
        for emu in (G.emulate_ksplit, G.emulate_gemv, G.emulate_pairs):
            r = float((emu(t).double() - ref).abs().max()) / cal
            print(f"K = {K} {emu.__name__}: {r:.2f} of the calibration")
            assert r <= 1.0


# ---- (b) mutants ------------------------------------------------------------------------------------------------------------------------------
def _drop(t, cols):
    W = t["W"].clone()
    W[:, cols] = 0
    return G.ref64(t, W=W)


def _tile(t, i):
    kt = G.KTILE[t["dtype"]]
    return slice(i * kt, (i + 1) * kt)


def _clamp_leak(t):
    X, M = t["X"].clone(), t["M"]
    X[(M - 1) // 32 * 32:M] = X[M - 1]
    return G.ref64(t, X=X)


def _truncated(t):
    y = G.ref64(t)[:t["M"]].float()
    return {"cf": y if t["out"] == "both" else None, "ct": G.truncate_bf16(y)}


_nk = lambda t: t["K"] // G.KTILE[t["dtype"]]
_modded = lambda t: t["res_mod"] > 0 and t["M"] > t["res_mod"]
# name -> (applies to the case, the mutant's fp64 values or its outputs).  Two mutants need more than a handful of outputs to show: a single
# element can sit where the activation is linear (GELU at 8: act(y) + R = act(y + R)), and truncation is the rounding of half of all values.
MUTANTS = {
    "first K tile dropped": (lambda t: True, lambda t: _drop(t, _tile(t, 0))),
    "last K tile dropped": (lambda t: True, lambda t: _drop(t, _tile(t, _nk(t) - 1))),
    "tile 8 of the K-split order dropped": (lambda t: _nk(t) > 8, lambda t: _drop(t, _tile(t, 8))),
    "the GEMV's last step dropped at an odd step count": (lambda t: t["family"] == "gemv" and G.gemv_steps(t)[0] % 2 == 1,
                                                          lambda t: _drop(t, slice((G.gemv_steps(t)[0] - 1) * 64 * G.gemv_steps(t)[1], None))),
    "bias shifted by one column": (lambda t: t["N"] > 1, lambda t: G.ref64(t, bias=t["b"].roll(1))),
    "residual from m % (r + 1)": (_modded, lambda t: G.ref64(t, mod=t["res_mod"] + 1)),
    "residual from row m under res_mod": (_modded, lambda t: G.ref64(t, mod=0)),
    "activation on the wrong side of the residual": (lambda t: t["R"] is not None and t["act"] != 0 and t["M"] * t["N"] >= 16, lambda t: G.ref64(t, swap_act=True)),
    "rows of the last partial tile computed from row M - 1": (lambda t: (t["M"] - 1) % 32 >= 1, _clamp_leak),
    "Ct rounded by truncation": (lambda t: t["dtype"] == G.BF16 and t["out"] != "f" and t["M"] * t["N"] >= 16, _truncated),
}


@pytest.mark.parametrize("name", RANDOM)
def test_mutants_are_rejected(name):
    t = G.case(name)
    for mutant, (applies, fn) in MUTANTS.items():
        if applies(t):
            out = fn(t)
            assert _rejected(t, out if isinstance(out, dict) else G.outputs(t, out)), f"{mutant} passes the gate of {name}"


def test_every_mutant_meets_a_case_in_every_family_it_can():
    """no mutant is rejected for want of a case: each applies in every kernel family and dtype it is defined for"""
    for mutant, (applies, _) in MUTANTS.items():
        hit = {(kw["family"], kw["dtype"]) for n, kw in G.CASES.items() if not kw.get("ints") and applies(_shape_only(kw))}
        want = {("gemv", 0), ("gemv", 1), ("ksplit", 0), ("tiled", 0), ("tiled", 1)}
        if "GEMV" in mutant:
            want = {("gemv", 0), ("gemv", 1)}
        elif "Ct" in mutant:
            want = {("gemv", 1), ("tiled", 1)}
        assert hit >= want, (mutant, want - hit)


def _shape_only(kw):
    """the fields of a case the mutants' `applies` look at, without drawing operands"""
    res = kw.get("res", "none")
    return {"M": kw["M"], "N": kw["N"], "K": kw["K"], "dtype": kw["dtype"], "family": kw["family"], "act": kw.get("act", 0), "out": kw.get("out", "both"),
            "res_mod": int(res[3:]) if res.startswith("mod") else 0, "R": None if res == "none" else True}


def test_worst_element_report_names_the_tile():
    t = G.case("form-res-own-f32-40x100x288")
    y = G.chain32(t)
    y[37, 70] += 1.0
    with pytest.raises(AssertionError, match=r"row 37 col 70 \(row % 32 = 5, col % 32 = 6\)"):
        G.check(t, G.outputs(t, y))
