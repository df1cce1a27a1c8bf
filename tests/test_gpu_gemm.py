"""The generic GEMM (diffsheg_amd/csrc/gemm.hip) through dsh_op_gemm_ex: every kernel family (weight-streaming GEMV, fp32 K-split, tiled), every
tile shape and the unswizzled form, and every epilogue form the callers use, against float64 on every element with the gates of
tests/gemm_gates.py.  The shared case list runs in one fresh worker process per latch setting (gemm_worker.py; the switches are read once per
process); each run is gated, its sentinels and launch counters are checked, and the runs are compared with each other bit for bit where the
code promises the same arithmetic.

Bit identity between tile shapes: every instantiation of gemm_nt_kernel walks the K tiles in ascending order with one accumulator per output
element and the same four (fp32: sixteen) matrix instructions per tile, and the unswizzled form only exchanges the two operands of each
instruction, so the outputs of DSH_GEMM_TILE=0 / 2 / 4 and DSH_GEMM_VARIANT=0 equal the default's on every tiled case."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
import gemm_gates as G  # noqa: E402
import gemm_worker as Wk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worker_runs(tmp_path_factory):
    """{setting: {case: {"cf", "ct", "counts"}}}: one fresh worker per latch setting, one after the other, each under a timeout; the first
    worker that does not exit 0 stops the fixture and none is started after it."""
    tmp = tmp_path_factory.mktemp("gemm")
    res = {}
    for setting, env in G.SETTINGS.items():
        f = str(tmp / f"gemm_{setting}.pt")
        clean = {k: v for k, v in os.environ.items() if k not in ("DSH_GEMM_TILE", "DSH_GEMM_VARIANT", "DSH_GEMV", "DSH_GEMM_KSPLIT")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_worker.py"), f], env=dict(clean, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "GEMM_WORKER_OK" in r.stdout, (setting, r.returncode, r.stdout[-500:], r.stderr[-2000:])
        res[setting] = torch.load(f)
    return res


def _same(a, b):
    bits = lambda v: v.contiguous().view(torch.uint8)
    return all((a[k] is None and b[k] is None) or torch.equal(bits(a[k]), bits(b[k])) for k in ("cf", "ct"))


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_list_in_every_latch_setting(name, worker_runs):
    """One case of gemm_gates.CASES in all seven settings: every element inside the gate against float64 (the integer cases bit-exact), every
    sentinel untouched, the launch counters naming the kernel family and tile pick the dispatch rules give, Ct the rounded Cf where both are
    stored, and the tiled forms bit-identical to the default."""
    t = G.case(name)
    assert set(worker_runs) == set(G.SETTINGS)
    outs = {}
    for setting, env in G.SETTINGS.items():
        res = worker_runs[setting][name]
        what = f"{name} [{setting}]"
        outs[setting], rest = Wk.split(t, res)
        want, pick = G.expected_counts(t, env)
        fam = G.expected_launch(t["M"], t["N"], t["K"], t["dtype"], env)[0]
        r, cal = G.ratio(t, outs[setting])
        print(f"[{what}] {fam}{'' if pick is None else f' pick {pick}'} kernel / calibration = {r:.2f} (calibration {cal:.2e})")
        assert Wk.sentinels_intact(rest), f"{what}: a guard row or a padding column was written"
        got = res["counts"]
        assert {k: got[k] for k in want} == want, (what, got, want)
        assert pick is None or got["gemm_tile_pick"] == pick, (what, got, pick)
        G.check(t, outs[setting], what)
    if t["family"] == "tiled":
        differ = [s for s in G.SETTINGS if not _same(outs["default"], outs[s])]
        assert not differ, f"{name}: tiled launches differ from the default in {differ}"


FORM_CASES = [n for n in G.CASES if n.startswith("form-ldcf+4-") or n.startswith("int-ldcf+4-")]


@pytest.mark.parametrize("name", FORM_CASES)
def test_scalar_epilogue_equals_the_vector_epilogue(name, worker_runs):
    """ldcf = N + 3 takes the scalar stores, ldcf = N + 4 the 16-byte ones: the same operands, the same bits, in every setting"""
    other = G.sibling(name, "ldcf+4", "ldcf+3")
    for setting in G.SETTINGS:
        a, _ = Wk.split(G.case(name), worker_runs[setting][name])
        b, _ = Wk.split(G.case(other), worker_runs[setting][other])
        assert _same(a, b), (name, other, setting)


@pytest.mark.parametrize("name", [n for n in G.CASES if n.startswith("form-res-alias-") or n.startswith("int-res-alias-")])
def test_residual_in_place_equals_a_residual_of_its_own(name, worker_runs):
    own = name.replace("-res-alias-", "-res-own-") if name.startswith("form-") else name.replace("int-res-alias-", "int-ldr+4-")
    for setting in G.SETTINGS:
        a, _ = Wk.split(G.case(name), worker_runs[setting][name])
        b, _ = Wk.split(G.case(own), worker_runs[setting][own])
        assert _same(a, b), (name, own, setting)


# ---- in-process tests (no latched switch is touched) --------------------------------------------------------------------------------------------
def test_rows_of_a_tiled_launch_do_not_depend_on_M():
    t = G.inputs(577, 100, 192, G.BF16, act=1, res="own")
    full, _ = Wk.split(t, Wk.run_case(t))
    _lib.launch_counts(reset=True)
    part, rest = Wk.split(t, Wk.run_case(t, M=130), M=130)
    assert _lib.launch_counts()["gemm_bf16_tiled"] == 1 and Wk.sentinels_intact(rest)
    assert _same({k: v[:130] for k, v in full.items()}, part)
    G.check(t, full, "M = 577")


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
@pytest.mark.parametrize("M,K", [(5, 512), (40, 320), (577, 192)])
@pytest.mark.parametrize("res", ["own", "alias", "mod11"])
def test_operands_off_their_alignment_give_the_same_bits(M, K, res, dtype):
    """bias, R, Cf and Ct one float (4 bytes) off a 16-byte boundary with N and every leading dimension a multiple of 4: the vector epilogue
    would make misaligned 16-byte (bf16 Ct: 8-byte) accesses, so the launch takes the scalar stores - the same bits as the aligned launch."""
    t = G.inputs(M, 104, K, dtype, act=1, res=res, ldcf_x=4, ldr_x=0 if res == "alias" else 8, ldct_x=4)
    aligned, _ = Wk.split(t, Wk.run_case(t))
    shifted, rest = Wk.split(t, Wk.run_case(t, shift=4))
    assert Wk.sentinels_intact(rest)
    assert _same(aligned, shifted)
    G.check(t, shifted, f"shifted M={M} K={K} {res}")


def test_refusals_launch_nothing():
    t = G.inputs(40, 104, 64, G.F32, res="own")
    M, N, K = t["M"], t["N"], t["K"]
    A, W = Wk.Buf(M, K + 32, 0.5), Wk.Buf(N, K + 32, 0.5)
    bias, R = Wk.Buf(1, N, 0.0), Wk.Buf(M, N, 0.0)
    Cf, Ct = Wk.Buf(M + 8, N, G.SENTINEL), Wk.Buf(M + 8, N, G.SENTINEL)
    good = dict(dtype=0, A=A.ptr, W=W.ptr, bias=bias.ptr, R=R.ptr, Cf=Cf.ptr, Ct=Ct.ptr, M=M, N=N, K=K, act=0, lda=K + 32, ldw=K + 32, ldr=N, res_mod=0, ldcf=N, ldct=N,
                act_after_res=0)
    refused = {
        "no output": dict(Cf=None, Ct=None), "ldcf below N": dict(ldcf=N - 4), "ldct below N": dict(ldct=N - 4), "ldr below N": dict(ldr=N - 4),
        "negative res_mod": dict(res_mod=-1), "unknown activation": dict(act=3), "negative activation": dict(act=-1), "unknown dtype": dict(dtype=2),
        "A off its alignment": dict(A=A.ptr + 4), "W off its alignment": dict(W=W.ptr + 4), "K no multiple of the K tile": dict(K=K - 16),
        "lda below K": dict(lda=K - 32), "ldw below K": dict(ldw=K - 32), "lda no 16-byte multiple": dict(lda=K + 33), "no rows": dict(M=0), "no columns": dict(N=0),
    }
    torch.cuda.synchronize()
    _lib.launch_counts(reset=True)
    for what, change in refused.items():
        assert Wk.call(**dict(good, **change)) == -1, what
        assert _lib.lib().dsh_last_error(), what
    assert set(_lib.launch_counts().values()) == {0}
    torch.cuda.synchronize()
    assert bool((Cf.flat == G.SENTINEL).all()) and bool((Ct.flat == G.SENTINEL).all())
    assert Wk.call(**good) == 0
    torch.cuda.synchronize()
    assert _lib.launch_counts()["gemm_f32_fewrow"] == 1 and bool((Cf.view[:M] == 0.5 * 0.5 * K).all()) and bool((Cf.view[M:] == G.SENTINEL).all())
