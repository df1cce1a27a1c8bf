"""Worker of tests/test_gpu_gemm.py: runs the shared case list of tests/gemm_gates.py through dsh_op_gemm_ex and writes every output buffer
and the launch counters of every case to argv[1].  DSH_GEMM_TILE, DSH_GEMM_VARIANT, DSH_GEMV and DSH_GEMM_KSPLIT are read once per process,
so the test starts one fresh worker per setting; run_case() is also what the in-process tests launch with.

Guards around every launch: the input rows behind M and the columns K .. lda - 1 of A are NaN (the kernels clamp rows to M - 1 and must never
read them), every output buffer has GUARD rows of gemm_gates.SENTINEL behind M, the columns N .. ld - 1 of every output row hold SENTINEL
when ld > N, and so does the other half of the wide Ct buffer of the column-slice form."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from diffsheg_amd import _lib  # noqa: E402
import gemm_gates as G  # noqa: E402

DEV = "cuda:0"
GUARD = G.GUARD
COUNTERS = ("gemv", "gemm_f32_fewrow", "gemm_f32_tiled", "gemm_bf16_tiled", "gemm_tile_pick")


def call(dtype, A, W, bias, R, Cf, Ct, M, N, K, act, lda, ldw, ldr, res_mod, ldcf, ldct, act_after_res):
    """dsh_op_gemm_ex on raw device addresses (int or None); returns the status"""
    p = lambda v: None if v is None else C.c_void_p(v)
    return _lib.lib().dsh_op_gemm_ex(None, dtype, p(A), p(W), p(bias), p(R), p(Cf), p(Ct), M, N, K, act, lda, ldw, ldr, res_mod, ldcf, ldct, act_after_res)


class Buf:
    """[rows, ld] of `dtype` filled with `fill`, `shift` bytes into a flat allocation (shift 0: 256-byte aligned, as the allocator returns it)"""

    def __init__(self, rows, ld, fill, dtype=torch.float32, shift=0):
        es = torch.empty((), dtype=dtype).element_size()
        assert shift % es == 0
        self.flat = torch.full((rows * ld + 16,), fill, dtype=dtype, device=DEV)
        self.view = self.flat[shift // es:shift // es + rows * ld].view(rows, ld)
        self.ptr = self.flat.data_ptr() + shift

    def put(self, x, col=0):
        self.view[:x.shape[0], col:col + x.shape[1]] = x.to(self.view.dtype).to(DEV)
        return self


def run_case(t, M=None, shift=0, check=True):
    """One launch of the case on its first M rows (default: the case's M).  shift: bytes by which bias, R, Cf and Ct are moved off their
    alignment.  Returns {"cf", "ct": the WHOLE buffers, guard rows and padding columns included, or None; "rc"}, on the CPU."""
    M = t["M"] if M is None else M
    N, K, dt = t["N"], t["K"], t["dtype"]
    tt = torch.float32 if dt == G.F32 else torch.bfloat16
    nan = float("nan")
    A = Buf(M + GUARD, t["lda"], nan, tt).put(t["X"][:M, :K])
    W = Buf(N, K, nan, tt).put(t["W"])
    bias = Buf(1, N, nan, shift=shift).put(t["b"][None, :])
    cf = Buf(M + GUARD, t["ldcf"], G.SENTINEL, shift=shift) if t["out"] != "t" else None
    ct = Buf(M + GUARD, t["ldct"], G.SENTINEL, tt, shift=shift) if t["out"] != "f" else None
    R = None
    if t["res"] == "alias":
        R = cf.put(t["R"][:M])                              # in place, as the residual stream is updated
    elif t["res"] == "own":
        R = Buf(M + GUARD, t["ldr"], nan, shift=shift).put(t["R"][:M])
    elif t["res_mod"]:
        R = Buf(t["res_mod"], t["ldr"], nan, shift=shift).put(t["R"][:t["res_mod"]])
    es = 4 if dt == G.F32 else 2
    rc = call(dt, A.ptr, W.ptr, bias.ptr, R.ptr if R else None, cf.ptr if cf else None, ct.ptr + t["ct_col"] * es if ct else None, M, N, K, t["act"],
              t["lda"], K, t["ldr"], t["res_mod"], t["ldcf"], t["ldct"], t["act_after_res"])
    if check:
        _lib.check(rc)
    torch.cuda.synchronize()
    return {"cf": cf.view.cpu() if cf else None, "ct": ct.view.cpu() if ct else None, "rc": rc}


def split(t, res, M=None):
    """(the outputs {"cf", "ct"}: [M, N] each, everything else of the two buffers as one flat tensor per buffer) of run_case's result"""
    M = t["M"] if M is None else M
    N, c0 = t["N"], t["ct_col"]
    outs, rest = {"cf": None, "ct": None}, {}
    if res["cf"] is not None:
        outs["cf"] = res["cf"][:M, :N]
        rest["cf"] = torch.cat((res["cf"][:M, N:].reshape(-1), res["cf"][M:].reshape(-1)))
    if res["ct"] is not None:
        outs["ct"] = res["ct"][:M, c0:c0 + N]
        rest["ct"] = torch.cat((res["ct"][:M, :c0].reshape(-1), res["ct"][:M, c0 + N:].reshape(-1), res["ct"][M:].reshape(-1)))
    return outs, rest


def sentinels_intact(rest):
    return all(bool((v == torch.tensor(G.SENTINEL, dtype=v.dtype)).all()) for v in rest.values())


if __name__ == "__main__":
    outs = {}
    for name, kw in G.CASES.items():
        t = G.inputs(**kw)                                 # (not through the cache: the worker needs each case once)
        _lib.launch_counts(reset=True)
        res = run_case(t)
        got = _lib.launch_counts()
        res["counts"] = {k: int(got[k]) for k in COUNTERS}
        outs[name] = res
    torch.save(outs, sys.argv[1])
    print("GEMM_WORKER_OK", len(outs))
