"""Worker of tests/test_gpu_gemm_f32_pro.py: runs the shared case list of tests/f32_gates.py (and the three launches of the first
bit-identity test) through gemm_f32_pro.hip and writes the outputs to argv[1].  DSH_GP_DMA is read once per process, so the test starts
one fresh worker per value; run_case() is also what the in-process tests launch with.

Guards around every launch: the input rows behind M are NaN (the kernel clamps rows to M - 1 and must never read them) and every output
buffer has 8 rows behind M filled with f32_gates.SENTINEL, which must come back untouched."""
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
import f32_gates as G  # noqa: E402

P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
DEV = "cuda:0"
GUARD = 8


def _rows(x, M, fill=float("nan")):
    """the first M rows of x on the device, GUARD rows of `fill` behind them"""
    out = torch.full((M + GUARD,) + tuple(x.shape[1:]), fill, dtype=torch.float32)
    out[:M] = x[:M]
    return out.to(DEV)


def _sentinel(M, *shape):
    return torch.full((M + GUARD,) + shape, G.SENTINEL, device=DEV)


def _launch(pro, segs, k_real, W, bias, fc, film, film_ld, film_off, frames, nb, R, out, M, N, act, stats, groups, stats_out):
    a = []
    for s, ld, w in segs:
        a += [P(s), ld, w]
    _lib.check(_lib.lib().dsh_op_gemm_f32_pro(None, pro, *a, k_real, P(W), P(bias), P(fc), P(film), film_ld, film_off, frames, nb, P(R), P(out), M, N, act,
                                              P(stats), groups, P(stats_out)))


_NOSEG = (None, 0, 0)


def run_pro0(t):
    M, N, K = t["M"], t["N"], t["K"]
    X, W, b = _rows(t["X"], M), t["W"].to(DEV), t["b"].to(DEV)
    out = _sentinel(M, N)
    R = None
    if t["R"] is not None and t["alias"]:
        out[:M] = t["R"][:M].to(DEV)
        R = out                                             # in place, as the residual stream is updated
    elif t["R"] is not None:
        R = _rows(t["R"], M)
    st = _sentinel(M, N // 32, 2) if t["stats_out"] else None
    _launch(0, [(X, K, K), _NOSEG, _NOSEG, _NOSEG], K, W, b, None, None, 0, 0, 1, 1, R, out, M, N, t["act"], None, 0, st)
    return out, st


def run_pro2(t, x=None, stats=None):
    """x / stats: device tensors of a producer launch (the side channel); default: the case's rows and its host-built group moments"""
    M, N, K = t["M"], t["N"], t["K"]
    X = _rows(t["X"], M) if x is None else x
    if stats is None and t["stat_groups"]:
        stats = _rows(t["stats"], M)
    film, W, b = t["film"].to(DEV), t["W"].to(DEV), t["b"].to(DEV)
    out = _sentinel(M, N)
    R = None
    if t["R"] is not None:
        out[:M] = t["R"][:M].to(DEV)
        R = out
    _launch(2, [(X, K, K), _NOSEG, _NOSEG, _NOSEG], K, W, b, None, film, film.shape[1], t["film_off"], t["frames"], t["nb"], R, out, M, N, 0,
            stats, t["stat_groups"] if stats is not None else 0, None)
    return out


def run_case(t):
    """{"y": [M + GUARD, N]} (+ "stats" of a PRO 0 launch with stats_out; + "y2", "stats" of the side channel's producer), on the CPU"""
    M, N = t["M"], t["N"]
    res = {}
    if t["kind"] == "pro0":
        out, st = run_pro0(t)
        if st is not None:
            res["stats"] = st
    elif t["kind"] == "pro1":
        segs = []
        for s, w in zip(G.pro1_segments(t, M), t["widths"]):
            segs.append(_NOSEG if s is None else (_rows(s, M), w + t["ld_extra"], w))
        out = _sentinel(M, N)
        _launch(1, segs, t["k_real"], t["Wf"].to(DEV), t["fd"].to(DEV), t["fc"].to(DEV), None, 0, 0, 1, 1, None, out, M, N, t["act"], None, 0, None)
    elif t["kind"] == "pro2":
        out = run_pro2(t)
    elif t["kind"] == "side":
        y2, st = run_pro0(t["prod"])
        out = run_pro2(t, x=y2, stats=st)
        res["y2"], res["stats"] = y2, st
    else:
        raise ValueError(t["kind"])
    res["y"] = out
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def legacy_cases():
    """The three launches of the first form of this worker (M = 1037; seeded operands): PRO 0 with the residual in place, PRO 1 over four
    concat segments with 13 padded columns and a REAL fold (fc = row sums of gamma (.) W), PRO 2 with 31 FiLM rows."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    M, d = 1000 + 37, DEV
    outs = {}
    A, W, b, R = torch.randn(M, 1024, generator=g), torch.randn(512, 1024, generator=g) / 32, torch.randn(512, generator=g), torch.randn(M, 512, generator=g)
    Ad, Wd, bd, o = A.to(d), W.to(d), b.to(d), R.to(d)
    _lib.check(L.dsh_op_gemm_f32_pro(None, 0, P(Ad), 1024, 1024, None, 0, 0, None, 0, 0, None, 0, 0, 1024, P(Wd), P(bd), None, None, 0, 0, 1, 1, P(o), P(o), M, 512, 0, None, 0, None))
    outs["pro0"] = o.cpu()
    segs = [torch.randn(M, w, generator=g) for w in (512, 256, 128, 64)]
    segs[3][:, 51:] = 0
    W1, b1 = torch.randn(1024, 947, generator=g) / 31, torch.randn(1024, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(947, generator=g), 0.3 * torch.randn(947, generator=g)
    Wf, fc, fd = G.fold(W1, b1, gamma, beta, 960)
    sd = [x.to(d) for x in segs]
    W1d, b1d, fcd = Wf.to(d), fd.to(d), fc.to(d)
    o1 = torch.empty(M, 1024, device=d)
    _lib.check(L.dsh_op_gemm_f32_pro(None, 1, P(sd[0]), 512, 512, P(sd[1]), 256, 256, P(sd[2]), 128, 128, P(sd[3]), 64, 64, 947, P(W1d), P(b1d), P(fcd), None, 0, 0, 1, 1, None, P(o1),
                                     M, 1024, 1, None, 0, None))
    outs["pro1"] = o1.cpu()
    X = torch.cat(segs, 1)[:, :947]
    outs["pro1_ref64"] = torch.nn.functional.silu(torch.nn.functional.layer_norm(X.double(), (947,), gamma.double(), beta.double(), 1e-5) @ W1.double().T + b1.double())
    y, film = torch.randn(M, 512, generator=g) * 2, torch.randn(31, 1024, generator=g)
    W2, b2 = torch.randn(512, 512, generator=g) / 23, torch.randn(512, generator=g)
    yd, fd_, W2d, b2d, o2 = y.to(d), film.to(d), W2.to(d), b2.to(d), R.to(d)
    _lib.check(L.dsh_op_gemm_f32_pro(None, 2, P(yd), 512, 512, None, 0, 0, None, 0, 0, None, 0, 0, 512, P(W2d), P(b2d), None, P(fd_), 1024, 0, 34, 31, P(o2), P(o2), M, 512, 0, None, 0, None))
    outs["pro2"] = o2.cpu()
    torch.cuda.synchronize()
    return outs


if __name__ == "__main__":
    outs = {"legacy": legacy_cases()}
    for name in G.CASES:
        fn, a, kw = G.CASES[name]                          # (not through the cache: the worker needs each case once)
        t = fn(*a, **kw)
        outs[name] = run_case(t)
    torch.save(outs, sys.argv[1])
    print("GP_DMA_WORKER_OK", os.environ.get("DSH_GP_DMA"), len(outs))
