"""Round 6: two properties of the rolling register-stationary kernels (tl2.hip) at whole-chip token counts that must not change a bit of
the output: the rotated weight-stream order and the skipped zero-padded k steps of the concat row.
Reference ops: models/transformer.py:284-289,304-338 (feat_proj), :119-125 (q | k | v behind one LayerNorm)."""
import ctypes as C

import pytest
import torch

from diffsheg_amd import _lib

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


# (K, N, pro, act, residual planes, real concat width); token rows: several rounds of 128- and 256-token tiles with a ragged last one
CASES = [(1024, 1024, 3, 1, False, 999), (1024, 1024, 3, 1, False, 896), (1024, 512, 0, 0, True, 1024), (512, 1536, 1, 0, False, 512)]


@pytest.mark.parametrize("K,N,pro,act,res,kreal", CASES + [(512, 512, 2, 0, True, 512)])
def test_rotated_weight_stream_order_changes_no_bit(K, N, pro, act, res, kreal, monkeypatch):
    """Round 6: DSH_TL2_ROT — block b of a rolling tl2 launch starts its weight stream at tile (b / 8) % tiles instead of tile 0 (the
    32 CUs of an XCD no longer ask their L2 for the same weight lines at the same moment).  Tiles are independent: every bit must agree."""
    Mv, T, nb = (256 * 130 + 77) if K == 512 else (128 * 130 + 50), 88, 400
    d = "cuda:0"
    g = torch.Generator().manual_seed(K + N + pro + kreal + 1)
    X = torch.randn(Mv, K, generator=g) * 1.5 + 0.3
    W = torch.randn(N, K, generator=g) / K ** 0.5
    gam = 1 + 0.1 * torch.randn(K, generator=g); bet = 0.1 * torch.randn(K, generator=g)
    if pro == 3:
        X[:, kreal:] = 0; W[:, kreal:] = 0; gam[kreal:] = 0; bet[kreal:] = 0
    X, W, gam, bet = X.bfloat16().to(d), W.bfloat16().to(d), gam.to(d), bet.to(d)
    b = torch.randn(N, generator=g).to(d)
    R = torch.randn(Mv, N, generator=g).to(d) if res else None
    film = (0.3 * torch.randn(nb, 2 * K, generator=g)).to(d) if pro == 2 else None
    monkeypatch.setenv("DSH_TL2", "1"); monkeypatch.setenv("DSH_HILO", "1" if res else "0")
    outs = {}
    P = lambda t: None if t is None else _p(t)
    for rot in ("0", "1"):
        monkeypatch.setenv("DSH_TL2_ROT", rot)
        Cf = torch.full((Mv, N), float("nan"), device=d) if res else None
        Ct = torch.full((Mv, N), float("nan"), device=d, dtype=torch.bfloat16)
        _lib.check(_lib.lib().dsh_op_tl_linear(None, pro, _p(X), _p(W), _p(b), P(R), P(Cf), _p(Ct), Mv, N, act, _p(gam), _p(bet), P(film),
                                               kreal if pro == 3 else T, nb, K))
        torch.cuda.synchronize()
        assert _lib.lib().dsh_debug_last_tl_variant() in (1, 2)
        outs[rot] = (Ct.view(torch.int16).cpu(), None if Cf is None else Cf.view(torch.int32).cpu())
    assert torch.isfinite(outs["1"][0].view(torch.bfloat16).float()).all()
    assert torch.equal(outs["0"][0], outs["1"][0])
    if res:
        assert torch.equal(outs["0"][1], outs["1"][1])


@pytest.mark.parametrize("kreal", [896, 999])
def test_skipping_the_zero_padded_k_steps_changes_no_bit(kreal, monkeypatch):
    """Round 6: the rolling feat_proj.1 kernel does not multiply the trailing all-zero fragments of the concat row (8 for the expression
    encoder's 896 columns, 1 for the gesture encoder's 999; DSH_TL2_KSKIP=0: all 64 fragments as before)."""
    K = N = 1024
    Mv = 128 * 130 + 50
    d = "cuda:0"
    g = torch.Generator().manual_seed(kreal)
    X = torch.randn(Mv, K, generator=g) * 1.5 + 0.3
    W = torch.randn(N, K, generator=g) / K ** 0.5
    gam = 1 + 0.1 * torch.randn(K, generator=g); bet = 0.1 * torch.randn(K, generator=g)
    X[:, kreal:] = 0; W[:, kreal:] = 0; gam[kreal:] = 0; bet[kreal:] = 0
    X, W, gam, bet = X.bfloat16().to(d), W.bfloat16().to(d), gam.to(d), bet.to(d)
    b = torch.randn(N, generator=g).to(d)
    monkeypatch.setenv("DSH_TL2", "1"); monkeypatch.setenv("DSH_HILO", "0")
    outs = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("DSH_TL2_KSKIP", sw)
        Ct = torch.full((Mv, N), float("nan"), device=d, dtype=torch.bfloat16)
        _lib.check(_lib.lib().dsh_op_tl_linear(None, 3, _p(X), _p(W), _p(b), None, None, _p(Ct), Mv, N, 1, _p(gam), _p(bet), None, kreal, 1, K))
        torch.cuda.synchronize()
        assert _lib.lib().dsh_debug_last_tl_variant() == 1
        outs[sw] = Ct.view(torch.int16).cpu()
    assert torch.isfinite(outs["1"].view(torch.bfloat16).float()).all()
    assert torch.equal(outs["0"], outs["1"])
