"""fp32 linear attention at the edges of its tiles, against fp64 (gates: tests/f32_gates.py, every element).

dsh_op_linear_attention (D = 512, eight 64-channel heads) instantiates linear_attention_f32_mfma_kernel for 32, 36, 64 and 96 frames and
leaves longer windows to the VALU loop kernel: the window lengths here sit on both sides of 32 | 33, 36 | 37, 64 | 65 and 96 | 97, with
odd lengths (the kernel walks the frames in pairs) and the one- and two-frame windows.  dsh_op_linear_attention_ragged variant 2 WITHOUT
lengths is the attention + StylizationBlock front of BASELINE configs[1] (linear_attention_f32_mfma_sty_kernel<false, .>: LayerNorm over the
eight heads -> xhat scale' + shift' -> SiLU, one FiLM row per clip); it serves up to 64 frames and must refuse 65 without writing.
(The library counts launches per family for the GEMMs and the bf16 attention only: there is no counter to assert the fp32 attention family
with, so the kernel choice is pinned by the window lengths alone.)

Guards: the rows behind the last clip are NaN in the input and f32_gates.SENTINEL in the output."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
import f32_gates as G  # noqa: E402

DEV = "cuda:0"
GUARD = 8


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _buffers(t):
    nb, T = t["nb"], t["T"]
    q = torch.full((nb * T + GUARD, 1536), float("nan"))
    q[:nb * T] = t["qkv"][:nb, :T].reshape(nb * T, 1536)
    return q.to(DEV), torch.full((nb * T + GUARD, 512), G.SENTINEL, device=DEV)


def _gate(t, out, what):
    n = t["nb"] * t["T"]
    out = out.cpu()
    assert bool((out[n:] == G.SENTINEL).all()), f"{what}: rows behind the last clip were written"
    r, cal = G.ratio(t, out)
    print(f"[{what}] kernel / calibration = {r:.2f} (calibration {cal:.2e})")
    G.check(t, out, what)


@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("T", G.ATTN_T)
def test_f32_attention_at_its_tile_edges(T, nb, family):
    t = G.attn_inputs(nb, T, family)
    q, out = _buffers(t)
    _lib.check(_lib.lib().dsh_op_linear_attention(None, _p(q), nb, T, 512, 64, _p(out)))
    torch.cuda.synchronize()
    _gate(t, out, f"attention T={T} nb={nb} {family}")


@pytest.mark.parametrize("family", G.ATTN_FAMILIES)
@pytest.mark.parametrize("T", G.ATTN_STY_T)
def test_f32_attention_with_the_stylization_front_without_lengths(T, family):
    nb = 3
    t = G.attn_inputs(nb, T, family, sty=True)
    q, out = _buffers(t)
    film = t["film"][:nb].contiguous().to(DEV)             # three distinct rows: clip b takes row b
    _lib.check(_lib.lib().dsh_op_linear_attention_ragged(None, 0, 2, _p(q), nb, T, 512, 64, _p(out), None, 0, _p(film)))
    torch.cuda.synchronize()
    _gate(t, out, f"attention + StylizationBlock front T={T} {family}")


def test_stylization_front_refuses_more_than_64_frames():
    nb, T = 3, 65
    t = G.attn_inputs(nb, T, "plain", sty=True)
    q, out = _buffers(t)
    film = t["film"][:nb].contiguous().to(DEV)
    rc = _lib.lib().dsh_op_linear_attention_ragged(None, 0, 2, _p(q), nb, T, 512, 64, _p(out), None, 0, _p(film))
    torch.cuda.synchronize()
    assert rc == -1, rc
    assert bool((out == G.SENTINEL).all()), "a refused call wrote to its output"
