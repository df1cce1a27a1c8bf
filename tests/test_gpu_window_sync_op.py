"""dsh_op_window_sync (synchronised window batches) against its restatement in eager torch on the device, bit for bit:
eager torch rounds every op on its own, the kernel does the same (rn_mul / rn_add / rn_sub), and its weights are torch.linspace's.
B = 5 rows of 12 frames, 7 channels, two streams (rows 0-2 and 3-4), with and without per-row lengths, every column-window form."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
from synchronised_ref import copies_equal, shared_pairs, window_sync  # noqa: E402

DEV = "cuda:0"
B, T, CH = 5, 12, 7
LEFT = [-1, 0, 1, -1, 3]
LENS = [12, 12, 7, 12, 11]
COLS = [(0, 0), (3, 7), (0, 3)]


def _op(x, left, L, lens=None, cols=(0, 0), left_dev=None, lens_dev=None, frames=None):
    """rc of dsh_op_window_sync on x (in place); the device copies default to the host values"""
    Bx, Tx, Cx = x.shape
    la = (C.c_int32 * len(left))(*left)
    ld = torch.tensor(left if left_dev is None else left_dev, dtype=torch.int32, device=DEV)
    na = nd = None
    if lens is not None:
        na = (C.c_int32 * len(lens))(*lens)
        nd = torch.tensor(lens if lens_dev is None else lens_dev, dtype=torch.int32, device=DEV)
    rc = _lib.lib().dsh_op_window_sync(None, x.data_ptr(), Bx, Tx if frames is None else frames, Cx, la, ld.data_ptr(), na,
                                       None if nd is None else nd.data_ptr(), L, cols[0], cols[1])
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("L", [1, 2, 5, 6])
@pytest.mark.parametrize("cols", COLS, ids=lambda c: f"cols{c[0]}_{c[1]}")
def test_window_sync_equals_eager_torch_bit_for_bit(L, cols):
    lens = LENS if L <= 3 else None
    g = torch.Generator().manual_seed(100 + L)
    x0 = torch.randn(B, T, CH, generator=g).to(DEV)
    x = x0.clone()
    assert _op(x, LEFT, L, lens, cols) == 0, _lib.lib().dsh_last_error()
    want = window_sync(x0, LEFT, L, lens, *cols)
    assert torch.equal(_bits(x), _bits(want)), (L, cols, float((x - want).abs().max()))
    # every element outside the shared regions and outside the column window keeps its bits
    touched = torch.zeros(B, T, CH, dtype=torch.bool, device=DEV)
    cs = slice(None) if cols == (0, 0) else slice(*cols)
    for p, sp, b, sb in shared_pairs(LEFT, L, lens, T):
        touched[p, sp, cs] = True
        touched[b, sb, cs] = True
    assert touched.any() and torch.equal(_bits(x)[~touched], _bits(x0)[~touched])
    # the two copies of every shared frame are equal inside the column window (and were not before)
    for p, sp, b, sb in shared_pairs(LEFT, L, lens, T):
        assert torch.equal(_bits(x[p, sp, cs]), _bits(x[b, sb, cs]))
        assert not torch.equal(x0[p, sp, cs], x0[b, sb, cs])
    if cols == (0, 0):
        assert copies_equal(x, LEFT, L, lens)
    if L > 1 and cols == (0, 0):          # w = 0 at the left window's interior end, 1 at the right window's
        n0 = (lens or [T] * B)[0]
        assert torch.equal(x[0, n0 - L], x0[0, n0 - L]) and torch.equal(x[1, L - 1], x0[1, L - 1])


def test_no_left_neighbour_changes_nothing():
    x0 = torch.randn(B, T, CH, generator=torch.Generator().manual_seed(1)).to(DEV)
    for lens in (None, LENS):
        x = x0.clone()
        assert _op(x, [-1] * B, 3, lens) == 0
        assert torch.equal(_bits(x), _bits(x0))


def test_more_than_one_block_and_a_cycle_of_rows():
    """1 200 rows of 34 frames, 192 channels (several grid strides of the launch) in chains of 4; and two rows that are each other's
    neighbour, which the conditions allow (both hold 2 L frames)."""
    Bb, Tb, Cb, L = 1200, 34, 192, 4
    left = [-1 if b % 4 == 0 else b - 1 for b in range(Bb)]
    x0 = torch.randn(Bb, Tb, Cb, generator=torch.Generator().manual_seed(2)).to(DEV)
    x = x0.clone()
    assert Bb * L * Cb > 2048 * 256
    assert _op(x, left, L) == 0
    assert torch.equal(_bits(x), _bits(window_sync(x0, left, L)))
    y0 = torch.randn(2, 12, CH, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = y0.clone()
    assert _op(y, [1, 0], 3) == 0
    assert torch.equal(_bits(y), _bits(window_sync(y0, [1, 0], 3))) and copies_equal(y, [1, 0], 3)


def test_refusals_leave_x_unchanged():
    lib = _lib.lib()
    x0 = torch.randn(B, T, CH, generator=torch.Generator().manual_seed(4)).to(DEV)
    cases = [
        (dict(left=[-1, 0, 5, -1, 3], L=3), b"outside the batch"),                       # an index out of range
        (dict(left=[-1, 0, -2, -1, 3], L=3), b"outside the batch"),
        (dict(left=[-1, 1, 1, -1, 3], L=3), b"own left neighbour"),                      # left[b] = b
        (dict(left=[-1, 0, 0, -1, 3], L=3), b"two rows"),                                # a duplicate left
        (dict(left=LEFT, L=0), b"overlap_len"),                                          # L < 1
        (dict(left=LEFT, L=-2), b"overlap_len"),
        (dict(left=LEFT, L=T + 1), b"overlap_len"),
        (dict(left=LEFT, L=3, lens=[12, 12, 2, 12, 11]), b"shorter than overlap_len"),   # a used row shorter than L (as a right row)
        (dict(left=LEFT, L=3, lens=[2, 12, 7, 12, 11]), b"shorter than overlap_len"),    # ... as a left row
        (dict(left=LEFT, L=3, lens=[12, 5, 7, 12, 11]), b"2 * overlap_len"),             # a two-sided row shorter than 2 L
        (dict(left=LEFT, L=5), None),                                                    # (allowed without lengths: 2 L <= 12)
        (dict(left=LEFT, L=7), b"2 * overlap_len"),                                      # two-sided row 1 of 12 frames, 2 L = 14
        (dict(left=LEFT, L=3, lens=[12, 13, 7, 12, 11]), b"beyond the frame count"),
        (dict(left=LEFT, L=3, cols=(2, 8)), b"channel range"),
        (dict(left=LEFT, L=3, cols=(-1, 3)), b"channel range"),
    ]
    for kw, frag in cases:
        x = x0.clone()
        rc = _op(x, **kw)
        if frag is None:
            assert rc == 0, kw
            continue
        assert rc == -1 and frag in lib.dsh_last_error(), (kw, lib.dsh_last_error())
        assert torch.equal(_bits(x), _bits(x0)), kw
    # lengths need both copies; the left neighbours too
    x = x0.clone()
    la = (C.c_int32 * B)(*LEFT)
    ld = torch.tensor(LEFT, dtype=torch.int32, device=DEV)
    na = (C.c_int32 * B)(*LENS)
    assert lib.dsh_op_window_sync(None, x.data_ptr(), B, T, CH, la, ld.data_ptr(), na, None, 3, 0, 0) == -1
    assert lib.dsh_op_window_sync(None, x.data_ptr(), B, T, CH, None, ld.data_ptr(), None, None, 3, 0, 0) == -1
    assert lib.dsh_op_window_sync(None, x.data_ptr(), B, T, CH, la, None, None, None, 3, 0, 0) == -1
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(x0))


def test_kernel_skips_rows_whose_device_copy_disagrees():
    """The host copy passes, the device copy names rows and lengths out of range: those rows are skipped (no address outside x is
    formed), the others are reconciled as usual."""
    x0 = torch.randn(B, T, CH, generator=torch.Generator().manual_seed(6)).to(DEV)
    x = x0.clone()
    assert _op(x, LEFT, 3, LENS, left_dev=[-1, 0, 7, -1, -9], lens_dev=LENS) == 0
    assert torch.equal(_bits(x), _bits(window_sync(x0, [-1, 0, -1, -1, -1], 3, LENS)))
    x = x0.clone()
    assert _op(x, LEFT, 3, LENS, lens_dev=[12, 12, 7, 400, -5]) == 0       # rows 3 / 4: their pair is skipped
    assert torch.equal(_bits(x), _bits(window_sync(x0, [-1, 0, 1, -1, -1], 3, LENS)))
    x = x0.clone()
    assert _op(x, LEFT, 3, LENS, left_dev=[-1, 0, 2, -1, 3]) == 0          # a row named as its own neighbour on the device
    assert torch.equal(_bits(x), _bits(window_sync(x0, [-1, 0, -1, -1, 3], 3, LENS)))
