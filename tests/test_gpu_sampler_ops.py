"""The sampler's small kernels (sampler_kernels.hip) one launch at a time on a real MI355X, against the CPU references of small_ops_ref.py:
the Philox generator value by value (known-answer reference, derived gate, counter-layout identities bit for bit), the fused DDIM / DDPM /
undo steps with torch.equal against one-rounded-op-per-op fp32 expressions, the timestep-cache copy and the fills.

Every output buffer carries GUARD sentinel elements behind its last element; every element a launch must not write (outside the channel
window, behind n) is compared with what it held before."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import small_ops_ref as R  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402

DEV = "cuda:0"


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(t):
    """device copy of t (flattened) with GUARD sentinel elements behind it"""
    flat = torch.full((t.numel() + R.GUARD,), R.SENTINEL, dtype=t.dtype)
    flat[:t.numel()] = t.reshape(-1)
    return flat.to(DEV)


def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, R.SENTINEL, dtype=dtype)


def _split(buf, shape):
    """(payload reshaped, guard intact) of a guarded device buffer"""
    n = int(np.prod(shape))
    h = buf.cpu()
    return h[:n].reshape(shape), bool((h[n:] == R.SENTINEL).all()) and h.numel() == n + R.GUARD


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------
def _randn(n, seed, offset):
    out = _guarded(_sentinel((n,)))
    _lib.check(_lib.lib().dsh_op_philox_randn(None, _p(out), n, seed, offset), "dsh_op_philox_randn")
    torch.cuda.synchronize()
    z, ok = _split(out, (n,))
    assert ok, "philox_randn wrote behind n"
    return z


def _randn_rows(keys, n_row, seed, offset=0, lens=None, draw=0, channels=0):
    rows = len(keys)
    out = _guarded(_sentinel((rows * n_row,)))
    karr = (C.c_uint64 * rows)(*keys)
    larr = (C.c_int32 * rows)(*lens) if lens is not None else None
    _lib.check(_lib.lib().dsh_op_philox_randn_rows_ragged(None, _p(out), rows, n_row, seed, offset, karr, larr, draw, channels),
               "dsh_op_philox_randn_rows_ragged")
    z, ok = _split(out, (rows, n_row))
    assert ok, "philox_randn_rows wrote behind its rows"
    return z


def _gate(z, **kw):
    z_ref, r_ref = R.randn_ref(z.numel(), with_r=True, **kw)
    return R.philox_ratio(z.reshape(-1).numpy(), z_ref, r_ref)


def test_philox_values_match_the_known_answer_reference():
    g = R.philox_gate_g()
    worst = 0.0
    for n, seed, off in R.PHILOX_CASES:
        ratio = _gate(_randn(n, seed, off), seed=seed, offset=off)
        worst = max(worst, ratio)
        print(f"[philox] n {n} seed {seed:#x} offset {off}: worst |z - ref| / (2^-23 max(r, 2^-23)) = {ratio:.3f}  (G = {g:.3f}, gate {R.MARGIN * g:.3f})")
        assert ratio <= R.MARGIN * g, (n, seed, off, ratio)
    print(f"[philox] small cases: device ratio {worst:.3f} of calibration {g:.3f}")


def test_philox_second_grid_stride_trip_and_shift():
    g = R.philox_gate_g()
    n, k = R.PHILOX_BIG_N, 524288
    big = _randn(n, 42, 0)
    ratio = _gate(big, seed=42, offset=0)
    print(f"[philox] n {n} (second grid-stride trip, ragged last quad): device ratio {ratio:.3f}, G = {g:.3f}, gate {R.MARGIN * g:.3f}")
    assert ratio <= R.MARGIN * g
    # shift: randn(m, offset = k) is randn(m + 4 k, offset = 0)[4 k:], bit for bit — behind the first trip's 524 288 quads, and small ones
    assert torch.equal(_randn(n - 4 * k, 42, k), big[4 * k:])
    for m, kk in ((1027, 3), (5, 600), (1, 1)):
        assert torch.equal(_randn(m, 42, kk), big[4 * kk:4 * kk + m]), (m, kk)
    # the carry into the second counter word: offset 2^32 - 1 + one quad = offset 2^32
    seed = (0xDEADBEEF << 32) | 7
    a, b = _randn(12, seed, 2 ** 32 - 1), _randn(8, seed, 2 ** 32)
    assert torch.equal(a[4:], b)


def test_philox_row_streams():
    g = R.philox_gate_g()
    seed, n_row, off = (0x1234 << 32) | 77, 1028, 3
    keys = list(R.PHILOX_ROW_KEYS)
    z = _randn_rows(keys, n_row, seed, off)
    z_ref, r_ref = R.randn_ref(len(keys) * n_row, seed, off, row_keys=keys, n_row=n_row, with_r=True)
    ratio = R.philox_ratio(z.reshape(-1).numpy(), z_ref, r_ref)
    print(f"[philox rows] device ratio {ratio:.3f}, G = {g:.3f}")
    assert ratio <= R.MARGIN * g
    for b, key in enumerate(keys):
        assert torch.equal(_randn_rows([key], n_row, seed, off)[0], z[b]), b          # a row does not depend on its batch
    assert torch.equal(z[0], _randn(n_row, seed, off))                                  # key 0 = the whole-tensor stream
    assert len({tuple(z[b, :8].tolist()) for b in range(len(keys))}) == len(keys)
    # (seed + 1, key 0) and (seed, key 1) are different streams (XORing the key into the seed made them one)
    assert not torch.equal(_randn_rows([0], n_row, 43, 0)[0], _randn_rows([1], n_row, 42, 0)[0])
    # the pre-existing entry forwards to the same launch
    out = torch.empty(len(keys), n_row, device=DEV)
    _lib.check(_lib.lib().dsh_op_philox_randn_rows(None, _p(out), len(keys), n_row, seed, off, (C.c_uint64 * len(keys))(*keys)))
    assert torch.equal(out.cpu(), z)


@pytest.mark.parametrize("channels", [232, 192])
def test_philox_ragged_rows_draw_their_own_streams(channels):
    g = R.philox_gate_g()
    T, lens, keys, seed = R.RAGGED_T, list(R.RAGGED_LENS), list(R.PHILOX_ROW_KEYS), 42
    n_row = T * channels
    for draw in (0, 1, 5):
        z = _randn_rows(keys, n_row, seed, 0, lens, draw, channels)
        z_ref, r_ref = R.randn_ref(len(keys) * n_row, seed, 0, row_keys=keys, n_row=n_row, row_lens=lens, draw=draw, channels=channels, with_r=True)
        ratio = R.philox_ratio(z.reshape(-1).numpy(), z_ref, r_ref)
        print(f"[philox ragged] C {channels} draw {draw}: device ratio {ratio:.3f}, G = {g:.3f}")
        assert ratio <= R.MARGIN * g
        for b, (key, ln) in enumerate(zip(keys, lens)):
            m = ln * channels
            solo = _randn_rows([key], m, seed, draw * m // 4)
            assert torch.equal(solo[0], z[b, :m]), (draw, b)
    buf = torch.empty(8, device=DEV)
    rc = _lib.lib().dsh_op_philox_randn_rows_ragged(None, _p(buf), 1, 8, 1, 0, (C.c_uint64 * 1)(0), (C.c_int32 * 1)(3), 0, 4)
    assert rc < 0 and b"row length" in _lib.lib().dsh_last_error()


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def _ddim_launch(dev, t, L, combo, c_lo, c_hi, x0_on, shape):
    B, T, Cc = shape
    e, clip, mk, bl, tb, tails = combo
    k, eta, has_n1 = R.ETA_MODES[e]
    c1, c2, sab, s1m, coef, sigma = R.ddim_scalars(k, eta)
    mask = dev["masks"][mk]
    xd = dev["x_guarded"].clone()
    x0d = dev["sent_n"].clone() if x0_on else None
    td = dev["sent_tail"].clone() if tails else None
    _lib.check(_lib.lib().dsh_op_ddim_step_full(
        None, _p(xd), _p(dev["eps"]), _p(x0d), _p(dev["gt"]), _p(mask), _p(dev["nz2"]), _p(dev["nz1"]) if has_n1 else None,
        _p(dev["tail_in"]) if (tails and mask is not None) else None, _p(td), B, T, Cc, c1, c2, sab, s1m, coef, sigma, L, bl, tb, clip, c_lo, c_hi),
        "dsh_op_ddim_step_full")
    return xd, x0d, td


def _ddim_dev(t, L, shape):
    B, T, Cc = shape
    dev = {n: t[n].to(DEV) for n in ("eps", "gt", "nz1", "nz2", "tail_in")}
    dev["masks"] = {n: (m.to(torch.uint8).to(DEV) if m is not None else None) for n, m in t["masks"].items()}
    dev["x_guarded"] = _guarded(t["x"])
    dev["sent_n"] = _guarded(_sentinel((B, T, Cc)))
    dev["sent_tail"] = _guarded(_sentinel((B, L, Cc)))
    return dev


def _ddim_check(bufs, full, t, L, c_lo, c_hi, shape, what):
    B, T, Cc = shape
    xd, x0d, td = bufs
    want = R.ddim_expect(full, (t["x"], _sentinel((B, T, Cc)), _sentinel((B, L, Cc))), c_lo, c_hi)
    for name, buf, w, shp in (("x", xd, want[0], (B, T, Cc)), ("x0_out", x0d, want[1], (B, T, Cc)), ("tail_out", td, want[2], (B, L, Cc))):
        if buf is None:
            continue
        got, ok = _split(buf, shp)
        assert ok, (what, name, "guard overwritten")
        assert torch.equal(got, w), (what, name, int((got != w).sum()), float((got - w).abs().max()))


@pytest.mark.parametrize("L", R.STEP_LS)
def test_ddim_step_full_is_bit_exact(L):
    shape = (R.STEP_B, R.STEP_T, R.STEP_C)
    t = R.step_inputs(L)
    dev = _ddim_dev(t, L, shape)
    n_cmp = 0
    for combo in R.step_combos():
        full = R.ddim_case_ref(t, L, combo)
        for (c_lo, c_hi) in R.STEP_WINDOWS:
            for x0_on in (0, 1):
                bufs = _ddim_launch(dev, t, L, combo, c_lo, c_hi, x0_on, shape)
                torch.cuda.synchronize()
                _ddim_check(bufs, full, t, L, c_lo, c_hi, shape, (L, combo, c_lo, c_hi, x0_on))
                n_cmp += 1
    assert n_cmp == 3 * 2 * 3 * 3 * 2 * 3 * 2


def test_ddim_step_crosses_the_grid_cap_and_refuses_tail_in_without_a_mask():
    L, shape = 10, R.STEP_BIG
    assert shape[0] * shape[1] * shape[2] > 2048 * 256
    t = R.step_inputs(L, shape)
    dev = _ddim_dev(t, L, shape)
    for combo, win in ((("eta", 1, "dense", 1, 1, 1), (0, 0)), (("eta0", 0, "head", 1, 0, 1), (R.STEP_SPLIT, R.STEP_C))):
        bufs = _ddim_launch(dev, t, L, combo, win[0], win[1], 1, shape)
        torch.cuda.synchronize()
        _ddim_check(bufs, R.ddim_case_ref(t, L, combo), t, L, win[0], win[1], shape, combo)
    x = torch.zeros(1, 6, 8, device=DEV)
    rc = _lib.lib().dsh_op_ddim_step_full(None, _p(x), _p(x), None, None, None, None, None, _p(x), None, 1, 6, 8, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 2, 0, 0, 0, 0, 0)
    assert rc < 0 and b"tail_in" in _lib.lib().dsh_last_error()
    m = torch.ones(1, 6, 8, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().dsh_op_ddim_step_full(None, _p(x), _p(x), None, _p(x), _p(m), _p(x), None, None, None, 1, 6, 8, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 4, 1, 1, 0, 0, 0)
    assert rc < 0 and b"tail_blend" in _lib.lib().dsh_last_error()


@pytest.mark.parametrize("shape", [(R.STEP_B, R.STEP_T, R.STEP_C), R.STEP_BIG])
def test_ddpm_step_is_bit_exact(shape):
    B, T, Cc = shape
    t = R.step_inputs(2, shape)
    eps_d, nz_d, xg, sent = t["eps"].to(DEV), t["nz1"].to(DEV), _guarded(t["x"]), _guarded(_sentinel(shape))
    big = shape == R.STEP_BIG
    for k in (0, 3):                                                    # sigma = 0 at the last level, > 0 elsewhere
        sc = R.ddpm_scalars(k)
        assert (sc[4] == 0.0) == (k == 0)
        for clip in ((1,) if big else (0, 1)):
            full = R.ddpm_step_ref(t["x"], t["eps"], t["nz1"], sc, clip)
            for (c_lo, c_hi) in (R.STEP_WINDOWS[:2] if big else R.STEP_WINDOWS):
                for x0_on in ((1,) if big else (0, 1)):
                    xd, x0d = xg.clone(), (sent.clone() if x0_on else None)
                    _lib.check(_lib.lib().dsh_op_ddpm_step(None, _p(xd), _p(eps_d), _p(nz_d), _p(x0d), B * T * Cc, *sc, clip, Cc, c_lo, c_hi), "dsh_op_ddpm_step")
                    torch.cuda.synchronize()
                    for name, buf, prev, new in (("x", xd, t["x"], full[0]), ("x0_out", x0d, _sentinel(shape), full[1])):
                        if buf is None:
                            continue
                        got, ok = _split(buf, shape)
                        assert ok and torch.equal(got, R.window(prev, new, c_lo, c_hi)), (name, k, clip, c_lo, c_hi)
    rc = _lib.lib().dsh_op_ddpm_step(None, _p(xg), _p(eps_d), _p(nz_d), None, 8, 1.0, 1.0, 1.0, 1.0, 0.0, 0, 0, 1, 3)
    assert rc < 0 and b"channel range" in _lib.lib().dsh_last_error()


@pytest.mark.parametrize("shape", [(R.STEP_B, R.STEP_T, R.STEP_C), R.STEP_BIG])
def test_undo_step_is_bit_exact(shape):
    B, T, Cc = shape
    t = R.step_inputs(1, shape)
    nz_d, xg = t["nz1"].to(DEV), _guarded(t["x"])
    for k in (0, 20):
        sc = R.undo_scalars(k)
        full = R.undo_step_ref(t["x"], t["nz1"], sc)
        for (c_lo, c_hi) in R.STEP_WINDOWS:
            xd = xg.clone()
            _lib.check(_lib.lib().dsh_op_undo_step(None, _p(xd), _p(nz_d), sc[0], sc[1], B * T * Cc, Cc, c_lo, c_hi), "dsh_op_undo_step")
            torch.cuda.synchronize()
            got, ok = _split(xd, shape)
            assert ok and torch.equal(got, R.window(t["x"], full, c_lo, c_hi)), (k, c_lo, c_hi)
    # without a window the channel count is not needed; with one it is
    xd = xg.clone()
    _lib.check(_lib.lib().dsh_op_undo_step(None, _p(xd), _p(nz_d), sc[0], sc[1], B * T * Cc, 0, 0, 0))
    torch.cuda.synchronize()
    assert torch.equal(_split(xd, shape)[0], full)
    rc = _lib.lib().dsh_op_undo_step(None, _p(xd), _p(nz_d), sc[0], sc[1], B * T * Cc, 0, 1, 3)
    assert rc < 0 and b"channel range needs the channel count" in _lib.lib().dsh_last_error()


# ---- timestep-cache copy and the fills -------------------------------------------------------------------------------------------------
def test_level_copy_saves_and_restores_one_slot():
    L = _lib.lib()
    PAT, GB = 0x5A, 0xA5
    nbytes = [16, 48, 0, 4 * 1024 * 1024 + 16]                          # the last one: more 16-byte pieces than 1024 blocks x 256 threads
    offs = [16, 64, 128, 160]                                           # gaps between the ranges, and in front of the first
    stride = offs[3] + nbytes[3] + 32
    assert nbytes[3] // 16 > 1024 * 256 and stride % 16 == 0
    g = torch.Generator().manual_seed(9)
    orig = [torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g) for n in nbytes]
    work = [torch.cat([o, torch.full((R.GUARD,), GB, dtype=torch.uint8)]).to(DEV) for o in orig]
    slots = torch.full((4 * stride + R.GUARD,), PAT, dtype=torch.uint8, device=DEV)
    level = torch.tensor([2], dtype=torch.int64, device=DEV)
    wp = (C.c_void_p * 4)(*[w.data_ptr() for w in work])
    ba, oa = (C.c_int64 * 4)(*nbytes), (C.c_int64 * 4)(*offs)
    _lib.check(L.dsh_op_level_copy(None, wp, ba, oa, 4, _p(slots), stride, _p(level), 0), "dsh_op_level_copy")
    torch.cuda.synchronize()
    want = torch.full((4 * stride + R.GUARD,), PAT, dtype=torch.uint8)
    for o, off in zip(orig, offs):
        want[2 * stride + off:2 * stride + off + o.numel()] = o
    assert torch.equal(slots.cpu(), want)                               # slot 2 holds the ranges; slots 0, 1, 3 and every gap are untouched
    for w in work:
        w[:w.numel() - R.GUARD] = 0                                     # clobber, then restore
    _lib.check(L.dsh_op_level_copy(None, wp, ba, oa, 4, _p(slots), stride, _p(level), 1), "dsh_op_level_copy")
    torch.cuda.synchronize()
    for w, o in zip(work, orig):
        h = w.cpu()
        assert torch.equal(h[:o.numel()], o) and bool((h[o.numel():] == GB).all())
    assert torch.equal(slots.cpu(), want)
    rc = L.dsh_op_level_copy(None, wp, (C.c_int64 * 4)(16, 24, 0, 16), oa, 4, _p(slots), stride, _p(level), 0)
    assert rc < 0 and b"16-byte multiples" in L.dsh_last_error()
    rc = L.dsh_op_level_copy(None, wp, ba, (C.c_int64 * 4)(16, 64, 128, 208), 4, _p(slots), stride, _p(level), 0)
    assert rc < 0 and b"outside its slot" in L.dsh_last_error()


def test_fill_step_and_store_values():
    L = _lib.lib()
    for n in (1, 256, 257):
        t, lv = _guarded(torch.full((n,), 777, dtype=torch.int64)), _guarded(torch.full((1,), 777, dtype=torch.int64))
        t[n:], lv[1:] = 12345, 12345
        c1, c2 = _guarded(_sentinel((n,))), _guarded(_sentinel((n,)))
        _lib.check(L.dsh_op_fill_step(None, _p(t), _p(c1), _p(c2), _p(lv), 960, 1.25, 0.75, 24, n), "dsh_op_fill_step")
        torch.cuda.synchronize()
        for buf, v, m in ((t, 960, n), (lv, 24, 1), (c1, 1.25, n), (c2, 0.75, n)):
            h = buf.cpu()
            assert bool((h[:m] == v).all()) and bool((h[m:] == 12345).all()), (n, v)
    for n in (1, 64, 65, 130):                                          # 64 values per launch: one, exactly one, one more, three launches
        host = np.arange(n, dtype=np.float32) * np.float32(0.37) - np.float32(3)
        p = _guarded(_sentinel((n,)))
        _lib.check(L.dsh_op_store_values_f32(None, _p(p), host.ctypes.data_as(C.POINTER(C.c_float)), n), "dsh_op_store_values_f32")
        torch.cuda.synchronize()
        got, ok = _split(p, (n,))
        assert ok and torch.equal(got, torch.from_numpy(host)), n


def test_zero_padded_frames_and_fill_cols():
    L = _lib.lib()
    B, T, Cc = 4, 9, 5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, Cc, generator=g)
    lens = [0, 1, T - 1, T]
    xd, lens_d = _guarded(x), torch.tensor(lens, dtype=torch.int32, device=DEV)
    _lib.check(L.dsh_op_zero_padded_frames(None, _p(xd), _p(lens_d), B, T, Cc), "dsh_op_zero_padded_frames")
    torch.cuda.synchronize()
    want = x.clone()
    for b, ln in enumerate(lens):
        want[b, ln:] = 0.0
    got, ok = _split(xd, (B, T, Cc))
    assert ok and torch.equal(got, want)
    # fill_cols: a window at either end, from a source with a wider leading dimension or zeros; 4100 x 260: more than 4096 blocks
    for M, C_, lo, hi in ((7, 11, 0, 3), (7, 11, 8, 11), (1, 11, 4, 5), (4100, 300, 0, 260), (4100, 300, 40, 300)):
        dst = torch.randn(M, C_, generator=g)
        src = torch.randn(M, hi - lo + 2, generator=g)
        for s in (src, None):
            dd, s_d = _guarded(dst), (s.to(DEV) if s is not None else None)
            _lib.check(L.dsh_op_fill_cols(None, _p(dd), C_, M, lo, hi, _p(s_d), hi - lo + 2), "dsh_op_fill_cols")
            torch.cuda.synchronize()
            want = dst.clone()
            want[:, lo:hi] = s[:, :hi - lo] if s is not None else 0.0
            got, ok = _split(dd, (M, C_))
            assert ok and torch.equal(got, want), (M, C_, lo, hi, s is None)
    rc = L.dsh_op_fill_cols(None, _p(dd), 300, 4100, 5, 5, None, 0)
    assert rc < 0 and b"fill_cols" in L.dsh_last_error()
