"""The row kernels around the denoiser (rowops.hip) one launch at a time on a real MI355X, against the CPU references of small_ops_ref.py:
temb, cfg_mix, im2col3 (with lens), the FiLM fold / expand / gather, the layer-0 seed of the residual stream, the expression-track pack,
and the LayerNorm row kernels every shape the fused launches refuse falls back to (ln_rows with pre_add, ln_film_silu_rows, concat_ln_rows).

Every output buffer carries GUARD sentinel elements behind its last element and sentinel pad columns where its leading dimension is wider
than the rows; every element a launch must not write is compared with what it held before."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_gates as G  # noqa: E402
import small_ops_ref as R  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(t):
    flat = torch.full((t.numel() + R.GUARD,), R.SENTINEL, dtype=t.dtype)
    flat[:t.numel()] = t.reshape(-1)
    return flat.to(DEV)


def _sent(shape, dtype=torch.float32):
    return torch.full(shape, R.SENTINEL, dtype=dtype)


def _split(buf, shape):
    n = int(np.prod(shape))
    h = buf.cpu()
    assert h.numel() == n + R.GUARD and bool((h[n:] == torch.tensor(R.SENTINEL, dtype=h.dtype)).all()), "guard behind the buffer overwritten"
    return h[:n].reshape(shape)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    eq = torch.equal(_bits(got), _bits(want)) if got.dtype == BF else torch.equal(got, want)
    assert eq, (what, int((got.float() != want.float()).sum()))


# ---- temb ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.TEMB_DIMS)
def test_temb_rows(dim):
    """fp32: every element within MARGIN x K x 2^-24 (2 t f_j + 1), K calibrated from torch's fp32 timestep_embedding over all timesteps and
    frequencies (small_ops_ref.temb_allow); t = 0 exact.  bf16: that plus half a bf16 ulp.  Measured on an MI355X: largest error 0.86 (dim
    128) and 0.97 (dim 512) of the scale, where torch's own is K = 0.86 and 0.91: 0.33 and 0.35 of the allowance."""
    t = list(R.TEMB_T)
    B, ldo = len(t), dim + 8
    td = torch.tensor(t, dtype=torch.int64, device=DEV)
    ref, allow = R.temb_ref64(t, dim), R.temb_allow(t, dim)
    out = _guarded(_sent((B, ldo)))
    _lib.check(_lib.lib().dsh_op_temb(None, 0, _p(td), B, dim, _p(out), ldo), "dsh_op_temb")
    torch.cuda.synchronize()
    got = _split(out, (B, ldo))
    assert bool((got[:, dim:] == R.SENTINEL).all())
    err = (got[:, :dim].double() - ref).abs()
    ratio = float((err / allow).max())
    print(f"[temb fp32] dim {dim}: worst |out - ref64| / (MARGIN x K x scale) = {ratio:.3f}, K = {R.temb_k(dim):.3f}, "
          f"device error in units of the scale {ratio * R.MARGIN * R.temb_k(dim):.3f}")
    assert t[0] == 0 and bool((err[0] == 0).all()), "t = 0: cos 0 = 1 and sin 0 = 0 are exact"
    assert bool((err <= allow).all()), ratio
    outb = _guarded(_sent((B, ldo), BF))
    _lib.check(_lib.lib().dsh_op_temb(None, 1, _p(td), B, dim, _p(outb), ldo), "dsh_op_temb")
    torch.cuda.synchronize()
    gotb = _split(outb, (B, ldo))
    assert bool((gotb[:, dim:] == torch.tensor(R.SENTINEL, dtype=BF)).all())
    rb = G.assert_rounded(gotb[:, :dim].contiguous(), ref, slack=allow, what=f"temb bf16 dim {dim}")
    print(f"[temb bf16] dim {dim}: worst |out - ref64| / (half a bf16 ulp + the fp32 allowance) = {rb:.3f}")
    assert bool((gotb[0, :dim].float() == ref[0].float()).all())


# ---- cfg_mix ---------------------------------------------------------------------------------------------------------------------------
def _cfg_run(t, has_null, x0_on):
    Mc, w, c0 = t["Mc"], t["w"], t["c0"]
    d = {n: t[n].to(DEV) for n in ("o", "x", "scale", "c1", "c2")}
    eps = _guarded(_sent((Mc, t["lde"])))
    x0 = _guarded(_sent((Mc, t["ldx0"]))) if x0_on else None
    _lib.check(_lib.lib().dsh_op_cfg_mix(None, _p(d["o"]), t["ldo"], Mc, t["cond_row0"], t["T"], w, has_null, _p(d["scale"]) if has_null else None,
                                        t["scale_row"], _p(eps), t["lde"], c0, _p(d["x"]), t["ldx"], _p(d["c1"]), _p(d["c2"]), _p(x0), t["ldx0"]),
               "dsh_op_cfg_mix")
    torch.cuda.synchronize()
    e_ref, x0_ref = R.cfg_mix_ref(t, has_null)
    want = _sent((Mc, t["lde"]))
    want[:, c0:c0 + w] = e_ref
    _same(_split(eps, want.shape), want, ("eps", w, c0, has_null))
    if x0_on:
        want0 = _sent((Mc, t["ldx0"]))
        want0[:, :w] = x0_ref
        _same(_split(x0, want0.shape), want0, ("x0", w, c0, has_null))
    return e_ref


@pytest.mark.parametrize("w", [103, 129])
def test_cfg_mix_is_exact(w):
    n = 0
    for c0, extra in ((0, 0), (3, 5), (103, 9)):
        for x0_on in (0, 1):
            t = R.cfg_inputs(w, c0=c0, ld_extra=extra)                     # per-clip scales 1.0 | 1.15 | 0
            e = _cfg_run(t, 1, x0_on)
            T, r0 = t["T"], t["cond_row0"]
            assert torch.equal(e[:T], t["o"][r0:r0 + T, :w])                # scale 1: o_c itself
            _cfg_run(t, 0, x0_on)                                           # has_null = 0: a copy of the first half
            for s in (1.0, 1.15, 0.0):                                      # one scale for the batch
                _cfg_run(R.cfg_inputs(w, c0=c0, ld_extra=extra, per_clip=False, scales=(s,)), 1, x0_on)
            n += 5
    assert n == 30
    o = torch.zeros(8, 4, device=DEV)
    rc = _lib.lib().dsh_op_cfg_mix(None, _p(o), 4, 2, 2, 1, 4, 1, None, 0, _p(o), 4, 0, None, 0, None, None, None, 0)
    assert rc < 0 and b"guidance scales" in _lib.lib().dsh_last_error()


# ---- im2col3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", [128, 1024])
def test_im2col3_is_exact_and_selects_padded_frames_away(Cin):
    B, n = 3, 0
    for T in (1, 2, 34):
        g = torch.Generator().manual_seed(Cin + T)
        x = torch.randn(B, T, Cin, generator=g)
        for lens in (None, [0, 1, T]):
            xs = x.clone()
            if lens is not None:
                for b, ln in enumerate(lens):
                    xs[b, ln:] = float("nan")                              # whatever the padding holds is selected away, not multiplied
            ldx, ldo = Cin + 8, 3 * Cin + 8
            src = torch.full((B * T, ldx), 7.0)
            src[:, :Cin] = xs.reshape(B * T, Cin)
            # fp32 -> fp32: the patches; fp32 -> bf16: their RNE rounding; bf16 -> bf16: the patches of the rounded source
            refs = {(0, 0): R.im2col3_ref(x, lens), (0, 1): R.rne_bf16(R.im2col3_ref(x, lens)), (1, 1): R.im2col3_ref(R.rne_bf16(x), lens)}
            ld = _i32(lens) if lens is not None else None
            for (din, dout), ref in refs.items():
                sd = (src.to(BF) if din else src).to(DEV)
                out = _guarded(_sent((B * T, ldo), BF if dout else torch.float32))
                _lib.check(_lib.lib().dsh_op_im2col3(None, din, dout, _p(sd), ldx, B, T, Cin, _p(out), ldo, _p(ld)), "dsh_op_im2col3")
                torch.cuda.synchronize()
                got = _split(out, (B * T, ldo))
                assert bool(torch.isfinite(got.float()).all())
                want = _sent((B * T, ldo), got.dtype)
                want[:, :3 * Cin] = ref
                _same(got, want, ("im2col3", Cin, T, lens, din, dout))
                n += 1
    assert n == 18
    rc = _lib.lib().dsh_op_im2col3(None, 1, 0, _p(sd), ldx, B, T, Cin, _p(out), ldo, None)
    assert rc < 0


# ---- FiLM fold / expand / gather -------------------------------------------------------------------------------------------------------
def _film_check(got, t, idx, like, what):
    """got [B, ld] against the fold of rows idx of t['tab']: A exact, B within one fp32 ulp, columns behind 2 D nblk as `like`"""
    A, Bc = R.film_fold_ref(t, idx)
    nb, nblk, D = A.shape
    w = 2 * D * nblk
    g = got[:, :w].reshape(nb, nblk, 2, D)
    assert torch.equal(g[:, :, 0], A), (what, "A")
    err = (g[:, :, 1].double() - Bc.double()).abs()
    ulp = R.ulp_f32(Bc)
    print(f"[film {what}] B coefficient: worst |out - rounded fp64| = {float((err / ulp).max()):.2f} ulp, {int((err > 0).sum())} of {err.numel()} differ")
    assert bool((err <= ulp).all()), what
    assert torch.equal(got[:, w:], like[:, w:]), (what, "pad columns")


@pytest.mark.parametrize("nblk,D,extra", [(1, 128, 0), (2, 512, 8), (16, 128, 4), (16, 512, 0)])
def test_film_fold_and_expand(nblk, D, extra):
    L = _lib.lib()
    B, n_src = 6, 4
    t = R.film_inputs(B, nblk, D, ld_extra=extra, n_src=n_src)
    ld, gd, bd = t["ld"], t["gamma"].to(DEV), t["beta"].to(DEV)
    src = t["tab"].to(DEV)
    idx = [3, 2, 2, 0, 1, 0]                                               # repeats, reversed order
    idx_d = _i32(idx)                                                      # (device operands stay referenced until the launch has run)
    # fold = 0: a plain copy of the gathered rows
    dst = _guarded(_sent((B, ld)))
    _lib.check(L.dsh_op_film_expand(None, _p(src), ld, _p(idx_d), _p(dst), B, nblk, D, None, None, 0), "dsh_op_film_expand")
    torch.cuda.synchronize()
    want = _sent((B, ld))
    want[:, :2 * D * nblk] = t["tab"][idx][:, :2 * D * nblk]
    _same(_split(dst, (B, ld)), want, "film_expand copy")
    # fold = 1 through idx
    dst = _guarded(_sent((B, ld)))
    _lib.check(L.dsh_op_film_expand(None, _p(src), ld, _p(idx_d), _p(dst), B, nblk, D, _p(gd), _p(bd), 1), "dsh_op_film_expand")
    torch.cuda.synchronize()
    _film_check(_split(dst, (B, ld)), t, idx, _sent((B, ld)), f"expand nblk {nblk} D {D}")
    assert torch.equal(src.cpu(), t["tab"])                                # the source rows are only read
    # film_fold in place = film_expand(fold = 1, idx = null), bit for bit
    tab = _guarded(t["tab"])
    _lib.check(L.dsh_op_film_fold(None, _p(tab), ld, n_src, nblk, D, _p(gd), _p(bd)), "dsh_op_film_fold")
    dst = _guarded(_sent((n_src, ld)))
    _lib.check(L.dsh_op_film_expand(None, _p(src), ld, None, _p(dst), n_src, nblk, D, _p(gd), _p(bd), 1), "dsh_op_film_expand")
    torch.cuda.synchronize()
    folded, expanded = _split(tab, (n_src, ld)), _split(dst, (n_src, ld))
    _film_check(folded, t, None, t["tab"], f"fold nblk {nblk} D {D}")
    w = 2 * D * nblk
    assert torch.equal(folded[:, :w], expanded[:, :w])


def test_film_grid_caps_and_gather_rows():
    L = _lib.lib()
    # 1030 clips x 16 blocks x 512: 8.4 M coefficients (4096-block cap of film_fold) in 2.1 M float4 pieces (8192-block cap of film_expand)
    B, nblk, D, n_src = 1030, 16, 512, 4
    assert B * nblk * D > 4096 * 256 and B * nblk * D // 4 > 8192 * 256
    t = R.film_inputs(B, nblk, D, n_src=n_src)
    ld, gd, bd, src = t["ld"], t["gamma"].to(DEV), t["beta"].to(DEV), t["tab"].to(DEV)
    idx = [(b * 7 + 1) % n_src for b in range(B)]
    idx_d = _i32(idx)
    tab = _guarded(_sent((B, ld)))
    _lib.check(L.dsh_op_film_expand(None, _p(src), ld, _p(idx_d), _p(tab), B, nblk, D, None, None, 0), "dsh_op_film_expand")
    dst = _guarded(_sent((B, ld)))
    _lib.check(L.dsh_op_film_expand(None, _p(src), ld, _p(idx_d), _p(dst), B, nblk, D, _p(gd), _p(bd), 1), "dsh_op_film_expand")
    torch.cuda.synchronize()
    copied = _split(tab, (B, ld))
    assert torch.equal(copied, t["tab"][idx])
    _lib.check(L.dsh_op_film_fold(None, _p(tab), ld, B, nblk, D, _p(gd), _p(bd)), "dsh_op_film_fold")
    torch.cuda.synchronize()
    folded, expanded = _split(tab, (B, ld)), _split(dst, (B, ld))
    assert torch.equal(folded, expanded)
    _film_check(expanded, t, idx, expanded, "grid caps")
    # gather_rows: repeats, reversed order, leading dimensions wider than w, more than 4096 blocks
    for Bg, w in ((6, 1), (6, 64), (5, 300), (2100, 512)):
        g = torch.Generator().manual_seed(w)
        s = torch.randn(5, w + 3, generator=g)
        ix = [(4 - b) % 5 if b % 3 else 2 for b in range(Bg)]
        out, s_d, ix_d = _guarded(_sent((Bg, w + 5))), s.to(DEV), _i32(ix)
        _lib.check(L.dsh_op_gather_rows(None, _p(s_d), w + 3, _p(ix_d), _p(out), w + 5, Bg, w), "dsh_op_gather_rows")
        torch.cuda.synchronize()
        want = _sent((Bg, w + 5))
        want[:, :w] = s[ix][:, :w]
        _same(_split(out, (Bg, w + 5)), want, ("gather_rows", Bg, w))


# ---- seed_stream -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mc", [1, 31, 32, 33, 88])
def test_seed_stream(Mc):
    L = _lib.lib()
    n = 0
    for D in (512, 128):
        g = torch.Generator().manual_seed(Mc + D)
        h0, c = torch.randn(Mc, D, generator=g) * 3, torch.randn(D, generator=g)
        h0d, cd = h0.to(DEV), c.to(DEV)
        base = (Mc + 31) // 32 * 32
        for has_null, row1 in ((0, 0), (1, base), (1, base + 64)):
            ref = R.seed_stream_ref(h0, c, has_null, row1)
            Rr = ref.shape[0]
            hi_ref = R.rne_bf16(ref)
            for hilo in (0, 1):
                h, h16, lo = _guarded(_sent((Rr, D))), _guarded(_sent((Rr, D), BF)), _guarded(_sent((Rr, D), BF))
                _lib.check(L.dsh_op_seed_stream(None, _p(h0d), Mc, D, _p(cd) if has_null else None, has_null, row1, hilo, _p(h), _p(h16), _p(lo)),
                           "dsh_op_seed_stream")
                got_h, got_16, got_lo = _split(h, (Rr, D)), _split(h16, (Rr, D)), _split(lo, (Rr, D))
                _same(got_16, hi_ref, ("h16 = RNE bf16 of h", Mc, D, has_null, row1, hilo))
                if hilo:
                    assert bool((got_h == R.SENTINEL).all()) , "the fp32 stream is not written with planes"
                    _same(got_lo, R.rne_bf16(ref - hi_ref.float()), ("lo = RNE bf16 of h - hi", Mc, D, has_null, row1))
                    rec = got_16.double() + got_lo.double()
                    assert bool(((rec - ref.double()).abs() <= G.ulp_bf16(got_lo.double())).all())
                else:
                    _same(got_h, ref, ("h", Mc, D, has_null, row1))          # rows [0, Mc) = h0 + c in one fp32 add, rows [row1, ..) = h0, the rest 0
                    assert bool((got_lo == torch.tensor(R.SENTINEL, dtype=BF)).all())
                n += 1
    assert n == 12
    rc = L.dsh_op_seed_stream(None, _p(h0d), Mc, D, _p(cd), 1, base + 8, 0, _p(h), _p(h16), None)
    assert rc < 0 and b"seed_stream" in L.dsh_last_error()


# ---- pack_expr_track -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [51, 100, 103])
def test_pack_expr_track(E):
    L = _lib.lib()
    B, T = 3, 34
    M = B * T
    g = torch.Generator().manual_seed(E)
    src = torch.randn(M, E, generator=g)
    n = 0
    for ld in (128, E):
        for lens in (None, [0, 1, T], [T, T - 1, 5]):
            s = src.clone()
            if lens is not None:
                sv = s.view(B, T, E)
                for b, ln in enumerate(lens):
                    sv[b, ln:] = float("nan")
            x0 = _guarded(_sent((M, ld)))
            x16, tl = _guarded(_sent((M, 128), BF)), _guarded(_sent((M, 128), BF))
            s_d, lens_d = s.to(DEV), (_i32(lens) if lens is not None else None)
            _lib.check(L.dsh_op_pack_expr_track(None, _p(s_d), E, B, T, _p(lens_d), _p(x0), ld, _p(x16), _p(tl)),
                       "dsh_op_pack_expr_track")
            ref = R.pack_expr_ref(src, B, T, ld, lens)
            got = _split(x0, (M, ld))
            assert bool(torch.isfinite(got).all())
            _same(got, ref, ("x0", E, ld, lens))
            want16 = torch.zeros(M, 128)
            want16[:, :ld] = ref
            g16 = _split(x16, (M, 128))
            _same(g16, R.rne_bf16(want16), ("x16", E, ld, lens))
            _same(g16, _split(tl, (M, 128)), ("x16 against the production tiler on x0", E, ld, lens))
            n += 1
    assert n == 6
    rc = L.dsh_op_pack_expr_track(None, _p(s_d), 129, B, T, None, _p(x0), 129, None, None)
    assert rc < 0 and b"pack_expr_track" in L.dsh_last_error()


# ---- LayerNorm family: the row kernels behind every shape the fused launches refuse ------------------------------------------------------
def _padded(rows, ld, fill=7.0, dtype=torch.float32):
    """[M, w] rows in a buffer with leading dimension ld (pad columns hold `fill`)"""
    out = torch.full((rows.shape[0], ld), fill, dtype=dtype)
    out[:, :rows.shape[1]] = rows.to(dtype)
    return out


def _ln_out(M, ldo, bf):
    return _guarded(_sent((M, ldo), BF if bf else torch.float32))


def _ln_finish(t, out, M, D, ldo, what):
    got = _split(out, (M, ldo))
    assert bool((got[:, D:] == torch.tensor(R.SENTINEL, dtype=got.dtype)).all()), (what, "pad columns written")
    return R.ln_check(t, got[:, :D].contiguous(), what)


@pytest.mark.parametrize("D", R.LN_DS)
def test_ln_rows_with_pre_add(D):
    L = _lib.lib()
    worst = {0: 0.0, 1: 0.0}
    for M in R.LN_MS:
        for family in R.LN_FAMILIES:
            t = R.ln_inputs("pre", M, D, family)
            ldh, ldo, n_pre = D + 4, D + 8, t["n_pre"]
            gd, bd, pd = t["gamma"].to(DEV), t["beta"].to(DEV), t["pre_add"].to(DEV)
            for bf in (0, 1):
                h = _guarded(_padded(t["h_in"][:M], ldh))
                out = _ln_out(M, ldo, bf)
                _lib.check(L.dsh_op_layernorm_pre(None, bf, _p(h), ldh, M, D, _p(pd), n_pre, _p(gd), _p(bd), _p(out), ldo), "dsh_op_layernorm_pre")
                torch.cuda.synchronize()
                # h comes back as h + pre_add on the first n_pre rows, untouched elsewhere (pad columns included)
                _same(_split(h, (M, ldh)), _padded(t["X"][:M], ldh), ("h in/out", M, D, family))
                worst[bf] = max(worst[bf], _ln_finish(t, out, M, D, ldo, f"ln_rows pre_add M {M} D {D} {family} bf16 {bf}"))
            if M == 5 and family == "plain":                                # pre_add == null: h is only read
                h = _guarded(_padded(t["X"][:M], ldh))
                out = _ln_out(M, ldo, 0)
                _lib.check(L.dsh_op_layernorm_pre(None, 0, _p(h), ldh, M, D, None, M, _p(gd), _p(bd), _p(out), ldo), "dsh_op_layernorm_pre")
                torch.cuda.synchronize()
                _same(_split(h, (M, ldh)), _padded(t["X"][:M], ldh), "h untouched")
                _ln_finish(t, out, M, D, ldo, "ln_rows without pre_add")
    print(f"[ln_rows pre_add] D {D}: worst |out - ref64| / calibration: fp32 out {worst[0]:.3f}, bf16 out (of half an ulp + allowance) {worst[1]:.3f}; gate {R.MARGIN}")


@pytest.mark.parametrize("D", R.LN_DS)
def test_ln_film_silu_rows(D):
    L = _lib.lib()
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    # 1, 3, 3 and 6 clips on a table of nb = 3 rows: at M = 77, frames = 13 the clip index (row / frames) % nb wraps
    for M, frames in ((1, 1), (5, 2), (77, 26), (77, 13)):
        for family in R.LN_FAMILIES:
            for variant, film_off in ((0, 0), (1, 8), (2, 8), (0, 2 * D)):
                t = R.ln_inputs("film", M, D, family, frames=frames, nb=3, film_off=film_off, bf16_in=variant == 2)
                ldy, ldo = D + 8, D + 8
                gd, bd, fd = t["gamma"].to(DEV), t["beta"].to(DEV), t["film"].to(DEV)
                y = _padded(t["X"][:M], ldy, dtype=BF if variant == 2 else torch.float32).to(DEV)
                out = _ln_out(M, ldo, variant > 0)
                _lib.check(L.dsh_op_ln_film_silu(None, variant, _p(y), ldy, M, D, _p(gd), _p(bd), _p(fd), t["film"].shape[1], film_off, frames, 3, _p(out), ldo),
                           "dsh_op_ln_film_silu")
                torch.cuda.synchronize()
                worst[variant] = max(worst[variant], _ln_finish(t, out, M, D, ldo, f"ln_film_silu M {M} D {D} {family} variant {variant} film_off {film_off}"))
    print(f"[ln_film_silu] D {D}: worst / calibration: fp32 {worst[0]:.3f}, fp32 -> bf16 {worst[1]:.3f}, bf16 -> bf16 {worst[2]:.3f}; gate {R.MARGIN}")


@pytest.mark.parametrize("widths", R.CONCAT_WIDTHS)
def test_concat_ln_rows(widths):
    L = _lib.lib()
    P = sum(widths)
    Ppad = 80 if P == 65 else 1024
    worst = {0: 0.0, 1: 0.0}
    for M in R.LN_MS:
        for family in R.LN_FAMILIES:
            for bf in (0, 1):
                t = R.ln_inputs("concat", M, P, family, bf16_in=bool(bf), widths=widths)
                x = t["X"][:M]
                segs, c = [], 0
                for j, w in enumerate(widths):
                    dt = BF if (bf and j in (1, 2)) else torch.float32
                    segs.append(_padded(x[:, c:c + w], w + 4 * (j + 1), dtype=dt).to(DEV) if w else None)
                    c += w
                ldo = Ppad + 8
                gd, bd = _padded(t["gamma"][None], Ppad, 0.0)[0].to(DEV), _padded(t["beta"][None], Ppad, 0.0)[0].to(DEV)
                out = _ln_out(M, ldo, bf)
                args = []
                for j, w in enumerate(widths):
                    args += [_p(segs[j]), w + 4 * (j + 1), w]
                _lib.check(L.dsh_op_concat_ln(None, bf, *args, M, _p(gd), _p(bd), _p(out), ldo, Ppad), "dsh_op_concat_ln")
                torch.cuda.synchronize()
                got = _split(out, (M, ldo))
                assert bool((got[:, Ppad:] == torch.tensor(R.SENTINEL, dtype=got.dtype)).all())
                assert bool((got[:, P:Ppad].float() == 0).all()), "pad columns [P, Ppad) must be exact zero"
                worst[bf] = max(worst[bf], R.ln_check(t, got[:, :P].contiguous(), f"concat_ln M {M} P {P} {family} bf16 {bf}"))
    print(f"[concat_ln] P {P} Ppad {Ppad}: worst / calibration: fp32 {worst[0]:.3f}, bf16 {worst[1]:.3f}; gate {R.MARGIN}")
