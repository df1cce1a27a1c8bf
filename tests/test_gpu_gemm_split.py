"""The split-bf16 main loop of the fp32 Linears (diffsheg_amd/csrc/gemm_f32_split.hip, precision "bf16x3") through the C ABI
(dsh_op_gemm_f32_pro_ex with mma = 1; + 16 / + 32 forces the 64 x 64 / 128 x 128 tile).

Every launch is gated twice on every element (tests/split_gates.py): against the CPU emulation of the loop with the fp32 allowance of
f32_gates.py alone - which pins that exactly three products are formed from RNE pieces, and that PRO 1 splits x - x0 - and against fp64
with the gate derived from the arithmetic.  Both tile shapes run at every case and must agree bit for bit; the GUARD rows behind M of every
output must come back untouched; the input rows behind M are NaN and must never be read.

The epilogue's row constant (the CFG-null constant of the next layer) has no argument in the op entry: it runs in the model tests
(test_gpu_bf16x3.py, SHOW with guidance).  The split loop does not carry the row-moment side channel; the refusal is tested here."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
import f32_gates as G  # noqa: E402
import gemm_gates  # noqa: E402
import split_gates as S  # noqa: E402

DEV = "cuda:0"
GUARD = 8
SPLIT, SPLIT_64, SPLIT_128 = 1, 1 + 16, 1 + 32
P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
_NOSEG = (None, 0, 0)


def _rows(x, M, row0=0):
    out = torch.full((M + GUARD,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float32)
    out[:M] = x[row0:row0 + M]
    return out.to(DEV)


def _sentinel(M, N):
    return torch.full((M + GUARD, N), G.SENTINEL, device=DEV)


def _call(mma, pro, segs, k_real, W, bias, fc, film, film_ld, film_off, frames, nb, R, out, M, N, act, stats=None, groups=0, stats_out=None):
    a = []
    for s, ld, w in segs:
        a += [P(s), ld, w]
    return _lib.lib().dsh_op_gemm_f32_pro_ex(None, pro, *a, k_real, P(W), P(bias), P(fc), P(film), film_ld, film_off, frames, nb, P(R), P(out), M, N, act,
                                             P(stats), groups, P(stats_out), mma)


def run(t, mma, M=None, row0=0):
    """The launch of an f32_gates case on rows row0 .. row0 + M of its operands; [M + GUARD, N] on the CPU."""
    M = t["M"] if M is None else M
    N = t["N"]
    out = _sentinel(M, N)
    if t["kind"] == "pro0":
        K, R = t["K"], None
        if t["R"] is not None and t["alias"]:
            out[:M] = t["R"][row0:row0 + M].to(DEV)
            R = out                                             # in place, as the residual stream is updated
        elif t["R"] is not None:
            R = _rows(t["R"], M, row0)
        rc = _call(mma, 0, [(_rows(t["X"], M, row0), K, K), _NOSEG, _NOSEG, _NOSEG], K, t["W"].to(DEV), t["b"].to(DEV), None, None, 0, 0, 1, 1, R, out, M, N, t["act"])
    elif t["kind"] == "pro1":
        segs = [_NOSEG if s is None else (_rows(s, M, row0), w + t["ld_extra"], w) for s, w in zip(G.pro1_segments(t), t["widths"])]
        rc = _call(mma, 1, segs, t["k_real"], t["Wf"].to(DEV), t["fd"].to(DEV), t["fc"].to(DEV), None, 0, 0, 1, 1, None, out, M, N, t["act"])
    else:
        K, R = t["K"], None
        film = t["film"].to(DEV)
        if t["R"] is not None:
            out[:M] = t["R"][row0:row0 + M].to(DEV)
            R = out
        rc = _call(mma, 2, [(_rows(t["X"], M, row0), K, K), _NOSEG, _NOSEG, _NOSEG], K, t["W"].to(DEV), t["b"].to(DEV), None, film, film.shape[1], t["film_off"],
                   t["frames"], t["nb"], R, out, M, N, 0)
    _lib.check(rc)
    torch.cuda.synchronize()
    return out.cpu()


def gated(t):
    """Both tiles, bit-equal; guard rows; the two gates.  Prints the figures in front of the assertions.  Returns the output."""
    M = t["M"]
    o64, o128 = run(t, SPLIT_64), run(t, SPLIT_128)
    assert torch.equal(o64[M:], torch.full_like(o64[M:], G.SENTINEL)) and torch.equal(o128[M:], torch.full_like(o128[M:], G.SENTINEL)), f"{t['name']}: rows behind M were written"
    assert torch.equal(o64, o128), f"{t['name']}: the 64 x 64 and 128 x 128 tiles disagree"
    err, dist, cal, sp = S.figures(t, o64)
    print(f"[{t['name']}] |out - fp64| {err:.2e}, |out - emulation| {dist:.2e} (fp32 calibration {cal:.2e}, largest split term {sp:.2e})")
    S.check_emul(t, o64, flip=t["kind"] == "pro2")
    S.check(t, o64)
    return o64


# ---- 2. the grid ------------------------------------------------------------------------------------------------------------------------------
GRID_M = (1, 63, 64, 65, 127, 128, 129, 449)
GRID_N = (64, 68, 1536)
GRID_K = (32, 64, 96, 512, 1024)


def _grid_case(pro, M, N, K):
    j = GRID_M.index(M) + GRID_N.index(N) + GRID_K.index(K)
    if pro == 0:
        t = G.pro0_inputs(M, N, K, act=j % 3, res=j % 2 == 0)
    elif pro == 1:
        t = G.pro1_inputs(M, N, (K, 0, 0, 0), K, act=j % 2, ld_extra=32 * (j % 2))
    else:
        t = G.pro2_inputs(M, N, K, *G.PRO2_CLIPS[j % 4])
    t["name"] = f"split-p{pro}-grid-{M}x{N}x{K}"
    return t


@pytest.mark.parametrize("N", GRID_N)
@pytest.mark.parametrize("M", GRID_M)
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_grid_against_the_emulation_and_fp64(pro, M, N):
    for K in GRID_K:
        gated(_grid_case(pro, M, N, K))


@pytest.mark.parametrize("K", [512, 960])
@pytest.mark.parametrize("fam", S.FAMILIES)
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_input_families(pro, fam, K):
    """every family of the CPU test on the kernel: whole-row offsets (the PRO 1 shift), outlier columns, low variance"""
    gated(S.family_case(pro, fam, K))


SPECIAL = {
    "p1-4seg-13pad": lambda: G.pro1_inputs(130, 192, G.FAMILY_WIDTHS, 947, act=1),
    "p1-4seg-25pad": lambda: G.pro1_inputs(130, 192, G.FAMILY_WIDTHS, 935, act=0),
    "p1-4seg-13pad-off-200": lambda: G.pro1_inputs(449, 64, G.FAMILY_WIDTHS, 947, act=0, family="off-200"),
    "p1-3seg": lambda: G.pro1_inputs(130, 192, (512, 0, 128, 64), 690, act=1),
    "p2-34x3-film-off": lambda: G.pro2_inputs(449, 128, 512, 34, 3, film_off=8),
    "p2-11x7-film-off-4K": lambda: G.pro2_inputs(130, 64, 1024, 11, 7, film_off=4 * 1024),
    "p0-in-place-residual": lambda: G.pro0_inputs(130, 192, 96, act=0, res=True, alias=True),
    "p0-own-residual": lambda: G.pro0_inputs(130, 192, 96, act=1, res=True, alias=False),
    "p0-gelu": lambda: G.pro0_inputs(449, 192, 512, act=2, res=False),
    "p0-gelu-in-place": lambda: G.pro0_inputs(130, 192, 96, act=2, res=True, alias=True),
}


@pytest.mark.parametrize("name", list(SPECIAL))
def test_segments_film_residual_and_activation_forms(name):
    t = SPECIAL[name]()
    t["name"] = "split-" + name
    gated(t)


@pytest.mark.parametrize("M", S.MODEL_M)
@pytest.mark.parametrize("name", list(S.MODEL_LINEARS))
def test_the_models_own_linear_forms(name, M):
    """Every (N, K, front, activation, residual) form Denoiser<float> launches on this loop (split_gates.MODEL_LINEARS, read off denoiser.hip):
    K = 3 072 / 2 048 / 384 and the narrow and the very wide N are outside the grid above, and the split error grows with K.  M = 513 is the
    smallest row count at which the model leaves the few-row kernels; 641 = 5 x 128 + 1 straddles the 128-row tile edge."""
    gated(S.model_case(name, M))


def test_row_moment_side_channel_is_refused():
    t = G.pro0_inputs(130, 64, 96, res=False)
    X, W, b = _rows(t["X"], 130), t["W"].to(DEV), t["b"].to(DEV)
    out, st = _sentinel(130, 64), torch.zeros(130 + GUARD, 2, 2, device=DEV)
    seg = [(X, 96, 96), _NOSEG, _NOSEG, _NOSEG]
    assert _call(SPLIT, 0, seg, 96, W, b, None, None, 0, 0, 1, 1, None, out, 130, 64, 0, stats_out=st) != 0
    assert "side channel" in _lib.lib().dsh_last_error().decode()
    t2 = G.pro2_inputs(130, 64, 64, 11, 7, stat_groups=2)
    film = t2["film"].to(DEV)
    rc = _call(SPLIT, 2, [(_rows(t2["X"], 130), 64, 64), _NOSEG, _NOSEG, _NOSEG], 64, t2["W"].to(DEV), t2["b"].to(DEV), None, film, film.shape[1], 0, 11, 7, None, out, 130, 64, 0,
               stats=_rows(t2["stats"], 130), groups=2)
    assert rc != 0 and "side channel" in _lib.lib().dsh_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((138, 64), G.SENTINEL)), "a refused launch wrote its output"
    assert _call(5, 0, seg, 96, W, b, None, None, 0, 0, 1, 1, None, out, 130, 64, 0) != 0                      # unknown mma


# ---- 3. bit identity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_a_row_gives_the_same_bits_alone_and_inside_a_batch(pro):
    """row 200 of M = 449 (fourth 64-row tile, second 128-row tile) against the same row as an M = 1 launch, every tile pick"""
    if pro == 0:
        t = G.pro0_inputs(449, 192, 512, act=1, res=True, alias=False)
    elif pro == 1:
        t = G.pro1_inputs(449, 192, G.FAMILY_WIDTHS, 947, act=1, family="off+50")
    else:
        t = G.pro2_inputs(449, 192, 512, 34, 5)               # row 200 = clip (200 // 34) % 5 = 0: the FiLM row of an M = 1 launch
        assert int(t["clip"][200]) == 0
    whole = {m: run(t, m) for m in (SPLIT, SPLIT_64, SPLIT_128)}
    alone = {m: run(t, m, M=1, row0=200) for m in (SPLIT, SPLIT_64, SPLIT_128)}
    for m in whole:
        assert torch.equal(whole[m], whole[SPLIT]) and torch.equal(alone[m], alone[SPLIT]), f"tile pick {m >> 4} changes the bits"
        assert torch.equal(alone[m][0], whole[m][200]), "a row's bits depend on where it sits in M"
        assert torch.equal(alone[m][1:], torch.full_like(alone[m][1:], G.SENTINEL))


# ---- 4. exact integers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(129, 68, 512), (449, 192, 1024)])
def test_small_integer_operands_are_exact(M, N, K):
    """operands of at most 8 significant bits have no lo piece: every product and every partial sum is an integer below 2^24"""
    g = torch.Generator().manual_seed(M + K)
    t = {"kind": "pro0", "M": M, "N": N, "K": K, "act": 0, "family": "ints", "stats_out": False, "alias": True, "name": f"split-ints-{M}x{N}x{K}",
         "X": gemm_gates._ints((M, K), g), "W": gemm_gates._ints((N, K), g), "b": gemm_gates._ints((N,), g, density=1.0),
         "R": gemm_gates._ints((M, N), g, top=3, density=1.0)}
    ref = G.pro0_chain(t, torch.float64)
    for m in (SPLIT_64, SPLIT_128):
        out = run(t, m)
        assert torch.equal(out[:M].double(), ref), f"tile {m >> 4}: max |diff| {float((out[:M].double() - ref).abs().max())}"


# ---- 5. counters, and mma = 0 is the exact-fp32 launch ------------------------------------------------------------------------------------------
def test_counters_and_the_exact_loop_through_the_same_entry():
    t = G.pro1_inputs(130, 192, G.FAMILY_WIDTHS, 947, act=1)
    _lib.launch_counts(reset=True)
    run(t, SPLIT)
    c = _lib.launch_counts(reset=True)
    assert c["gemm_f32_split"] == 1 and c["gemm_f32_pro"] == 0, c
    exact = run(t, 0)
    c = _lib.launch_counts(reset=True)
    assert c["gemm_f32_split"] == 0 and c["gemm_f32_pro"] == 1, c
    # the entry without the argument
    M, N = t["M"], t["N"]
    out = _sentinel(M, N)
    Wf, fd, fc = t["Wf"].to(DEV), t["fd"].to(DEV), t["fc"].to(DEV)
    segs = [_rows(s, M) for s in G.pro1_segments(t)]
    a = []
    for s, w in zip(segs, t["widths"]):
        a += [P(s), w + t["ld_extra"], w]
    _lib.check(_lib.lib().dsh_op_gemm_f32_pro(None, 1, *a, t["k_real"], P(Wf), P(fd), P(fc), None, 0, 0, 1, 1, None, P(out), M, N, t["act"], None, 0, None))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), exact), "mma = 0 is not dsh_op_gemm_f32_pro bit for bit"
    split = run(t, SPLIT)
    assert not torch.equal(exact, split)
    G.check(t, exact)
    # the weight packed by the one packer and passed packed (+ 64): the launch alone, the same bits
    Wp = torch.empty(Wf.shape, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().dsh_op_split_pack_weight(None, P(Wf), N, t["K"], P(Wp)))
    out = _sentinel(M, N)
    _lib.check(_lib.lib().dsh_op_gemm_f32_pro_ex(None, 1, *a, t["k_real"], P(Wp), P(fd), P(fc), None, 0, 0, 1, 1, None, P(out), M, N, t["act"], None, 0, None, SPLIT + 64))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), split)
    hi, lo = S.split(t["Wf"])
    words = Wp.cpu().view(N, t["K"] // 32, 2, 16)                     # per K tile: 16 words of hi pairs, 16 of lo pairs (even k in the low half)
    pair = lambda v: (v.bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF).view(N, t["K"] // 32, 16, 2)
    for piece, want in ((0, pair(hi)), (1, pair(lo))):
        assert torch.equal(words[:, :, piece] & 0xFFFF, want[..., 0]) and torch.equal((words[:, :, piece] >> 16) & 0xFFFF, want[..., 1])
