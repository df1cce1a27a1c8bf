"""CPU restatement of the bf16 precision mode of the HuBERT encoder (dsh_hubert_set_precision(1), csrc/hubert.hip step 5): plain torch,
dtype-generic.  Everything in front of the layers and the last LayerNorm are hubert_ref's; the layers carry exactly the documented rounding
points (include/diffsheg_hip.h at dsh_hubert_set_precision):

  W' = RNE_bf16(gamma (.) W) in ONE rounding from the fp64 fold (q rows x 1 / 8 first), b' = fp32(b + W beta)
  a  = RNE_bf16((h - mean) rstd), two-pass moments of the fp32 row               LayerNorm in front of q|k|v and intermediate_dense
  qkv = RNE_bf16(a W'^T + b')
  attention per head, keys in tiles of 32 with a running maximum: s = q^ k^^T, p = exp(s - m), l += sum p (unrounded), o += RNE_bf16(p) v,
      both rescaled by exp(m_old - m_new) when the maximum moves; att = RNE_bf16(o / l).  The tiles matter: p is rounded against the RUNNING
      maximum, so a chain that rounds against the final one would round different numbers.
  h += att Wo'^T + bo;  f = RNE_bf16(GELU(a2 W1'^T + b1'));  h += f W2'^T + b2      (h stays in dt: the fp32 residual stream)

float64 is the reference of the kernel tests, float32 (one accumulator per output, K ascending or descending: f32_gates._mm) the calibration
chain.  The keyword mutants are what test_hubert_bf16_cpu.py must see fail."""
import functools

import torch
import torch.nn.functional as F

import hubert_ref
from bf16_gates import GELU_LIP, MARGIN, attn_inputs, flip_bound, ulp_bf16  # noqa: F401  (re-exported for the tests)
from f32_gates import CAL_ROWS, _mm, _seed, family_rows, two_pass

EPS = 1e-5
KEY_TILE = 32


def rne64(x):
    """nearest bf16 value of every element, ties to even, in ONE rounding from x's own precision (x.double().bfloat16() would round an fp64
    value to fp32 first); returned in fp64"""
    x = x.double()
    _, e = torch.frexp(x)                                     # x = m 2^e, 0.5 <= |m| < 1
    e = e.clamp_min(-125)                                     # below 2^-126: the denormal spacing 2^-133
    return torch.ldexp(torch.round(torch.ldexp(x, 8 - e)), e - 8)          # torch.round: half to even


def rne(x, dt):
    return rne64(x).to(dt)


def trunc(x, dt):
    """the store mutant: the low 16 bits of the fp32 pattern dropped"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(dt)


def fold_bf16(W, b, gamma=None, beta=None):
    """(W' [N, K] bf16 values in fp64, b' fp32) of one Linear; gamma / beta: the LayerNorm folded in front of it"""
    W, b = W.double(), b.double()
    if gamma is None:
        return rne64(W), b.float()
    return rne64(W * gamma.double()), (b + W @ beta.double()).float()


def layer_weights(sd, l):
    k = f"encoder.layers.{l}."
    sc = (("q", 0.125), ("k", 1.0), ("v", 1.0))
    Wq = torch.cat([sd[k + f"attention.{p}_proj.weight"].double() * s for p, s in sc])
    bq = torch.cat([sd[k + f"attention.{p}_proj.bias"].double() * s for p, s in sc])
    return {"qkv": fold_bf16(Wq, bq, sd[k + "layer_norm.weight"], sd[k + "layer_norm.bias"]),
            "out_proj": fold_bf16(sd[k + "attention.out_proj.weight"], sd[k + "attention.out_proj.bias"]),
            "ffn_in": fold_bf16(sd[k + "feed_forward.intermediate_dense.weight"], sd[k + "feed_forward.intermediate_dense.bias"],
                                sd[k + "final_layer_norm.weight"], sd[k + "final_layer_norm.bias"]),
            "ffn_out": fold_bf16(sd[k + "feed_forward.output_dense.weight"], sd[k + "feed_forward.output_dense.bias"])}


def ln_operand(x, dt, store=rne):
    """the A operand of a LayerNorm Linear: normalise first (two-pass moments), then round"""
    x = x.to(dt)
    mean, rstd = two_pass(x, EPS)
    return store((x - mean) * rstd, dt)


def linear(A, W16, bias, dt, a_f32, act=0, R=None, out_bf16=False, reverse=False, store=rne, ln="first", gelu_before_bias=False):
    """dsh_op_gemm_bf16_pro on rows A [M, K]: act(pro(A) W'^T + bias) (+ R), stored in dt or rounded to bf16.
    Mutants: ln = "fold" is the fold-after-accumulate LayerNorm rstd (bf16(x) W'^T - mean fc) + b' (fc = row sums of W'), whose error scales
    with |x| instead of |x - mean|; store = trunc; gelu_before_bias."""
    W = W16.to(dt)
    if a_f32 and ln == "fold":
        x = A.to(dt)
        mean, rstd = two_pass(x, EPS)
        y = rstd * (_mm(store(x, dt), W, reverse) - mean * W.sum(1)[None, :])
    else:
        y = _mm(ln_operand(A, dt, store) if a_f32 else A.to(dt), W, reverse)
    if act == 2:
        y = F.gelu(y) + bias.to(dt) if gelu_before_bias else F.gelu(y + bias.to(dt))
    else:
        y = y + bias.to(dt)
    if R is not None:
        y = y + R.to(dt)
    return store(y, dt) if out_bf16 else y


def _bmm(a, b, reverse):
    """a [H, n, K] @ b [H, K, m]; fp32: one accumulator per output, K ascending (reverse: descending)"""
    if a.dtype != torch.float32:
        return a.flip(2) @ b.flip(1) if reverse else a @ b
    acc = torch.zeros(a.shape[0], a.shape[1], b.shape[2])
    for k in (range(a.shape[2] - 1, -1, -1) if reverse else range(a.shape[2])):
        acc.addcmul_(a[:, :, k:k + 1], b[:, k:k + 1, :])
    return acc


def attention(qkv, H, dt, lens=None, reverse=False, store=rne, l_rounded=False, key_delta=0, round_out=True):
    """dsh_op_softmax_attention_bf16[_ragged]: qkv [B, M, 3 H 64] holding bf16 values -> [B, M, H 64] in dt (bf16 values; round_out=False: o / l
    in front of the store, what assert_rounded compares a bf16 output with); rows behind lens[b] are 0 and no frame behind lens[b] is touched.
    Mutants: l_rounded sums the ROUNDED p into l; key_delta = +1 / -1 one key more / fewer (the key behind the row's frames, clamped to M);
    store = trunc."""
    B, M, _ = qkv.shape
    D = H * 64
    out = torch.zeros(B, M, D, dtype=dt)
    for b in range(B):
        n = M if lens is None else int(lens[b])
        nk = max(1, min(M, n + key_delta))
        q, k, v = (qkv[b, :, i * D:(i + 1) * D].to(dt).reshape(M, H, 64).permute(1, 0, 2) for i in range(3))        # [H, M, 64]
        q, k, v = q[:, :n], k[:, :nk], v[:, :nk]
        m_run = torch.full((H, n, 1), float("-inf"), dtype=dt)
        l = torch.zeros(H, n, 1, dtype=dt)
        o = torch.zeros(H, n, 64, dtype=dt)
        for k0 in range(0, nk, KEY_TILE):
            s = _bmm(q, k[:, k0:k0 + KEY_TILE].transpose(1, 2).contiguous(), reverse)
            m_new = torch.maximum(m_run, s.max(-1, keepdim=True).values)
            alpha = torch.exp(m_run - m_new)
            p = torch.exp(s - m_new)
            ph = store(p, dt)
            l = l * alpha + (ph if l_rounded else p).sum(-1, keepdim=True)
            o = o * alpha + _bmm(ph, v[:, k0:k0 + KEY_TILE].contiguous(), reverse)
            m_run = m_new
        y = o / l
        out[b, :n] = (store(y, dt) if round_out else y).permute(1, 0, 2).reshape(n, D)
    return out


def attn_flip_slack(qkv, H, lens=None):
    """What a p that rounds the other way may cost, per output element [B, M, H 64], from the fp64 operands alone (the form of
    bf16_gates.attn_flip_slack).  The kernel's logit s and the running maximum m are fp32 accumulations of 64 exact products in the matrix
    pipe's own order: each within 64 2^-23 sum_c |q_c k_c| of the exact value (bf16_gates.accum_bound), the maximum within the largest such
    bound of its row; the subtraction and a libm exp add 2^-22 (|s - m| + 2) relative on p.  Where the exact p lies within that eps p of a
    bf16 rounding tie the kernel may round it to the other neighbour: one ulp_bf16(p) on that key's weight, i.e. ulp(p_j) |v_j| / l on the
    output.  Exactly 0 for an output none of whose weights sits that close to a tie."""
    B, M, _ = qkv.shape
    D = H * 64
    out = torch.zeros(B, M, D, dtype=torch.float64)
    for b in range(B):
        n = M if lens is None else int(lens[b])
        q, k, v = (qkv[b, :n, i * D:(i + 1) * D].double().reshape(n, H, 64).permute(1, 0, 2) for i in range(3))
        m_run = torch.full((H, n, 1), float("-inf"), dtype=torch.float64)
        l = torch.zeros(H, n, 1, dtype=torch.float64)
        f = torch.zeros(H, n, 64, dtype=torch.float64)
        for k0 in range(0, n, KEY_TILE):
            kt = k[:, k0:k0 + KEY_TILE].transpose(1, 2)
            s = q @ kt
            acc = 64 * 2.0 ** -23 * (q.abs() @ kt.abs())
            acc_run = acc.max(-1, keepdim=True).values if k0 == 0 else torch.maximum(acc_run, acc.max(-1, keepdim=True).values)
            m_new = torch.maximum(m_run, s.max(-1, keepdim=True).values)
            alpha = torch.exp(m_run - m_new)
            p = torch.exp(s - m_new)
            u = ulp_bf16(p)
            tie = ((p / u) % 1.0 - 0.5).abs() * u
            flip = torch.where(tie <= (acc + acc_run + 2.0 ** -22 * ((s - m_new).abs() + 2)) * p, u, torch.zeros_like(p))
            l = l * alpha + p.sum(-1, keepdim=True)
            f = f * alpha + flip @ v[:, k0:k0 + KEY_TILE].abs()
            m_run = m_new
        out[b, :n] = (f / l).permute(1, 0, 2).reshape(n, D)
    return out


def front(sd, cfg, x, dt, reverse=False):
    """steps 1 .. 4 of hubert_ref.encode: h [B, M, hidden] as the positional convolution leaves it"""
    T = lambda k: sd[k].to(dt)
    h = hubert_ref.features(sd, cfg, x, dt, reverse)
    h = F.layer_norm(h, (h.shape[-1],), T("feature_projection.layer_norm.weight"), T("feature_projection.layer_norm.bias"), cfg["ln_eps"])
    h = _mm(h.reshape(-1, h.shape[-1]), T("feature_projection.projection.weight"), reverse).reshape(h.shape[:-1] + (-1,)) + \
        T("feature_projection.projection.bias")
    return hubert_ref.pos_conv(h, hubert_ref.pos_conv_weight(sd, dt), T(hubert_ref.POS + "bias"), cfg["pos_groups"], dt, reverse)


def layers(sd, cfg, h, dt, reverse=False, store=rne, ln="first", l_rounded=False, key_delta=0, gelu_before_bias=False, lens=None):
    """step 5 on h [B, M, hidden] in dt"""
    B, M, Hd = h.shape
    kw = dict(reverse=reverse, store=store)
    for l in range(cfg["layers"]):
        w = layer_weights(sd, l)
        x = h.reshape(B * M, Hd)
        qkv = linear(x, *w["qkv"], dt, True, out_bf16=True, ln=ln, **kw).reshape(B, M, 3 * Hd)
        att = attention(qkv, cfg["heads"], dt, lens=lens, l_rounded=l_rounded, key_delta=key_delta, **kw).reshape(B * M, Hd)
        x = linear(att, *w["out_proj"], dt, False, R=x, **kw)
        f = linear(x, *w["ffn_in"], dt, True, act=2, out_bf16=True, ln=ln, gelu_before_bias=gelu_before_bias, **kw)
        h = linear(f, *w["ffn_out"], dt, False, R=x, **kw).reshape(B, M, Hd)
    return h


def encode_bf16(sd, cfg, x, dt=torch.float64, reverse=False, **mutant):
    """last_hidden_state [B, M, hidden] of x [B, n] as the bf16 precision mode computes it, in dtype dt"""
    h = layers(sd, cfg, front(sd, cfg, x, dt, reverse), dt, reverse, **mutant)
    return F.layer_norm(h, (h.shape[-1],), sd["encoder.layer_norm.weight"].to(dt), sd["encoder.layer_norm.bias"].to(dt), cfg["ln_eps"])


# ---- operands and gates of the op tests (test_gpu_hubert_bf16_ops.py builds them here, test_hubert_bf16_cpu.py checks the gates on them) ----
# (bf16 store, act, residual aliased to C): the residual goes with the fp32 store
GEMM_COMBOS = [(True, 0, False), (True, 2, False), (False, 0, False), (False, 2, False), (False, 0, True), (False, 2, True)]


@functools.lru_cache(maxsize=4)
def gemm_case(K, N, kind, family, rows):
    """Operands of dsh_op_gemm_bf16_pro and the three pre-bias accumulations S = pro(A) W'^T (fp64, fp32 K ascending, fp32 K descending)
    over P = max(rows, CAL_ROWS) rows; a launch of M <= rows rows takes the first M.  kind "f32": LayerNorm rows of f32_gates.family_rows
    (the constant row of the "const" family is row 0, so every M has it); "bf16": bf16 rows, staged as they are."""
    P = max(rows, CAL_ROWS)
    g = torch.Generator().manual_seed(_seed("gemm_bf16_pro", K, N, kind, family))
    X = family_rows(family, P, K, g, 1) if kind == "f32" else (torch.randn(P, K, generator=g) * 1.5 + 0.3).bfloat16()
    t = {"X": X, "W": (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16(), "b": torch.randn(N, generator=g), "R": torch.randn(P, N, generator=g)}
    zero = torch.zeros(N)
    S = lambda dt, rev: linear(X, t["W"], zero, dt, kind == "f32", reverse=rev)
    t["S64"], t["S32"] = S(torch.float64, False), (S(torch.float32, False), S(torch.float32, True))
    t["flip"] = flip_bound(ln_operand(X, torch.float64), t["W"]) if kind == "f32" else torch.zeros(P, N, dtype=torch.float64)
    return t


def gemm_epilogue(S, t, act, res):
    y = S + t["b"].to(S.dtype)
    if act == 2:
        y = F.gelu(y)
    return y + t["R"].to(S.dtype) if res else y


def gemm_gate(t, K, kind, family, act, res, own_moments=True):
    """(ref64 in front of the store [P, N], slack [P, N]): MARGIN x max |chain32 - ref64| over both K orders and all P rows, plus one flip of
    the LayerNorm operand (through the GELU's Lipschitz constant), plus const_row_slack on the constant row when the op computes the moments"""
    ref64 = gemm_epilogue(t["S64"], t, act, res)
    cal = max(float((gemm_epilogue(s, t, act, res).double() - ref64).abs().max()) for s in t["S32"])
    slack = MARGIN * cal + t["flip"] * (GELU_LIP if act == 2 else 1.0)
    if kind == "f32" and family == "const" and own_moments:
        slack[0] += const_row_slack(K, float(t["X"][0, 0]), t["W"], act)
    return ref64, slack


def attn_qkv(B, M, H, family):
    """bf16_gates.attn_inputs at 64-wide heads with the q part scaled by 1 / 8 (exact in bf16), as the encoder's q rows are"""
    x = attn_inputs(B, M, family, D=H * 64, hd=64)
    x[:, :, :H * 64] *= 0.125
    return x


def attn_gate(qkv, H, lens=None):
    """(ref64 in front of the store, slack) [B, M, H 64]: MARGIN x max |chain32 - ref64| over both orders, plus attn_flip_slack"""
    r64 = attention(qkv, H, torch.float64, lens=lens, round_out=False)
    cal = max(float((attention(qkv, H, torch.float32, lens=lens, reverse=rev, round_out=False).double() - r64).abs().max()) for rev in (False, True))
    return r64, MARGIN * cal + attn_flip_slack(qkv, H, lens)


def const_row_slack(K, c, W16, act=0):
    """An all-constant LayerNorm row (every channel = c) in front of a Linear.  The moments launch adds the K / 64 channels of a lane one after
    the other and joins the 64 lanes by a butterfly, which doubles equal partial sums exactly: the row sum carries the K / 64 - 1 roundings of
    a lane's chain, each at most 2^-24 of a partial sum <= (K / 64) |c|, so the mean is off by at most delta = (K / 64 - 1) 2^-24 |c| (torch's
    sum happens to be exact on such rows, so no chain shows the term).  Every channel is then -delta instead of 0, the variance is
    delta^2 << eps, rstd = eps^-1/2, and the operand row is the constant delta eps^-1/2 (its bf16 rounding included in the factor 1 + 2^-8):
    |y_n - b'_n| <= delta eps^-1/2 (1 + 2^-8) sum_k |W'_nk|, through the GELU's Lipschitz constant where there is one.  (At K = 128 a lane adds c + c, which is exact: the bound is
    not attained there.)  Moments passed in by the caller (K = 4096 in the op test) are torch's and carry no such term."""
    delta = (-(-K // 64) - 1) * 2.0 ** -24 * abs(c)
    return delta * EPS ** -0.5 * (1 + 2.0 ** -8) * W16.double().abs().sum(1) * (GELU_LIP if act == 2 else 1.0)
