"""The token-side kernels -- csrc/attention.hip, csrc/vit.hip, the attention / LayerNorm / depth-wise parts of csrc/segformer.hip, transpose_heads
and softmax_* of csrc/elementwise.hip -- launched through the C ABI on canary-guarded operands (tests/strided_util.py) and compared with the
hand-written float64 references of tests/token_ref.py (held to torch autograd by tests/test_token_ref_host.py) on the 16-bit-rounded inputs.

Every case asserts
  (a) every canary is intact: inputs sit between NaN guard rows (a load of a row >= T that reaches the result poisons it), outputs between
      bit-pattern guard rows (a store past the last row, or into the side channels of a strided operand, is seen);
  (b) every role-"out" view is fully written and no output holds a NaN;
  (c) accumulated outputs (dgamma / dbeta, dw / dbias) start from NON-ZERO values and end at start + gradient;
  (d) the norm-wise bound the existing test of the same op uses (quoted at each *_TOL below), and a per-row bound (strided_util.row_errors:
      the row's error relative to the RMS row norm) on every [.., rows, C] output;
  (e) L / lse within 2^-12 absolute of the float64 logsumexp of the scaled logits: an error d in L multiplies every P the backward
      recomputes by e^d, so d has to stay below the fp16 rounding (2^-11 relative) that P then receives;
  (f) entry points that take strides (jg_vit_attention_*, jg_attn_smallkv_*, jg_transpose_heads) run through run_pair: the layout the model uses
      (q / k / v three channel views of ONE packed operand: ld = 3C, head_stride = head_dim; ldkv = 2C) and the ABI_MIN placement; plain-store
      outputs bit-equal between the two, dk / dv of smallkv (fp32 atomics, then rounded) within one rounding (TOL16) of each other.

Input regimes: "flat" = N(0, 1) rounded to the 16-bit type (outputs and gradients compared); "peaked" (attention forwards only) = q, k ~
N(0, 2.5^2), logit standard deviation about 6, softmax close to one-hot, the running maximum moves between chunks and lanes.  Gradients are not
compared there: with a one-hot row dP - Dq cancels down to the 16-bit rounding of O and float64 is no fair yardstick for a correct kernel.

Per-row bound = ROW_FACTOR (4) x the norm-wise bound of that output: independent 16-bit roundings give a row the same expected relative error as
the whole tensor, the factor covers the spread over at most 4096 rows (32000 in the two tiles_per_wave = 2 cases).  Checked on the CPU against
the float32 emulation of token_ref.py (prec = the 16-bit type: P, dS and every output rounded as the kernels round them), same seeds, worst row
of emulation vs float64 over all cases of the op, as a fraction of the per-row bound [fp16, bf16]; below one half everywhere, so the factor
stays 4 for every output:
  jg_attention_fwd/_bwd      a flat [0.061, 0.054] peaked [0.047, 0.050]   dqkv [0.054, 0.047]
  jg_vit_attention_fwd/_bwd  o flat [0.079, 0.086] peaked [0.048, 0.079]   dq / dk / dv [0.042, 0.063]
  jg_attn_smallkv_fwd/_bwd2  o flat [0.036, 0.044] peaked [0.037, 0.043]   dq [0.049, 0.055]   dkv [0.053, 0.042]
  LayerNorm family           y [0.027, 0.031]   dx [0.027, 0.030]   xsum [0.026, 0.030]
  jg_dwconv3x3_*             pre / y [0.024, 0.027]   du [0.011, 0.016]   dx [0.018, 0.021]
  jg_softmax_fwd/_bwd        P [0.152, 0.143]   dS [0.172, 0.192]
Measured |L - float64 logsumexp| of the float32 evaluation (max over all cases, both regimes): jg_attention 6.5e-6, jg_vit_attention 8.6e-6,
jg_attn_smallkv 1.1e-5 -- more than an order of magnitude under the 2^-12 = 2.4e-4 bound.

tiles_per_wave = 2 (SMALLKV_TPW2 below): the dispatch rule of jg_attn_smallkv_fwd / _bwd2 (csrc/segformer.hip) is
    ntiles = (Tq + 63) / 64;  tpw = 1;
    while (tpw < 8 && 4 * tpw * 2 <= ntiles && ((ntiles + 4 * tpw * 2 - 1) / (4 * tpw * 2)) * heads * B >= 512) tpw *= 2;
    grid.x = (ntiles + 4 * tpw - 1) / (4 * tpw)
At Tq = 4000, heads * B = 64: ntiles = 63; tpw 1 -> 2 (8 <= 63, ceil(63 / 8) * 64 = 512 >= 512); 2 -> 4 refused (ceil(63 / 16) * 64 = 256 < 512).
grid.x = 8 blocks of 4 waves x 2 tiles = 64 tile slots for 63 tiles: one dead trailing slot (live == false), last live tile 4000 - 62 * 64 = 32 queries.
"""
import math

import pytest
import torch

import strided_util as su
import token_ref as tr
from strided_util import Operand

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
G = 32                    # guard rows: a multiple of 8 rows of any row length keeps the view 16-byte aligned; 32 so that a 64-key tile read
#                           unmasked at Tkv = 37 (27 rows past the end) still lands in the NaN guard, not outside the allocation
ROW_FACTOR = 4
L_BOUND = 2.0 ** -12
TOL16 = {torch.float16: 1e-3, torch.bfloat16: 8e-3}          # tests/test_gpu_0_ops.py:18 (TOL)
ATTN_TOL = {"a": 2, "dqkv": 4}                              # x TOL16: tests/test_gpu_0_ops.py:739-740 (test_attention_core)
VIT_TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}      # tests/test_gpu_8_projd_vit.py:19; forward :56, gradients 2.5 x (:62)
SEG_TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}        # tests/test_gpu_4_segformer.py:16; smallkv o :181, gradients 2 x (:182);
#                                                              LayerNorm y / dx :48, dgamma / dbeta 1e-3 (:49), add forms 2 x (:104);
#                                                              dwconv y :126, dx / dw / dbias 2 x (:126-127)
LN_PARAM_TOL = 1e-3
STAT_BOUND = 1e-5         # mr = (mean, rstd) in fp32: a sum tree of depth <= 14 over |x| < 8 errs by < 14 * 2^-24 * 8 = 7e-6 (absolute, mean); the
#                           rstd of it by a few fp32 roundings (relative)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _ld(v):
    assert v.stride(-1) == 1
    return v.stride(-2)


def _code(dtype):
    from joligen_amd import _lib

    return _lib.JG_F16 if dtype == torch.float16 else _lib.JG_BF16


def _st():
    from joligen_amd import ops

    return ops._st()


def _L():
    from joligen_amd import _lib

    return _lib.lib()


def p(v, off=0):
    return None if v is None else v.data_ptr() + off * v.element_size()


def rnd(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def tok(B, T, C):
    return (B, 1, T, C)


def mat(R, C):
    return (1, 1, R, C)


def d64(v):
    return v.detach().double().cpu()


def _pair(launch, operands, fixed=(), share=None):
    return su.run_pair(launch, operands, kind=su.ABI_MIN, device=dev(), guard=G, fixed=fixed, share=share)


class Once:
    """one launch on contiguous guarded operands: entry points without stride arguments"""

    def __init__(self, operands):
        self.bufs, self.v = {}, {}
        for name, op in operands.items():
            self.bufs[name], self.v[name] = su.make_slice(op.shape, op.dtype, op.seed, left=0, right=0, guard=G, role=op.role, values=op.values,
                                                          scale=op.scale, device=dev())

    def check(self, unwritten=()):
        """(a) and (b); names in `unwritten` must still hold the pre-fill everywhere (a refused launch)"""
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            try:
                su.assert_canary_intact(buf)
                if buf.spec.role == "out" and name not in unwritten:
                    su.assert_fully_written(buf)
            except AssertionError as e:
                raise AssertionError(f"operand {name!r}: {e}") from None
            if buf.spec.role != "in":
                assert not bool(torch.isnan(self.v[name].float()).any()), f"NaN in output {name!r}"
        for name in unwritten:
            v = self.v[name]
            idt = su._INT[v.element_size()]
            assert bool((v.contiguous().view(idt) == su._patterns(v.dtype)[1]).all()), f"a refused launch wrote into {name!r}"


def close(got, ref, tol, what, rows=True):
    """(d): norm-wise bound, then the per-row bound"""
    e = su.relerr(got, ref)
    assert e < tol, f"{what}: {e:.3e} against the float64 reference (bound {tol:.1e})"
    if rows:
        su.assert_rows_close(got, ref, ROW_FACTOR * tol, what)


def lse_close(got, ref, what):
    e = float((d64(got).reshape(-1) - ref.reshape(-1)).abs().max())
    assert e <= L_BOUND, f"{what}: |L - logsumexp| = {e:.3e} (bound 2^-12 = {L_BOUND:.2e})"


def acc_close(got, start, grad, tol, what):
    """(c): an accumulated output ends at start + gradient"""
    e = su.relerr(got, start.double() + grad)
    assert e < tol, (f"{what}: {e:.3e} from start + gradient (bound {tol:.1e}); from the gradient alone {su.relerr(got, grad):.3e} -- "
                     f"the kernel has to ADD to what the buffer holds")


def peak(x, regime):
    return x * 2.5 if regime == "peaked" else x


# ======================================================================================================================================
# jg_attention_fwd / _bwd: legacy layout, head dim 32, T % 128 == 0; no stride arguments
# ======================================================================================================================================
ATTN_CASES = [(2, 2, 128), (1, 3, 384), (2, 1, 256)]        # (B, heads, T): 1, 3 (odd: the double-buffer parity) and 2 key chunks
REGIMES = ["flat", "peaked"]


def attn_inputs(case, regime, dtype):
    B, heads, T = case
    x = torch.randn((B, T, heads, 3, 32), generator=torch.Generator().manual_seed(61))
    x[:, :, :, :2] = peak(x[:, :, :, :2], regime)
    return x.reshape(B, T, heads * 96).to(dtype), rnd((B, T, heads * 32), dtype, 62)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_attention_legacy(case, regime, dtype):
    from joligen_amd import _lib

    B, heads, T = case
    C = heads * 32
    qkv, da = attn_inputs(case, regime, dtype)
    o = Once({"qkv": Operand(tok(B, T, 3 * C), dtype, "in", values=qkv), "a": Operand(tok(B, T, C), dtype, "out"),
              "L": Operand(mat(B * heads, T), torch.float32, "out"), "da": Operand(tok(B, T, C), dtype, "in", values=da),
              "dqkv": Operand(tok(B, T, 3 * C), dtype, "out"), "Dq": Operand(mat(B * heads, T), torch.float32, "out")})
    v = o.v
    _lib.check(_L().jg_attention_fwd(_code(dtype), p(v["qkv"]), p(v["a"]), p(v["L"]), B, T, heads, 32, _st()), "jg_attention_fwd")
    if regime == "peaked":
        o.check(unwritten=("dqkv", "Dq"))
        ref = tr.attention_legacy(qkv.double(), heads)
    else:
        _lib.check(_L().jg_attention_bwd(_code(dtype), p(v["qkv"]), p(v["a"]), p(v["L"]), p(v["da"]), p(v["dqkv"]), p(v["Dq"]), B, T, heads, 32, _st()),
                   "jg_attention_bwd")
        o.check()
        ref = tr.attention_legacy(qkv.double(), heads, da.double())
        close(v["dqkv"][:, 0], ref["dqkv"], ATTN_TOL["dqkv"] * TOL16[dtype], "dqkv")
        close(v["Dq"][0, 0], ref["D"], ATTN_TOL["dqkv"] * TOL16[dtype], "Dq", rows=False)
    close(v["a"][:, 0], ref["a"], ATTN_TOL["a"] * TOL16[dtype], "a")
    lse_close(v["L"], ref["L"], "L")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T,hd", [(200, 32), (128, 16)])
def test_attention_legacy_refuses(T, hd, dtype):
    from joligen_amd import _lib

    B, heads = 1, 2
    C = heads * hd
    o = Once({"qkv": Operand(tok(B, T, 3 * C), dtype, "in", 1), "a": Operand(tok(B, T, C), dtype, "out"),
              "L": Operand(mat(B * heads, T), torch.float32, "out"), "da": Operand(tok(B, T, C), dtype, "in", 2),
              "dqkv": Operand(tok(B, T, 3 * C), dtype, "out"), "Dq": Operand(mat(B * heads, T), torch.float32, "out")})
    v = o.v
    assert _L().jg_attention_fwd(_code(dtype), p(v["qkv"]), p(v["a"]), p(v["L"]), B, T, heads, hd, _st()) == _lib.JG_ERR_UNSUPPORTED
    assert _L().jg_attention_bwd(_code(dtype), p(v["qkv"]), p(v["a"]), p(v["L"]), p(v["da"]), p(v["dqkv"]), p(v["Dq"]), B, T, heads, hd,
                                 _st()) == _lib.JG_ERR_UNSUPPORTED
    o.check(unwritten=("a", "L", "dqkv", "Dq"))


# ======================================================================================================================================
# jg_transpose_heads (strides: ldsrc, coff, hstride), jg_softmax_fwd / _bwd
# ======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [37, 130])
@pytest.mark.parametrize("ch", [16, 32])
def test_transpose_heads(ch, T, dtype):
    from joligen_amd import _lib

    B, nh = 2, 3
    C3 = 3 * nh * ch
    for coff in (0, ch, 2 * ch):
        def launch(v):
            _lib.check(_L().jg_transpose_heads(_code(dtype), p(v["src"]), _ld(v["src"]), coff, 3 * ch, p(v["dst"]), B, T, nh, ch, _st()), "jg_transpose_heads")

        pair = _pair(launch, {"src": Operand(tok(B, T, C3), dtype, "in", 5), "dst": Operand(mat(B * nh * ch, T), dtype, "out")}, fixed=("dst",))
        su.verify(pair, exact=["dst"])
        for views in (pair.contig, pair.strided):
            want = views["src"][:, 0].reshape(B, T, nh, 3 * ch)[..., coff:coff + ch].permute(0, 2, 3, 1).reshape(B * nh * ch, T)
            assert torch.equal(views["dst"][0, 0], want), (ch, coff)


def softmax_inputs(rows, T):
    S = torch.randn((rows, T), generator=torch.Generator().manual_seed(7)) * 3.0
    S[0, ::3] = float("-inf")               # masked entries: P = 0 there, finite everywhere (index 1 is never masked)
    S[rows - 1, 1] += 80.0                  # one logit about 80 above the rest: exp(-80) underflows nothing, the row is one-hot
    return S, torch.randn((rows, T), generator=torch.Generator().manual_seed(8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [1, 37, 130])
def test_softmax(rows, dtype):
    """rows not a multiple of the 4 rows of a block; T = 4 leaves 63 lanes without an element, 260 and 1028 are n4 = 65 and 257 (not a multiple
    of 64).  dS against the reference evaluated on the kernel's own rounded P, its input."""
    from joligen_amd import _lib

    alpha = 1.0 / math.sqrt(32)
    for T in (4, 96, 260, 1028):
        S, dP = softmax_inputs(rows, T)
        o = Once({"S": Operand(mat(rows, T), torch.float32, "in", values=S), "P": Operand(mat(rows, T), dtype, "out"),
                  "dP": Operand(mat(rows, T), torch.float32, "in", values=dP), "dS": Operand(mat(rows, T), dtype, "out")})
        v = o.v
        _lib.check(_L().jg_softmax_fwd(_code(dtype), p(v["S"]), p(v["P"]), rows, T, _st()), "jg_softmax_fwd")
        _lib.check(_L().jg_softmax_bwd(_code(dtype), p(v["P"]), p(v["dP"]), p(v["dS"]), rows, T, alpha, _st()), "jg_softmax_bwd")
        o.check()
        P, dS = d64(v["P"][0, 0]), d64(v["dS"][0, 0])
        assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(dS).all()), T
        assert float(P[0, ::3].abs().max()) == 0.0 and float(dS[0, ::3].abs().max()) == 0.0, T
        close(P, torch.softmax(S.double(), -1), TOL16[dtype], f"P at T = {T}")
        close(dS, alpha * P * (dP.double() - (dP.double() * P).sum(-1, keepdim=True)), TOL16[dtype], f"dS at T = {T}")


# ======================================================================================================================================
# jg_vit_attention_fwd / _bwd (strides: ld, head_stride, ldd)
# ======================================================================================================================================
VIT_CASES = [(257, 2, 64, 2), (37, 3, 32, 2), (1, 2, 64, 1), (64, 2, 32, 1), (65, 1, 32, 2)]     # (T, heads, hd, B); 65: one key into the second chunk


def vit_inputs(case, regime, dtype):
    T, heads, hd, B = case
    C = heads * hd
    x = torch.randn((B, T, 3 * C), generator=torch.Generator().manual_seed(31))
    x[..., :2 * C] = peak(x[..., :2 * C], regime)
    return x.to(dtype), rnd((B, T, C), dtype, 32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", VIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_vit_attention(case, regime, dtype):
    from joligen_amd import _lib

    T, heads, hd, B = case
    C, scale, bwd = heads * hd, hd ** -0.5, regime == "flat"
    qkv, do = vit_inputs(case, regime, dtype)
    operands = {"qkv": Operand(tok(B, T, 3 * C), dtype, "in", values=qkv), "o": Operand(tok(B, T, C), dtype, "out"),
                "L": Operand(mat(B * heads, T), torch.float32, "out")}
    if bwd:
        operands.update({"do": Operand(tok(B, T, C), dtype, "in", values=do), "dqkv": Operand(tok(B, T, 3 * C), dtype, "out"),
                         "Dq": Operand(mat(B * heads, T), torch.float32, "out")})

    def launch(v):
        x, ld = v["qkv"], _ld(v["qkv"])
        _lib.check(_L().jg_vit_attention_fwd(_code(dtype), p(x), p(x, C), p(x, 2 * C), ld, hd, p(v["o"]), p(v["L"]), B, T, heads, hd, scale, _st()),
                   "jg_vit_attention_fwd")
        if bwd:
            g = v["dqkv"]
            _lib.check(_L().jg_vit_attention_bwd(_code(dtype), p(x), p(x, C), p(x, 2 * C), ld, hd, p(v["o"]), p(v["L"]), p(v["do"]), p(g), p(g, C),
                                                 p(g, 2 * C), _ld(g), p(v["Dq"]), B, T, heads, hd, scale, _st()), "jg_vit_attention_bwd")

    pair = _pair(launch, operands, fixed=("o", "L", "do", "Dq"))
    assert _ld(pair.contig["qkv"]) == 3 * C and _ld(pair.strided["qkv"]) > 3 * C
    su.verify(pair, exact=["o", "L"] + (["dqkv", "Dq"] if bwd else []))
    ref = tr.attention_timm(qkv.double(), heads, scale, do.double() if bwd else None)
    v = pair.strided
    close(v["o"][:, 0], ref["o"], VIT_TOL[dtype], "o")
    lse_close(v["L"], ref["L"], "L")
    if bwd:
        for i, n in enumerate(("dq", "dk", "dv")):
            if T == 1 and n != "dv":        # one key: softmax = 1, dq and dk are exactly zero (tests/test_gpu_8_projd_vit.py:59-60, same bound)
                assert float(ref["dqkv"][..., i * C:(i + 1) * C].abs().max()) < 1e-12
                assert float(v["dqkv"][:, 0, :, i * C:(i + 1) * C].float().abs().max()) < 1e-5, n
                continue
            close(v["dqkv"][:, 0, :, i * C:(i + 1) * C], ref["dqkv"][..., i * C:(i + 1) * C], 2.5 * VIT_TOL[dtype], n)
        close(v["Dq"][0, 0], ref["D"], 2.5 * VIT_TOL[dtype], "Dq", rows=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vit_attention_refuses_head_dim_16(dtype):
    from joligen_amd import _lib

    T, heads, hd, B = 37, 2, 16, 1
    C = heads * hd
    o = Once({"qkv": Operand(tok(B, T, 3 * C), dtype, "in", 1), "o": Operand(tok(B, T, C), dtype, "out"), "L": Operand(mat(B * heads, T), torch.float32, "out")})
    x = o.v["qkv"]
    assert _L().jg_vit_attention_fwd(_code(dtype), p(x), p(x, C), p(x, 2 * C), 3 * C, hd, p(o.v["o"]), p(o.v["L"]), B, T, heads, hd, 0.25,
                                     _st()) == _lib.JG_ERR_UNSUPPORTED
    o.check(unwritten=("o", "L"))


# ======================================================================================================================================
# jg_attn_smallkv_fwd / _bwd2 (strides: ldq, ldkv, ldo, lddkv)
# ======================================================================================================================================
SMALLKV_SMALL = [(1, 70, 37, 2), (2, 64, 64, 1),         # (B, Tq, Tkv, heads): the matrix-core kernel (Tkv <= 64), ragged queries and keys
                 (1, 100, 65, 2), (1, 70, 256, 1)]       # the scalar kernel: just above 64 keys, and at AKV_MAX
# tiles_per_wave = 2 by the dispatch rule quoted in the module text (ntiles = 63, heads * B = 64): one dead trailing tile slot, a last live tile of
# 32 queries; with 64 keys and with a ragged key tail
SMALLKV_TPW2 = [(8, 4000, 64, 8), (8, 4000, 37, 8)]


def smallkv_inputs(case, regime, dtype):
    B, Tq, Tkv, heads = case
    C = heads * 32
    q = peak(torch.randn((B, Tq, C), generator=torch.Generator().manual_seed(9)), regime)
    kv = torch.randn((B, Tkv, 2 * C), generator=torch.Generator().manual_seed(10))
    kv[..., :C] = peak(kv[..., :C], regime)
    return q.to(dtype), kv.to(dtype), rnd((B, Tq, C), dtype, 11)


def _smallkv(case, regime, dtype, acc_pair):
    from joligen_amd import _lib

    B, Tq, Tkv, heads = case
    C, scale, bwd = heads * 32, 1.0 / math.sqrt(32.0), regime == "flat"
    nkv = B * Tkv * C
    q, kv, do = smallkv_inputs(case, regime, dtype)
    operands = {"q": Operand(tok(B, Tq, C), dtype, "in", values=q), "kv": Operand(tok(B, Tkv, 2 * C), dtype, "in", values=kv),
                "o": Operand(tok(B, Tq, C), dtype, "out"), "lse": Operand(mat(B * heads, Tq), torch.float32, "out")}
    fixed, share = ["lse"], {}
    if bwd:
        operands.update({"do": Operand(tok(B, Tq, C), dtype, "in", values=do), "dq": Operand(tok(B, Tq, C), dtype, "out"),
                         "dkv": Operand(tok(B, Tkv, 2 * C), dtype, "out")})
        share = {"do": "o", "dq": "q"}            # the ABI has ONE stride for q and dq (ldq), one for o and dout (ldo)
        if acc_pair:                              # dvf == dkf + nkv: one fill
            operands["acc"] = Operand(mat(2 * B * Tkv, C), torch.float32, "out")
            fixed += ["acc"]
        else:                                     # two fills
            operands["dkf"], operands["dvf"] = Operand(mat(B * Tkv, C), torch.float32, "out"), Operand(mat(B * Tkv, C), torch.float32, "out")
            fixed += ["dkf", "dvf"]

    def launch(v):
        _lib.check(_L().jg_attn_smallkv_fwd(_code(dtype), p(v["q"]), p(v["kv"]), p(v["kv"], C), p(v["o"]), p(v["lse"]), B, Tq, Tkv, heads, _ld(v["q"]),
                                            _ld(v["kv"]), _ld(v["o"]), scale, _st()), "jg_attn_smallkv_fwd")
        if bwd:
            assert _ld(v["dq"]) == _ld(v["q"]) and _ld(v["do"]) == _ld(v["o"])
            dkf, dvf = (p(v["acc"]), p(v["acc"], nkv)) if acc_pair else (p(v["dkf"]), p(v["dvf"]))
            _lib.check(_L().jg_attn_smallkv_bwd2(_code(dtype), p(v["q"]), p(v["kv"]), p(v["kv"], C), p(v["o"]), p(v["do"]), p(v["lse"]), p(v["dq"]), dkf,
                                                 dvf, p(v["dkv"]), p(v["dkv"], C), _ld(v["dkv"]), B, Tq, Tkv, heads, _ld(v["q"]), _ld(v["kv"]),
                                                 _ld(v["o"]), scale, _st()), "jg_attn_smallkv_bwd2")

    pair = _pair(launch, operands, fixed=fixed, share=share)
    assert _ld(pair.contig["kv"]) == 2 * C and _ld(pair.strided["kv"]) > 2 * C
    su.verify(pair, exact=["o", "lse"] + (["dq"] if bwd else []), approx={"dkv": TOL16[dtype]} if bwd else None)
    ref = tr.attention_smallkv(q.double(), kv.double(), heads, scale, do.double() if bwd else None)
    v = pair.strided
    close(v["o"][:, 0], ref["o"], SEG_TOL[dtype], "o")
    lse_close(v["lse"], ref["lse"], "lse")
    if bwd:
        close(v["dq"][:, 0], ref["dq"], 2 * SEG_TOL[dtype], "dq")
        close(v["dkv"][:, 0], ref["dkv"], 2 * SEG_TOL[dtype], "dkv")
        close(pair.contig["dkv"][:, 0], ref["dkv"], 2 * SEG_TOL[dtype], "dkv (contiguous launch)")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("acc_pair", [True, False], ids=["one-fill", "two-fills"])
@pytest.mark.parametrize("case", SMALLKV_SMALL, ids=lambda c: "x".join(map(str, c)))
def test_attn_smallkv(case, acc_pair, dtype):
    _smallkv(case, "flat", dtype, acc_pair)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", SMALLKV_SMALL + SMALLKV_TPW2, ids=lambda c: "x".join(map(str, c)))
def test_attn_smallkv_peaked_forward(case, dtype):
    _smallkv(case, "peaked", dtype, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", SMALLKV_TPW2, ids=lambda c: "x".join(map(str, c)))
def test_attn_smallkv_two_tiles_per_wave(case, dtype):
    _smallkv(case, "flat", dtype, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attn_smallkv_refuses_257_keys(dtype):
    from joligen_amd import _lib

    B, Tq, Tkv, heads, C = 1, 70, 257, 1, 32
    o = Once({"q": Operand(tok(B, Tq, C), dtype, "in", 1), "kv": Operand(tok(B, Tkv, 2 * C), dtype, "in", 2), "o": Operand(tok(B, Tq, C), dtype, "out"),
              "lse": Operand(mat(B * heads, Tq), torch.float32, "out"), "do": Operand(tok(B, Tq, C), dtype, "in", 3),
              "dq": Operand(tok(B, Tq, C), dtype, "out"), "dkv": Operand(tok(B, Tkv, 2 * C), dtype, "out"),
              "acc": Operand(mat(2 * B * Tkv, C), torch.float32, "out")})
    v = o.v
    assert _L().jg_attn_smallkv_fwd(_code(dtype), p(v["q"]), p(v["kv"]), p(v["kv"], C), p(v["o"]), p(v["lse"]), B, Tq, Tkv, heads, C, 2 * C, C, 0.2,
                                    _st()) == _lib.JG_ERR_UNSUPPORTED
    assert _L().jg_attn_smallkv_bwd2(_code(dtype), p(v["q"]), p(v["kv"]), p(v["kv"], C), p(v["o"]), p(v["do"]), p(v["lse"]), p(v["dq"]), p(v["acc"]),
                                     p(v["acc"], B * Tkv * C), p(v["dkv"]), p(v["dkv"], C), 2 * C, B, Tq, Tkv, heads, C, 2 * C, C, 0.2,
                                     _st()) == _lib.JG_ERR_UNSUPPORTED
    o.check(unwritten=("o", "lse", "dq", "dkv", "acc"))


# ======================================================================================================================================
# LayerNorm family: jg_layernorm_fwd, _bwd, _fwd_add, _bwd_add, _bwd_add2, jg_layernorm_bwd_res; no stride arguments
# ======================================================================================================================================
LN_CASES = [(3, 8), (77, 160), (130, 504), (5, 512), (1000, 64)]
EPS = 1e-6
SCALES = [0.0, 1 / 0.7, 0.5, 1 / 0.7, 1.0]


def ln_rows_per_image(R):
    """odd, so that it divides the row count of no block (4 waves of 64 / lanes_per_row rows: a power of two)"""
    return (R // 3) | 1


def ln_inputs(R, C, dtype):
    return dict(x=rnd((R, C), dtype, 1), add=rnd((R, C), dtype, 2), dy=rnd((R, C), dtype, 3), res=rnd((R, C), dtype, 4),
                gamma=1 + 0.2 * rnd((C,), torch.float32, 5), beta=0.1 * rnd((C,), torch.float32, 6),
                g0=rnd((C,), torch.float32, 7, math.sqrt(R)), b0=rnd((C,), torch.float32, 8, math.sqrt(R)))


def _mr_close(mr, x16, what):
    m = d64(x16).mean(-1)
    r = 1.0 / torch.sqrt(d64(x16).var(-1, unbiased=False) + EPS)
    got = d64(mr)
    assert float((got[:, 0] - m).abs().max()) < STAT_BOUND, (what, float((got[:, 0] - m).abs().max()))
    assert float(((got[:, 1] - r) / r).abs().max()) < STAT_BOUND, (what, float(((got[:, 1] - r) / r).abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("full", [False, True], ids=["scale-res-NULL", "scale-res"])
@pytest.mark.parametrize("R,C", LN_CASES)
def test_layernorm_family(R, C, full, dtype):
    """full: scale and res non-NULL where the entry point takes them (jg_layernorm_bwd_add always gets a res: without one it IS jg_layernorm_bwd).
    dgamma / dbeta accumulate from N(0, R) start values, the size of the gradient itself."""
    from joligen_amd import _lib

    t = ln_inputs(R, C, dtype)
    rpi = ln_rows_per_image(R)
    nimg = (R + rpi - 1) // rpi
    scale = torch.tensor(SCALES[:nimg]) if full else None
    sc = tr.image_scale(scale, rpi, R, torch.float64)
    code, tol = _code(dtype), SEG_TOL[dtype]
    gm, bt = t["gamma"].double(), t["beta"].double()
    vec = lambda n: Operand(mat(1, C), torch.float32, "in", values=t[n])
    rows = lambda n: Operand(mat(R, C), dtype, "in", values=t[n])
    out = lambda: Operand(mat(R, C), dtype, "out")
    acc = lambda n: Operand(mat(1, C), torch.float32, "acc", values=t[n])

    # jg_layernorm_fwd, then jg_layernorm_bwd on its mr
    o = Once({"x": rows("x"), "gamma": vec("gamma"), "beta": vec("beta"), "y": out(), "mr": Operand(mat(R, 2), torch.float32, "out")})
    v = o.v
    _lib.check(_L().jg_layernorm_fwd(code, p(v["x"]), p(v["gamma"]), p(v["beta"]), p(v["y"]), p(v["mr"]), R, C, EPS, _st()), "jg_layernorm_fwd")
    o.check()
    close(v["y"][0, 0], tr.layernorm_fwd(t["x"].double(), gm, bt, EPS)[0], tol, "y")
    _mr_close(v["mr"][0, 0], t["x"], "mr")
    mr = v["mr"][0, 0].cpu()
    mr_in = lambda m=mr: Operand(mat(R, 2), torch.float32, "in", values=m)

    o = Once({"x": rows("x"), "dy": rows("dy"), "gamma": vec("gamma"), "mr": mr_in(), "dx": out(), "dgamma": acc("g0"), "dbeta": acc("b0")})
    v = o.v
    _lib.check(_L().jg_layernorm_bwd(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), p(v["dx"]), p(v["dgamma"]), p(v["dbeta"]), R, C, _st()),
               "jg_layernorm_bwd")
    o.check()
    dx, dg, db = tr.layernorm_bwd(t["x"].double(), t["dy"].double(), gm, EPS)
    close(v["dx"][0, 0], dx, tol, "dx")
    acc_close(v["dgamma"][0, 0, 0], t["g0"], dg, LN_PARAM_TOL, "dgamma")
    acc_close(v["dbeta"][0, 0, 0], t["b0"], db, LN_PARAM_TOL, "dbeta")

    # jg_layernorm_fwd_add: xsum = x + add * scale[image], y = LayerNorm of the ROUNDED sum -- the reference of y and mr reads the kernel's xsum
    ops = {"x": rows("x"), "add": rows("add"), "gamma": vec("gamma"), "beta": vec("beta"), "xsum": out(), "y": out(),
           "mr": Operand(mat(R, 2), torch.float32, "out")}
    if full:
        ops["scale"] = Operand(mat(1, nimg), torch.float32, "in", values=scale)
    o = Once(ops)
    v = o.v
    _lib.check(_L().jg_layernorm_fwd_add(code, p(v["x"]), p(v["add"]), p(v.get("scale")), rpi, p(v["xsum"]), p(v["gamma"]), p(v["beta"]), p(v["y"]),
                                         p(v["mr"]), R, C, EPS, _st()), "jg_layernorm_fwd_add")
    o.check()
    xsum = v["xsum"][0, 0].cpu()
    close(xsum, t["x"].double() + t["add"].double() * sc, tol, "xsum")
    close(v["y"][0, 0], tr.layernorm_fwd(xsum.double(), gm, bt, EPS)[0], tol, "y of the sum")
    _mr_close(v["mr"][0, 0], xsum, "mr of the sum")
    mrs = v["mr"][0, 0].cpu()
    xs = Operand(mat(R, C), dtype, "in", values=xsum)
    dxr, dgr, dbr = tr.layernorm_bwd(xsum.double(), t["dy"].double(), gm, EPS, t["res"].double())
    dxn = tr.layernorm_bwd(xsum.double(), t["dy"].double(), gm, EPS)[0]

    # jg_layernorm_bwd_add (res), accumulating
    o = Once({"x": xs, "dy": rows("dy"), "gamma": vec("gamma"), "mr": mr_in(mrs), "res": rows("res"), "dx": out(), "dgamma": acc("g0"), "dbeta": acc("b0")})
    v = o.v
    _lib.check(_L().jg_layernorm_bwd_add(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), p(v["res"]), p(v["dx"]), p(v["dgamma"]), p(v["dbeta"]),
                                         R, C, _st()), "jg_layernorm_bwd_add")
    o.check()
    close(v["dx"][0, 0], dxr, tol, "dx + res")
    acc_close(v["dgamma"][0, 0, 0], t["g0"], dgr, 2 * tol, "dgamma (bwd_add)")
    acc_close(v["dbeta"][0, 0, 0], t["b0"], dbr, 2 * tol, "dbeta (bwd_add)")

    # jg_layernorm_bwd_add2: dx2 = the ROUNDED dx * scale[image] (scale NULL: a copy)
    ops = {"x": xs, "dy": rows("dy"), "gamma": vec("gamma"), "mr": mr_in(mrs), "dx": out(), "dx2": out(), "dgamma": acc("g0"), "dbeta": acc("b0")}
    if full:
        ops.update(res=rows("res"), scale=Operand(mat(1, nimg), torch.float32, "in", values=scale))
    o = Once(ops)
    v = o.v
    _lib.check(_L().jg_layernorm_bwd_add2(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), p(v.get("res")), p(v["dx"]), p(v.get("scale")), rpi,
                                          p(v["dx2"]), p(v["dgamma"]), p(v["dbeta"]), R, C, _st()), "jg_layernorm_bwd_add2")
    o.check()
    close(v["dx"][0, 0], dxr if full else dxn, tol, "dx (bwd_add2)")
    if full:
        close(v["dx2"][0, 0], d64(v["dx"][0, 0]) * sc, tol, "dx2")
        assert float(d64(v["dx2"][0, 0])[:rpi].abs().max()) == 0.0          # scale[0] = 0: a dropped path
    else:
        assert torch.equal(v["dx2"], v["dx"])
    acc_close(v["dgamma"][0, 0, 0], t["g0"], dgr, 2 * tol, "dgamma (bwd_add2)")
    acc_close(v["dbeta"][0, 0, 0], t["b0"], dbr, 2 * tol, "dbeta (bwd_add2)")

    # jg_layernorm_bwd_res: frozen LayerNorm, no parameter gradients
    ops = {"x": xs, "dy": rows("dy"), "gamma": vec("gamma"), "mr": mr_in(mrs), "dx": out()}
    if full:
        ops["res"] = rows("res")
    o = Once(ops)
    v = o.v
    _lib.check(_L().jg_layernorm_bwd_res(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), p(v.get("res")), p(v["dx"]), R, C, _st()),
               "jg_layernorm_bwd_res")
    o.check()
    close(v["dx"][0, 0], dxr if full else dxn, tol, "dx (bwd_res)")


@pytest.mark.parametrize("C", [520, 12])
def test_layernorm_refuses(C):
    from joligen_amd import _lib

    R, dtype = 5, torch.float16
    o = Once({"x": Operand(mat(R, C), dtype, "in", 1), "dy": Operand(mat(R, C), dtype, "in", 2), "gamma": Operand(mat(1, C), torch.float32, "in", 3),
              "beta": Operand(mat(1, C), torch.float32, "in", 4), "y": Operand(mat(R, C), dtype, "out"), "mr": Operand(mat(R, 2), torch.float32, "out"),
              "dgamma": Operand(mat(1, C), torch.float32, "out"), "dbeta": Operand(mat(1, C), torch.float32, "out")})
    v = o.v
    code, L = _code(dtype), _L()
    bad = _lib.JG_ERR_BAD_ARG
    assert L.jg_layernorm_fwd(code, p(v["x"]), p(v["gamma"]), p(v["beta"]), p(v["y"]), p(v["mr"]), R, C, EPS, _st()) == bad
    assert L.jg_layernorm_fwd_add(code, p(v["x"]), p(v["dy"]), None, 1, p(v["y"]), p(v["gamma"]), p(v["beta"]), p(v["y"]), p(v["mr"]), R, C, EPS, _st()) == bad
    assert L.jg_layernorm_bwd(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), p(v["y"]), p(v["dgamma"]), p(v["dbeta"]), R, C, _st()) == bad
    assert L.jg_layernorm_bwd_add(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), None, p(v["y"]), p(v["dgamma"]), p(v["dbeta"]), R, C, _st()) == bad
    assert L.jg_layernorm_bwd_add2(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), None, p(v["y"]), None, 1, p(v["y"]), p(v["dgamma"]),
                                   p(v["dbeta"]), R, C, _st()) == bad
    assert L.jg_layernorm_bwd_res(code, p(v["x"]), p(v["dy"]), p(v["gamma"]), p(v["mr"]), None, p(v["y"]), R, C, _st()) == bad
    o.check(unwritten=("y", "mr", "dgamma", "dbeta"))


# ======================================================================================================================================
# jg_dwconv3x3_fwd_pad / _bwd_ws_pad; no stride arguments
# ======================================================================================================================================
DW_CASES = [(1, 1, 1, 8, 0), (2, 1, 5, 64, 0), (1, 9, 7, 2048, 0),          # (B, H, W, C, pad_mode): zero padding
            (1, 4, 4, 64, 1), (2, 4, 5, 2048, 1)]                            # reflect


def dw_inputs(case, dtype):
    B, H, W, C, _ = case
    return dict(x=rnd((B, H, W, C), dtype, 5), dy=rnd((B, H, W, C), dtype, 6), w=rnd((C, 3, 3), torch.float32, 7, 0.4),
                bias=rnd((C,), torch.float32, 8, 0.1), dw0=rnd((C, 3, 3), torch.float32, 9, math.sqrt(B * H * W)),
                db0=rnd((C,), torch.float32, 10, math.sqrt(B * H * W)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("use_ws", [False, True], ids=["atomics", "workspace"])
@pytest.mark.parametrize("gelu", [0, 1], ids=["linear", "gelu"])
@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv3x3(case, gelu, use_ws, dtype):
    """dw / dbias accumulate from N(0, B H W) start values; the workspace is exactly jg_dwconv3x3_bwd_ws_floats floats between canaries and is
    NOT zeroed (it holds the pre-fill pattern, about 1e27 as a float); one float less is refused."""
    from joligen_amd import _lib

    B, H, W, C, pad = case
    t = dw_inputs(case, dtype)
    code, tol, shape = _code(dtype), SEG_TOL[dtype], (B, H, W, C)
    img = lambda n: Operand(shape, dtype, "in", values=t[n])
    wop = lambda: Operand(mat(1, 9 * C), torch.float32, "in", values=t["w"])
    ops = {"x": img("x"), "w": wop(), "bias": Operand(mat(1, C), torch.float32, "in", values=t["bias"]), "y": Operand(shape, dtype, "out")}
    if gelu:
        ops["pre"] = Operand(shape, dtype, "out")
    o = Once(ops)
    v = o.v
    _lib.check(_L().jg_dwconv3x3_fwd_pad(code, p(v["x"]), p(v["w"]), p(v["bias"]), p(v.get("pre")), p(v["y"]), B, H, W, C, gelu, pad, _st()),
               "jg_dwconv3x3_fwd_pad")
    o.check()
    pre_ref, y_ref = tr.dwconv3x3_fwd(t["x"].double(), t["w"].double(), t["bias"].double(), bool(gelu), bool(pad))
    close(v["y"], y_ref, tol, "y")
    pre16 = None
    if gelu:
        close(v["pre"], pre_ref, tol, "pre")
        pre16 = v["pre"].cpu()

    nws = int(_L().jg_dwconv3x3_bwd_ws_floats(B, H, W, C)) if use_ws else 0
    ops = {"x": img("x"), "dy": img("dy"), "w": wop(), "du": Operand(shape, dtype, "out"), "dx": Operand(shape, dtype, "out"),
           "dw": Operand(mat(1, 9 * C), torch.float32, "acc", values=t["dw0"]), "dbias": Operand(mat(1, C), torch.float32, "acc", values=t["db0"])}
    if gelu:
        ops["pre"] = Operand(shape, dtype, "in", values=pre16)
    if use_ws:
        assert nws > 0
        ops["ws"] = Operand(mat(1, nws), torch.float32, "out")
    o = Once(ops)
    v = o.v
    args = lambda n: (code, p(v["x"]), p(v.get("pre")), p(v["dy"]), p(v["w"]), p(v["du"]), p(v["dx"]), p(v["dw"]), p(v["dbias"]), p(v.get("ws")), n,
                      B, H, W, C, gelu, pad, _st())
    if use_ws:
        assert _L().jg_dwconv3x3_bwd_ws_pad(*args(nws - 1)) == _lib.JG_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert torch.equal(v["dw"][0, 0, 0].cpu(), t["dw0"].reshape(-1)) and torch.equal(v["dbias"][0, 0, 0].cpu(), t["db0"])
    _lib.check(_L().jg_dwconv3x3_bwd_ws_pad(*args(nws)), "jg_dwconv3x3_bwd_ws_pad")
    o.check()                                           # (the workspace too: every float of it is a partial the summing launch reads)
    du, dx, dw, db = tr.dwconv3x3_bwd(t["x"].double(), None if pre16 is None else pre16.double(), t["dy"].double(), t["w"].double(), bool(gelu), bool(pad))
    close(v["du"], du, 2 * tol, "du")
    close(v["dx"], dx, 2 * tol, "dx")
    acc_close(v["dw"][0, 0, 0], t["dw0"].reshape(-1), dw.reshape(-1), 2 * tol, "dw")
    acc_close(v["dbias"][0, 0, 0], t["db0"], db, 2 * tol, "dbias")
    if not gelu:
        assert torch.equal(v["du"].cpu(), t["dy"])          # du = dy: a bit-exact copy


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dwconv3x3_refuses_2056_channels(dtype):
    from joligen_amd import _lib

    B, H, W, C = 1, 2, 4, 2056
    shape = (B, H, W, C)
    o = Once({"x": Operand(shape, dtype, "in", 1), "dy": Operand(shape, dtype, "in", 2), "w": Operand(mat(1, 9 * C), torch.float32, "in", 3),
              "y": Operand(shape, dtype, "out"), "du": Operand(shape, dtype, "out"), "dx": Operand(shape, dtype, "out"),
              "dw": Operand(mat(1, 9 * C), torch.float32, "out"), "dbias": Operand(mat(1, C), torch.float32, "out")})
    v = o.v
    assert _L().jg_dwconv3x3_fwd_pad(_code(dtype), p(v["x"]), p(v["w"]), None, None, p(v["y"]), B, H, W, C, 0, 0, _st()) == _lib.JG_ERR_UNSUPPORTED
    assert _L().jg_dwconv3x3_bwd_ws_pad(_code(dtype), p(v["x"]), None, p(v["dy"]), p(v["w"]), p(v["du"]), p(v["dx"]), p(v["dw"]), p(v["dbias"]), None, 0,
                                        B, H, W, C, 0, 0, _st()) == _lib.JG_ERR_UNSUPPORTED
    o.check(unwritten=("y", "du", "dx", "dw", "dbias"))
