"""The launch layer: one function per kernel launch (or fixed launch sequence) that BOTH Python surfaces use -- the module graph's JGFunction
nodes (ops.py, ops_segformer.py, modules/) and the functional `torch.ops.jg355.*` ops (ops.py, ops_library_cut.py).

A helper derives the sizes from its tensors, allocates the outputs its caller asked for, marshals the pointers, calls the C entry point of
include/jg355.h on torch's current stream and returns the tensors.  It knows nothing of autograd contexts, `needs_input_grad`, arenas or
torch.library; what differs between the surfaces comes in as arguments:
  * gradient destinations the kernels ACCUMULATE into (`dg`, `db`, `dw`, `dW`, `g`): arena `.grad` views, fresh torch.zeros, or None = not wanted;
  * optional outputs by a flag (`want_dx`, `want_dpred`, `want_mr`, `want_dk`); an output that is not produced is None.
Inputs are taken as they are: `.contiguous()` and dtype conversions stay with the callers, a helper never adds a copy.  This module imports
nothing of the package but _lib (the raw plumbing below lives here for that reason; ops.py re-exports it under the same names).
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import JG_ACT_NONE, check

_DT = {torch.float16: _lib.JG_F16, torch.bfloat16: _lib.JG_BF16}


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"joligen_amd activations must be float16/bfloat16, got {t.dtype}") from None


# torch.cuda.current_stream() builds a Stream object per call (~8 us): too slow for a per-launch lookup.  The raw accessor is a private
# symbol: a torch build without it (or without CUDA / HIP at all) falls back to the public API instead of failing at import time
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda dev: torch.cuda.current_stream(dev).cuda_stream)
_cur_device = torch.cuda.current_device


def _st() -> int:
    """raw hipStream_t of torch's current stream on the current device"""
    return _raw_stream(_cur_device())


def _p(t):
    return None if t is None else t.data_ptr()


def sgemm(A, B, C, M, N, K, sa, sb, sc, nbatch=1, bstr=(0, 0, 0), bias=None, E=None, alpha=1.0, beta=0.0,
          act_a=JG_ACT_NONE, act_b=JG_ACT_NONE, act_e=JG_ACT_NONE):
    """C[z][m][n] = alpha sum_k actA(A[z][m][k]) actB(B[z][n][k]) (+bias, *act'(E), +beta C); sa=(sam,sak), sb=(sbn,sbk), sc=(scm,scn)."""
    check(_lib.lib().jg_sgemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(bias), _p(E), M, N, K, sa[0], sa[1], sb[0], sb[1],
                              sc[0], sc[1], nbatch, bstr[0], bstr[1], bstr[2], alpha, beta, act_a, act_b, act_e, _st()), "jg_sgemm")
    return C


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, weight, bias, eps, want_mr=True):
    """-> (y, mr [rows, 2] = mean | rstd for the backward, None unless wanted)"""
    C = x.shape[-1]
    R = x.numel() // C
    y = torch.empty_like(x)
    mr = torch.empty((R, 2), device=x.device, dtype=torch.float32) if want_mr else None
    check(_lib.lib().jg_layernorm_fwd(_dt(x), x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), mr.data_ptr() if want_mr else None,
                                      R, C, eps, _st()), "jg_layernorm_fwd")
    return y, mr


def layernorm_bwd(x, dy, weight, mr, dg, db, want_dx=True):
    """dg / db [C] fp32 are accumulated into (None: not wanted) -> dx"""
    C = x.shape[-1]
    dx = torch.empty_like(x) if want_dx else None
    check(_lib.lib().jg_layernorm_bwd(_dt(x), x.data_ptr(), dy.data_ptr(), weight.data_ptr(), mr.data_ptr(), _p(dx), _p(dg), _p(db),
                                      x.numel() // C, C, _st()), "jg_layernorm_bwd")
    return dx


# ---- depth-wise 3x3 (+ GELU) -----------------------------------------------------------------------------------------------------------
def dwconv3x3_fwd(x, weight, bias, gelu, reflect=False):
    """-> (y, pre-activation; None without gelu)"""
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    pre = torch.empty_like(x) if gelu else None
    check(_lib.lib().jg_dwconv3x3_fwd_pad(_dt(x), x.data_ptr(), weight.data_ptr(), _p(bias), pre.data_ptr() if gelu else None, y.data_ptr(),
                                          B, H, W, C, int(gelu), int(reflect), _st()), "jg_dwconv3x3_fwd_pad")
    return y, pre


def dwconv3x3_bwd(x, pre, dy, weight, dw, db, gelu, reflect=False, want_dx=True, two_phase=False):
    """dw [C, 1, 3, 3] / db [C] fp32 are accumulated into (None: not wanted).  two_phase: the blocks' weight / bias partials go through a
    workspace and a summing launch; else atomics from every block -> dx"""
    B, H, W, C = x.shape
    du = torch.empty_like(x)
    dx = torch.empty_like(x) if want_dx else None
    ws, nws = None, 0
    if two_phase:
        nws = int(_lib.lib().jg_dwconv3x3_bwd_ws_floats(B, H, W, C))
        ws = torch.empty((nws,), device=x.device, dtype=torch.float32)
    check(_lib.lib().jg_dwconv3x3_bwd_ws_pad(_dt(x), x.data_ptr(), _p(pre), dy.data_ptr(), weight.data_ptr(), du.data_ptr(), _p(dx), _p(dw), _p(db),
                                             _p(ws), nws, B, H, W, C, int(gelu), int(reflect), _st()), "jg_dwconv3x3_bwd_ws_pad")
    return dx


# ---- attention cores -------------------------------------------------------------------------------------------------------------------
def attn_smallkv_fwd(q, kv, heads):
    """q [B, Tq, C], kv [B, Tkv, 2C] packed (k | v), head dim 32 -> (o [B, Tq, C], logsumexp [B, heads, Tq])"""
    B, Tq, C = q.shape
    Tkv = kv.shape[1]
    o = torch.empty_like(q)
    lse = torch.empty((B, heads, Tq), device=q.device, dtype=torch.float32)
    es = q.element_size()
    check(_lib.lib().jg_attn_smallkv_fwd(_dt(q), q.data_ptr(), kv.data_ptr(), kv.data_ptr() + C * es, o.data_ptr(), lse.data_ptr(), B, Tq, Tkv,
                                         heads, C, 2 * C, C, 1.0 / math.sqrt(32.0), _st()), "jg_attn_smallkv_fwd")
    return o, lse


def attn_smallkv_bwd(q, kv, o, lse, do, heads):
    """-> (dq, dkv: the gradient of the packed kv projection, written in place)"""
    B, Tq, C = q.shape
    Tkv = kv.shape[1]
    dq = torch.empty_like(q)
    acc = torch.empty((2, B, Tkv, C), device=q.device, dtype=torch.float32)       # dk | dv fp32 accumulators: one buffer, one fill
    dkv = torch.empty_like(kv)
    es = q.element_size()
    check(_lib.lib().jg_attn_smallkv_bwd2(_dt(q), q.data_ptr(), kv.data_ptr(), kv.data_ptr() + C * es, o.data_ptr(), do.data_ptr(), lse.data_ptr(),
                                          dq.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), dkv.data_ptr(), dkv.data_ptr() + C * es, 2 * C, B, Tq,
                                          Tkv, heads, C, 2 * C, C, 1.0 / math.sqrt(32.0), _st()), "jg_attn_smallkv_bwd2")
    return dq, dkv


def vit_attention_fwd(qkv, heads):
    """timm Attention core on the packed projection qkv [B, T, 3C] (channel order [3][heads][head_dim]) -> (a [B, T, C], logsumexp)"""
    B, T, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    a = torch.empty((B, T, C), device=qkv.device, dtype=qkv.dtype)
    L = torch.empty((B * heads, T), device=qkv.device, dtype=torch.float32)
    es = qkv.element_size()
    check(_lib.lib().jg_vit_attention_fwd(_dt(qkv), qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es, C3, hd, a.data_ptr(),
                                          L.data_ptr(), B, T, heads, hd, hd ** -0.5, _st()), "jg_vit_attention_fwd")
    return a, L


def vit_attention_bwd(qkv, a, L, da, heads):
    B, T, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    dqkv = torch.empty_like(qkv)
    Dq = torch.empty((B * heads, T), device=qkv.device, dtype=torch.float32)
    es = qkv.element_size()
    check(_lib.lib().jg_vit_attention_bwd(_dt(qkv), qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es, C3, hd, a.data_ptr(),
                                          L.data_ptr(), da.data_ptr(), dqkv.data_ptr(), dqkv.data_ptr() + C * es, dqkv.data_ptr() + 2 * C * es, C3,
                                          Dq.data_ptr(), B, T, heads, hd, hd ** -0.5, _st()), "jg_vit_attention_bwd")
    return dqkv


# ---- element-wise: GELU, ReLU / LeakyReLU / Tanh ---------------------------------------------------------------------------------------
def gelu_fwd(x):
    y = torch.empty_like(x)
    check(_lib.lib().jg_gelu_fwd(_dt(x), x.data_ptr(), y.data_ptr(), x.numel(), _st()), "jg_gelu_fwd")
    return y


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    check(_lib.lib().jg_gelu_bwd(_dt(x), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), _st()), "jg_gelu_bwd")
    return dx


def act_fwd(x, kind):
    y = torch.empty_like(x)
    check(_lib.lib().jg_act_fwd(_dt(x), x.data_ptr(), y.data_ptr(), x.numel(), kind, _st()), "jg_act_fwd")
    return y


def act_bwd(y, dy, kind):
    """the derivative is taken from the OUTPUT y of the activation"""
    dx = torch.empty_like(y)
    check(_lib.lib().jg_act_bwd(_dt(y), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.numel(), kind, _st()), "jg_act_bwd")
    return dx


# ---- nn.Dropout inside the normalise + activate passes (csrc/dropout.hip) ----------------------------------------------------------------
def gn_apply_drop(x, ab, act, keep, u, key, stream, call):
    """y = m * act(a x + b) / keep on x [B, H, W, C] with m = (u < keep); ab [B, C, 2] or None (no normalisation); u fp32 [B, C, H, W] or None:
    drawn in the kernel from the two words of `key` on the counter (pixel, b, stream | (c / 4) << 16, call)"""
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    check(_lib.lib().jg_gn_apply_drop(_dt(x), x.data_ptr(), C, _p(ab), y.data_ptr(), C, B, H, W, C, act, keep, _p(u), _p(key), stream, call, _st()),
          "jg_gn_apply_drop")
    return y


def gn_bwd_reduce_drop(x, dy, ab, red, act, keep, u, key, stream, call):
    """red [B, C, 2] += (sum du, sum du x) with du = (dy m / keep) act'(a x + b): the mask of gn_apply_drop, regenerated"""
    B, H, W, C = x.shape
    check(_lib.lib().jg_gn_bwd_reduce_drop(_dt(x), x.data_ptr(), C, dy.data_ptr(), C, ab.data_ptr(), red.data_ptr(), B, H, W, C, act, keep, _p(u),
                                           _p(key), stream, call, _st()), "jg_gn_bwd_reduce_drop")


def gn_bwd_apply_drop(x, dy, ab, pqr, act, keep, u, key, stream, call):
    """-> dx = du P + x Q + R (ab, pqr None: dx = du = (dy m / keep) act'(x))"""
    B, H, W, C = x.shape
    dx = torch.empty_like(x)
    check(_lib.lib().jg_gn_bwd_apply_drop(_dt(x), x.data_ptr(), C, dy.data_ptr(), C, _p(ab), _p(pqr), dx.data_ptr(), C, B, H, W, C, act, keep, _p(u),
                                          _p(key), stream, call, _st()), "jg_gn_bwd_apply_drop")
    return dx


def gn_apply_drop_up2(x, ab, act, keep, u, key, stream, call):
    """y [B, 2H, 2W, C] = m * act(a up2(x) + b) / keep from x [B, H, W, C] (rows may be a channel slice): the mask of gn_apply_drop on the
    materialised upsample; u fp32 [B, C, 2H, 2W] or None = drawn"""
    B, H, W, C = x.shape
    y = torch.empty((B, 2 * H, 2 * W, C), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_gn_apply_drop_up2(_dt(x), x.data_ptr(), x.stride(2), _p(ab), y.data_ptr(), C, B, H, W, C, act, keep, _p(u), _p(key), stream,
                                          call, _st()), "jg_gn_apply_drop_up2")
    return y


def drop_pool2_bwd(dy, keep, u, key, stream, call):
    """g [B, H, W, C] = 2 x 2 sums of dy * m / keep from dy [B, 2H, 2W, C]: the adjoint of gn_apply_drop_up2's mask and upsample"""
    B, H2, W2, C = dy.shape
    g = torch.empty((B, H2 // 2, W2 // 2, C), device=dy.device, dtype=dy.dtype)
    check(_lib.lib().jg_drop_pool2_bwd(_dt(dy), dy.data_ptr(), dy.stride(2), g.data_ptr(), C, B, H2 // 2, W2 // 2, C, keep, _p(u), _p(key), stream,
                                       call, _st()), "jg_drop_pool2_bwd")
    return g


# ---- reflection padding, bilinear resize -----------------------------------------------------------------------------------------------
def reflect_pad2d(x, pad):
    B, H, W, C = x.shape
    y = torch.empty((B, H + 2 * pad, W + 2 * pad, C), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_reflect_pad2d(_dt(x), x.data_ptr(), y.data_ptr(), B, H, W, C, pad, _st()), "jg_reflect_pad2d")
    return y


def reflect_pad2d_bwd(dy, pad):
    """adjoint of ReflectionPad2d(pad): dy [B, H + 2 pad, W + 2 pad, C] folded back onto [B, H, W, C]"""
    B, Hp, Wp, C = dy.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    dx = torch.empty((B, H, W, C), device=dy.device, dtype=dy.dtype)
    check(_lib.lib().jg_reflect_pad2d_bwd(_dt(dy), dy.data_ptr(), dx.data_ptr(), B, H, W, C, pad, _st()), "jg_reflect_pad2d_bwd")
    return dx


def bilinear2_fwd(x, Ho, Wo, align_corners):
    B, H, W, C = x.shape
    y = torch.empty((B, Ho, Wo, C), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_bilinear2_fwd(_dt(x), x.data_ptr(), y.data_ptr(), B, H, W, C, Ho, Wo, C, int(align_corners), _st()), "jg_bilinear2_fwd")
    return y


def bilinear2_bwd(dy, H, W, align_corners):
    B, Ho, Wo, C = dy.shape
    dx = torch.empty((B, H, W, C), device=dy.device, dtype=dy.dtype)
    check(_lib.lib().jg_bilinear2_bwd(_dt(dy), dy.data_ptr(), dx.data_ptr(), B, H, W, C, Ho, Wo, C, int(align_corners), _st()), "jg_bilinear2_bwd")
    return dx


# ---- data_online_context_pixels: the crop and its framed image (csrc/context.hip) ------------------------------------------------------------
def context_split(x, c, act_dtype, cpad=None):
    """x fp32 NCHW [B, C, H, W] (contiguous), read once -> (ctx [B, H, W, cpad], crop [B, H - 2c, W - 2c, cpad] = ctx[:, c:-c, c:-c]), 16-bit NHWC"""
    B, C, H, W = x.shape
    cpad = cpad or (C + 7) // 8 * 8
    ctx = torch.empty((B, H, W, cpad), device=x.device, dtype=act_dtype)
    crop = torch.empty((B, max(H - 2 * c, 0), max(W - 2 * c, 0), cpad), device=x.device, dtype=act_dtype)
    check(_lib.lib().jg_context_split(_DT[act_dtype], x.data_ptr(), ctx.data_ptr(), crop.data_ptr(), B, C, H, W, c, cpad, _st()), "jg_context_split")
    return ctx, crop


def context_frame(inner, ctx, c, C, sigma, z, key, noise_stream, call, out=None, out_noisy=None, want_noisy=False):
    """out = inner inside the window of ctx, ctx on the frame; out_noisy = out + sigma z (written when `out_noisy` is given or `want_noisy`); z fp32
    [B, C, H, W] of the framed size or None: drawn in the kernel from the two words of `key` -> (out, out_noisy or None)"""
    B, H, W, cpad = ctx.shape
    out = torch.empty_like(ctx) if out is None else out
    if out_noisy is None and want_noisy:
        out_noisy = torch.empty_like(ctx)
    check(_lib.lib().jg_context_frame(_dt(ctx), inner.data_ptr(), ctx.data_ptr(), out.data_ptr(), _p(out_noisy), sigma, _p(z), _p(key), noise_stream,
                                      call, B, H, W, c, C, cpad, _st()), "jg_context_frame")
    return out, out_noisy


# ---- fp32 linear -----------------------------------------------------------------------------------------------------------------------
def linear_fwd(x, W, b, act):
    """y = act(x) @ W.T + b, fp32"""
    Bn, K = x.shape
    N = W.shape[0]
    y = torch.empty((Bn, N), device=x.device, dtype=torch.float32)
    check(_lib.lib().jg_linear_fwd(x.data_ptr(), W.data_ptr(), _p(b), y.data_ptr(), Bn, K, N, act, _st()), "jg_linear_fwd")
    return y


def linear_bwd(x, W, dy, act, dW, db, want_dx=True):
    """dW / db are accumulated into (None: not wanted) -> dx"""
    Bn, K = x.shape
    dx = torch.empty_like(x) if want_dx else None
    check(_lib.lib().jg_linear_bwd(x.data_ptr(), W.data_ptr(), dy.data_ptr(), _p(dx), _p(dW), _p(db), Bn, K, W.shape[0], act, _st()), "jg_linear_bwd")
    return dx


# ---- L2 normalisation, PatchNCE / MoNCE, SRC_hDCE (fp32) -------------------------------------------------------------------------------
def l2norm_fwd(x, eps):
    R, D = x.shape
    y = torch.empty_like(x)
    nrm = torch.empty((R,), device=x.device, dtype=torch.float32)
    check(_lib.lib().jg_l2norm_fwd(x.data_ptr(), y.data_ptr(), nrm.data_ptr(), R, D, eps, _st()), "jg_l2norm_fwd")
    return y, nrm


def l2norm_bwd(y, nrm, dy, eps):
    dx = torch.empty_like(y)
    check(_lib.lib().jg_l2norm_bwd(y.data_ptr(), nrm.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.shape[0], y.shape[1], eps, _st()), "jg_l2norm_bwd")
    return dx


SINKHORN_ITERS = 50  # monce.py:24


def _logits(q, k, nimg, P, D):
    """S[b] = q[b] k[b]^T of the nimg problems"""
    return sgemm(q, k, torch.empty((nimg, P, P), device=q.device, dtype=torch.float32), P, P, D, (D, 1), (D, 1), (P, 1), nimg, (P * D, P * D, P * P))


def _contrastive_grads(q, k, dS, gpos, nimg, P, D, want_dk, ot=None):
    """the tail of the PatchNCE and hDCE backward: dk_j = sum_i dS_ij q_i over the negatives only (the diagonal of dS is zero, the positive pair is
    detached); then -- MoNCE, ot = (K, uh, vh, gW) -- the gradient through the optimal-transport weights is added to dS (k is detached
    there, hence AFTER dk); dq = dS k + gpos * k -> (dq, dk)"""
    dk = None
    if want_dk:
        dk = sgemm(dS, q, torch.empty_like(k), P, D, P, (1, P), (1, D), (D, 1), nimg, (P * P, P * D, P * D))
    if ot is not None:
        K, uh, vh, gW = ot
        dsh, drh = torch.empty_like(uh), torch.empty_like(uh)
        check(_lib.lib().jg_nce_sinkhorn_bwd(K.data_ptr(), uh.data_ptr(), vh.data_ptr(), gW.data_ptr(), dsh.data_ptr(), drh.data_ptr(), dS.data_ptr(),
                                             nimg, P, SINKHORN_ITERS, _st()), "jg_nce_sinkhorn_bwd")
    dq = sgemm(dS, k, torch.empty_like(q), P, D, P, (P, 1), (1, D), (D, 1), nimg, (P * P, P * D, P * D))
    check(_lib.lib().jg_row_axpy(dq.data_ptr(), gpos.data_ptr(), k.data_ptr(), nimg * P, D, _st()), "jg_row_axpy")
    return dq, dk


def _nce_ce(S, uh, vh, out, dS, gW, dloss, gpos, nimg, P, temp, pm1):
    """forward (out = the loss, the gradient arguments None) and backward mode of jg_nce_ce; uh / vh: the Sinkhorn histories, whose last rows
    are the transport scalings (None: plain PatchNCE)"""
    u = v = None
    if uh is not None:
        u, v = uh[:, -1], vh[:, -1]
    check(_lib.lib().jg_nce_ce(S.data_ptr(), _p(u), SINKHORN_ITERS * P, _p(v), (SINKHORN_ITERS + 1) * P, out.data_ptr(), _p(dS), _p(gW), nimg, P, temp,
                               pm1, _p(dloss), _p(gpos), 1.0, _st()), "jg_nce_ce")


def nce_fwd(q, k, nimg, temp, pm1, monce):
    """per-patch PatchNCE / MoNCE loss of q, k [nimg * P, D] -> (loss [nimg * P], logits S, and the optimal-transport state K, u-history,
    v-history: None without monce)"""
    R, D = q.shape
    P = R // nimg
    S = _logits(q, k, nimg, P, D)
    loss = torch.empty((R,), device=q.device, dtype=torch.float32)
    K = uh = vh = None
    if monce:
        K = torch.empty_like(S)
        uh = torch.empty((nimg, SINKHORN_ITERS, P), device=q.device, dtype=torch.float32)
        vh = torch.empty((nimg, SINKHORN_ITERS + 1, P), device=q.device, dtype=torch.float32)
        check(_lib.lib().jg_nce_sinkhorn_fwd(S.data_ptr(), K.data_ptr(), uh.data_ptr(), vh.data_ptr(), nimg, P, SINKHORN_ITERS, 1.0, _st()),
              "jg_nce_sinkhorn_fwd")
    _nce_ce(S, uh, vh, loss, None, None, None, None, nimg, P, temp, pm1)
    return loss, S, K, uh, vh


def nce_bwd(q, k, S, K, uh, vh, dloss, nimg, temp, pm1, monce, want_dk=True):
    """dloss: fp32 [nimg * P] -> (dq, dk; None unless wanted)"""
    R, D = q.shape
    P = R // nimg
    dS = torch.empty_like(S)
    gW = torch.empty_like(S) if monce else None
    gpos = torch.empty((R,), device=q.device, dtype=torch.float32)
    scratch = torch.empty_like(q)
    _nce_ce(S, uh if monce else None, vh, scratch, dS, gW, dloss, gpos, nimg, P, temp, pm1)
    return _contrastive_grads(q, k, dS, gpos, nimg, P, D, want_dk, (K, uh, vh, gW) if monce else None)


def _hdce(S, G, stats, loss, dS, gpos, dloss, W, nimg, P, temp, gamma, wperiod, wcount):
    check(_lib.lib().jg_nce_hdce(S.data_ptr(), _p(G), stats.data_ptr(), _p(loss), _p(dS), _p(gpos), _p(dloss), _p(W), nimg, P, temp, gamma, wperiod,
                                 wcount, _st()), "jg_nce_hdce")


def _hdce_gram(k, nimg, P, D, wperiod, wcount):
    """k k^T of the problems whose weights are needed: the leading `wcount` problems when there is a single weighted run, else every problem in
    ONE launch (the weighted runs are not a strided batch; the kernel never reads the Gram matrix of an unweighted problem)"""
    if wcount < 1:
        return None
    return _logits(k, k, min(wcount, nimg) if wperiod >= nimg else nimg, P, D)


def _hdce_check(nimg, R, gamma, wperiod, wcount):
    if nimg < 1 or R % nimg or not gamma > 0 or wperiod < 1 or not 0 <= wcount <= wperiod:
        raise ValueError(f"patch_hdce: nimg={nimg} rows={R} gamma={gamma} wperiod={wperiod} wcount={wcount}")


def hdce_fwd(q, k, nimg, temp, gamma, wperiod, wcount):
    """per-patch SRC_hDCE loss of q, k [nimg * P, D]; problem b is weighted iff (b % wperiod) < wcount -> (loss [nimg * P], logits S, key Gram
    matrix G (None with wcount == 0), stats [3, nimg * P] = m | A | rinv for the backward)"""
    R, D = q.shape
    _hdce_check(nimg, R, gamma, wperiod, wcount)
    P = R // nimg
    S = _logits(q, k, nimg, P, D)
    G = _hdce_gram(k, nimg, P, D, wperiod, wcount)
    loss = torch.empty((R,), device=q.device, dtype=torch.float32)
    stats = torch.empty((3, R), device=q.device, dtype=torch.float32)
    _hdce(S, G, stats, loss, None, None, None, None, nimg, P, temp, gamma, wperiod, wcount)
    return loss, S, G, stats


def hdce_bwd(q, k, S, G, stats, dloss, nimg, temp, gamma, wperiod, wcount, want_dk=True):
    """dloss: fp32 [nimg * P] -> (dq, dk; None unless wanted)"""
    R, D = q.shape
    P = R // nimg
    dS = torch.empty_like(S)
    gpos = torch.empty((R,), device=q.device, dtype=torch.float32)
    _hdce(S, G, stats, None, dS, gpos, dloss, None, nimg, P, temp, gamma, wperiod, wcount)
    return _contrastive_grads(q, k, dS, gpos, nimg, P, D, want_dk)


def hdce_weights(k, nimg, gamma):
    """the hDCE weights [nimg, P, P] of SRC_Loss(only_weight=True) with a zero diagonal"""
    R, D = k.shape
    _hdce_check(nimg, R, gamma, 1, 1)
    P = R // nimg
    G = _hdce_gram(k, nimg, P, D, 1, 1)
    W = torch.empty_like(G)
    scratch = torch.empty((4, R), device=k.device, dtype=torch.float32)
    _hdce(G, G, scratch, scratch[3], None, None, None, W, nimg, P, 1.0, float(gamma), 1, 1)
    return W


# ---- GAN objectives, DDPM loss: (loss, d loss / d prediction) in one pass -----------------------------------------------------------------
def gan_loss(pred, mode, target, scale, want_dpred=True):
    """GANLoss: mode 0 lsgan, 1 vanilla (BCE with logits), 2 wgangp, on an NHWC logit map whose channel 0 is valid"""
    cpad = pred.shape[-1]
    loss = torch.zeros((), device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_dpred else None
    check(_lib.lib().jg_gan_loss(_dt(pred), mode, pred.data_ptr(), target, loss.data_ptr(), _p(dpred), pred.numel() // cpad, cpad, scale, 1.0, _st()),
          "jg_gan_loss")
    return loss, dpred


def hinge_loss(pred, mode, scale, want_dpred=True):
    """GANLoss("projected"): mode 0 mean relu(1 - p), 1 mean relu(1 + p), 2 mean(-p) over every element"""
    loss = torch.zeros((), device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_dpred else None
    check(_lib.lib().jg_hinge_loss(_dt(pred), pred.data_ptr(), loss.data_ptr(), _p(dpred), pred.numel(), 1, 1, mode, scale, 1.0, _st()), "jg_hinge_loss")
    return loss, dpred


def ddpm_mse_loss(nh, noise, mask, w, lam, grad_scale, channels):
    """(lambda MSE(w m noise, w m noise_hat), its gradient w.r.t. noise_hat [B, H, W, cpad] times grad_scale)"""
    B, H, W, cpad = nh.shape
    loss = torch.zeros((), device=nh.device, dtype=torch.float32)
    dnh = torch.empty_like(nh)
    check(_lib.lib().jg_ddpm_mse_loss(_dt(nh), noise.data_ptr(), nh.data_ptr(), _p(mask), _p(w), loss.data_ptr(), dnh.data_ptr(), B, channels, H, W,
                                      cpad, lam, grad_scale, _st()), "jg_ddpm_mse_loss")
    return loss, dnh


# ---- spectral normalisation of a weight W: physical [Cout][RS][Cin] fp32 -------------------------------------------------------------------
def spectral_power_iter(W, u, v, sigma, Cout, RS, Cin):
    """one power iteration: u, v are updated in place, sigma [1] = u . W v is written"""
    ws = torch.empty((RS * Cin + Cout + 2,), device=W.device, dtype=torch.float32)
    check(_lib.lib().jg_spectral_power_iter(W.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr(), ws.data_ptr(), Cout, RS, Cin, 1e-12, _st()),
          "jg_spectral_power_iter")


def spectral_wgrad_fix(dwsn, W, u, v, sigma, g, Cout, RS, Cin):
    """the gradient w.r.t. W of W / sigma(W) with u, v constant, from dwsn = d / d(W / sigma), is accumulated into g"""
    ws = torch.empty((1,), device=W.device, dtype=torch.float32)
    check(_lib.lib().jg_spectral_wgrad_fix(dwsn.data_ptr(), W.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr(), g.data_ptr(), ws.data_ptr(),
                                           Cout, RS, Cin, _st()), "jg_spectral_wgrad_fix")
