"""Plain references of the token-side kernels (attention in its three layouts, LayerNorm with its add forms, the depth-wise 3x3 convolution)
with their gradients written out by hand -- no autograd, no GPU.  tests/test_token_ref_host.py holds them to torch's own float64
F.scaled_dot_product_attention / F.layer_norm / F.conv2d(groups=C) and autograd; tests/test_gpu_18_token_kernels_guarded.py compares the kernels
with them.

prec = None evaluates in float64.  prec = torch.float16 / torch.bfloat16 evaluates in float32 and rounds to that type where the kernels do
(P in front of P V, dS in front of the dq / dk products, every 16-bit output): the emulation the per-row bounds of the GPU module are
checked against.  It models the roundings, not any kernel's order of summation."""
import math

import torch


def _wk(prec):
    return torch.float64 if prec is None else torch.float32


def _r(t, prec):
    return t if prec is None else t.to(prec).to(t.dtype)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def attn_core(q, k, v, scale, do=None, prec=None):
    """q [N, Tq, d], k / v [N, Tkv, d], do [N, Tq, d] or None -> dict(o, L[, dq, dk, dv, D]); L = logsumexp of the scaled logits,
    D = rowsum(do * o).  o = (round(exp(S - max)) V) / rowsum(exp(S - max)), the flash form."""
    w = _wk(prec)
    q, k, v = q.to(w), k.to(w), v.to(w)
    S = scale * (q @ k.transpose(1, 2))
    m = S.max(-1, keepdim=True).values
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    out = {"o": _r((_r(E, prec) @ v) / l, prec), "L": (m + torch.log(l)).squeeze(-1)}
    if do is None:
        return out
    do = do.to(w)
    P = torch.exp(S - out["L"][..., None])
    D = (do * out["o"]).sum(-1)
    dS = _r(P * (do @ v.transpose(1, 2) - D[..., None]), prec)
    out.update(D=D, dq=_r(scale * (dS @ k), prec), dk=_r(scale * (dS.transpose(1, 2) @ q), prec), dv=_r(_r(P, prec).transpose(1, 2) @ do, prec))
    return out


def split_heads(x, heads):
    """[B, T, heads * d] -> [B * heads, T, d]"""
    B, T, C = x.shape
    return x.reshape(B, T, heads, C // heads).permute(0, 2, 1, 3).reshape(B * heads, T, C // heads)


def merge_heads(x, heads):
    """[B * heads, T, d] -> [B, T, heads * d]"""
    N, T, d = x.shape
    return x.reshape(N // heads, heads, T, d).permute(0, 2, 1, 3).reshape(N // heads, T, heads * d)


def attention_legacy(qkv, heads, da=None, prec=None):
    """jg_attention_fwd / _bwd: qkv [B, T, 3C], channel = h * 3 ch + {q, k, v} * ch + c; scale 1 / sqrt(ch).
    -> dict(a [B, T, C], L [B * heads, T][, dqkv [B, T, 3C], D [B * heads, T]])"""
    B, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    x = qkv.reshape(B, T, heads, 3, ch)
    q, k, v = (x[:, :, :, i].permute(0, 2, 1, 3).reshape(B * heads, T, ch) for i in range(3))
    r = attn_core(q, k, v, 1.0 / math.sqrt(ch), None if da is None else split_heads(da, heads), prec)
    out = {"a": merge_heads(r["o"], heads), "L": r["L"]}
    if da is not None:
        g = torch.stack([r[n].reshape(B, heads, T, ch).permute(0, 2, 1, 3) for n in ("dq", "dk", "dv")], 3)      # [B, T, heads, 3, ch]
        out.update(dqkv=g.reshape(B, T, C3), D=r["D"])
    return out


def attention_timm(qkv, heads, scale, do=None, prec=None):
    """jg_vit_attention_fwd / _bwd on the packed projection: qkv [B, T, 3C], channel order [3][heads][head_dim].
    -> dict(o [B, T, C], L [B * heads, T][, dqkv [B, T, 3C], D])"""
    C = qkv.shape[-1] // 3
    q, k, v = (split_heads(qkv[..., i * C:(i + 1) * C], heads) for i in range(3))
    r = attn_core(q, k, v, scale, None if do is None else split_heads(do, heads), prec)
    out = {"o": merge_heads(r["o"], heads), "L": r["L"]}
    if do is not None:
        out.update(dqkv=torch.cat([merge_heads(r[n], heads) for n in ("dq", "dk", "dv")], -1), D=r["D"])
    return out


def attention_smallkv(q, kv, heads, scale, do=None, prec=None):
    """jg_attn_smallkv_fwd / _bwd2: q [B, Tq, C], kv [B, Tkv, 2C] = (k | v), head dim C / heads.
    -> dict(o [B, Tq, C], lse [B * heads, Tq][, dq [B, Tq, C], dkv [B, Tkv, 2C]])"""
    C = q.shape[-1]
    r = attn_core(split_heads(q, heads), split_heads(kv[..., :C], heads), split_heads(kv[..., C:], heads), scale,
                  None if do is None else split_heads(do, heads), prec)
    out = {"o": merge_heads(r["o"], heads), "lse": r["L"]}
    if do is not None:
        out.update(dq=merge_heads(r["dq"], heads), dkv=torch.cat([merge_heads(r["dk"], heads), merge_heads(r["dv"], heads)], -1))
    return out


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def image_scale(scale, rows_per_image, R, w):
    """[R, 1] factor of row r: scale[r // rows_per_image] (scale None: 1)"""
    if scale is None:
        return torch.ones(R, 1, dtype=w)
    return scale.to(w)[torch.arange(R) // rows_per_image][:, None]


def layernorm_fwd(x, gamma, beta, eps, prec=None):
    """x [R, C] -> y [R, C], mr [R, 2] = (mean, rstd), biased variance"""
    w = _wk(prec)
    x = x.to(w)
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return _r((x - mean) * rstd * gamma.to(w) + beta.to(w), prec), torch.cat([mean, rstd], -1)


def layernorm_bwd(x, dy, gamma, eps, res=None, prec=None):
    """-> dx = (res +) rstd (g - mean(g) - xh mean(g xh)) with g = dy gamma, xh = (x - mean) rstd;  dgamma = sum dy xh;  dbeta = sum dy"""
    w = _wk(prec)
    x, dy = x.to(w), dy.to(w)
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    g = dy * gamma.to(w)
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if res is not None:
        dx = dx + res.to(w)
    return _r(dx, prec), (dy * xh).sum(0), dy.sum(0)


# ---- depth-wise 3x3 convolution, NHWC, weight [C, 3, 3] ----------------------------------------------------------------------------------------
def gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _tap(n, d, reflect):
    """source index and validity of tap offset d in {-1, 0, 1} along an axis of length n"""
    i = torch.arange(n) + d
    if reflect:
        i = torch.where(i < 0, -i, i)
        i = torch.where(i >= n, 2 * (n - 1) - i, i)
        return i, torch.ones(n, dtype=torch.bool)
    ok = (i >= 0) & (i < n)
    return i.clamp(0, n - 1), ok


def dwconv3x3_fwd(x, wgt, bias, gelu_on, reflect, prec=None):
    """x [B, H, W, C], wgt [C, 3, 3] (cross-correlation, padding 1, zero or reflect), bias [C] or None -> (pre, y), y = gelu(pre) or pre"""
    w = _wk(prec)
    x, wgt = x.to(w), wgt.to(w)
    B, H, W, C = x.shape
    pre = torch.zeros_like(x)
    for ky in range(3):
        iy, oky = _tap(H, ky - 1, reflect)
        for kx in range(3):
            ix, okx = _tap(W, kx - 1, reflect)
            m = (oky[:, None] & okx[None, :]).to(w)[None, :, :, None]
            pre = pre + x[:, iy][:, :, ix] * m * wgt[:, ky, kx]
    if bias is not None:
        pre = pre + bias.to(w)
    return _r(pre, prec), _r(gelu(pre) if gelu_on else pre, prec)


def dwconv3x3_bwd(x, pre, dy, wgt, gelu_on, reflect, prec=None):
    """-> (du = dy gelu'(pre) or dy, dx, dw [C, 3, 3], dbias [C]); dx from the rounded du, as the kernels read it back"""
    w = _wk(prec)
    x, dy, wgt = x.to(w), dy.to(w), wgt.to(w)
    B, H, W, C = x.shape
    du = dy * gelu_grad(pre.to(w)) if gelu_on else dy
    dur = _r(du, prec)
    dx = torch.zeros_like(x)
    dw = torch.zeros(C, 3, 3, dtype=w)
    for ky in range(3):
        iy, oky = _tap(H, ky - 1, reflect)
        for kx in range(3):
            ix, okx = _tap(W, kx - 1, reflect)
            m = (oky[:, None] & okx[None, :]).to(w)[None, :, :, None]
            dw[:, ky, kx] = (du * m * x[:, iy][:, :, ix]).sum((0, 1, 2))
            flat = (iy[:, None] * W + ix[None, :]).reshape(-1)
            dx.view(B, H * W, C).index_add_(1, flat, (dur * m * wgt[:, ky, kx]).reshape(B, H * W, C))
    return dur, _r(dx, prec), dw, du.sum((0, 1, 2))
