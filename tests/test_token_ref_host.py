"""tests/token_ref.py -- the hand-written float64 references the guarded token-kernel tests (test_gpu_18_token_kernels_guarded.py) compare the
kernels with -- against torch's own float64 F.scaled_dot_product_attention, F.layer_norm and F.conv2d(groups=C) with autograd.  One small case
per reference; no GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import token_ref as tr

EXACT = 1e-12


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def _sdpa(q, k, v, scale):
    """[B, heads, T, d] operands -> o, logsumexp of the scaled logits"""
    return F.scaled_dot_product_attention(q, k, v, scale=scale), torch.logsumexp(scale * q @ k.transpose(-1, -2), -1)


def test_attention_legacy_layout():
    B, T, heads, ch = 2, 9, 3, 8
    qkv, da = rnd((B, T, 3 * heads * ch), 1).requires_grad_(True), rnd((B, T, heads * ch), 2)
    x = qkv.view(B, T, heads, 3, ch)                                  # channel = h * 3 ch + {q, k, v} * ch + c
    q, k, v = (x[:, :, :, i].transpose(1, 2) for i in range(3))
    o, L = _sdpa(q, k, v, 1 / math.sqrt(ch))
    a = o.transpose(1, 2).reshape(B, T, heads * ch)
    a.backward(da)
    r = tr.attention_legacy(qkv.detach(), heads, da)
    assert rel(r["a"], a.detach()) < EXACT and rel(r["L"], L.detach().reshape(B * heads, T)) < EXACT and rel(r["dqkv"], qkv.grad) < EXACT
    assert rel(r["D"], (da * a.detach()).view(B, T, heads, ch).sum(-1).transpose(1, 2).reshape(B * heads, T)) < EXACT
    assert set(tr.attention_legacy(qkv.detach(), heads)) == {"a", "L"}


def test_attention_timm_layout():
    B, T, heads, hd = 2, 7, 2, 16
    C = heads * hd
    qkv, do = rnd((B, T, 3 * C), 3).requires_grad_(True), rnd((B, T, C), 4)
    q, k, v = qkv.view(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)     # timm Attention.forward
    o, L = _sdpa(q, k, v, 0.3)
    o = o.transpose(1, 2).reshape(B, T, C)
    o.backward(do)
    r = tr.attention_timm(qkv.detach(), heads, 0.3, do)
    assert rel(r["o"], o.detach()) < EXACT and rel(r["L"], L.detach().reshape(B * heads, T)) < EXACT and rel(r["dqkv"], qkv.grad) < EXACT


def test_attention_smallkv_layout():
    B, Tq, Tkv, heads = 2, 11, 5, 3
    C = heads * 32
    q, kv, do = rnd((B, Tq, C), 5).requires_grad_(True), rnd((B, Tkv, 2 * C), 6).requires_grad_(True), rnd((B, Tq, C), 7)
    qh = q.view(B, Tq, heads, 32).transpose(1, 2)
    kh, vh = (kv[..., i * C:(i + 1) * C].reshape(B, Tkv, heads, 32).transpose(1, 2) for i in range(2))
    o, L = _sdpa(qh, kh, vh, 1 / math.sqrt(32))
    o = o.transpose(1, 2).reshape(B, Tq, C)
    o.backward(do)
    r = tr.attention_smallkv(q.detach(), kv.detach(), heads, 1 / math.sqrt(32), do)
    assert rel(r["o"], o.detach()) < EXACT and rel(r["lse"], L.detach().reshape(B * heads, Tq)) < EXACT
    assert rel(r["dq"], q.grad) < EXACT and rel(r["dkv"], kv.grad) < EXACT


def test_attention_emulation_stays_near_the_exact_value():
    """prec = a 16-bit type: same function, float32 with the kernels' roundings -- a few units of that type's rounding away, no more"""
    q, kv, do = rnd((1, 40, 64), 8).half(), rnd((1, 24, 128), 9).half(), rnd((1, 40, 64), 10).half()
    ex = tr.attention_smallkv(q, kv, 2, 1 / math.sqrt(32), do)
    em = tr.attention_smallkv(q, kv, 2, 1 / math.sqrt(32), do, prec=torch.float16)
    for n in ("o", "dq", "dkv"):
        assert em[n].dtype == torch.float32 and 1e-5 < rel(em[n].double(), ex[n]) < 2e-3, (n, rel(em[n].double(), ex[n]))
    assert float((em["lse"].double() - ex["lse"]).abs().max()) < 1e-5


def test_layernorm_and_add_forms():
    R, C, rpi, eps = 10, 24, 4, 1e-6                                    # rows_per_image does not divide R
    x, add, dy, res = rnd((R, C), 11), rnd((R, C), 12), rnd((R, C), 13), rnd((R, C), 14)
    g, b = (1 + 0.2 * rnd((C,), 15)).requires_grad_(True), (0.1 * rnd((C,), 16)).requires_grad_(True)
    scale = torch.tensor([0.0, 1 / 0.7, 0.5], dtype=torch.float64)
    sc = tr.image_scale(scale, rpi, R, torch.float64)
    assert sc[:, 0].tolist() == [0.0] * 4 + [1 / 0.7] * 4 + [0.5] * 2 and float(tr.image_scale(None, rpi, R, torch.float64).min()) == 1.0
    xs, ad = x.clone().requires_grad_(True), add.clone().requires_grad_(True)
    xsum = xs + ad * sc                                                # jg_layernorm_fwd_add
    y = F.layer_norm(xsum, (C,), g, b, eps)
    (y * dy).sum().backward(retain_graph=True)
    (xsum * res).sum().backward()                                      # the gradient that reaches the sum past the LayerNorm: `res`
    yr, mr = tr.layernorm_fwd(xsum.detach(), g.detach(), b.detach(), eps)
    assert rel(yr, y.detach()) < EXACT
    assert rel(mr[:, 0], xsum.detach().mean(-1)) < EXACT and rel(mr[:, 1], 1 / torch.sqrt(xsum.detach().var(-1, unbiased=False) + eps)) < EXACT
    dx, dg, db = tr.layernorm_bwd(xsum.detach(), dy, g.detach(), eps, res)
    assert rel(dx, xs.grad) < EXACT and rel(dx * sc, ad.grad) < EXACT and rel(dg, g.grad) < EXACT and rel(db, b.grad) < EXACT
    dx0 = tr.layernorm_bwd(xsum.detach(), dy, g.detach(), eps)[0]
    assert rel(dx0 + res, dx) < EXACT


@pytest.mark.parametrize("reflect", [False, True], ids=["zero", "reflect"])
@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
def test_dwconv3x3(gelu, reflect):
    B, H, W, C = 2, 4, 5, 6
    x, dy = rnd((B, C, H, W), 17).requires_grad_(True), rnd((B, C, H, W), 18)
    w, b = rnd((C, 1, 3, 3), 19, 0.4).requires_grad_(True), rnd((C,), 20, 0.1).requires_grad_(True)
    pre = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b, groups=C) if reflect else F.conv2d(x, w, b, padding=1, groups=C)
    y = F.gelu(pre) if gelu else pre
    y.backward(dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    pr, yr = tr.dwconv3x3_fwd(nhwc(x), w.detach().view(C, 3, 3), b.detach(), gelu, reflect)
    assert rel(pr, nhwc(pre)) < EXACT and rel(yr, nhwc(y)) < EXACT
    du, dx, dw, db = tr.dwconv3x3_bwd(nhwc(x), pr, nhwc(dy), w.detach().view(C, 3, 3), gelu, reflect)
    assert rel(dx, nhwc(x.grad)) < EXACT and rel(dw, w.grad.view(C, 3, 3)) < EXACT and rel(db, b.grad) < EXACT
    if not gelu:
        assert torch.equal(du, nhwc(dy))
    assert rel(tr.dwconv3x3_fwd(nhwc(x), w.detach().view(C, 3, 3), None, gelu, reflect)[0] + b.detach(), pr) < EXACT
