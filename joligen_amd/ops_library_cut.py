"""`torch.ops.jg355.*` for the CUT family (VERDICT r4 missing #2; north_star: the kernels "exposed to the Python host as torch.ops"; precedent in
the reference: /root/reference/models/modules/op/upfirdn2d.py:19-167, a custom op with its own forward / backward pair).

Every op here is a torch.library custom op over the C ABI of include/jg355.h with a fake (meta) kernel and an autograd formula made of
other jg355 ops, so it traces (FakeTensor / torch.compile), composes with autograd and passes torch.library.opcheck
(tests/test_gpu_0_ops.py::test_torch_ops_surface_cut).  The ops are FUNCTIONAL: parameter gradients are RETURNED as fresh tensors (the
module graph's arena-accumulating nodes add them in place; `ops.torch_ops_boundary()` switches the modules to these ops, and
tests/test_gpu_5_cutloss.py::test_cut_step_through_torch_ops holds the two forms together on one CUT step).  The launches themselves are
the helpers of launch.py, the same ones the module graph calls: an op here is a schema, a fake kernel and an autograd formula; it makes its
inputs contiguous, hands fresh zeros to the accumulating kernels and turns a None output into the empty tensor its schema needs (`_z`).

  layer_norm / layer_norm_bwd                nn.LayerNorm of the SegFormer blocks and the ViT projector
  dwconv3x3_gelu / _bwd                      MixFFN's depth-wise 3x3 (+ GELU)
  attention_smallkv / _bwd                   EfficientMultiheadAttention core (spatially reduced keys / values)
  vit_attention / _bwd, gelu / gelu_bwd      timm Attention core / nn.GELU of the ViT projector
  reflect_pad2d / _bwd, reflect_conv2d / reflect_conv2d_wgrad      ReflectionPad2d(+ 3x3 conv in one launch) of the ResnetBlocks
  dilate2d                                   zero insertion (ConvTranspose2d = dilate + stride-1 conv on the flipped weights; stride-s dgrad)
  act / act_bwd                              stand-alone ReLU / LeakyReLU / Tanh
  gather_patches / scatter_patches, l2_normalize / _bwd, patch_nce / patch_nce_bwd      PatchSampleF + PatchNCE / MoNCE (Sinkhorn inside)
  patch_hdce / patch_hdce_bwd                SRC_hDCE: weights from the key Gram matrix + weighted contrastive loss, one fused kernel
  pixel_loss / pixel_loss_bwd                paired (supervised) and identity L1 / MSE between 16-bit images, both terms in one launch set
  cls_loss                                   train_semantic_cls: cross entropy / MSE / L1 with the device-side gate, gradient and argmax, one launch
  d_aug, apa_update                          dataaug_D_noise + adaptive pseudo augmentation: the discriminators' inputs of a step; the update of p
  context_split, context_frame / _bwd        data_online_context_pixels: crop + framed image from one read; the translated crop inside its frame (+ D noise)
  d_diffusion / _bwd, d_diffusion_update     dataaug_D_diffusion: the noised backbone features of the projected discriminator; the update of its state
  gan_loss, hinge_loss                       GANLoss (lsgan / vanilla / wgangp) and the projected hinge; return (loss, d loss / d pred)
  spectral_weight / _bwd                     torch.nn.utils.spectral_norm: one power iteration, W / sigma; gradient through 1 / sigma
  bilinear2 / bilinear2_bwd                  F.interpolate(mode="bilinear", align_corners=...)
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib, launch, ops
from ._lib import check
from .launch import SINKHORN_ITERS, _DT, _dt, _st
from .ops import conv_nt, wgrad_tn

T = torch.Tensor
op = torch.library.custom_op


def _z(like, dtype=torch.float32):
    return torch.zeros(0, device=like.device, dtype=dtype)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
@op("jg355::layer_norm", mutates_args=())
def layer_norm(x: T, weight: T, bias: T, eps: float) -> Tuple[T, T]:
    """nn.LayerNorm(C, eps) over the last dimension of a 16-bit tensor -> (y, mr [rows, 2] = mean | rstd saved for the backward)"""
    return launch.layernorm_fwd(x.contiguous(), weight, bias, eps)


@layer_norm.register_fake
def _(x, weight, bias, eps):
    return torch.empty_like(x), x.new_empty((x.numel() // x.shape[-1], 2), dtype=torch.float32)


@op("jg355::layer_norm_bwd", mutates_args=())
def layer_norm_bwd(x: T, dy: T, weight: T, mr: T) -> Tuple[T, T, T]:
    C = x.shape[-1]
    dg, db = torch.zeros(C, device=x.device, dtype=torch.float32), torch.zeros(C, device=x.device, dtype=torch.float32)
    return launch.layernorm_bwd(x.contiguous(), dy.contiguous(), weight, mr, dg, db), dg, db


@layer_norm_bwd.register_fake
def _(x, dy, weight, mr):
    C = x.shape[-1]
    return torch.empty_like(x), x.new_empty((C,), dtype=torch.float32), x.new_empty((C,), dtype=torch.float32)


def _ln_setup(ctx, inputs, output):
    x, weight, bias, eps = inputs
    ctx.save_for_backward(x, weight, output[1])


def _ln_backward(ctx, dy, dmr):
    x, weight, mr = ctx.saved_tensors
    dx, dg, db = torch.ops.jg355.layer_norm_bwd(x, dy, weight, mr)
    return dx, dg, db, None


layer_norm.register_autograd(_ln_backward, setup_context=_ln_setup)


# ---- depth-wise 3x3 (+ GELU) ---------------------------------------------------------------------------------------------------------
@op("jg355::dwconv3x3_gelu", mutates_args=())
def dwconv3x3_gelu(x: T, weight: T, bias: Optional[T], gelu: bool) -> Tuple[T, T]:
    """nn.Conv2d(C, C, 3, padding=1, groups=C) (+ nn.GELU()) on an NHWC map; weight fp32 [C, 1, 3, 3] -> (y, pre-activation; empty without gelu)"""
    y, pre = launch.dwconv3x3_fwd(x.contiguous(), weight.contiguous(), bias, gelu)
    return y, (pre if gelu else _z(x, x.dtype))


@dwconv3x3_gelu.register_fake
def _(x, weight, bias, gelu):
    return torch.empty_like(x), (torch.empty_like(x) if gelu else x.new_empty((0,)))


@op("jg355::dwconv3x3_gelu_bwd", mutates_args=())
def dwconv3x3_gelu_bwd(x: T, pre: T, dy: T, weight: T, gelu: bool) -> Tuple[T, T, T]:
    C = x.shape[-1]
    dw = torch.zeros((C, 1, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.zeros(C, device=x.device, dtype=torch.float32)
    return launch.dwconv3x3_bwd(x.contiguous(), pre if gelu else None, dy.contiguous(), weight.contiguous(), dw, db, gelu), dw, db


@dwconv3x3_gelu_bwd.register_fake
def _(x, pre, dy, weight, gelu):
    C = x.shape[-1]
    return torch.empty_like(x), x.new_empty((C, 1, 3, 3), dtype=torch.float32), x.new_empty((C,), dtype=torch.float32)


def _dw_setup(ctx, inputs, output):
    x, weight, bias, gelu = inputs
    ctx.save_for_backward(x, output[1], weight)
    ctx.gelu, ctx.has_bias = gelu, bias is not None


def _dw_backward(ctx, dy, dpre):
    x, pre, weight = ctx.saved_tensors
    dx, dw, db = torch.ops.jg355.dwconv3x3_gelu_bwd(x, pre, dy, weight, ctx.gelu)
    return dx, dw, (db if ctx.has_bias else None), None


dwconv3x3_gelu.register_autograd(_dw_backward, setup_context=_dw_setup)


# ---- attention cores -------------------------------------------------------------------------------------------------------------------
@op("jg355::attention_smallkv", mutates_args=())
def attention_smallkv(q: T, kv: T, heads: int) -> Tuple[T, T]:
    """q [B, Tq, C], kv [B, Tkv, 2C] packed (k | v), head dim 32 -> (o [B, Tq, C], logsumexp [B, heads, Tq])"""
    return launch.attn_smallkv_fwd(q.contiguous(), kv.contiguous(), heads)


@attention_smallkv.register_fake
def _(q, kv, heads):
    return torch.empty_like(q), q.new_empty((q.shape[0], heads, q.shape[1]), dtype=torch.float32)


@op("jg355::attention_smallkv_bwd", mutates_args=())
def attention_smallkv_bwd(q: T, kv: T, o: T, lse: T, do: T, heads: int) -> Tuple[T, T]:
    return launch.attn_smallkv_bwd(q.contiguous(), kv.contiguous(), o, lse, do.contiguous(), heads)


@attention_smallkv_bwd.register_fake
def _(q, kv, o, lse, do, heads):
    return torch.empty_like(q), torch.empty_like(kv)


def _skv_setup(ctx, inputs, output):
    q, kv, heads = inputs
    ctx.save_for_backward(q, kv, output[0], output[1])
    ctx.heads = heads


def _skv_backward(ctx, do, dlse):
    q, kv, o, lse = ctx.saved_tensors
    dq, dkv = torch.ops.jg355.attention_smallkv_bwd(q, kv, o, lse, do, ctx.heads)
    return dq, dkv, None


attention_smallkv.register_autograd(_skv_backward, setup_context=_skv_setup)


@op("jg355::vit_attention", mutates_args=())
def vit_attention(qkv: T, heads: int) -> Tuple[T, T]:
    """timm Attention core on the packed projection [B, T, 3C] (channel order [3][heads][head_dim], head dim 32 / 64, any T) -> (a, logsumexp)"""
    return launch.vit_attention_fwd(qkv.contiguous(), heads)


@vit_attention.register_fake
def _(qkv, heads):
    B, Tn, C3 = qkv.shape
    return qkv.new_empty((B, Tn, C3 // 3)), qkv.new_empty((B * heads, Tn), dtype=torch.float32)


@op("jg355::vit_attention_bwd", mutates_args=())
def vit_attention_bwd(qkv: T, a: T, lse: T, da: T, heads: int) -> T:
    return launch.vit_attention_bwd(qkv.contiguous(), a, lse, da.contiguous(), heads)


@vit_attention_bwd.register_fake
def _(qkv, a, lse, da, heads):
    return torch.empty_like(qkv)


def _va_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output[0], output[1])
    ctx.heads = inputs[1]


def _va_backward(ctx, da, dl):
    qkv, a, lse = ctx.saved_tensors
    return torch.ops.jg355.vit_attention_bwd(qkv, a, lse, da, ctx.heads), None


vit_attention.register_autograd(_va_backward, setup_context=_va_setup)


@op("jg355::gelu", mutates_args=())
def gelu(x: T) -> T:
    return launch.gelu_fwd(x.contiguous())


@gelu.register_fake
def _(x):
    return torch.empty_like(x)


@op("jg355::gelu_bwd", mutates_args=())
def gelu_bwd(x: T, dy: T) -> T:
    return launch.gelu_bwd(x.contiguous(), dy.contiguous())


@gelu_bwd.register_fake
def _(x, dy):
    return torch.empty_like(x)


gelu.register_autograd(lambda ctx, dy: torch.ops.jg355.gelu_bwd(ctx.saved_tensors[0], dy),
                       setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0]))


# ---- padding / dilation / activation ----------------------------------------------------------------------------------------------------
@op("jg355::reflect_pad2d", mutates_args=())
def reflect_pad2d(x: T, pad: int) -> T:
    return launch.reflect_pad2d(x.contiguous(), pad)


@reflect_pad2d.register_fake
def _(x, pad):
    B, H, W, C = x.shape
    return x.new_empty((B, H + 2 * pad, W + 2 * pad, C))


@op("jg355::reflect_pad2d_bwd", mutates_args=())
def reflect_pad2d_bwd(dy: T, pad: int) -> T:
    """adjoint of ReflectionPad2d(pad): dy [B, H + 2 pad, W + 2 pad, C] folded back onto [B, H, W, C]"""
    return launch.reflect_pad2d_bwd(dy.contiguous(), pad)


@reflect_pad2d_bwd.register_fake
def _(dy, pad):
    B, Hp, Wp, C = dy.shape
    return dy.new_empty((B, Hp - 2 * pad, Wp - 2 * pad, C))


reflect_pad2d.register_autograd(lambda ctx, dy: (torch.ops.jg355.reflect_pad2d_bwd(dy, ctx.pad), None),
                                setup_context=lambda ctx, inputs, output: setattr(ctx, "pad", inputs[1]))
reflect_pad2d_bwd.register_autograd(lambda ctx, g: (torch.ops.jg355.reflect_pad2d(g, ctx.pad), None),
                                    setup_context=lambda ctx, inputs, output: setattr(ctx, "pad", inputs[1]))


@op("jg355::dilate2d", mutates_args=())
def dilate2d(x: T, Ho: int, Wo: int, stride: int) -> T:
    """zero insertion: y[:, s i, s j] = x[:, i, j] in a [B, Ho, Wo, C] buffer"""
    return ops.dilate2d(x.contiguous(), Ho, Wo, stride)


@dilate2d.register_fake
def _(x, Ho, Wo, stride):
    return x.new_empty((x.shape[0], Ho, Wo, x.shape[-1]))


def _dil_setup(ctx, inputs, output):
    ctx.geo = (inputs[0].shape[1], inputs[0].shape[2], inputs[3])


def _dil_backward(ctx, dy):
    H, W, s = ctx.geo
    return dy[:, ::s, ::s][:, :H, :W].contiguous(), None, None, None       # the adjoint of zero insertion is a strided view


dilate2d.register_autograd(_dil_backward, setup_context=_dil_setup)


@op("jg355::act", mutates_args=())
def act(x: T, kind: int) -> T:
    return launch.act_fwd(x.contiguous(), kind)


@act.register_fake
def _(x, kind):
    return torch.empty_like(x)


@op("jg355::act_bwd", mutates_args=())
def act_bwd(y: T, dy: T, kind: int) -> T:
    return launch.act_bwd(y.contiguous(), dy.contiguous(), kind)


@act_bwd.register_fake
def _(y, dy, kind):
    return torch.empty_like(y)


def _act_setup(ctx, inputs, output):
    ctx.save_for_backward(output)
    ctx.kind = inputs[1]


act.register_autograd(lambda ctx, dy: (torch.ops.jg355.act_bwd(ctx.saved_tensors[0], dy, ctx.kind), None), setup_context=_act_setup)


# ---- ReflectionPad2d(1) + 3x3 convolution in one launch ------------------------------------------------------------------------------------
@op("jg355::reflect_conv2d", mutates_args=())
def reflect_conv2d(x: T, w: T, bias: Optional[T]) -> T:
    """conv3x3(reflection_pad(x, 1)): x [B, H, W, Cin] 16-bit (Cin, Cout % 64 == 0, H, W % 16 == 0), w [Cout, 3, 3, Cin] (fp32 master or 16-bit)"""
    x = x.contiguous()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    y = torch.empty((B, H, W, Cout), device=x.device, dtype=x.dtype)
    conv_nt(x, w.to(x.dtype).contiguous(), y, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=Cin, ldw=9 * Cin,
            ldy=Cout, bias=bias, pad_mode=1)
    return y


@reflect_conv2d.register_fake
def _(x, w, bias):
    return x.new_empty((*x.shape[:3], w.shape[0]))


@op("jg355::reflect_conv2d_wgrad", mutates_args=())
def reflect_conv2d_wgrad(dy: T, x: T) -> Tuple[T, T]:
    dy, x = dy.contiguous(), x.contiguous()
    B, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    dw = torch.zeros((Cout, 3, 3, Cin), device=x.device, dtype=torch.float32)
    db = torch.zeros((Cout,), device=x.device, dtype=torch.float32)
    wgrad_tn(dy, x, dw, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, lddy=Cout, ldx=Cin, lddw=9 * Cin, dbias=db,
             splitk=ops._wgrad_splitk(((Cout + 127) // 128) * ((9 * Cin + 127) // 128), B * H * W), pad_mode=1)
    return dw, db


@reflect_conv2d_wgrad.register_fake
def _(dy, x):
    return x.new_empty((dy.shape[-1], 3, 3, x.shape[-1]), dtype=torch.float32), x.new_empty((dy.shape[-1],), dtype=torch.float32)


def _rc_setup(ctx, inputs, output):
    x, w, bias = inputs
    ctx.save_for_backward(x, w)
    ctx.has_bias = bias is not None


def _rc_backward(ctx, dy):
    x, w = ctx.saved_tensors
    dy = dy.contiguous()
    dx = dw = db = None
    if ctx.needs_input_grad[0]:      # full convolution over the padded domain, folded back by the reflection's adjoint
        wT = w.to(dy.dtype).permute(3, 1, 2, 0).flip(1, 2).contiguous()
        dx = torch.ops.jg355.reflect_pad2d_bwd(torch.ops.jg355.conv2d_nt(dy, wT, None, None, 2, 1, 1.0, 0.0), 1)
    if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
        dwf, dbf = torch.ops.jg355.reflect_conv2d_wgrad(dy, x)
        dw = dwf.to(w.dtype) if ctx.needs_input_grad[1] else None
        db = dbf if (ctx.has_bias and ctx.needs_input_grad[2]) else None
    return dx, dw, db


reflect_conv2d.register_autograd(_rc_backward, setup_context=_rc_setup)


# ---- PatchSampleF / PatchNCE ------------------------------------------------------------------------------------------------------------
@op("jg355::gather_patches", mutates_args=())
def gather_patches(feat: T, ids: T, C: int) -> T:
    """feat [B, H, W, ld] 16-bit -> [B * P, C] fp32 rows at the flattened positions ids (int64 [P], shared by the batch)"""
    feat, ids = feat.contiguous(), ids.contiguous()
    B, H, W, ld = feat.shape
    P = ids.numel()
    out = torch.empty((B * P, C), device=feat.device, dtype=torch.float32)
    check(_lib.lib().jg_gather_rows(_dt(feat), feat.data_ptr(), ld, ids.data_ptr(), out.data_ptr(), B, H * W, C, P, _st()), "jg_gather_rows")
    return out


@gather_patches.register_fake
def _(feat, ids, C):
    return feat.new_empty((feat.shape[0] * ids.numel(), C), dtype=torch.float32)


@op("jg355::scatter_patches", mutates_args=())
def scatter_patches(dout: T, ids: T, B: int, H: int, W: int, ld: int, fp16: bool) -> T:
    dout, ids = dout.contiguous(), ids.contiguous()
    dt = torch.float16 if fp16 else torch.bfloat16
    dfeat = torch.zeros((B, H, W, ld), device=dout.device, dtype=dt)
    check(_lib.lib().jg_scatter_rows(_DT[dt], dfeat.data_ptr(), ld, ids.data_ptr(), dout.data_ptr(), B, H * W, dout.shape[1], ids.numel(), _st()),
          "jg_scatter_rows")
    return dfeat


@scatter_patches.register_fake
def _(dout, ids, B, H, W, ld, fp16):
    return dout.new_empty((B, H, W, ld), dtype=torch.float16 if fp16 else torch.bfloat16)


def _gp_setup(ctx, inputs, output):
    feat, ids, C = inputs
    ctx.save_for_backward(ids)
    ctx.geo = (*feat.shape, feat.dtype == torch.float16)


def _gp_backward(ctx, dout):
    (ids,) = ctx.saved_tensors
    B, H, W, ld, fp16 = ctx.geo
    return torch.ops.jg355.scatter_patches(dout, ids, B, H, W, ld, fp16), None, None


gather_patches.register_autograd(_gp_backward, setup_context=_gp_setup)


@op("jg355::l2_normalize", mutates_args=())
def l2_normalize(x: T, eps: float) -> Tuple[T, T]:
    return launch.l2norm_fwd(x.contiguous(), eps)


@l2_normalize.register_fake
def _(x, eps):
    return torch.empty_like(x), x.new_empty((x.shape[0],))


@op("jg355::l2_normalize_bwd", mutates_args=())
def l2_normalize_bwd(y: T, nrm: T, dy: T, eps: float) -> T:
    return launch.l2norm_bwd(y, nrm, dy.contiguous(), eps)


@l2_normalize_bwd.register_fake
def _(y, nrm, dy, eps):
    return torch.empty_like(y)


def _l2_setup(ctx, inputs, output):
    ctx.save_for_backward(output[0], output[1])
    ctx.eps = inputs[1]


l2_normalize.register_autograd(lambda ctx, dy, dn: (torch.ops.jg355.l2_normalize_bwd(ctx.saved_tensors[0], ctx.saved_tensors[1], dy, ctx.eps), None),
                               setup_context=_l2_setup)


@op("jg355::patch_nce", mutates_args=())
def patch_nce(q: T, k: T, nimg: int, temp: float, pm1: float, monce: bool) -> Tuple[T, T, T, T, T]:
    """per-patch PatchNCE / MoNCE loss (base_NCE.py:17-66, monce.py:16-33; Sinkhorn iterations inside): q, k [nimg * P, D] fp32 L2-normalised
    -> (loss [nimg * P], logits S, and the optimal-transport state K, u-history, v-history: empty without monce)"""
    loss, S, K, uh, vh = launch.nce_fwd(q.contiguous(), k.contiguous(), nimg, temp, pm1, monce)
    return (loss, S, K, uh, vh) if monce else (loss, S, _z(q), _z(q), _z(q))


@patch_nce.register_fake
def _(q, k, nimg, temp, pm1, monce):
    R = q.shape[0]
    P = R // nimg
    e = q.new_empty((0,))
    if monce:
        return q.new_empty((R,)), q.new_empty((nimg, P, P)), q.new_empty((nimg, P, P)), q.new_empty((nimg, SINKHORN_ITERS, P)), q.new_empty((nimg, SINKHORN_ITERS + 1, P))
    return q.new_empty((R,)), q.new_empty((nimg, P, P)), e, q.new_empty((0,)), q.new_empty((0,))


@op("jg355::patch_nce_bwd", mutates_args=())
def patch_nce_bwd(q: T, k: T, S: T, K: T, uh: T, vh: T, dloss: T, nimg: int, temp: float, pm1: float, monce: bool) -> Tuple[T, T]:
    return launch.nce_bwd(q, k, S, K, uh, vh, dloss.contiguous().float(), nimg, temp, pm1, monce)


@patch_nce_bwd.register_fake
def _(q, k, S, K, uh, vh, dloss, nimg, temp, pm1, monce):
    return torch.empty_like(q), torch.empty_like(k)


def _nce_setup(ctx, inputs, output):
    q, k, nimg, temp, pm1, monce = inputs
    ctx.save_for_backward(q, k, *output[1:])
    ctx.cfg = (nimg, temp, pm1, monce)


def _nce_backward(ctx, dloss, *unused):
    q, k, S, K, uh, vh = ctx.saved_tensors
    dq, dk = torch.ops.jg355.patch_nce_bwd(q, k, S, K, uh, vh, dloss, *ctx.cfg)
    return dq, dk, None, None, None, None


patch_nce.register_autograd(_nce_backward, setup_context=_nce_setup)


@op("jg355::patch_hdce", mutates_args=())
def patch_hdce(q: T, k: T, nimg: int, temp: float, gamma: float, wperiod: int, wcount: int) -> Tuple[T, T, T, T]:
    """per-patch SRC_hDCE loss (NCE/SRC.py:46-75, NCE/hDCE.py:16-38): q, k [nimg * P, D] fp32; problem b is weighted iff (b % wperiod) < wcount
    -> (loss [nimg * P], logits S, key Gram matrix G (empty with wcount == 0), stats [3, nimg * P] = m | A | rinv for the backward)"""
    loss, S, G, stats = launch.hdce_fwd(q.contiguous(), k.contiguous(), nimg, temp, gamma, wperiod, wcount)
    return loss, S, (_z(q) if G is None else G), stats


def _hdce_ng(nimg, wperiod, wcount):
    return 0 if wcount < 1 else (min(wcount, nimg) if wperiod >= nimg else nimg)


@patch_hdce.register_fake
def _(q, k, nimg, temp, gamma, wperiod, wcount):
    R = q.shape[0]
    P = R // nimg
    ng = _hdce_ng(nimg, wperiod, wcount)
    return q.new_empty((R,)), q.new_empty((nimg, P, P)), (q.new_empty((ng, P, P)) if ng else q.new_empty((0,))), q.new_empty((3, R))


@op("jg355::patch_hdce_bwd", mutates_args=())
def patch_hdce_bwd(q: T, k: T, S: T, G: T, stats: T, dloss: T, nimg: int, temp: float, gamma: float, wperiod: int, wcount: int) -> Tuple[T, T]:
    return launch.hdce_bwd(q, k, S, G if G.numel() else None, stats, dloss.contiguous().float(), nimg, temp, gamma, wperiod, wcount)


@patch_hdce_bwd.register_fake
def _(q, k, S, G, stats, dloss, nimg, temp, gamma, wperiod, wcount):
    return torch.empty_like(q), torch.empty_like(k)


def _hdce_setup(ctx, inputs, output):
    q, k, nimg, temp, gamma, wperiod, wcount = inputs
    ctx.save_for_backward(q, k, *output[1:])
    ctx.cfg = (nimg, temp, gamma, wperiod, wcount)


def _hdce_backward(ctx, dloss, *unused):
    q, k, S, G, stats = ctx.saved_tensors
    dq, dk = torch.ops.jg355.patch_hdce_bwd(q, k, S, G, stats, dloss, *ctx.cfg)
    return dq, dk, None, None, None, None, None


patch_hdce.register_autograd(_hdce_backward, setup_context=_hdce_setup)


# ---- paired / identity pixel losses ---------------------------------------------------------------------------------------------------
@op("jg355::pixel_loss", mutates_args=())
def pixel_loss(x: T, y: T, C: int, modes: List[int], lambdas: List[float]) -> T:
    """nn.L1Loss / nn.MSELoss between 16-bit NHWC images (cut_model.py:771-786): x [S*M, H, W, 8] in S = len(modes) segments, each against
    y [M, H, W, 8] over the C valid channels; mode 0 off, 1 L1, 2 MSE -> the S weighted losses (fp32 [S])"""
    return ops._pixel_loss_launch(x.contiguous(), y.contiguous(), C, modes, lambdas)


@pixel_loss.register_fake
def _(x, y, C, modes, lambdas):
    return x.new_empty((len(modes),), dtype=torch.float32)


@op("jg355::pixel_loss_bwd", mutates_args=())
def pixel_loss_bwd(x: T, y: T, g: T, C: int, modes: List[int], lambdas: List[float]) -> T:
    """d (sum_s g[s] loss[s]) / dx: g [S] read on the device, d = x - y recomputed; zero pad channels / off segments"""
    return ops._pixel_loss_bwd_launch(x.contiguous(), y.contiguous(), g, C, modes, lambdas)


@pixel_loss_bwd.register_fake
def _(x, y, g, C, modes, lambdas):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


def _pl_setup(ctx, inputs, output):
    x, y, C, modes, lambdas = inputs
    ctx.save_for_backward(x, y)
    ctx.cfg = (C, list(modes), list(lambdas))


def _pl_backward(ctx, g):
    x, y = ctx.saved_tensors
    return torch.ops.jg355.pixel_loss_bwd(x, y, g, *ctx.cfg), None, None, None, None


pixel_loss.register_autograd(_pl_backward, setup_context=_pl_setup)


# ---- class loss of the semantic-consistency branch ------------------------------------------------------------------------------------
@op("jg355::cls_loss", mutates_args=())
def cls_loss(logits: T, target: T, mode: int, lam: float, prev: Optional[T], threshold: float) -> Tuple[T, T, T]:
    """ops.cls_loss as a functional op: -> (loss fp32 scalar, d loss / d logits [B, n] for a unit upstream gradient, argmax int64 [B]); mode 0
    cross entropy (int64 labels), 1 MSE, 2 L1 (fp32 targets, n == 1); gate = !(prev > threshold) on the device.  The gate state that the
    C entry point can write in the same launch is an in-place update: a functional op leaves it to the caller"""
    return ops._cls_loss_launch(logits, target, mode, lam, prev, threshold, None, False)


@cls_loss.register_fake
def _(logits, target, mode, lam, prev, threshold):
    B, n = logits.shape
    return logits.new_empty((), dtype=torch.float32), logits.new_empty((B, n)), logits.new_empty((B,), dtype=torch.int64)


def _cls_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.set_materialize_grads(False)


def _cls_backward(ctx, gloss, gd, gargmax):
    (dlogits,) = ctx.saved_tensors
    g = None if gloss is None else ops._cls_loss_scale(dlogits, gloss)
    return (g,) + (None,) * 5


cls_loss.register_autograd(_cls_backward, setup_context=_cls_setup)


# ---- discriminator-input augmentations (not differentiable: the reference detaches their inputs) -----------------------------------------
@op("jg355::d_aug", mutates_args=())
def d_aug(src: T, alts: List[T], ps: List[T], us: List[T], streams: List[int], C: int, sigma: float, z: Optional[T], key: Optional[T],
          noise_stream: int, call: int) -> Tuple[T, T]:
    """ops.d_aug as a functional op: -> (out [nd, B, H, W, Cpad], flags int32 [nd, B]); nd = max(len(alts), 1); empty lists = not given"""
    nd = max(len(alts), 1)
    src = src.contiguous()
    out = torch.empty((nd,) + tuple(src.shape), device=src.device, dtype=src.dtype)
    flags = torch.zeros((nd, src.shape[0]), device=src.device, dtype=torch.int32)
    has = len(alts) > 0
    ops._d_aug_launch(src, C, sigma, z, key, noise_stream, call, [a.contiguous() for a in alts] if has else None, list(ps) if has else None,
                      list(us) if has and len(us) else None, list(streams) if has else None, list(out.unbind(0)), flags if has else None)
    return out, flags


@d_aug.register_fake
def _(src, alts, ps, us, streams, C, sigma, z, key, noise_stream, call):
    nd = max(len(alts), 1)
    return src.new_empty((nd,) + tuple(src.shape)), src.new_empty((nd, src.shape[0]), dtype=torch.int32)


@op("jg355::apa_update", mutates_args=("state",))
def apa_update(pred: T, state: T, n: int, stride: int, target: float, num: float, den: float) -> None:
    """ops.apa_update: `state` = fp32 [3] (p, adjust, s) is updated in place from the n elements pred[i * stride]"""
    ops._apa_update_launch(pred, state, n, stride, target, num, den)


@apa_update.register_fake
def _(pred, state, n, stride, target, num, den):
    return None


# ---- data_online_context_pixels: the loader's image split into crop + surroundings; the frame around the translated crop -----------------
@op("jg355::context_split", mutates_args=())
def context_split(x: T, c: int, fp16: bool, cpad: int) -> Tuple[T, T]:
    """ops.context_split as a functional op: fp32 NCHW [B, C, H, W] -> (ctx [B, H, W, Cpad], crop = ctx[:, c:-c, c:-c]), 16-bit NHWC; cpad 0: C
    rounded up to a multiple of 8.  Not differentiable (the images are data)"""
    ops._context_split_check(x, c)
    return launch.context_split(x.contiguous(), c, torch.float16 if fp16 else torch.bfloat16, cpad or None)


@context_split.register_fake
def _(x, c, fp16, cpad):
    B, C, H, W = x.shape
    dt, cp = torch.float16 if fp16 else torch.bfloat16, cpad or (C + 7) // 8 * 8
    return x.new_empty((B, H, W, cp), dtype=dt), x.new_empty((B, H - 2 * c, W - 2 * c, cp), dtype=dt)


@op("jg355::context_frame", mutates_args=())
def context_frame(inner: T, ctx: T, c: int, C: int, sigma: float, z: Optional[T], key: Optional[T], noise_stream: int, call: int,
                  want_noisy: bool) -> Tuple[T, T]:
    """ops.context_frame as a functional op: -> (out = inner inside the window of ctx, ctx on the frame; out_noisy = out + sigma z, or an empty
    tensor unless `want_noisy`)"""
    ctx = ctx.contiguous()
    ops._context_frame_check(inner, ctx, c, C, z, key, None)
    out, noisy = launch.context_frame(inner.contiguous(), ctx, c, C, sigma, z, key, noise_stream, call, want_noisy=want_noisy)
    return out, noisy if noisy is not None else _z(ctx, ctx.dtype)


@context_frame.register_fake
def _(inner, ctx, c, C, sigma, z, key, noise_stream, call, want_noisy):
    out = torch.empty_like(ctx, memory_format=torch.contiguous_format)
    return out, torch.empty_like(out) if want_noisy else ctx.new_empty((0,))


@op("jg355::context_frame_bwd", mutates_args=())
def context_frame_bwd(dout: T, c: int) -> T:
    """the adjoint of the frame with respect to `inner`: the window dout[:, c:-c, c:-c]"""
    B, H, W, _ = dout.shape
    return ops._crop_window(dout.contiguous(), c, c, H - 2 * c, W - 2 * c)


@context_frame_bwd.register_fake
def _(dout, c):
    B, H, W, Cp = dout.shape
    return dout.new_empty((B, H - 2 * c, W - 2 * c, Cp))


context_frame.register_autograd(lambda ctx, dout, dnoisy: (torch.ops.jg355.context_frame_bwd(dout, ctx.c),) + (None,) * 9,
                                setup_context=lambda ctx, inputs, output: setattr(ctx, "c", inputs[2]))


# ---- dataaug_D_diffusion: noise on the backbone features of the projected discriminator ----------------------------------------------------
@op("jg355::d_diffusion", mutates_args=())
def d_diffusion(xs: List[T], a: T, b: T, t_epl: T, noise_std: float, key: Optional[T], ts: List[T], zs: List[T], call: int) -> List[T]:
    """ops.d_diffusion as a functional op: -> the n noised maps followed by the n int32 [B, C_l] tensors of the t used; ts / zs: one entry
    per map (injected) or empty (drawn in the kernel from `key`)"""
    xs = [x.contiguous() for x in xs]
    outs = [torch.empty_like(x) for x in xs]
    t_outs = [torch.empty((x.shape[0], x.shape[3]), device=x.device, dtype=torch.int32) for x in xs]
    ops._d_diffusion_launch(xs, a, b, t_epl, noise_std, key, call, list(ts) if len(ts) else None, list(zs) if len(zs) else None, outs, t_outs)
    return outs + t_outs


@d_diffusion.register_fake
def _(xs, a, b, t_epl, noise_std, key, ts, zs, call):
    return [torch.empty_like(x, memory_format=torch.contiguous_format) for x in xs] + [x.new_empty((x.shape[0], x.shape[3]), dtype=torch.int32) for x in xs]


@op("jg355::d_diffusion_bwd", mutates_args=())
def d_diffusion_bwd(dys: List[T], ts: List[T], a: T) -> List[T]:
    """dx_l = a[t_l[b, c]] * dy_l for every level in one launch"""
    return ops._d_diffusion_bwd_launch([d.contiguous() for d in dys], list(ts), a)


@d_diffusion_bwd.register_fake
def _(dys, ts, a):
    return [torch.empty_like(d, memory_format=torch.contiguous_format) for d in dys]


def _dd_setup(ctx, inputs, output):
    n = len(inputs[0])
    ctx.save_for_backward(inputs[1], *output[n:])
    ctx.n_inj = (len(inputs[6]), len(inputs[7]))      # the gradient of a list input is a list of its length


def _dd_backward(ctx, grads):
    a, *ts = ctx.saved_tensors
    n = len(ts)
    return torch.ops.jg355.d_diffusion_bwd(list(grads[:n]), ts, a), None, None, None, None, None, [None] * ctx.n_inj[0], [None] * ctx.n_inj[1], None


d_diffusion.register_autograd(_dd_backward, setup_context=_dd_setup)


@op("jg355::d_diffusion_update", mutates_args=("p", "Tn", "a", "b", "t_epl"))
def d_diffusion_update(p: T, Tn: T, a: T, b: T, t_epl: T, loss: T, num: float, den: float, u: Optional[T], key: Optional[T], call: int) -> None:
    """ops.d_diffusion_update: the device state (p, Tn = (T, n), the tables a / b, t_epl) is rewritten in place from the fp32 scalar `loss`"""
    ops._d_diffusion_update_launch(p, Tn, a, b, t_epl, loss, num, den, u, key, call)


@d_diffusion_update.register_fake
def _(p, Tn, a, b, t_epl, loss, num, den, u, key, call):
    return None


# ---- GAN objectives: (loss, d loss / d pred) -------------------------------------------------------------------------------------------------
@op("jg355::gan_loss", mutates_args=())
def gan_loss(pred: T, mode: int, target: float, scale: float) -> Tuple[T, T]:
    """GANLoss: mode 0 lsgan, 1 vanilla (BCE with logits), 2 wgangp, on an NHWC logit map whose channel 0 is valid"""
    return launch.gan_loss(pred.contiguous(), mode, target, scale)


@gan_loss.register_fake
def _(pred, mode, target, scale):
    return pred.new_empty((), dtype=torch.float32), torch.empty_like(pred)


@op("jg355::hinge_loss", mutates_args=())
def hinge_loss(pred: T, mode: int, scale: float) -> Tuple[T, T]:
    """GANLoss("projected"): mode 0 mean relu(1 - p), 1 mean relu(1 + p), 2 mean(-p) over every element"""
    return launch.hinge_loss(pred.contiguous(), mode, scale)


@hinge_loss.register_fake
def _(pred, mode, scale):
    return pred.new_empty((), dtype=torch.float32), torch.empty_like(pred)


def _loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _loss_backward_n(n):
    def bwd(ctx, g, gd):
        (dpred,) = ctx.saved_tensors
        return ((dpred.float() * g).to(dpred.dtype),) + (None,) * n
    return bwd


gan_loss.register_autograd(_loss_backward_n(3), setup_context=_loss_setup)
hinge_loss.register_autograd(_loss_backward_n(2), setup_context=_loss_setup)


# ---- spectral normalisation of a convolution weight -------------------------------------------------------------------------------------------
@op("jg355::spectral_weight", mutates_args=())
def spectral_weight(weight: T, u: T, v: T, training: bool) -> Tuple[T, T, T, T]:
    """torch.nn.utils.spectral_norm on W [Cout, R, S, Cin] fp32 (physical layout of the arena): one power iteration when `training`
    (returned as NEW u, v: the module copies them into its buffers), sigma = u . W v, W / sigma -> (W_sn, u', v', sigma)"""
    W = weight.contiguous()
    Cout = W.shape[0]
    K = W.numel() // Cout
    RS = W.shape[1] * W.shape[2] if W.dim() == 4 else 1
    un, vn = u.clone(), v.clone()
    sigma = torch.empty(1, device=W.device, dtype=torch.float32)
    if training:
        launch.spectral_power_iter(W, un, vn, sigma, Cout, RS, K // RS)
    else:
        sigma.copy_(torch.dot(un, W.reshape(Cout, K) @ vn).reshape(1))
    return W / sigma, un, vn, sigma


@spectral_weight.register_fake
def _(weight, u, v, training):
    return torch.empty_like(weight), torch.empty_like(u), torch.empty_like(v), weight.new_empty((1,))


@op("jg355::spectral_weight_bwd", mutates_args=())
def spectral_weight_bwd(dwsn: T, weight: T, u: T, v: T, sigma: T) -> T:
    """gradient w.r.t. W of W / sigma(W) with u, v constant: (dWsn - (u^T dWsn v) u v^T ... ) / sigma (jg_spectral_wgrad_fix)"""
    W = weight.contiguous()
    Cout = W.shape[0]
    K = W.numel() // Cout
    RS = W.shape[1] * W.shape[2] if W.dim() == 4 else 1
    g = torch.zeros_like(W)
    launch.spectral_wgrad_fix(dwsn.contiguous().float(), W, u, v, sigma, g, Cout, RS, K // RS)
    return g


@spectral_weight_bwd.register_fake
def _(dwsn, weight, u, v, sigma):
    return torch.empty_like(weight)


def _sw_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output[1], output[2], output[3])


def _sw_backward(ctx, dwsn, du, dv, ds):
    W, un, vn, sigma = ctx.saved_tensors
    return torch.ops.jg355.spectral_weight_bwd(dwsn, W, un, vn, sigma), None, None, None


spectral_weight.register_autograd(_sw_backward, setup_context=_sw_setup)


# ---- bilinear resize ---------------------------------------------------------------------------------------------------------------------
@op("jg355::bilinear2", mutates_args=())
def bilinear2(x: T, Ho: int, Wo: int, align_corners: bool) -> T:
    return launch.bilinear2_fwd(x.contiguous(), Ho, Wo, align_corners)


@bilinear2.register_fake
def _(x, Ho, Wo, align_corners):
    return x.new_empty((x.shape[0], Ho, Wo, x.shape[-1]))


@op("jg355::bilinear2_bwd", mutates_args=())
def bilinear2_bwd(dy: T, H: int, W: int, align_corners: bool) -> T:
    return launch.bilinear2_bwd(dy.contiguous(), H, W, align_corners)


@bilinear2_bwd.register_fake
def _(dy, H, W, align_corners):
    return dy.new_empty((dy.shape[0], H, W, dy.shape[-1]))


def _bil_setup(ctx, inputs, output):
    ctx.geo = (inputs[0].shape[1], inputs[0].shape[2], inputs[3])


bilinear2.register_autograd(lambda ctx, dy: (torch.ops.jg355.bilinear2_bwd(dy, *ctx.geo), None, None, None), setup_context=_bil_setup)


# ---- compositions used by the boundary mode (no new kernels: autograd chains the ops above) -------------------------------------------------
def conv_transpose2d_via_ops(x, m, output_padding=0):
    """nn.ConvTranspose2d on jg355 ops: zero insertion + stride-1 convolution with the flipped / transposed MASTER weight (differentiable views:
    autograd carries the weight gradient back through flip / permute)"""
    B, H, W, Cin_t = x.shape
    Ho = (H - 1) * m.stride - 2 * m.pad + m.R + output_padding
    Wo = (W - 1) * m.stride - 2 * m.pad + m.S + output_padding
    Hd, Wd = Ho + 2 * m.pad - m.R + 1, Wo + 2 * m.pad - m.S + 1
    xd = torch.ops.jg355.dilate2d(x, Hd, Wd, m.stride)
    # module weight [Cin_t, Cout_t, k, k] -> forward conv weight [Cout_t][R][S][Cin_t] = w[ci_t][co_t][R-1-r][S-1-s]
    wf = m.weight.permute(1, 2, 3, 0).flip(1, 2)
    return torch.ops.jg355.conv2d_nt(xd, wf, m.bias, None, m.R - 1 - m.pad, 1, 1.0, 0.0)
