"""torch.autograd wrappers of the SegFormer-generator kernels (csrc/segformer.hip): LayerNorm, depth-wise 3x3 + GELU, small-KV
attention, bilinear resize + concat, BatchNorm2d (on the GroupNorm kernels), attention composition, DropPath / Dropout2d scaling.
Activations are NHWC 16-bit ([B, N, C] token sequences are the same memory as [B, H, W, C] maps); parameters are fp32 arena views
whose `.grad` the backward kernels accumulate into."""
from __future__ import annotations

import os

import torch

from ._autograd import JGFunction
from . import _lib, launch
from ._lib import JG_ACT_NONE, JG_ACT_RELU, check
from .ops import _DT, _dt, _p, _require_cuda, _st, copy_channels

# depth-wise 3x3 weight gradient: per-block partials through a workspace + one summing launch (1) or atomics from every block (0)
DW_TWO_PHASE = os.environ.get("JG_DW_TWO_PHASE", "1") != "0"
# round 6: backward of resize_sum through jg_resize_sum_bwd (separable adjoint, two launches); 0 = activation gradient + one gather launch per term
RESIZE_BWD_SEPARABLE = os.environ.get("JG_RESIZE_BWD_SEPARABLE", "1") != "0"


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
class _LayerNormFn(JGFunction):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _require_cuda(x)
        x = x.contiguous()
        y, mr = launch.layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, mr, weight)
        ctx.gw, ctx.gb = weight.grad, bias.grad
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, mr, weight = ctx.saved_tensors
        want_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if want_p and (ctx.gw is None or ctx.gb is None):
            raise RuntimeError("LayerNorm parameters have no arena-backed .grad")
        dx = launch.layernorm_bwd(x, dy.contiguous(), weight, mr, ctx.gw if want_p else None, ctx.gb if want_p else None, ctx.needs_input_grad[0])
        return dx, None, None, None


def layer_norm(x, weight, bias, eps=1e-6):
    """nn.LayerNorm(C, eps) over the last dimension."""
    return _LayerNormFn.apply(x, weight, bias, float(eps))


class _LayerNormIdFn(JGFunction):
    """(x, LayerNorm(x)) for a pre-norm residual block `x + f(norm(x))`: the gradient that comes back through the identity output is added
    inside the LayerNorm-backward pass (jg_layernorm_bwd_add) instead of by autograd's separate accumulation launch."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _require_cuda(x)
        x = x.contiguous()
        y, mr = launch.layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, mr, weight)
        ctx.gw, ctx.gb = weight.grad, bias.grad
        return x.view_as(x), y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, did, dy):
        x, mr, weight = ctx.saved_tensors
        if dy is None:
            return did, None, None, None
        dy = dy.contiguous()
        C = x.shape[-1]
        R = x.numel() // C
        want_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if want_p and (ctx.gw is None or ctx.gb is None):
            raise RuntimeError("LayerNorm parameters have no arena-backed .grad")
        need_x = ctx.needs_input_grad[0]
        dx = torch.empty_like(x) if need_x else None
        res = did.contiguous() if (did is not None and need_x) else None
        check(_lib.lib().jg_layernorm_bwd_add(_dt(x), x.data_ptr(), dy.data_ptr(), weight.data_ptr(), mr.data_ptr(), _p(res), _p(dx),
                                              _p(ctx.gw) if want_p else None, _p(ctx.gb) if want_p else None, R, C, _st()), "jg_layernorm_bwd_add")
        return dx, None, None, None


class _AddLayerNormIdFn(JGFunction):
    """(y, LayerNorm(y)) with y = identity + branch * scale[image]: the DropPath-scaled residual sum and the LayerNorm behind it in one pass
    (jg_layernorm_fwd_add).  Backward: the LayerNorm backward with the identity output's gradient added in its pass, as _LayerNormIdFn; the
    result is the gradient of `identity` and, times the scale, of `branch`."""

    @staticmethod
    def forward(ctx, identity, branch, scale, weight, bias, eps):
        _require_cuda(identity, branch)
        identity, branch = identity.contiguous(), branch.contiguous()
        C = identity.shape[-1]
        R = identity.numel() // C
        B = identity.shape[0]
        y = torch.empty_like(identity)
        h = torch.empty_like(identity)
        mr = torch.empty((R, 2), device=identity.device, dtype=torch.float32)
        sc = None if scale is None else scale.contiguous().float()
        check(_lib.lib().jg_layernorm_fwd_add(_dt(identity), identity.data_ptr(), branch.data_ptr(), _p(sc), R // B, y.data_ptr(), weight.data_ptr(),
                                              bias.data_ptr(), h.data_ptr(), mr.data_ptr(), R, C, eps, _st()), "jg_layernorm_fwd_add")
        ctx.save_for_backward(y, mr, weight, sc)
        ctx.gw, ctx.gb = weight.grad, bias.grad
        return y, h

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, did, dh):
        y, mr, weight, sc = ctx.saved_tensors
        C = y.shape[-1]
        R = y.numel() // C
        B = y.shape[0]
        if dh is None:
            dtot = did
        else:
            dh = dh.contiguous()
            want_p = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
            if want_p and (ctx.gw is None or ctx.gb is None):
                raise RuntimeError("LayerNorm parameters have no arena-backed .grad")
            dtot = torch.empty_like(y)
            res = did.contiguous() if did is not None else None
            if sc is not None and ctx.needs_input_grad[1]:          # the scaled branch gradient from the same pass
                dbranch = torch.empty_like(y)
                check(_lib.lib().jg_layernorm_bwd_add2(_dt(y), y.data_ptr(), dh.data_ptr(), weight.data_ptr(), mr.data_ptr(), _p(res), dtot.data_ptr(),
                                                       sc.data_ptr(), R // B, dbranch.data_ptr(), _p(ctx.gw) if want_p else None,
                                                       _p(ctx.gb) if want_p else None, R, C, _st()), "jg_layernorm_bwd_add2")
                return (dtot if ctx.needs_input_grad[0] else None), dbranch, None, None, None, None
            check(_lib.lib().jg_layernorm_bwd_add(_dt(y), y.data_ptr(), dh.data_ptr(), weight.data_ptr(), mr.data_ptr(), _p(res), dtot.data_ptr(),
                                                  _p(ctx.gw) if want_p else None, _p(ctx.gb) if want_p else None, R, C, _st()), "jg_layernorm_bwd_add")
        dbranch = None
        if ctx.needs_input_grad[1] and dtot is not None:
            if sc is None:
                dbranch = dtot
            else:
                dbranch = torch.empty_like(dtot)
                check(_lib.lib().jg_scale(_dt(dtot), dtot.data_ptr(), sc.data_ptr(), None, dbranch.data_ptr(), B, R // B, C, 0, _st()), "jg_scale")
        return (dtot if ctx.needs_input_grad[0] else None), dbranch, None, None, None, None


def add_layer_norm_id(identity, branch, scale, weight, bias, eps=1e-6):
    """(y, nn.LayerNorm(C, eps)(y)) for y = identity + branch * scale[b] (scale None: plain sum): one launch for the residual sum and the norm"""
    return _AddLayerNormIdFn.apply(identity, branch, scale, weight, bias, float(eps))


def layer_norm_id(x, weight, bias, eps=1e-6):
    """(x, nn.LayerNorm(C, eps)(x)): use the FIRST output as the residual branch's identity so that its gradient is summed into the
    LayerNorm backward's pass."""
    return _LayerNormIdFn.apply(x, weight, bias, float(eps))


# ---- depth-wise 3x3 + GELU ---------------------------------------------------------------------------------------------------------
class _DWConvGeluFn(JGFunction):
    @staticmethod
    def forward(ctx, x, weight, bias, gelu, reflect=False):
        _require_cuda(x)
        x = x.contiguous()
        y, pre = launch.dwconv3x3_fwd(x, weight, bias, gelu, reflect)
        ctx.save_for_backward(x, pre, weight)
        ctx.gelu, ctx.gw, ctx.gb, ctx.reflect = gelu, weight.grad, None if bias is None else bias.grad, bool(reflect)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, pre, weight = ctx.saved_tensors
        want_w = ctx.needs_input_grad[1]
        if want_w and ctx.gw is None:
            raise RuntimeError("depth-wise conv weight has no arena-backed .grad")
        # weight / bias partials of the blocks go through a workspace and a second launch (DW_TWO_PHASE): straight atomics put a
        # 1024-deep same-address chain on every one of the C * 10 destinations
        dx = launch.dwconv3x3_bwd(x, pre, dy.contiguous(), weight, ctx.gw if want_w else None, ctx.gb if want_w else None, ctx.gelu, ctx.reflect,
                                  want_dx=ctx.needs_input_grad[0], two_phase=want_w and DW_TWO_PHASE)
        return dx, None, None, None, None


DW_REFLECT = os.environ.get("JG_DW_REFLECT", "1") != "0"


def dwconv3x3(x, weight, bias, gelu=True, reflect=False):
    """nn.Conv2d(C, C, 3, padding=1, groups=C) (+ nn.GELU()) on an NHWC map; weight is the arena view of [C, 1, 3, 3].
    reflect: padding_mode='reflect' -- one launch with mirrored taps (round 6), or (JG_DW_REFLECT=0 / under the torch.ops boundary, whose op
    schema knows zero padding only) reflect-pad -> zero-padded depth-wise kernel -> crop as in rounds 3-5."""
    from . import ops

    if reflect and (not DW_REFLECT or ops.TORCH_OPS_BOUNDARY or x.shape[1] < 4 or x.shape[2] < 4):
        B, H, W, C = x.shape
        return ops.crop2d(_DWConvGeluFn.apply(ops.reflect_pad2d(x, 1), weight, bias, bool(gelu), False), 1, 1, H, W)
    return _DWConvGeluFn.apply(x, weight, bias, bool(gelu), bool(reflect))


# ---- attention with a spatially reduced key / value set ---------------------------------------------------------------------------------
class _AttnSmallKVFn(JGFunction):
    """q: [B, Tq, C]; kv: [B, Tkv, 2C] packed (k | v) -- the output of ONE projection with the stacked (W_k; W_v) rows."""

    @staticmethod
    def forward(ctx, q, kv, heads):
        _require_cuda(q, kv)
        q, kv = q.contiguous(), kv.contiguous()
        C = q.shape[2]
        assert kv.shape[2] == 2 * C and C == heads * 32, (tuple(kv.shape), C, heads)
        o, lse = launch.attn_smallkv_fwd(q, kv, heads)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.heads = heads
        return o

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        return (*launch.attn_smallkv_bwd(q, kv, o, lse, do.contiguous(), ctx.heads), None)


def attention_smallkv(q, kv, heads):
    return _AttnSmallKVFn.apply(q, kv, heads)


# ---- bilinear resize of several maps into one channel-concatenated buffer -------------------------------------------------------------
class _ResizeConcatFn(JGFunction):
    @staticmethod
    def forward(ctx, Ho, Wo, *xs):
        _require_cuda(*xs)
        xs = [x.contiguous() for x in xs]
        B = xs[0].shape[0]
        Ct = sum(x.shape[-1] for x in xs)
        y = torch.empty((B, Ho, Wo, Ct), device=xs[0].device, dtype=xs[0].dtype)
        es, off = y.element_size(), 0
        for x in xs:
            _, H, W, C = x.shape
            if (H, W) == (Ho, Wo):
                copy_channels(x, 0, y, off, C)
            else:
                check(_lib.lib().jg_bilinear_fwd(_dt(x), x.data_ptr(), y.data_ptr() + off * es, B, H, W, C, Ho, Wo, Ct, _st()), "jg_bilinear_fwd")
            off += C
        ctx.shapes = [tuple(x.shape) for x in xs]
        ctx.Ho, ctx.Wo = Ho, Wo
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        dy = dy.contiguous()
        Ct = dy.shape[-1]
        es, off, outs = dy.element_size(), 0, []
        for i, (B, H, W, C) in enumerate(ctx.shapes):
            dx = None
            if ctx.needs_input_grad[2 + i]:
                dx = torch.empty((B, H, W, C), device=dy.device, dtype=dy.dtype)
                if (H, W) == (ctx.Ho, ctx.Wo):
                    copy_channels(dy, off, dx, 0, C)
                else:
                    check(_lib.lib().jg_bilinear_bwd(_dt(dy), dy.data_ptr() + off * es, dx.data_ptr(), B, H, W, C, ctx.Ho, ctx.Wo, Ct, _st()),
                          "jg_bilinear_bwd")
            outs.append(dx)
            off += C
        return (None, None) + tuple(outs)


def resize_concat(xs, Ho, Wo):
    """torch.cat([F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False) for x in xs], dim=1) on NHWC maps."""
    return _ResizeConcatFn.apply(Ho, Wo, *xs)


# ---- BatchNorm2d (+ ReLU) on the GroupNorm kernels ---------------------------------------------------------------------------------------
# Multi-GPU: the reference converts every BatchNorm to SyncBatchNorm before wrapping the network in DDP (models/base_model.py:725-737):
# the batch statistics -- and the two reductions of the backward -- are taken over the GLOBAL batch.  Here the per-(image, channel)
# sums of the local batch are reduced over the images, all-reduced (one [C, 2] message per BatchNorm and direction) and fed to the
# same coefficient kernels as "one image of world * B * HW pixels".  FORCE_SYNC_BN runs that path with a single rank (tests).
FORCE_SYNC_BN = False


def _sync_active(training):
    from . import parallel

    return training and (parallel.world_size() > 1 or FORCE_SYNC_BN)


def _all_reduce_sum(t):
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return dist.get_world_size()
    return 1


class _BatchNormFn(JGFunction):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, act):
        _require_cuda(x)
        L = _lib.lib()
        x = x.contiguous()
        B, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * C)
        dev, st, dt = x.device, _st(), _dt(x)
        ab = torch.empty((B, C, 2), device=dev, dtype=torch.float32)
        mr = torch.empty((C, 2), device=dev, dtype=torch.float32)
        sums = None
        sync = _sync_active(training)
        world = 1
        if training:
            sums = torch.empty((B, C, 2), device=dev, dtype=torch.float32)
            check(L.jg_gn_stats(dt, x.data_ptr(), sums.data_ptr(), B, HW, C, st), "jg_gn_stats")
        if sync:
            tot = sums.sum(0, keepdim=True).contiguous()         # [1, C, 2]: the local batch as one "image"
            world = _all_reduce_sum(tot)
            ab1 = torch.empty((1, C, 2), device=dev, dtype=torch.float32)
            check(L.jg_bn_coef(tot.data_ptr(), weight.data_ptr(), bias.data_ptr(), _p(running_mean), _p(running_var), ab1.data_ptr(), mr.data_ptr(), 1,
                               world * B * HW, C, eps, momentum, 1, st), "jg_bn_coef")
            ab.copy_(ab1.expand(B, C, 2))
        else:
            check(L.jg_bn_coef(_p(sums), weight.data_ptr(), bias.data_ptr(), _p(running_mean), _p(running_var), ab.data_ptr(), mr.data_ptr(), B, HW, C,
                               eps, momentum, int(training), st), "jg_bn_coef")
        y = torch.empty_like(x)
        check(L.jg_gn_apply(dt, x.data_ptr(), ab.data_ptr(), y.data_ptr(), B, HW, C, act, st), "jg_gn_apply")
        ctx.save_for_backward(x, ab, mr, weight)
        ctx.cfg = (training, act, weight.grad, bias.grad, sync, world)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, ab, mr, weight = ctx.saved_tensors
        training, act, gw, gb, sync, world = ctx.cfg
        L = _lib.lib()
        dy = dy.contiguous()
        B, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * C)
        dev, st, dt = x.device, _st(), _dt(x)
        red = torch.empty((B, C, 2), device=dev, dtype=torch.float32)
        pqr = torch.empty((B, C, 3), device=dev, dtype=torch.float32)
        want_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if want_p and (gw is None or gb is None):
            raise RuntimeError("BatchNorm parameters have no arena-backed .grad")
        check(L.jg_gn_bwd_reduce(dt, x.data_ptr(), dy.data_ptr(), ab.data_ptr(), red.data_ptr(), B, HW, C, act, st), "jg_gn_bwd_reduce")
        if sync:
            # dgamma / dbeta: the LOCAL reductions (the data-parallel gradient exchange averages them over the ranks like every other
            # parameter gradient); dx: the reductions of the GLOBAL batch
            if want_p:
                scratch = torch.empty((B, C, 3), device=dev, dtype=torch.float32)
                check(L.jg_bn_bwd_coef(red.data_ptr(), weight.data_ptr(), mr.data_ptr(), scratch.data_ptr(), _p(gw), _p(gb), B, HW, C, 1, st),
                      "jg_bn_bwd_coef")
            tot = red.sum(0, keepdim=True).contiguous()
            _all_reduce_sum(tot)
            pqr1 = torch.empty((1, C, 3), device=dev, dtype=torch.float32)
            check(L.jg_bn_bwd_coef(tot.data_ptr(), weight.data_ptr(), mr.data_ptr(), pqr1.data_ptr(), None, None, 1, world * B * HW, C, 1, st),
                  "jg_bn_bwd_coef")
            pqr.copy_(pqr1.expand(B, C, 3))
        else:
            check(L.jg_bn_bwd_coef(red.data_ptr(), weight.data_ptr(), mr.data_ptr(), pqr.data_ptr(), _p(gw) if want_p else None,
                                   _p(gb) if want_p else None, B, HW, C, int(training), st), "jg_bn_bwd_coef")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(L.jg_gn_bwd_apply(dt, x.data_ptr(), dy.data_ptr(), ab.data_ptr(), pqr.data_ptr(), dx.data_ptr(), B, HW, C, act, st), "jg_gn_bwd_apply")
        return (dx,) + (None,) * 8


def batch_norm(x, bn, act=JG_ACT_NONE):
    """nn.BatchNorm2d `bn` (affine, running statistics) followed by an optional fused activation; train mode uses the batch statistics
    (of the global batch when several ranks train: SyncBatchNorm semantics) and updates the running ones in place (momentum 0.1,
    unbiased variance), like the reference."""
    training = bn.training
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return _BatchNormFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, float(bn.momentum), float(bn.eps), act)


# ---- attention-mask composition ---------------------------------------------------------------------------------------------------------------
class _AttnComposeFn(JGFunction):
    @staticmethod
    def forward(ctx, img, logits, xin, na, ni, nc):
        _require_cuda(img, logits, xin)
        img, logits, xin = img.contiguous(), logits.contiguous(), xin.contiguous()
        B, S = img.shape[0], img.shape[1]
        f = S // logits.shape[1]
        out = torch.empty_like(xin)
        check(_lib.lib().jg_attn_compose_fwd(_dt(img), img.data_ptr(), logits.data_ptr(), xin.data_ptr(), out.data_ptr(), B, S, f, na, ni, nc,
                                             img.shape[-1], logits.shape[-1], xin.shape[-1], out.shape[-1], _st()), "jg_attn_compose_fwd")
        ctx.save_for_backward(img, logits, xin)
        ctx.cfg = (f, na, ni, nc)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        img, logits, xin = ctx.saved_tensors
        f, na, ni, nc = ctx.cfg
        dout = dout.contiguous()
        B, S = img.shape[0], img.shape[1]
        dimg, dlog = torch.empty_like(img), torch.empty_like(logits)
        dxin = torch.empty_like(xin) if ctx.needs_input_grad[2] else None
        check(_lib.lib().jg_attn_compose_bwd(_dt(img), img.data_ptr(), logits.data_ptr(), xin.data_ptr(), dout.data_ptr(), dimg.data_ptr(),
                                             dlog.data_ptr(), _p(dxin), B, S, f, na, ni, nc, img.shape[-1], logits.shape[-1], xin.shape[-1],
                                             dout.shape[-1], _st()), "jg_attn_compose_bwd")
        return dimg, dlog, dxin, None, None, None


def attention_compose(img, logits, xin, na, ni, nc):
    """BaseGenerator_attn.forward (attn_network.py:14-46): softmax over the `na` logits of each cell (nearest-upsampled), blend of the
    `ni` generated images (channels [nc i, nc i + nc) of img) and the input."""
    return _AttnComposeFn.apply(img, logits, xin, na, ni, nc)


# ---- DropPath / Dropout2d as given factors ----------------------------------------------------------------------------------------------------
class _ScaleFn(JGFunction):
    @staticmethod
    def forward(ctx, x, s, res, per_channel):
        _require_cuda(x)
        x = x.contiguous()
        B, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * C)
        y = torch.empty_like(x)
        r = None if res is None else res.contiguous()
        check(_lib.lib().jg_scale(_dt(x), x.data_ptr(), s.data_ptr(), _p(r), y.data_ptr(), B, HW, C, int(per_channel), _st()), "jg_scale")
        ctx.save_for_backward(s)
        ctx.per_channel, ctx.has_res = per_channel, res is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (s,) = ctx.saved_tensors
        dy = dy.contiguous()
        B, C = dy.shape[0], dy.shape[-1]
        HW = dy.numel() // (B * C)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(dy)
            check(_lib.lib().jg_scale(_dt(dy), dy.data_ptr(), s.data_ptr(), None, dx.data_ptr(), B, HW, C, int(ctx.per_channel), _st()), "jg_scale")
        return dx, None, (dy if ctx.has_res and ctx.needs_input_grad[2] else None), None


def scale_add(x, s, res=None, per_channel=False):
    """x * s (+ res) with s of shape [B] (DropPath: floor(keep + U) / keep) or [B, C] (Dropout2d: (U >= p) / (1 - p))."""
    return _ScaleFn.apply(x, s.contiguous().float(), res, per_channel)


# ---- linear on a row slice of a stacked projection (nn.MultiheadAttention's packed in_proj) -----------------------------------------------
class _SlicedLinearFn(JGFunction):
    """y = x W[row0 : row0 + n]^T + b[row0 : row0 + n] for a ConvMeta that holds the stacked [rows, Cin] projection."""

    @staticmethod
    def forward(ctx, x, weight, bias, meta, row0, n):
        from .ops import conv_nt

        _require_cuda(x)
        x = x.contiguous()
        B, N, Cin = x.shape
        m = meta
        y = torch.empty((B, N, n), device=x.device, dtype=x.dtype)
        conv_nt(x, m.w16, y, B=B, H=1, W=N, Cin=Cin, Cout=n, R=1, S=1, pad=0, stride=1, Ho=1, Wo=N, ldx=Cin, ldw=Cin, ldy=n,
                bias=None if m.bias is None else m.bias[row0:row0 + n], w_off=row0 * Cin)
        ctx.save_for_backward(x)
        ctx.cfg = (m, row0, n)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from .ops import _wgrad_splitk, conv_nt, wgrad_tn

        (x,) = ctx.saved_tensors
        m, row0, n = ctx.cfg
        dy = dy.contiguous()
        B, N, Cin = x.shape
        rows = m.Cout
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            conv_nt(dy, m.w16T, dx, B=B, H=1, W=N, Cin=n, Cout=Cin, R=1, S=1, pad=0, stride=1, Ho=1, Wo=N, ldx=n, ldw=rows, ldy=Cin, w_off=row0)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            wg = m.weight.grad
            if wg is None:
                raise RuntimeError("projection weight has no arena-backed .grad")
            dbias = m.bias.grad[row0:row0 + n] if (m.bias is not None and ctx.needs_input_grad[2]) else None
            tiles = ((n + 127) // 128) * ((Cin + 127) // 128)
            wgrad_tn(dy, x, wg, B=B, H=1, W=N, Cin=Cin, Cout=n, R=1, S=1, pad=0, stride=1, Ho=1, Wo=N, lddy=n, ldx=Cin, lddw=Cin, dbias=dbias,
                     Cin_out=Cin, Cout_out=n, splitk=_wgrad_splitk(tiles, B * N), dw_off=row0 * Cin)
        return dx, None, None, None, None, None


class _SlicedInConvFn(JGFunction):
    """y = x W[:, col0 : col0 + k]^T (+ b) for a 1x1 ConvMeta whose weight is [Cout, Cin_total]: one term of a convolution over a channel
    concatenation, taken on the term's own (smaller) map.  Weight and bias gradients go into the arena rows / columns of the slice."""

    @staticmethod
    def forward(ctx, x, weight, bias, meta, col0, with_bias):
        from .ops import conv_nt

        _require_cuda(x)
        x = x.contiguous()
        B, H, W, k = x.shape
        m = meta
        y = torch.empty((B, H, W, m.Cout), device=x.device, dtype=x.dtype)
        conv_nt(x, m.w16, y, B=B, H=H, W=W, Cin=k, Cout=m.Cout, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldx=k, ldw=m.Cin, ldy=m.Cout,
                bias=(m.bias_pad if m.bias_pad is not None else m.bias) if with_bias else None, w_off=col0)
        ctx.save_for_backward(x)
        ctx.cfg = (m, col0, with_bias)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from .ops import _wgrad_splitk, conv_nt, wgrad_tn

        (x,) = ctx.saved_tensors
        m, col0, with_bias = ctx.cfg
        dy = dy.contiguous()
        B, H, W, k = x.shape
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            conv_nt(dy, m.w16T, dx, B=B, H=H, W=W, Cin=m.Cout, Cout=k, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldx=m.Cout, ldw=m.Cout, ldy=k,
                    w_off=col0 * m.Cout)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            wg = m.weight.grad
            if wg is None:
                raise RuntimeError("convolution weight has no arena-backed .grad")
            dbias = m.bias.grad if (with_bias and m.bias is not None and ctx.needs_input_grad[2]) else None
            tiles = ((m.Cout + 127) // 128) * ((k + 127) // 128)
            wgrad_tn(dy, x, wg, B=B, H=H, W=W, Cin=k, Cout=m.Cout, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, lddy=m.Cout, ldx=k, lddw=m.Cin_real,
                     dbias=dbias, Cin_out=k, Cout_out=m.Cout_real, splitk=_wgrad_splitk(tiles, B * H * W), dw_off=col0)
        return dx, None, None, None, None, None


def sliced_in_conv(x, meta, col0, with_bias=False):
    """1x1 convolution of x [B,H,W,k] with input-channel slice [col0, col0 + k) of `meta`'s weight."""
    if meta.R != 1 or meta.S != 1 or meta.Cin != meta.Cin_real or col0 % 8 or x.shape[-1] % 8:
        raise ValueError("sliced_in_conv: 1x1 convolution with unpadded input channels, slices on multiples of 8")
    return _SlicedInConvFn.apply(x, meta.weight, meta.bias, meta, col0, with_bias)


class _ResizeSumFn(JGFunction):
    """act(x0 + sum_i bilinear(x_i -> size of x0)) [* chscale[b, c]] (jg_resize_sum); backward: jg_resize_sum_bwd (separable adjoint of all
    terms, two launches) or act' once + the gather adjoint per resized term."""

    @staticmethod
    def forward(ctx, act, chscale, x0, *xs):
        _require_cuda(x0, *xs)
        x0 = x0.contiguous()
        xs = [x.contiguous() for x in xs]
        if len(xs) > 3:
            raise ValueError("resize_sum: at most three resized terms")
        B, Ho, Wo, C = x0.shape
        y = torch.empty_like(x0)
        a = []
        for i in range(3):
            a += [xs[i].data_ptr(), xs[i].shape[1], xs[i].shape[2]] if i < len(xs) else [None, 1, 1]
        if chscale is not None:
            chscale = chscale.contiguous().float()
            assert tuple(chscale.shape) == (B, C), tuple(chscale.shape)
        check(_lib.lib().jg_resize_sum(_dt(x0), x0.data_ptr(), *a, y.data_ptr(), B, Ho, Wo, C, act, _p(chscale), _st()), "jg_resize_sum")
        ctx.save_for_backward(y, chscale)
        ctx.cfg = (act, [tuple(x.shape) for x in xs])
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, chscale = ctx.saved_tensors
        act, shapes = ctx.cfg
        dy = dy.contiguous()
        B, Ho, Wo, C = y.shape
        need0, needs = ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        if (RESIZE_BWD_SEPARABLE and Wo * C * dy.element_size() <= 65536 and any(needs)) or chscale is not None:
            # round 6 (jg_resize_sum_bwd): activation gradient + the bilinear adjoints of all terms in two launches, dy read once
            if Wo * C * dy.element_size() > 65536:
                raise NotImplementedError("resize_sum with a channel scale: rows of more than 64 KB")
            plain = act == JG_ACT_NONE and chscale is None       # g is dy itself
            g = torch.empty_like(y) if (need0 and not plain) else None
            outs, a = [], []
            for i in range(3):
                dx = None
                if i < len(shapes) and needs[i]:
                    dx = torch.empty((B, shapes[i][1], shapes[i][2], C), device=dy.device, dtype=dy.dtype)
                if i < len(shapes):
                    outs.append(dx)
                a += [_p(dx), shapes[i][1] if dx is not None else 1, shapes[i][2] if dx is not None else 1]
            nws = int(_lib.lib().jg_resize_sum_bwd_ws_floats(B, Ho, C, *(a[3 * i + 2] if a[3 * i] else 0 for i in range(3))))
            ws = torch.empty(max(nws, 1), device=dy.device, dtype=torch.float32)
            check(_lib.lib().jg_resize_sum_bwd(_dt(y), y.data_ptr(), dy.data_ptr(), _p(g), *a, ws.data_ptr(), B, Ho, Wo, C, act, _p(chscale), _st()),
                  "jg_resize_sum_bwd")
            return (None, None, (dy if plain else g) if need0 else None) + tuple(outs)
        g = dy
        if act != JG_ACT_NONE:
            g = launch.act_bwd(y, dy, act)
        outs = []
        for i, (_, H, W, _c) in enumerate(shapes):
            dx = None
            if needs[i]:
                dx = torch.empty((B, H, W, C), device=dy.device, dtype=dy.dtype)
                check(_lib.lib().jg_bilinear_bwd(_dt(g), g.data_ptr(), dx.data_ptr(), B, H, W, C, Ho, Wo, C, _st()), "jg_bilinear_bwd")
            outs.append(dx)
        return (None, None, g if need0 else None) + tuple(outs)


def resize_sum(x0, xs, act=JG_ACT_NONE, chscale=None):
    """chscale: optional fp32 [B, C] factors >= 0 applied behind the activation (Dropout2d of the SegFormer head)."""
    return _ResizeSumFn.apply(act, chscale, x0, *xs)


def sliced_linear(x, meta, row0, n):
    return _SlicedLinearFn.apply(x, meta.weight, meta.bias, meta, row0, n)
