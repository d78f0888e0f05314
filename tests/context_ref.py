"""Restatement of data_online_context_pixels in plain torch (float64 / integer indexing), test helper: the two kernels of csrc/context.hip
(jg_context_split, jg_context_frame), the noise of the framed image and the adjoint of the frame.

Written from the reference's models/base_model.py:389-431 (set_input: the loader's image is real_*_with_context, its centre [c:-c, c:-c] is
real_*), :609-636 (compute_fake_with_context: zero-pad the translated crop by c, add mask_context * real_A_with_context),
models/base_gan_model.py:186-215 (mask_context: ones with a zero window) and models/cut_model.py:668-682 (util.gaussian on the framed images).
For finite inputs pad(inner) + mask * ctx is a select -- 0 + 1 * ctx on the frame, inner + 0 * ctx inside -- which is what `frame` writes;
`frame_literal` evaluates the reference's expression as it stands, for the comparison of the two.

Layouts: images are NHWC [B, H, W, Cpad] with C valid channels as the kernels see them (padding channels of every output: 0); z is the
reference's NCHW [B, C, H, W]."""
import torch
import torch.nn.functional as F

import d_aug_ref


def split(x_nchw, c, dtype, cpad=8):
    """x fp32 [B, C, S + 2c, S + 2c] -> (ctx [B, S + 2c, S + 2c, cpad], crop [B, S, S, cpad] = ctx[:, c:-c, c:-c]) in the 16-bit `dtype`:
    one rounding of every fp32 value, zeros in the padding channels"""
    B, C, H, W = x_nchw.shape
    ctx = torch.zeros(B, H, W, cpad, dtype=dtype)
    ctx[..., :C] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    return ctx, ctx[:, c:H - c, c:W - c].clone()


def frame(inner, ctx, c, C):
    """out = inner inside the window, ctx on the frame (values copied, nothing computed); padding channels 0"""
    H, W = ctx.shape[1:3]
    out = torch.zeros_like(ctx)
    out[..., :C] = ctx[..., :C]
    out[:, c:H - c, c:W - c, :C] = inner[..., :C]
    return out


def mask_context(B, C, H, W, c, dtype=torch.float64):
    """ones [B, C, H, W] with a zero window [c:-c, c:-c]"""
    m = torch.ones(B, C, H, W, dtype=dtype)
    m[:, :, c:H - c, c:W - c] = 0
    return m


def frame_literal(inner_nchw, ctx_nchw, c):
    """the reference's expression on NCHW tensors: F.pad(inner, (c, c, c, c)) + mask_context * ctx"""
    return F.pad(inner_nchw, (c, c, c, c)) + mask_context(*ctx_nchw.shape, c, dtype=ctx_nchw.dtype) * ctx_nchw


def noisy(out, C, sigma, z_nchw):
    """float64 [B, H, W, Cpad]: out + fp32(sigma) * z over the whole framed image BEFORE the rounding to the storage type; padding channels 0"""
    res = torch.zeros(out.shape, dtype=torch.float64)
    res[..., :C] = out[..., :C].double() + float(torch.tensor(sigma, dtype=torch.float32)) * z_nchw.double().permute(0, 2, 3, 1)
    return res


def drawn_z(key, B, C, H, W, call=0, stream=d_aug_ref.NOISE_STREAM):
    """float64 [B, C, H, W]: what the kernel draws for the framed image -- jg_d_aug's convention on the (H, W) = (S + 2c)^2 grid"""
    return torch.from_numpy(d_aug_ref.normals(key, B, C, H, W, stream=stream, call=call))


def frame_grad(dout, c):
    """the adjoint of `frame` with respect to inner: the window of the incoming gradient (the frame contributes nothing)"""
    H, W = dout.shape[1:3]
    return dout[:, c:H - c, c:W - c].clone()
