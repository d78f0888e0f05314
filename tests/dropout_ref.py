"""Restatement of the mask and the three kernels of csrc/dropout.hip (jg_gn_apply_drop, jg_gn_bwd_reduce_drop, jg_gn_bwd_apply_drop) in numpy,
test helper.  Generator and uniform map: tests/d_aug_ref.py (Philox4x32-10, u = ((x >> 9) + 0.5) * 2^-23).
Counter layout: (pixel h * W + w,  sample b,  stream | (c // 4) << 16,  call): the 4 words are the uniforms of channels 4 (c // 4) .. + 3;
m[b, c, h, w] = (u < keep).  The kernels in float64 on the caller's 16-bit values, NHWC; ab [B, C, 2] / pqr [B, C, 3] float32 tables or None
(no normalisation: a = 1, b = 0; dx = du)."""
import numpy as np

from d_aug_ref import key_words, philox4x32_10, uniform_open

NONE, SILU, RELU, LRELU = "none", "silu", "relu", "lrelu"


def uniforms(key, B, C, H, W, stream, call):
    """float64 [B, C, H, W]: the uniforms the kernels draw for this key / stream / call"""
    q = (C + 3) // 4
    pix = np.arange(H * W, dtype=np.uint64)[None, None, :]
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    grp = np.arange(q, dtype=np.uint64)[None, :, None]
    r = philox4x32_10((pix, b, np.uint64(stream) | (grp << np.uint64(16)), np.uint64(call)), key_words(key))      # 4 x [B, q, HW]
    return np.stack([uniform_open(w) for w in r], axis=2).reshape(B, 4 * q, H, W)[:, :C]


def mask(u, keep):
    """bool [B, H, W, C] from uniforms [B, C, H, W]: the comparison in fp32, as in the kernel"""
    return (np.asarray(u, dtype=np.float32) < np.float32(keep)).transpose(0, 2, 3, 1)


def _act(v, act):
    if act == RELU:
        return np.maximum(v, 0.0)
    if act == LRELU:
        return np.where(v > 0, v, 0.2 * v)
    if act == SILU:
        return v / (1.0 + np.exp(-v))
    return v


def _act_grad(v, act):
    if act == RELU:
        return (v > 0).astype(np.float64)
    if act == LRELU:
        return np.where(v > 0, 1.0, 0.2)
    if act == SILU:
        s = 1.0 / (1.0 + np.exp(-v))
        return s * (1.0 + v * (1.0 - s))
    return np.ones_like(v)


def _pre(x, ab):
    x = np.asarray(x, dtype=np.float64)
    if ab is None:
        return x, x
    ab = np.asarray(ab, dtype=np.float64)
    return x, ab[:, None, None, :, 0] * x + ab[:, None, None, :, 1]


def apply_drop(x, ab, act, m, keep):
    """y = m * act(a x + b) / keep, float64 [B, H, W, C] BEFORE the rounding to the storage type"""
    _, v = _pre(x, ab)
    return np.where(m, _act(v, act) / np.float64(np.float32(keep)), 0.0)


def _du(x, dy, ab, act, m, keep):
    x, v = _pre(x, ab)
    return x, np.where(m, np.asarray(dy, dtype=np.float64) / np.float64(np.float32(keep)), 0.0) * _act_grad(v, act)


def bwd_reduce_drop(x, dy, ab, act, m, keep):
    """red float64 [B, C, 2] = (sum du, sum du x) over the pixels"""
    x, du = _du(x, dy, ab, act, m, keep)
    return np.stack((du.sum(axis=(1, 2)), (du * x).sum(axis=(1, 2))), axis=-1)


def bwd_apply_drop(x, dy, ab, pqr, act, m, keep):
    """dx = du P + x Q + R (pqr None: du), float64 [B, H, W, C] before rounding"""
    x, du = _du(x, dy, ab, act, m, keep)
    if pqr is None:
        return du
    pqr = np.asarray(pqr, dtype=np.float64)[:, None, None]
    return du * pqr[..., 0] + x * pqr[..., 1] + pqr[..., 2]
