"""Host side of the super-resolution conditioning of the palette model (reference models/palette_model.py:120-130, 546-548):

    cond_image = Resize((S, S))(Resize((S_lo, S_lo))(gt_image)),   S_lo = int(S / alg_diffusion_super_resolution_scale)

`torchvision.transforms.Resize` on a tensor is `F.interpolate(mode="bilinear", align_corners=False, antialias=True)`: a separable
triangle filter whose support grows with the down-scaling ratio.  As with `pil_bicubic_tables` (data_device.py) the caller computes
the per-axis tap tables and the kernel (`jg_lowres_roundtrip_f32`, csrc/resize_aa.hip) only applies them.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

MAX_TAPS = _lib.JG_LOWRES_MAX_TAPS      # taps per output position the kernel accepts for the down pass


def aa_bilinear_tables(n_in, n_out):
    """tap tables of ATen's anti-aliased linear filter for one axis (UpSampleKernel.cpp `_compute_indices_min_size_weights_aa`,
    align_corners=False): xmin int32 [n_out] = first source index, size int32 [n_out] = tap count, w float32 [n_out, K] = normalised
    taps (unused ones 0), K = 2 ceil(support) + 1.  All arithmetic in float32, as ATen does it for a float32 image: with float64 the
    taps of non-integer ratios drift by 2e-6."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"aa_bilinear_tables({n_in}, {n_out})")
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    support = scale if scale >= 1 else f32(1)
    inv = f32(1) / scale if scale >= 1 else f32(1)
    K = 2 * int(math.ceil(float(support))) + 1
    half = f32(0.5)
    c = scale * (np.arange(n_out, dtype=f32) + half)
    lo = np.maximum((c - support + half).astype(np.int64), 0)
    hi = np.minimum((c + support + half).astype(np.int64), n_in)
    size = hi - lo
    j = np.arange(K, dtype=np.int64)[None, :]
    w = np.maximum(f32(0), f32(1) - np.abs((j + lo[:, None]).astype(f32) - c[:, None] + half) * inv).astype(f32)
    w = np.where(j < size[:, None], w, f32(0))
    tot = np.zeros(n_out, dtype=f32)
    for k in range(K):          # fp32 running sum in tap order
        tot = tot + w[:, k]
    w = np.where(tot[:, None] != 0, w / np.where(tot == 0, f32(1), tot)[:, None], w).astype(f32)
    return torch.from_numpy(lo.astype(np.int32)), torch.from_numpy(size.astype(np.int32)), torch.from_numpy(w)


def apply_tables(x, tables, dim):
    """reference application of one axis' tables with torch ops on any device (tests, tools): y[i] = sum_k w[i, k] x[xmin[i] + k]"""
    xmin, size, w = tables
    K = w.shape[1]
    idx = (xmin.long()[:, None] + torch.arange(K)[None, :]).clamp_(max=x.shape[dim] - 1).to(x.device)       # unused taps weigh 0
    xm = x.movedim(dim, -1)
    y = torch.zeros(xm.shape[:-1] + (w.shape[0],), dtype=x.dtype, device=x.device)
    for k in range(K):
        y = y + xm[..., idx[:, k]] * w[:, k].to(x.device)
    return y.movedim(-1, dim)


def low_size(size, scale):
    """the reference's low-resolution edge (palette_model.py:122-124)"""
    return int(size / scale)


_CACHE = {}


def device_tables(n_in, n_out, device, taps=None):
    """`aa_bilinear_tables` on `device`, computed once per (n_in, n_out, device); `taps`: row length of w (zero-padded: the kernel reads
    both down passes with one K)"""
    device = torch.device(device)
    key = (int(n_in), int(n_out), device, taps)
    if key not in _CACHE:
        xmin, size, w = aa_bilinear_tables(n_in, n_out)
        if taps is not None and taps != w.shape[1]:
            if taps < w.shape[1]:
                raise ValueError(f"{taps} taps cannot hold the {w.shape[1]} of {n_in} -> {n_out}")
            w = torch.nn.functional.pad(w, (0, taps - w.shape[1]))
        _CACHE[key] = tuple(t.to(device).contiguous() for t in (xmin, size, w))
    return _CACHE[key]


def aa_taps(n_in, n_out):
    """K of `aa_bilinear_tables(n_in, n_out)`"""
    scale = np.float32(n_in) / np.float32(n_out)
    return 2 * int(math.ceil(float(max(scale, np.float32(1))))) + 1


def band_rows(H, W, Hlo, Wlo):
    """output rows per workgroup of jg_lowres_roundtrip_f32 for the shape -- the library's own support probe (no launch, no GPU).
    NotImplementedError where the kernel does not take the shape: callers probe at construction, not mid-step."""
    kd = max(aa_taps(H, Hlo), aa_taps(W, Wlo))
    rc = _lib.lib().jg_lowres_roundtrip_band(int(H), int(W), int(Hlo), int(Wlo), kd)
    if rc == _lib.JG_ERR_UNSUPPORTED:
        raise NotImplementedError(f"jg_lowres_roundtrip_f32 does not take {H}x{W} -> {Hlo}x{Wlo} ({kd} taps): the input rows of one band of "
                                  "output rows must fit LDS, 65 taps at most")
    if rc <= 0:
        raise ValueError(f"low-resolution round trip {H}x{W} -> {Hlo}x{Wlo}: bad shape")
    return rc
