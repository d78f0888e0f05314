"""Sub-pixel input gradient of conv3x3(Upsample_nearest(h)) (jg_conv_args.y_mode 2, csrc/conv_halo.hip PHASE == 2) and the fold launch that
writes its weights (jg_subpixel_fold_pair): against fp32 torch autograd, against the pooled-store form it replaces (y_mode 1), on packed
operands and on channel slices of wider buffers, and the refusal outside its shape limits."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}     # the project's values (tests/test_gpu_0_ops.py)
ALPHA = 0.5

# (B, H_up, W_up, C_in, C_out) of the FORWARD layer: the gradient is [B, H_up / 2, W_up / 2, C_in] from dO [B, H_up, W_up, C_out]
CASES = [
    (2, 32, 32, 64, 64),       # one low-resolution tile per image: every border; 64-wide tile
    (1, 32, 64, 128, 128),     # horizontal tile neighbours, two chunks; 128-wide tile
    (1, 64, 32, 64, 192),      # vertical neighbours, C_out not a multiple of 128 (three chunks of dO)
    (2, 32, 32, 256, 192),     # two 128-wide channel tiles (four 64-channel ones under cfg 2), three chunks of dO
]
# JG_SUBPIXEL_DGRAD_CFG per case: the automatic choice, plus the other instantiations a 128-multiple channel count can run on (1: the
# double-buffered 8-wave tile, 2: the 64-wide tile)
CFGS = [(c, cfg) for c in CASES for cfg in ((0, 1, 2) if c[3] % 128 == 0 else (0,))]
NAMES = {128: {0: "conv3x3_halo_kernel<subpixel dgrad,128-wide,4 waves>", 1: "conv3x3_halo_kernel<subpixel dgrad,128-wide,8 waves>",
               2: "conv3x3_halo_kernel<subpixel dgrad,64-wide>"},
         64: {0: "conv3x3_halo_kernel<subpixel dgrad,64-wide>"}}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


_REF = {}


def problem(case, dtype):
    """(w32 [Co][3][3][Ci] fp32, dO [B, H, W, Co] dtype, fp32 autograd gradient w.r.t. the low-resolution input [B, H/2, W/2, Ci]) on the CPU,
    computed once per (case, dtype) and never written to"""
    key = (case, dtype)
    if key not in _REF:
        B, H, W, Ci, Co = case
        w32 = rnd((Co, Ci, 3, 3), torch.float32, 71, 1.0 / math.sqrt(Ci * 9))
        dO = rnd((B, Co, H, W), dtype, 72)
        x = torch.zeros((B, Ci, H // 2, W // 2), dtype=torch.float32, requires_grad=True)
        F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w32, None, 1, 1).backward(dO.float())
        _REF[key] = (w32.permute(0, 2, 3, 1).contiguous(), dO.permute(0, 2, 3, 1).contiguous(), ALPHA * x.grad.permute(0, 2, 3, 1).contiguous())
    return _REF[key]


def folds(w32d, dtype):
    from joligen_amd import _lib
    from joligen_amd.modules import unet_exec as ue

    Co, _, _, Ci = w32d.shape
    code = _lib.JG_F16 if dtype == torch.float16 else _lib.JG_BF16
    wf = torch.empty((4, Co, 2, 2, Ci), device=w32d.device, dtype=dtype)
    wfT = torch.empty((4, Ci, 2, 2, Co), device=w32d.device, dtype=dtype)
    _lib.check(_lib.lib().jg_subpixel_fold_pair(code, w32d.data_ptr(), wf.data_ptr(), wfT.data_ptr(), Co, Ci, ue._st()), "jg_subpixel_fold_pair")
    return wf, wfT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_fold_pair_against_definition(case, dtype):
    """`out` is bit-identical to jg_subpixel_fold, `outT` is its transpose, and both are the fp32 tap sums rounded once"""
    from joligen_amd import _lib
    from joligen_amd.modules import unet_exec as ue

    w32, _, _ = problem(case, dtype)
    w32d = w32.to(dev())
    Co, _, _, Ci = w32d.shape
    wf, wfT = folds(w32d, dtype)
    wf1 = torch.empty_like(wf)
    _lib.check(_lib.lib().jg_subpixel_fold(_lib.JG_F16 if dtype == torch.float16 else _lib.JG_BF16, w32d.data_ptr(), wf1.data_ptr(), Co, Ci,
                                           ue._st()), "jg_subpixel_fold")
    torch.cuda.synchronize()
    assert torch.equal(wf, wf1)
    assert torch.equal(wfT, wf.permute(0, 4, 2, 3, 1))
    wr = w32.double()
    sets = {(0, 0): [0], (0, 1): [1, 2], (1, 0): [0, 1], (1, 1): [2]}
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    taps = [(r, s) for r in sets[(py, a)] for s in sets[(px, b)]]
                    ref_t = sum(wr[:, r, s, :] for r, s in taps)          # [Co][Ci]
                    assert relerr(wfT[py * 2 + px, :, a, b, :].double(), ref_t.t()) < TOL[dtype]
                    acc = torch.zeros((Co, Ci), dtype=torch.float32)      # the kernel's fp32 sum, in its order, rounded ONCE
                    for r, s in taps:
                        acc = acc + w32[:, r, s, :]
                    assert torch.equal(wfT[py * 2 + px, :, a, b, :].cpu(), acc.to(dtype).t())


@pytest.mark.parametrize("sliced", [False, True], ids=["packed", "slices"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,cfg", CFGS)
def test_subpixel_dgrad(case, cfg, dtype, sliced):
    """y_mode 2 against fp32 autograd of conv2d(interpolate(x, 2, "nearest"), w32, padding=1) and against the y_mode 1 launch on the 16-bit
    working weights.  `slices`: dO is a channel slice of a wider buffer (ldx > C) and the result goes into a channel slice of a NaN-prefilled
    buffer: nothing outside the slice is written, everything inside is finite."""
    from joligen_amd import _lib, ops

    B, H, W, Ci, Co = case
    d = dev()
    w32, dO, ref = problem(case, dtype)
    w32d = w32.to(d)
    _, wfT = folds(w32d, dtype)
    w16T = w32d.to(dtype).flip(1, 2).permute(3, 1, 2, 0).contiguous()        # [Ci][3][3][Co]: the flipped / transposed working weights
    if sliced:
        dbuf = torch.full((B, H, W, Co + 72), float("nan"), device=d, dtype=dtype)
        dOd = dbuf[..., 40:40 + Co]
        dOd.copy_(dO)
    else:
        dOd = dO.to(d)
    outs = []
    prev = _lib.set_tuning("JG_SUBPIXEL_DGRAD_CFG", cfg)
    try:
        for mode, w, ldw in ((2, wfT, 4 * Co), (1, w16T, 9 * Co)):
            ybuf = torch.full((B, H // 2, W // 2, Ci + (24 if sliced else 0)), float("nan"), device=d, dtype=dtype)
            y = ybuf[..., 8:8 + Ci] if sliced else ybuf
            ops.conv_nt(dOd, w, y, B=B, H=H, W=W, Cin=Co, Cout=Ci, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=dOd.stride(-2), ldw=ldw,
                        ldy=y.stride(-2), alpha=ALPHA, y_mode=mode)
            if mode == 2:
                assert _lib.lib().jg_last_kernel().decode() == NAMES[128 if Ci % 128 == 0 else 64][cfg]
            outs.append((y, ybuf))
    finally:
        _lib.set_tuning("JG_SUBPIXEL_DGRAD_CFG", prev)
    torch.cuda.synchronize()
    (y2, buf2), (y1, _) = outs
    assert torch.isfinite(y2.float()).all()
    if sliced:
        assert torch.isnan(buf2[..., :8]).all() and torch.isnan(buf2[..., 8 + Ci:]).all()
        assert torch.isnan(dbuf[..., :40]).all() and torch.isnan(dbuf[..., 40 + Co:]).all() and torch.equal(dOd.cpu(), dO)
    e_ref, e_old = relerr(y2, ref), relerr(y2.float(), y1.float())
    print(f"subpixel dgrad {case} cfg {cfg} {dtype} sliced={sliced}: vs fp32 {e_ref:.3e}, vs y_mode 1 {e_old:.3e}")
    assert e_ref < TOL[dtype]
    assert e_old < 2 * TOL[dtype]


@pytest.mark.parametrize("shape", [(1, 48, 32, 64, 64), (1, 32, 48, 64, 64), (1, 32, 32, 96, 64), (1, 32, 32, 64, 96)])
def test_subpixel_dgrad_refuses_shapes_outside_its_limits(shape):
    """upsampled size not a multiple of 32, channel counts not multiples of 64: JG_ERR_UNSUPPORTED, nothing launched"""
    from joligen_amd import ops

    B, H, W, Ci, Co = shape
    d = dev()
    dO = torch.zeros((B, H, W, Co), device=d, dtype=torch.bfloat16)
    wfT = torch.zeros((4, Ci, 2, 2, Co), device=d, dtype=torch.bfloat16)
    y = torch.full((B, H // 2, W // 2, Ci), float("nan"), device=d, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="jg_conv2d_nt"):
        ops.conv_nt(dO, wfT, y, B=B, H=H, W=W, Cin=Co, Cout=Ci, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=Co, ldw=4 * Co, ldy=Ci, y_mode=2)
    with pytest.raises(RuntimeError, match="jg_conv2d_nt"):      # no bias / residual / statistics in this mode
        ops.conv_nt(dO, wfT, y, B=B, H=H, W=W, Cin=Co, Cout=Ci, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=Co, ldw=4 * Co, ldy=Ci, y_mode=2,
                    bias=torch.zeros(Ci, device=d))
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
