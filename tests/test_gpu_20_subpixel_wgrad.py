"""Sub-pixel weight gradient of conv3x3(Upsample_nearest(h)) (jg_wgrad_args.x_mode 2, csrc/wgrad_halo.hip wgrad3x3_subpixel_kernel): against
the x_mode 1 launch it replaces (same 16-bit products, another fp32 summation order), against fp32 torch autograd, as an accumulation,
on channel slices of canaried buffers, in deterministic mode, its refusals, and through the UNet executor."""
import math

import pytest
import torch
import torch.nn.functional as F

import strided_util as SU

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}     # the project's values (tests/test_gpu_0_ops.py)
SAME_PRODUCTS = 3e-6      # "same products, other summation order" on an fp32 gradient (test_wgrad_sliding_window_modes_match_the_round5_tile)
KERNEL = "wgrad3x3_halo_kernel<subpixel,4 rows,64 co>"

# (B, H_up, W_up, C_in, C_out): x is [B, H_up / 2, W_up / 2, C_in], dO is [B, H_up, W_up, C_out]
CASES = [
    (2, 32, 32, 64, 64),       # one 16-wide low-resolution tile column per image: every tile touches a border; two images
    (1, 32, 64, 128, 128),     # horizontal tile neighbours; two input chunks
    (1, 64, 32, 64, 192),      # vertical neighbours; C_out not a multiple of 128
    # three input chunks and a ragged split-K.  At B = 3 the launch has 12 tiles for 3 x 12 workgroups of one tile each: nothing is ragged
    # below 256 workgroups.  B = 43 is the smallest batch at which pick_split leaves a shorter last slice (172 tiles, 58 slices of 3: the last
    # one walks a single tile); test_the_ragged_case_is_ragged checks that on the host
    (43, 32, 32, 192, 64),
]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


relerr = SU.relerr


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def pick_split(npairs, ntiles, ovh=14, slots=256):
    """csrc/wgrad_params.h jg_wgrad_pick_split with wgrad_halo.hip launch_subpixel's arguments: (tiles per slice, slices)"""
    best, bper, bsk = -1, ntiles, 1
    for sk in range(1, min(ntiles, 2048 // npairs + 1) + 1):
        per = (ntiles + sk - 1) // sk
        ske = (ntiles + per - 1) // per
        cost = (per + ovh) * ((npairs * ske + slots - 1) // slots)
        if best < 0 or cost < best:
            best, bper, bsk = cost, per, ske
    return bper, bsk


_REF = {}


def problem(case, dtype):
    """(x [B, H/2, W/2, Ci] dtype, dO [B, H, W, Co] dtype, fp32 autograd dw [Co][3][3][Ci], db [Co]) on the CPU, computed once per
    (case, dtype) and never written to"""
    key = (case, dtype)
    if key not in _REF:
        B, H, W, Ci, Co = case
        x = rnd((B, Ci, H // 2, W // 2), dtype, 81)
        dO = rnd((B, Co, H, W), dtype, 82)
        w = torch.zeros((Co, Ci, 3, 3), requires_grad=True)
        b = torch.zeros(Co, requires_grad=True)
        F.conv2d(F.interpolate(x.float(), scale_factor=2, mode="nearest"), w, b, padding=1).backward(dO.float())
        _REF[key] = (x.permute(0, 2, 3, 1).contiguous(), dO.permute(0, 2, 3, 1).contiguous(), w.grad.permute(0, 2, 3, 1).contiguous(),
                     b.grad.clone())
    return _REF[key]


def launch(dO, x, dw, db, case, x_mode, alpha=1.0, dbias_scale=1.0, cin_out=0, pad_mode=0):
    from joligen_amd import _lib, ops

    B, H, W, Ci, Co = case
    ops.wgrad_tn(dO, x, dw, B=B, H=H, W=W, Cin=Ci, Cout=Co, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, lddy=dO.stride(-2), ldx=x.stride(-2),
                 lddw=9 * (cin_out or Ci), dbias=db, Cin_out=cin_out, alpha=alpha, dbias_scale=dbias_scale, x_mode=x_mode, pad_mode=pad_mode)
    return _lib.lib().jg_last_kernel().decode()


def test_the_ragged_case_is_ragged():
    B, H, W, Ci, Co = CASES[3]
    ntiles = B * (H // 2 // 4) * (W // 32)
    per, sk = pick_split((Co // 64) * (Ci // 64), ntiles)
    assert sk > 1 and 0 < ntiles - (sk - 1) * per < per, (ntiles, per, sk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_against_x_mode_1_and_autograd(case, dtype):
    """zeroed dw / dbias: x_mode 2 against the x_mode 1 launch on identical operands (3e-6) and against fp32 autograd (TOL); the dispatch
    names the new instantiation"""
    B, H, W, Ci, Co = case
    d = dev()
    x, dO, ref_w, ref_b = problem(case, dtype)
    xd, dOd = x.to(d), dO.to(d)
    out = {}
    for mode in (2, 1):
        dw = torch.zeros(Co, 3, 3, Ci, device=d)
        db = torch.zeros(Co, device=d)
        name = launch(dOd, xd, dw, db, case, mode)
        assert (name == KERNEL) == (mode == 2), name
        out[mode] = (dw, db)
    torch.cuda.synchronize()
    ew, eb = relerr(out[2][0], out[1][0]), relerr(out[2][1], out[1][1])
    rw, rb = relerr(out[2][0], ref_w), relerr(out[2][1], ref_b)
    print(f"subpixel wgrad {case} {dtype}: vs x_mode 1 dw {ew:.3e} dbias {eb:.3e}; vs fp32 autograd dw {rw:.3e} dbias {rb:.3e}")
    assert float(out[1][0].norm()) > 0
    assert ew < SAME_PRODUCTS and eb < SAME_PRODUCTS, (ew, eb)
    assert rw < TOL[dtype] and rb < TOL[dtype], (rw, rb)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_accumulates_onto_the_start_values(case, dtype):
    """dw and dbias start from random non-zero values, alpha = 0.5, dbias_scale = 2: the result is start + scaled gradient"""
    B, H, W, Ci, Co = case
    d = dev()
    x, dO, _, _ = problem(case, dtype)
    xd, dOd = x.to(d), dO.to(d)
    # of the size of the gradient itself (a sum over B H W pixels), so that neither addend drowns the other
    s = math.sqrt(B * H * W)
    w0, b0 = rnd((Co, 3, 3, Ci), torch.float32, 83, s).to(d), rnd((Co,), torch.float32, 84, s).to(d)
    gw, gb = torch.zeros(Co, 3, 3, Ci, device=d), torch.zeros(Co, device=d)
    launch(dOd, xd, gw, gb, case, 1)
    dw, db = w0.clone(), b0.clone()
    assert launch(dOd, xd, dw, db, case, 2, alpha=0.5, dbias_scale=2.0) == KERNEL
    torch.cuda.synchronize()
    ew, eb = relerr(dw, w0.double() + 0.5 * gw.double()), relerr(db, b0.double() + 2.0 * gb.double())
    print(f"subpixel wgrad accumulate {case} {dtype}: dw {ew:.3e} dbias {eb:.3e}")
    assert ew < SAME_PRODUCTS and eb < SAME_PRODUCTS, (ew, eb)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_channel_slices_and_canaries(case, dtype):
    """x and dO are channel slices (offset 8, ldx > Cin, lddy > Cout) of NaN-filled buffers, dw [Cout][3][3][Cin - 8] (Cin_out < Cin,
    lddw = 9 Cin_out) and dbias sit inside canaried fp32 buffers: within the atomics bound of the packed launch, canaries intact, finite"""
    B, H, W, Ci, Co = case
    d = dev()
    x, dO, _, _ = problem(case, dtype)
    cio = Ci - 8
    gw, gb = torch.zeros(Co, 3, 3, Ci, device=d), torch.zeros(Co, device=d)
    assert launch(dO.to(d), x.to(d), gw, gb, case, 2) == KERNEL
    xbuf, xv = SU.make_slice(x.shape, dtype, 0, left=8, right=24, guard=3, role="in", values=x, device=d)
    ybuf, yv = SU.make_slice(dO.shape, dtype, 0, left=8, right=40, guard=3, role="in", values=dO, device=d)
    wbuf, wv = SU.make_slice((1, 1, Co, 9 * cio), torch.float32, 0, left=0, right=0, guard=3, role="acc", device=d)
    bbuf, bv = SU.make_slice((1, 1, 1, Co), torch.float32, 0, left=8, right=8, guard=3, role="acc", device=d)
    assert xv.stride(-2) > Ci and yv.stride(-2) > Co
    assert launch(yv, xv, wv, bv, case, 2, cin_out=cio) == KERNEL
    torch.cuda.synchronize()
    for buf in (xbuf, ybuf, wbuf, bbuf):
        SU.assert_canary_intact(buf)
    dw = wv.reshape(Co, 3, 3, cio)
    assert torch.isfinite(dw).all() and torch.isfinite(bv).all()
    ew, eb = relerr(dw, gw[..., :cio]), relerr(bv.reshape(Co), gb)
    print(f"subpixel wgrad slices {case} {dtype}: dw {ew:.3e} dbias {eb:.3e}")
    assert ew < SAME_PRODUCTS and eb < SAME_PRODUCTS, (ew, eb)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_deterministic_mode_is_bit_reproducible(case, dtype):
    """JG_DETERMINISTIC: one workgroup per (co block, ci chunk), one writer per element -- two launches are bit-identical"""
    from joligen_amd import _lib

    B, H, W, Ci, Co = case
    d = dev()
    x, dO, ref_w, _ = problem(case, dtype)
    xd, dOd = x.to(d), dO.to(d)
    prev = _lib.set_tuning("JG_DETERMINISTIC", 1)
    try:
        runs = []
        for _ in range(2):
            dw, db = torch.zeros(Co, 3, 3, Ci, device=d), torch.zeros(Co, device=d)
            assert launch(dOd, xd, dw, db, case, 2) == KERNEL
            runs.append((dw, db))
    finally:
        _lib.set_tuning("JG_DETERMINISTIC", prev)
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert relerr(runs[0][0], ref_w) < TOL[dtype]


@pytest.mark.parametrize("shape,x_mode,pad_mode", [((1, 48, 32, 64, 64), 2, 0), ((1, 32, 48, 64, 64), 2, 0), ((1, 32, 32, 96, 64), 2, 0),
                                                   ((1, 32, 32, 64, 96), 2, 0), ((1, 32, 32, 64, 64), 2, 1), ((1, 32, 32, 64, 64), 3, 0)])
def test_refusals_launch_nothing(shape, x_mode, pad_mode):
    """outside the limits of x_mode 2 (upsampled size a multiple of 32, channel counts multiples of 64, no mirrored borders) and for an
    unknown x_mode, jg_conv2d_wgrad_tn raises and a NaN-prefilled dw stays as it is"""
    B, H, W, Ci, Co = shape
    d = dev()
    x = torch.zeros((B, H // 2, W // 2, Ci), device=d, dtype=torch.bfloat16)
    dO = torch.zeros((B, H, W, Co), device=d, dtype=torch.bfloat16)
    dw = torch.full((Co, 3, 3, Ci), float("nan"), device=d)
    db = torch.full((Co,), float("nan"), device=d)
    with pytest.raises(RuntimeError, match="jg_conv2d_wgrad_tn"):
        launch(dO, x, dw, db, shape, x_mode, pad_mode=pad_mode)
    torch.cuda.synchronize()
    assert torch.isnan(dw).all() and torch.isnan(db).all()


def test_through_the_executor(golden_dir, monkeypatch):
    """One backward of the smallest UNet of the executor tests with an up-block that passes subpixel_ok (128 channels, 32^2 -> 64^2), with
    unet_exec.SUBPIXEL_WGRAD off and on, in deterministic mode (every other sum of the step is then the same from run to run): weight and
    bias gradient of the up-block's convolution over Upsample(h) agree to 3e-6, every other gradient is bit-equal."""
    from joligen_amd import _lib, ops
    from joligen_amd.modules import unet_exec
    from test_gpu_1_model import build_net

    c = dict(ngf=64, mults=[1, 2], res_blocks=[1, 1], attn_res=[2], efficient=True, S=64, B=2)
    dtype = torch.bfloat16
    prev = _lib.set_tuning("JG_DETERMINISTIC", 1)
    try:
        net, _ = build_net(c, dtype, golden_dir)
        unet = net.denoise_fn.model
        net.arena.ensure_fresh()
        d = dev()
        g = torch.Generator().manual_seed(23)
        x0 = ops.to_nhwc(torch.randn(c["B"], 6, c["S"], c["S"], generator=g).to(d), dtype, 8)
        emb0 = torch.randn(c["B"], unet.cond_embed_dim, generator=g).to(d)
        R = ops.to_nhwc(torch.randn(c["B"], 3, c["S"], c["S"], generator=g).to(d), dtype, 8)
        seen = []
        real = unet_exec.wgrad_tn
        monkeypatch.setattr(unet_exec, "wgrad_tn", lambda *a, **kw: (seen.append(kw.get("x_mode", 0)), real(*a, **kw))[1])
        res = {}
        for on in (False, True):
            monkeypatch.setattr(unet_exec, "SUBPIXEL_WGRAD", on)
            del seen[:]
            net.arena.g.zero_()
            x = x0.clone().requires_grad_(True)
            emb = emb0.clone().requires_grad_(True)
            unet(x, emb).backward(R)
            torch.cuda.synchronize()
            assert (2 in seen) == on and (1 in seen) == (not on), seen
            res[on] = (x.grad.clone(), emb.grad.clone(), {k: p.grad.clone() for k, p in unet.named_parameters() if p.grad is not None})
    finally:
        _lib.set_tuning("JG_DETERMINISTIC", prev)
    # the convolutions over Upsample(h): conv2 of the efficient up-blocks whose output passes subpixel_ok
    up = set()
    for name, m in unet.named_modules():
        if getattr(m, "updown", False) and getattr(m, "up", False) and getattr(m, "efficient", False):
            conv = m.out_layers[3]
            if conv.meta.Cin % 64 == 0 and conv.meta.Cout % 64 == 0 and conv.meta.Cin_real == conv.meta.Cin:
                up |= {f"{name}.out_layers.3.weight", f"{name}.out_layers.3.bias"}
    assert up and up <= set(res[True][2]), (up, sorted(res[True][2])[:8])
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for k, gon in res[True][2].items():
        goff = res[False][2][k]
        if k in up:
            e = relerr(gon, goff)
            print(f"executor {k}: x_mode 2 vs x_mode 1 {e:.3e}")
            assert float(goff.norm()) > 0 and e < SAME_PRODUCTS, (k, e)
        else:
            assert torch.equal(gon, goff), k
