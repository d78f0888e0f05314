"""One list of the convolution / weight-gradient kernel instances the dispatch can name, with the geometry and tuning switches that reach each
(ConvCase / WgCase rows), the float64 CPU formulas the GPU tests compare with, and the exact-integer problems built on them.

Plain torch, no GPU, no test functions (as strided_util.py): tests/test_gpu_17_strided_operands.py and tests/test_gpu_23_exact_integer.py
launch the rows, tests/test_exact_integer_host.py checks the integer problems on the CPU.

Exact-integer problems.  With small integer operands every 16-bit product is exact in the MFMA, every partial sum is an integer below 2^24
(exact in fp32 in any order: split-K slices, atomics, another tile order), the epilogue alpha * acc + bias + res_scale * res with
power-of-two scales is exact and the result fits the 8-bit mantissa of bf16: a kernel's output must equal the float64 reference BIT FOR BIT.
  K = R * S * Cin, density p = min(2/3, 24 / sqrt(K)) (12 / sqrt(K) where the result sums four outputs: y_mode 1 / 2);
  x, w: +1 / -1 with probability p / 2 each, else 0; forward epilogue alpha = 0.5, integer bias in [-3, 3], res_scale = 2, integer residual
  in [-4, 4]; weight gradients: dy integer in [-2, 2] with density p, alpha = 0.5, dbias_scale = 2, dw / dbias start from integers in [-8, 8].
Preconditions (asserted by check_conv_preconditions / check_wgrad_preconditions, never used to skip):
  (i)  ref.to(dtype).double() == ref for every element, for fp16 and bf16;
  (ii) for every fp32 accumulator the sum of |addends| in units of the smallest addend is below 2^24.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

DTYPES = [torch.float16, torch.bfloat16]
NSLOT = 16
TWO24 = float(1 << 24)

# ======================================================================================================================================
# jg_conv2d_nt
# ======================================================================================================================================
ConvCase = namedtuple("ConvCase", "id inst geo tune opts", defaults=({}, {}))
G128, G256, G64, G32 = ("conv_nt_glds_kernel<128,128,64,2,2>", "conv_nt_glds_kernel<256,64,64,4,1>", "conv_nt_glds_kernel<64,64,64,2,2>",
                        "conv_nt_glds_kernel<256,32,64,4,1>")
NO_SMALL = {"JG_CONV_SMALL_TILE": 0}       # the default tiles at test-sized grids (the automatic choice there is the 64 x 64 tile)

CONV_ROWS = [
    # geo = (B, H, W, Cin, Cout, R, S, pad, stride)
    # generic LDS-DMA kernel (CONV_CASES / SPLITK_CASES of test_gpu_0_ops.py)
    ConvCase("glds128-raggedM", G128, (1, 10, 12, 64, 128, 3, 3, 1, 1), NO_SMALL),
    ConvCase("glds256x64", G256, (2, 16, 16, 32, 64, 3, 3, 1, 1), NO_SMALL),
    ConvCase("glds64", G64, (2, 16, 16, 32, 64, 3, 3, 1, 1)),
    ConvCase("glds256x32-cout8", G32, (1, 208, 208, 16, 8, 3, 3, 1, 1)),      # >= 160 tiles of 256 pixels: the 32-wide tile, unsplit
    ConvCase("glds-K72", G64, (2, 16, 16, 8, 64, 3, 3, 1, 1)),
    ConvCase("glds-stride2", G64, (2, 16, 16, 32, 64, 3, 3, 1, 2)),
    ConvCase("glds-1x1", G128, (2, 12, 12, 64, 192, 1, 1, 0, 1), NO_SMALL),
    ConvCase("glds-4x4", G64, (1, 9, 9, 16, 32, 4, 4, 1, 1)),
    ConvCase("glds256x32+splitK", G32 + "+splitK", (4, 7, 7, 512, 8, 4, 4, 1, 1)),
    ConvCase("glds128+splitK", G128 + "+splitK", (2, 16, 16, 256, 256, 4, 4, 1, 2)),
    # halo-resident 3x3 kernel: every forced configuration at the HALO_FORCED shapes, then the modes on one shape
    ConvCase("halo-cfg3", "conv3x3_halo_kernel<256-wide,8 waves>", (2, 32, 32, 192, 256, 3, 3, 1, 1), {"JG_HALO_CFG": 3}),
    ConvCase("halo-cfg2", "conv3x3_halo_kernel<128-wide,8 waves>", (2, 32, 16, 128, 128, 3, 3, 1, 1), {"JG_HALO_CFG": 2}),
    ConvCase("halo-cfg4", "conv3x3_halo_kernel<64-wide>", (2, 16, 32, 192, 64, 3, 3, 1, 1), {"JG_HALO_CFG": 4}),
    ConvCase("halo-cfg1", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 16, 192, 256, 3, 3, 1, 1), {"JG_HALO_CFG": 1}),
    ConvCase("halo-stats", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 16, 192, 256, 3, 3, 1, 1), {"JG_HALO_CFG": 1}, dict(stats=True)),
    ConvCase("halo-reflect", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 32, 128, 128, 3, 3, 1, 1), {}, dict(pad_mode=1)),
    ConvCase("halo-x_up", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 32, 128, 128, 3, 3, 1, 1), {}, dict(x_mode=1)),
    ConvCase("halo-subpixel", "conv3x3_halo_kernel<subpixel>", (1, 32, 64, 128, 128, 3, 3, 1, 1), {}, dict(x_mode=2)),
    ConvCase("halo-y_pool", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 32, 128, 128, 3, 3, 1, 1), {}, dict(y_mode=1, bias=False, res=False)),
    ConvCase("halo-res_up", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 32, 128, 128, 3, 3, 1, 1), {}, dict(res_mode=1)),
    # persistent Cin == 64 kernel, forced (first four rows of P64_CASES), fused statistics into a wider row
    ConvCase("p64-2streams", "conv3x3_p64_kernel", (2, 32, 48, 64, 64, 3, 3, 1, 1), {"JG_PERSIST64": 2}, dict(res=False, stats=True)),
    ConvCase("p64-5streams", "conv3x3_p64_kernel", (3, 64, 64, 64, 128, 3, 3, 1, 1), {"JG_PERSIST64": 5}, dict(stats=True)),
    ConvCase("p64-3blocks", "conv3x3_p64_kernel", (1, 48, 32, 64, 192, 3, 3, 1, 1), {"JG_PERSIST64": 3}, dict(stats=True)),
    ConvCase("p64-1tile", "conv3x3_p64_kernel", (1, 16, 16, 64, 64, 3, 3, 1, 1), {"JG_PERSIST64": 7}, dict(stats=True)),
    # streaming kernels (>= 65536 pixels)
    ConvCase("1x1-stream", "conv1x1_stream_kernel", (1, 256, 256, 64, 128, 1, 1, 0, 1)),
    ConvCase("c8-stem", "conv3x3_c8_stream_kernel", (1, 256, 256, 8, 64, 3, 3, 1, 1), {}, dict(fixed=("x",))),
    ConvCase("c8-stem-stats", "conv3x3_c8_stream_kernel", (1, 256, 256, 8, 128, 3, 3, 1, 1), {}, dict(fixed=("x",), stats=True)),
    # halo-resident few-output-channel kernels: no residual operand in these kernels
    ConvCase("kxk-7x7", "conv_kxk_halo_kernel<7x7>", (3, 80, 80, 32, 8, 7, 7, 3, 1), {}, dict(res=False)),
    ConvCase("kxk-1x7", "conv_kxk_halo_kernel<1x7>", (1, 134, 134, 64, 32, 1, 7, 0, 1), {}, dict(res=False)),
    ConvCase("kxk-3x3", "conv_kxk_halo_kernel<3x3>", (4, 256, 256, 64, 8, 3, 3, 1, 1), {}, dict(res=False)),
]

# sub-pixel input gradient (y_mode 2): CASES / NAMES of test_gpu_19_subpixel_dgrad.py, (B, H_up, W_up, C_in, C_out) of the FORWARD layer
SUBPIXEL_DGRAD_SHAPES = [(2, 32, 32, 64, 64), (1, 32, 64, 128, 128), (1, 64, 32, 64, 192), (2, 32, 32, 256, 192)]
SUBPIXEL_DGRAD_NAMES = {128: {0: "conv3x3_halo_kernel<subpixel dgrad,128-wide,4 waves>", 1: "conv3x3_halo_kernel<subpixel dgrad,128-wide,8 waves>",
                              2: "conv3x3_halo_kernel<subpixel dgrad,64-wide>"},
                        64: {0: "conv3x3_halo_kernel<subpixel dgrad,64-wide>"}}


def _subpixel_dgrad_rows():
    rows = []
    for i, (B, H, W, Ci, Co) in enumerate(SUBPIXEL_DGRAD_SHAPES):
        names = SUBPIXEL_DGRAD_NAMES[128 if Ci % 128 == 0 else 64]
        for cfg, inst in names.items():
            # in the sense of the launch: Cin = channels of dO, Cout = channels of the gradient
            rows.append(ConvCase(f"subpixel-dgrad{i}-cfg{cfg}", inst, (B, H, W, Co, Ci, 3, 3, 1, 1), {"JG_SUBPIXEL_DGRAD_CFG": cfg},
                                 dict(y_mode=2, bias=False, res=False)))
    return rows


# the instances CONV_ROWS does not reach; test_gpu_17 keeps to CONV_ROWS
CONV_ROWS_NEW = [
    # generic split-K 1x1 instance (SPLITK_CASES of test_gpu_0_ops.py): K = 1024, exactly 16 K-steps
    ConvCase("glds256x64+splitK-1x1", G256 + "+splitK", (1, 4, 4, 1024, 64, 1, 1, 0, 1)),
    *_subpixel_dgrad_rows(),
    # y_mode 1 and x_mode 1 on the forced 8-wave tiles (HALO_FORCED shapes)
    ConvCase("halo-cfg2-x_up", "conv3x3_halo_kernel<128-wide,8 waves>", (2, 32, 16, 128, 128, 3, 3, 1, 1), {"JG_HALO_CFG": 2}, dict(x_mode=1)),
    ConvCase("halo-cfg3-x_up", "conv3x3_halo_kernel<256-wide,8 waves>", (2, 32, 32, 192, 256, 3, 3, 1, 1), {"JG_HALO_CFG": 3}, dict(x_mode=1)),
    ConvCase("halo-cfg2-y_pool", "conv3x3_halo_kernel<128-wide,8 waves>", (2, 32, 16, 128, 128, 3, 3, 1, 1), {"JG_HALO_CFG": 2},
             dict(y_mode=1, bias=False, res=False)),
    ConvCase("halo-cfg3-y_pool", "conv3x3_halo_kernel<256-wide,8 waves>", (2, 32, 32, 192, 256, 3, 3, 1, 1), {"JG_HALO_CFG": 3},
             dict(y_mode=1, bias=False, res=False)),
    # automatic conv3x3_p64_kernel dispatch (csrc/conv_p64.hip jg_conv_p64_try, JG_PERSIST64 1): B * (H / 16) * (W / 16) >= 1024 spatial tiles and
    # no residual operand -- 262144 pixels whatever the shape, so nothing smaller than the (4, 256, 256, 64) row of P64_CASES reaches it
    ConvCase("p64-auto", "conv3x3_p64_kernel", (4, 256, 256, 64, 64, 3, 3, 1, 1), {}, dict(res=False, stats=True)),
]
CONV_ROWS_ALL = CONV_ROWS + CONV_ROWS_NEW


def conv_out_hw(H, W, R, S, pad, stride):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def conv_opts(case):
    o = dict(bias=True, res=True, stats=False, pad_mode=0, x_mode=0, y_mode=0, res_mode=0, fixed=())
    o.update(case.opts)
    return o


def conv_shapes(case):
    """(x, y, res) shapes [B, H, W, C] of a ConvCase"""
    B, H, W, Cin, Cout, R, S, pad, stride = case.geo
    o = conv_opts(case)
    Ho, Wo = conv_out_hw(H, W, R, S, pad, stride)
    xs = (B, H // 2, W // 2, Cin) if o["x_mode"] else (B, H, W, Cin)
    ys = (B, Ho // 2, Wo // 2, Cout) if o["y_mode"] else (B, Ho, Wo, Cout)
    rs = (B, Ho // 2, Wo // 2, Cout) if o["res_mode"] else (B, Ho, Wo, Cout)
    return xs, ys, rs


def nchw(v):
    return v.double().cpu().permute(0, 3, 1, 2)


def up2(t_nchw):
    return t_nchw.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def conv_reference(x, res, wref, bias, case, alpha, res_scale):
    """float64 CPU evaluation of jg_conv2d_nt for a ConvCase: x / res NHWC tensors (res None or unused without o["res"]), wref
    [Cout][R][S][Cin] float64, bias [Cout] or None; returns NCHW float64"""
    stride, pad = case.geo[8], case.geo[7]
    o = conv_opts(case)
    x = nchw(x)
    if o["x_mode"]:
        x = up2(x)
    if o["pad_mode"]:
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wref.permute(0, 3, 1, 2), None, stride, 0)
    else:
        y = F.conv2d(x, wref.permute(0, 3, 1, 2), None, stride, pad)
    y = alpha * y
    if o["y_mode"]:
        y = 4 * F.avg_pool2d(y, 2)
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if o["res"]:
        r = nchw(res)
        y = y + res_scale * (up2(r) if o["res_mode"] else r)
    return y


# ======================================================================================================================================
# jg_conv2d_wgrad_tn
# ======================================================================================================================================
WgCase = namedtuple("WgCase", "id inst geo splitk tune opts", defaults=({}, {}))
WG_ROWS = [
    # geo = (B, H, W, Cin, Cout, R, S, pad, stride); splitk 1 + store = JG_OUT_STORE_F32 (plain stores: bit-exact), otherwise fp32 atomics
    WgCase("tr1-1x1-store", "wgrad_tn_tr_kernel<1>", (2, 20, 12, 64, 64, 1, 1, 0, 1), 1, {"JG_WGRAD_VARIANT": 2}, dict(store=True)),
    WgCase("tr1-1x1-splitk3", "wgrad_tn_tr_kernel<1>", (2, 20, 12, 64, 64, 1, 1, 0, 1), 3, {"JG_WGRAD_VARIANT": 2}),
    WgCase("tr2-3x3-s2-store", "wgrad_tn_tr_kernel<2>", (2, 17, 17, 32, 160, 3, 3, 1, 2), 1, {"JG_WGRAD_VARIANT": 2}, dict(store=True)),
    WgCase("tr1-3x3-ragged-onestep", "wgrad_tn_tr_kernel<1>", (1, 9, 7, 24, 40, 3, 3, 1, 1), 1, {"JG_WGRAD_VARIANT": 2}, dict(store=True)),
    WgCase("big-1x1-ragged", "wgrad_tn_big_kernel", (3, 64, 48, 256, 320, 1, 1, 0, 1), 4, {}, dict(real_cout=316)),
    WgCase("big-4x4-s2", "wgrad_tn_big_kernel", (2, 128, 128, 32, 256, 4, 4, 1, 2), 2),
    WgCase("halo-cfg1", "wgrad3x3_halo_kernel<16 rows,64 co>", (2, 32, 32, 64, 128, 3, 3, 1, 1), 1, {"JG_WGRAD_HALO_CFG": 1}),
    WgCase("halo-cfg2", "wgrad3x3_halo_kernel<8 rows,128 co>", (2, 32, 32, 128, 128, 3, 3, 1, 1), 1, {"JG_WGRAD_HALO_CFG": 2}),
    WgCase("halo-cfg3", "wgrad3x3_halo_kernel<8 rows,64 co,4 waves>", (2, 32, 32, 128, 64, 3, 3, 1, 1), 1, {"JG_WGRAD_HALO_CFG": 3}),
    WgCase("halo-cfg4", "wgrad3x3_halo_kernel<8 rows,32 co,4 waves>", (3, 16, 48, 64, 128, 3, 3, 1, 1), 1, {"JG_WGRAD_HALO_CFG": 4}),
    WgCase("sw-cfg6", "wgrad3x3_sw_kernel<16 rows,64 co>", (3, 16, 48, 192, 64, 3, 3, 1, 1), 1, {"JG_WGRAD_HALO_CFG": 6}),
    WgCase("halo-narrow", "wgrad3x3_halo_kernel<16 rows,<64 co>", (4, 256, 256, 64, 8, 3, 3, 1, 1), 1, {}, dict(real_cout=3)),
    WgCase("halo-reflect", "wgrad3x3_halo_kernel<16 rows,64 co>", (2, 16, 32, 128, 64, 3, 3, 1, 1), 1, {}, dict(pad_mode=1)),
    WgCase("halo-x_up", "wgrad3x3_halo_kernel<16 rows,64 co>", (2, 16, 32, 128, 64, 3, 3, 1, 1), 1, {}, dict(x_mode=1)),
    WgCase("kxk-7x7", "wgrad_kxk_halo_kernel<7x7,2 tap rows>", (4, 128, 128, 64, 8, 7, 7, 3, 1), 1, {}, dict(real_cout=3)),
    WgCase("kxk-1x7", "wgrad_kxk_halo_kernel<1x7>", (1, 256, 262, 64, 32, 1, 7, 0, 1), 1),
]

SUBPIXEL_WGRAD_KERNEL = "wgrad3x3_halo_kernel<subpixel,4 rows,64 co>"
WG_ROWS_NEW = [
    # sub-pixel weight gradient (x_mode 2): the first three CASES of test_gpu_20_subpixel_wgrad.py, geo = (B, H_up, W_up, C_in, C_out, ...)
    WgCase("subpixel0", SUBPIXEL_WGRAD_KERNEL, (2, 32, 32, 64, 64, 3, 3, 1, 1), 1, {}, dict(x_mode=2)),
    WgCase("subpixel1", SUBPIXEL_WGRAD_KERNEL, (1, 32, 64, 128, 128, 3, 3, 1, 1), 1, {}, dict(x_mode=2)),
    WgCase("subpixel2", SUBPIXEL_WGRAD_KERNEL, (1, 64, 32, 64, 192, 3, 3, 1, 1), 1, {}, dict(x_mode=2)),
    # Wo % 4 != 0: the per-pixel decomposition path (BWD_CASES of test_gpu_0_ops.py)
    WgCase("tr1-3x3-ragged-Wo7", "wgrad_tn_tr_kernel<1>", (2, 9, 7, 32, 32, 3, 3, 1, 1), 1, {"JG_WGRAD_VARIANT": 2}),
]
WG_ROWS_ALL = WG_ROWS + WG_ROWS_NEW
# jg_conv2d_wgrad_tn_group: the members of test_wgrad_group_on_channel_slices (64-row tile, 128-row tile, a 4x4 stride-2 geometry)
WG_GROUP_GEOS = [(1, 1, 1024, 64, 64, 1, 1, 0, 1), (1, 1, 520, 64, 128, 1, 1, 0, 1), (2, 16, 16, 32, 128, 4, 4, 1, 2)]


def wgrad_opts(case):
    o = dict(store=False, real_cout=case.geo[4], pad_mode=0, x_mode=0)
    o.update(case.opts)
    return o


def wgrad_reference(x, dy, geo, o):
    """float64 autograd of conv2d w.r.t. its weight and bias: (dw [Cout][R * S * Cin], dbias [Cout]); x, dy NHWC"""
    B, H, W, Cin, Cout, R, S, pad, stride = geo
    xin = nchw(x)
    if o.get("x_mode"):
        xin = up2(xin)
    if o.get("pad_mode"):
        xin, pad = F.pad(xin, (1, 1, 1, 1), mode="reflect"), 0
    wr = torch.zeros(Cout, Cin, R, S, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, wr, None, stride, pad).backward(nchw(dy))
    return wr.grad.permute(0, 2, 3, 1).reshape(Cout, -1), dy.double().cpu().sum((0, 1, 2))


# ======================================================================================================================================
# exact-integer problems
# ======================================================================================================================================
ALPHA, RES_SCALE, DBIAS_SCALE = 0.5, 2.0, 2.0
# per-row factor on the density where a precondition fails at the recipe's value.  p64-auto: 4 * sum y^2 over the 65536 pixels of an image
# is 2.0e7 > 2^24 at p = 2 / 3 (E y^2 = K p^2 / 4 + bias^2 = 64 + 9); at 0.6 p it is 0.5 of 2^24
DENSITY_FACTOR = {"p64-auto": 0.6}


def density(K, four_outputs=False):
    return min(2.0 / 3.0, (12.0 if four_outputs else 24.0) / math.sqrt(K))


def ternary(shape, p, seed):
    """+1 / -1 with probability p / 2 each, else 0 (fp32)"""
    u = torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    return (u < p / 2).float() - ((u >= p / 2) & (u < p)).float()


def integers(shape, lo, hi, seed, p=1.0):
    """uniform integers in [lo, hi] (fp32), each kept with probability p, else 0"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    if p < 1.0:
        v = v * (torch.rand(shape, generator=g) < p).float()
    return v


IntConv = namedtuple("IntConv", "x w bias res ref o p")
_CONV_CACHE = {}


def int_conv_problem(case):
    """IntConv of a ConvCase: x / res NHWC fp32 integers, w the fp32 master weights [Cout][R][S][Cin] in the sense of the launch, bias [Cout],
    ref the float64 NCHW reference; the last problem is kept (both dtypes of a row share it), never written to"""
    if case.id in _CONV_CACHE:
        return _CONV_CACHE[case.id]
    B, H, W, Cin, Cout, R, S, pad, stride = case.geo
    o = conv_opts(case)
    xs, ys, rs = conv_shapes(case)
    p = density(R * S * Cin, bool(o["y_mode"])) * DENSITY_FACTOR.get(case.id, 1.0)
    x = ternary(xs, p, 101)
    w = ternary((Cout, R, S, Cin), p, 102)
    bias = integers((Cout,), -3, 3, 103) if o["bias"] else None
    res = integers(rs, -4, 4, 104) if o["res"] else None
    ref = conv_reference(x, res, w.double(), bias, case, ALPHA, RES_SCALE)
    _CONV_CACHE.clear()
    _CONV_CACHE[case.id] = IntConv(x, w, bias, res, ref, o, p)
    return _CONV_CACHE[case.id]


def representable(ref, dtype):
    return bool((ref.to(dtype).double() == ref).all())


def check_conv_preconditions(case, prob):
    """(i) and (ii) on the reference of an IntConv; returns (worst |y|, worst fused-statistics sum in units of its smallest addend)"""
    ref = prob.ref
    for dtype in DTYPES:
        bad = ref.to(dtype).double() != ref
        assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} reference values are not representable in {dtype} (worst |y| {float(ref.abs().max())})"
    worst = 0.0
    if prob.o["stats"]:
        # addends of (sum y, sum y^2) are multiples of 0.5 / 0.25
        worst = max(float((2 * ref.abs()).sum((2, 3)).max()), float((4 * ref * ref).sum((2, 3)).max()))
        assert worst < TWO24, f"{case.id}: fused statistics reach {worst:.3e} units, 2^24 = {TWO24:.3e}"
    return float(ref.abs().max()), worst


IntWgrad = namedtuple("IntWgrad", "x dy dw0 db0 o p")


def int_wgrad_problem(geo, o, seed=0):
    """IntWgrad: x ternary, dy integers in [-2, 2] with density p (zero in the padding channels), start values of dw / dbias in [-8, 8]"""
    B, H, W, Cin, Cout, R, S, pad, stride = geo
    Ho, Wo = conv_out_hw(H, W, R, S, pad, stride)
    real = o.get("real_cout", Cout)
    p = density(R * S * Cin)
    xs = (B, H // 2, W // 2, Cin) if o.get("x_mode") else (B, H, W, Cin)
    x = ternary(xs, p, 111 + seed)
    dy = integers((B, Ho, Wo, Cout), -2, 2, 112 + seed, p)
    dy[..., real:] = 0
    dw0 = integers((real, R * S * Cin), -8, 8, 113 + seed)
    db0 = integers((real,), -8, 8, 114 + seed)
    return IntWgrad(x, dy, dw0, db0, o, p)


def check_wgrad_preconditions(name, prob):
    """(ii) for dw and dbias: |x| <= 1, so sum_p |dy[p][co]| bounds the |addends| of every dw[co][k] (units of alpha = 0.5: one per product);
    dbias adds dbias_scale * dy onto an integer.  Returns the worst (dw, dbias) sums in units."""
    ady = prob.dy.double().abs().sum((0, 1, 2))
    # x_mode != 0: every x pixel meets up to four dy pixels per tap, still one product per (pixel of dy, tap)
    dw_units = float((2 * 8 + ady).max())
    db_units = float((8 + DBIAS_SCALE * ady).max())
    assert dw_units < TWO24 and db_units < TWO24, f"{name}: dw {dw_units:.3e} / dbias {db_units:.3e} units, 2^24 = {TWO24:.3e}"
    return dw_units, db_units


def int_wgrad_reference(prob, geo):
    """(dw, dbias) float64 the launch must leave: start + alpha * gradient (start 0 for plain stores), start + dbias_scale * sum dy"""
    real = prob.o.get("real_cout", geo[4])
    gw, gb = wgrad_reference(prob.x, prob.dy, geo, prob.o)
    dw = ALPHA * gw[:real] + (0 if prob.o.get("store") else prob.dw0.double())
    return dw, prob.db0.double() + DBIAS_SCALE * gb[:real]


# instances outside the two tables that tests/test_gpu_23_exact_integer.py launches by name
GN_APPLY_KERNEL, GN_BWD_APPLY_KERNEL = "conv1x1_stream_kernel+gn_apply", "conv1x1_stream_kernel+gn_bwd_apply"
REFLECT_RING_KERNEL = "reflect_ring_gemm_kernel"


def all_instance_names():
    return {c.inst for c in CONV_ROWS_ALL} | {c.inst for c in WG_ROWS_ALL} | {GN_APPLY_KERNEL, GN_BWD_APPLY_KERNEL, REFLECT_RING_KERNEL}
