"""The stride contract of include/jg355.h ("every tensor carries its own pixel stride (elements, multiple of 8, >= C)") per kernel instance:
every convolution, weight-gradient and streaming GroupNorm / resample kernel launched on channel slices of wider NHWC buffers, the way
joligen_amd/modules/unet_exec.py launches them (it never concatenates), with every operand on a DIFFERENT stride.

Every case runs the same launch twice under the same tuning switches (tests/strided_util.py: run_pair) -- on contiguous operands and on slices
holding the same values, surrounded by canaries -- and asserts
  (a) jg_last_kernel() names the same instance for both launches, the one the case lists: dispatch does not change with the stride;
  (b) the strided result equals the contiguous one: bit for bit where the output is written by plain stores (same kernel, grid and
      arithmetic, only addresses differ); where fp32 atomics accumulate it, the bounds this suite already uses for re-ordered fp32 sums:
      1e-5 norm-wise for fused statistics / reductions (test_conv_p64_persistent_kernel), 2e-5 for weight gradients (the comment above
      HALO_FORCED in test_gpu_0_ops.py);
  (c) the strided result agrees with a float64 CPU evaluation of the op on the 16-bit-rounded inputs within the file-level TOL of
      test_gpu_0_ops.py (1e-3 fp16, 8e-3 bf16; 3 * TOL for GroupNorm gradients, as there);
  (d) every canary is intact (input canaries are NaN: an out-of-slice read that reaches the result poisons it), every element of every
      output view was written, no output holds a NaN.
Two placements per case: "exec" (left offsets multiples of 64 channels, as in the UNet concat buffers) and "abi" (left 8, right 24 + 16 i:
16-byte aligned and nothing more, the weakest alignment the header promises).

A combination the library does not serve on a slice is listed in REFUSED with its reason and asserted as such.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import strided_util as su
from kernel_cases import CONV_ROWS, NSLOT, WG_ROWS, ConvCase, conv_opts, conv_reference, conv_shapes
from kernel_cases import conv_out_hw as _conv_out_hw
from kernel_cases import nchw as _nchw
from kernel_cases import wgrad_opts
from kernel_cases import wgrad_reference as _wgrad_reference
from strided_util import Operand

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
STATS_BOUND = 1e-5      # fp32 atomics in another order: fused statistics, GroupNorm reductions (test_conv_p64_persistent_kernel)
WGRAD_BOUND = 2e-5      # weight gradients accumulated across workgroups (comment above HALO_FORCED in test_gpu_0_ops.py)
SILU = 1


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _ld(v):
    assert v.stride(-1) == 1
    return v.stride(-2)


def _code(dtype):
    from joligen_amd import _lib

    return _lib.JG_F16 if dtype == torch.float16 else _lib.JG_BF16


def _rnd(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _pair(launch, operands, kind, tuning=None, fixed=()):
    return su.run_pair(launch, operands, kind=kind, tuning=tuning, device=dev(), fixed=fixed)


def _close(got, ref, tol, what):
    e = su.relerr(got, ref)
    assert e < tol, f"{what}: {e:.3e} against the float64 reference (bound {tol:.1e})"


# ======================================================================================================================================
# jg_conv2d_nt: x, y and res strided; bias; alpha = 0.5, res_scale = 0.7
# ======================================================================================================================================
# ConvCase / CONV_ROWS: tests/kernel_cases.py (one list of kernel instances, shared with the exact-integer tests)

# combinations the library does not serve on a channel slice; each is asserted in test_refused_combinations
REFUSED = [
    # (id, reason)
    ("c8-stem-strided-x", "conv3x3_c8_stream_kernel reads whole 16-byte pixels of the 8-channel image: its dispatch requires ldx == 8.  An x "
                          "slice (ldx > 8) is served by the generic kernel instead -- correct, another instance; the c8 rows above keep x contiguous"),
]


def _conv_problem(case, dtype, strided_x_for_c8=False):
    """operands, launch and float64 reference of one ConvCase"""
    from joligen_amd import _lib, ops

    B, H, W, Cin, Cout, R, S, pad, stride = case.geo
    o = conv_opts(case)
    Ho, Wo = _conv_out_hw(H, W, R, S, pad, stride)
    d = dev()
    xs, ys, rs = conv_shapes(case)
    operands = {"x": Operand(xs, dtype, "in", 1), "y": Operand(ys, dtype, "out")}
    if o["res"]:
        operands["res"] = Operand(rs, dtype, "in", 4)
    if o["stats"]:
        operands["stats"] = Operand((B, NSLOT, 1, 2 * Cout), torch.float32, "acc", unit=2)
    w32 = _rnd((Cout, R, S, Cin), torch.float32, 2, 1.0 / math.sqrt(Cin * R * S))
    w16 = w32.to(dtype)
    bias = _rnd((Cout,), torch.float32, 3) if o["bias"] else None
    if o["x_mode"] == 2:
        wd = torch.empty((4, Cout, 2, 2, Cin), device=d, dtype=dtype)
        _lib.check(_lib.lib().jg_subpixel_fold(_code(dtype), w32.to(d).data_ptr(), wd.data_ptr(), Cout, Cin, ops._st()), "jg_subpixel_fold")
        ldw, wref = 4 * Cin, w32.double()        # the folded taps are sums of the fp32 master weights, rounded once
    else:
        wd, ldw, wref = w16.to(d), R * S * Cin, w16.double()
    bd = None if bias is None else bias.to(d)

    def launch(v):
        st = v.get("stats")
        ops.conv_nt(v["x"], wd, v["y"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo, ldx=_ld(v["x"]), ldw=ldw,
                    ldy=_ld(v["y"]), bias=bd, res=v.get("res"), ldres=_ld(v["res"]) if "res" in v else 0, alpha=0.5, res_scale=0.7, stats=st,
                    ldstats=_ld(st) // 2 if st is not None else 0, stats_slots=NSLOT if st is not None else 1, pad_mode=o["pad_mode"],
                    res_mode=o["res_mode"], x_mode=o["x_mode"], y_mode=o["y_mode"])

    def reference(v):
        return conv_reference(v["x"], v.get("res"), wref, bias, case, 0.5, 0.7)

    return operands, launch, reference, o


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
@pytest.mark.parametrize("case", CONV_ROWS, ids=[c.id for c in CONV_ROWS])
def test_conv_nt_on_channel_slices(case, kind, dtype):
    operands, launch, reference, o = _conv_problem(case, dtype)
    pair = _pair(launch, operands, kind, case.tune, o["fixed"])
    su.verify(pair, exact=["y"], approx={"stats": STATS_BOUND} if o["stats"] else None, kernel=case.inst)
    ref = reference(pair.strided)
    _close(_nchw(pair.strided["y"]), ref, TOL[dtype], f"{case.id} y")
    if o["stats"]:
        st = pair.strided["stats"].double().cpu().sum(1).reshape(ref.shape[0], ref.shape[1], 2)
        _close(st[..., 0], ref.sum((2, 3)), TOL[dtype], f"{case.id} fused sum")
        _close(st[..., 1], (ref * ref).sum((2, 3)), TOL[dtype], f"{case.id} fused sum of squares")


def test_refused_combinations():
    """REFUSED, asserted: the 8-channel stem shape with an x slice does not reach conv3x3_c8_stream_kernel (its dispatch requires ldx == 8);
    the generic kernel serves it with the same result, and nothing outside the slices is touched."""
    from joligen_amd import _lib

    assert [r[0] for r in REFUSED] == ["c8-stem-strided-x"]
    dtype = torch.bfloat16
    case = ConvCase("c8-stem-strided-x", None, (1, 256, 256, 8, 64, 3, 3, 1, 1))
    operands, launch, reference, o = _conv_problem(case, dtype)
    pair = _pair(launch, operands, su.ABI_MIN)
    assert pair.kernels[0] == "conv3x3_c8_stream_kernel" and pair.kernels[1] != "conv3x3_c8_stream_kernel", pair.kernels
    assert pair.kernels[1].startswith("conv_nt_glds_kernel"), pair.kernels
    for bufs in (pair.contig_bufs, pair.strided_bufs):
        for b in bufs.values():
            su.assert_canary_intact(b)
        su.assert_fully_written(bufs["y"])
    _close(_nchw(pair.strided["y"]), reference(pair.strided), TOL[dtype], "c8 stem shape on the generic kernel")
    assert su.relerr(pair.strided["y"], pair.contig["y"]) < TOL[dtype]        # another kernel: same products, another summation order
    assert _lib.JG_ERR_UNSUPPORTED == -2


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
def test_conv1x1_gn_apply_on_channel_slices(kind, dtype):
    """conv1x1_stream_kernel+gn_apply: x, y and the normalised copy y_norm (ldyn > Cin) each on its own stride"""
    from joligen_amd import ops

    B, H, W, Cin, Cout = 1, 256, 256, 64, 128
    d = dev()
    w = _rnd((Cout, 1, 1, Cin), dtype, 2, 1.0 / math.sqrt(Cin))
    bias = _rnd((Cout,), torch.float32, 3)
    g = torch.Generator().manual_seed(5)
    ab = torch.stack([torch.rand(B, Cin, generator=g) + 0.5, torch.randn(B, Cin, generator=g)], -1).contiguous()
    wd, bd, abd = w.to(d), bias.to(d), ab.to(d)
    operands = {"x": Operand((B, H, W, Cin), dtype, "in", 1, scale=1.5), "y": Operand((B, H, W, Cout), dtype, "out"),
                "yn": Operand((B, H, W, Cin), dtype, "out")}

    def launch(v):
        ok = ops.conv_nt(v["x"], wd, v["y"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldx=_ld(v["x"]), ldw=Cin,
                         ldy=_ld(v["y"]), bias=bd, apply=(abd, v["yn"], _ld(v["yn"]), SILU))
        assert ok is not False

    pair = _pair(launch, operands, kind)
    su.verify(pair, exact=["y", "yn"], kernel="conv1x1_stream_kernel+gn_apply")
    x = pair.strided["x"].double().cpu()
    _close(pair.strided["y"], x @ w.double().view(Cout, Cin).t() + bias.double(), TOL[dtype], "y")
    _close(pair.strided["yn"], F.silu(ab[:, None, None, :, 0].double() * x + ab[:, None, None, :, 1].double()), TOL[dtype], "y_norm")


def _silu_grad(u):
    sg = torch.sigmoid(u)
    return sg * (1 + u * (1 - sg))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
def test_conv1x1_gn_bwd_apply_on_channel_slices(kind, dtype):
    """conv1x1_stream_kernel+gn_bwd_apply: dO, y, gx, gdy, add1 and add2 each on its own stride"""
    from joligen_amd import ops

    B, H, W, Cf, C = 1, 256, 256, 128, 64         # input gradient of a 1x1 convolution 64 -> 128
    d = dev()
    wT = _rnd((C, 1, 1, Cf), dtype, 2, 0.1)
    g = torch.Generator().manual_seed(7)
    ab = torch.stack([torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g)], -1).contiguous()
    pqr = torch.stack([torch.rand(B, C, generator=g) + 0.5, 0.1 * torch.randn(B, C, generator=g), 0.1 * torch.randn(B, C, generator=g)], -1).contiguous()
    wd, abd, pqrd = wT.to(d), ab.to(d), pqr.to(d)
    s1, s2, alpha = 0.7, -1.3, 0.70710678
    operands = {"dO": Operand((B, H, W, Cf), dtype, "in", 1), "y": Operand((B, H, W, C), dtype, "out"), "gx": Operand((B, H, W, C), dtype, "in", 3, scale=1.3),
                "gdy": Operand((B, H, W, C), dtype, "in", 4), "add1": Operand((B, H, W, C), dtype, "in", 5), "add2": Operand((B, H, W, C), dtype, "in", 6)}

    def launch(v):
        ok = ops.conv_nt(v["dO"], wd, v["y"], B=B, H=H, W=W, Cin=Cf, Cout=C, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldx=_ld(v["dO"]), ldw=Cf,
                         ldy=_ld(v["y"]), alpha=alpha, gn_bwd_apply=(v["gx"], v["gdy"], abd, pqrd, v["add1"], s1, v["add2"], s2, SILU))
        assert ok is not False

    pair = _pair(launch, operands, kind)
    su.verify(pair, exact=["y"], kernel="conv1x1_stream_kernel+gn_bwd_apply")
    v = {k: t.double().cpu() for k, t in pair.strided.items()}
    a, b = ab[:, None, None, :, 0].double(), ab[:, None, None, :, 1].double()
    du = v["gdy"] * _silu_grad(a * v["gx"] + b)
    p = pqr[:, None, None].double()
    want = du * p[..., 0] + v["gx"] * p[..., 1] + p[..., 2] + s1 * v["add1"] + s2 * v["add2"] + alpha * (v["dO"] @ wT.double().view(C, Cf).t())
    _close(pair.strided["y"], want, TOL[dtype], "y")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
def test_reflect_dgrad_border_on_channel_slices(kind, dtype):
    """jg_reflect_dgrad_border (reflect_ring_gemm_kernel + the fold): dy (lddy) and dx (lddx) strided; dx enters holding the zero-padded
    input gradient and leaves as the gradient of ReflectionPad2d(1) + conv3x3; pixels off the ring keep their bits."""
    from joligen_amd import _lib, ops

    B, H, W, Cin, Cout = 2, 16, 16, 64, 64
    d = dev()
    w = _rnd((Cout, Cin, 3, 3), dtype, 2, 1.0 / math.sqrt(9 * Cin))
    wT = w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(d)         # [Cin][3][3][Cout], flipped / transposed
    dy = _rnd((B, H, W, Cout), dtype, 24)
    grads = []
    for reflect in (False, True):
        xr = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
        xin = F.pad(xr, (1, 1, 1, 1), mode="reflect") if reflect else xr
        F.conv2d(xin, w.double(), None, 1, 0 if reflect else 1).backward(_nchw(dy))
        grads.append(xr.grad.permute(0, 2, 3, 1))
    dx0 = grads[0].to(dtype)
    ref = dx0.double() + (grads[1] - grads[0])
    ws = torch.empty(_lib.lib().jg_reflect_dgrad_border_ws_floats(B, H, W, Cin), device=d, dtype=torch.float32)
    operands = {"dy": Operand((B, H, W, Cout), dtype, "in", values=dy), "dx": Operand((B, H, W, Cin), dtype, "acc", values=dx0)}

    def launch(v):
        _lib.check(_lib.lib().jg_reflect_dgrad_border(_code(dtype), v["dy"].data_ptr(), _ld(v["dy"]), wT.data_ptr(), v["dx"].data_ptr(), _ld(v["dx"]),
                                                      ws.data_ptr(), B, H, W, Cout, Cin, 1.0, ops._st()), "jg_reflect_dgrad_border")
        return _lib.lib().jg_last_kernel().decode()

    pair = _pair(launch, operands, kind)
    su.verify(pair, exact=["dx"])
    assert pair.returns == ("reflect_ring_gemm_kernel",) * 2, pair.returns
    got = pair.strided["dx"].cpu()
    _close(got, ref, TOL[dtype], "dx")
    ring = torch.zeros(H, W, dtype=torch.bool)
    ring[[1, H - 2], :] = True
    ring[:, [1, W - 2]] = True
    assert torch.equal(got[:, ~ring], dx0[:, ~ring])                # no atomics: every target pixel is increased once, the others are not touched
    _close(got[:, ring], ref[:, ring], 1.5 * TOL[dtype], "ring pixels")       # 1.5 TOL on the border lines: test_reflect_conv_input_gradient_ring


# ======================================================================================================================================
# jg_conv2d_wgrad_tn: dy and x strided; dbias
# ======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
@pytest.mark.parametrize("case", WG_ROWS, ids=[c.id for c in WG_ROWS])
def test_wgrad_tn_on_channel_slices(case, kind, dtype):
    from joligen_amd import _lib, ops

    B, H, W, Cin, Cout, R, S, pad, stride = case.geo
    o = wgrad_opts(case)
    Ho, Wo = _conv_out_hw(H, W, R, S, pad, stride)
    real = o["real_cout"]
    dyv = _rnd((B, Ho, Wo, Cout), dtype, 12)
    dyv[..., real:] = 0                          # the zero padding of the activation layout
    xs = (B, H // 2, W // 2, Cin) if o["x_mode"] else (B, H, W, Cin)
    K = R * S * Cin
    operands = {"dy": Operand((B, Ho, Wo, Cout), dtype, "in", values=dyv), "x": Operand(xs, dtype, "in", 11),
                "dw": Operand((1, 1, real, K), torch.float32, "out" if o["store"] else "acc"),
                "db": Operand((1, 1, 1, real), torch.float32, "acc")}

    def launch(v):
        ops.wgrad_tn(v["dy"], v["x"], v["dw"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo, lddy=_ld(v["dy"]),
                     ldx=_ld(v["x"]), lddw=K, dbias=None if o["store"] else v["db"], Cin_out=Cin, Cout_out=real, splitk=case.splitk,
                     out_mode=_lib.JG_OUT_STORE_F32 if o["store"] else _lib.JG_OUT_ATOMIC_F32, dbias_scale=1.0, pad_mode=o["pad_mode"], x_mode=o["x_mode"],
                     defer=False)

    pair = _pair(launch, operands, kind, case.tune, fixed=("dw", "db"))
    if o["store"]:
        su.verify(pair, exact=["dw"], kernel=case.inst)
    else:
        su.verify(pair, approx={"dw": WGRAD_BOUND, "db": WGRAD_BOUND}, kernel=case.inst)
    ref_w, ref_b = _wgrad_reference(pair.strided["x"], pair.strided["dy"], case.geo, o)
    _close(pair.strided["dw"].reshape(real, K), ref_w[:real], TOL[dtype], f"{case.id} dw")
    if not o["store"]:
        _close(pair.strided["db"].reshape(real), ref_b[:real], TOL[dtype], f"{case.id} dbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
def test_wgrad_group_on_channel_slices(kind, dtype):
    """jg_conv2d_wgrad_tn_group: three members (64-row tile, 128-row tile, a 4x4 stride-2 geometry), each member's dy and x on its own stride"""
    from joligen_amd import ops

    geos = [(1, 1, 1024, 64, 64, 1, 1, 0, 1), (1, 1, 520, 64, 128, 1, 1, 0, 1), (2, 16, 16, 32, 128, 4, 4, 1, 2)]
    operands = {}
    for i, (B, H, W, Cin, Cout, R, S, pad, stride) in enumerate(geos):
        Ho, Wo = _conv_out_hw(H, W, R, S, pad, stride)
        operands[f"dy{i}"] = Operand((B, Ho, Wo, Cout), dtype, "in", 20 + i)
        operands[f"x{i}"] = Operand((B, H, W, Cin), dtype, "in", 30 + i)
        operands[f"dw{i}"] = Operand((1, 1, Cout, R * S * Cin), torch.float32, "acc")
        operands[f"db{i}"] = Operand((1, 1, 1, Cout), torch.float32, "acc")

    def launch(v):
        with ops.deferred_wgrads():
            for i, (B, H, W, Cin, Cout, R, S, pad, stride) in enumerate(geos):
                Ho, Wo = _conv_out_hw(H, W, R, S, pad, stride)
                ops.wgrad_tn(v[f"dy{i}"], v[f"x{i}"], v[f"dw{i}"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo,
                             lddy=_ld(v[f"dy{i}"]), ldx=_ld(v[f"x{i}"]), lddw=R * S * Cin, dbias=v[f"db{i}"], splitk=1 + i)
            assert len(ops.WGRAD_DEFER) == 3         # all three ride in the grouped launch

    pair = _pair(launch, operands, kind, fixed=[n for n in operands if n[:2] in ("dw", "db")])
    su.verify(pair, approx={n: WGRAD_BOUND for n in operands if n[:2] in ("dw", "db")})
    for i, geo in enumerate(geos):
        ref_w, ref_b = _wgrad_reference(pair.strided[f"x{i}"], pair.strided[f"dy{i}"], geo, {})
        _close(pair.strided[f"dw{i}"].reshape(ref_w.shape), ref_w, TOL[dtype], f"member {i} dw")
        _close(pair.strided[f"db{i}"].reshape(-1), ref_b, TOL[dtype], f"member {i} dbias")


# ======================================================================================================================================
# streaming passes: every operand on its own stride; float64 formulas of the header comments
# ======================================================================================================================================
STREAM_SHAPES = [(2, 16, 16, 64), (2, 16, 16, 192)]
G = 32
S1, S2 = 0.7, -1.3


def _coefs(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    ab = torch.stack([torch.rand(B, C, generator=g) + 0.5, 0.5 * torch.randn(B, C, generator=g)], -1).contiguous()
    pqr = torch.stack([torch.rand(B, C, generator=g) + 0.5, 0.1 * torch.randn(B, C, generator=g), 0.1 * torch.randn(B, C, generator=g)], -1).contiguous()
    return ab, pqr


def _bc(t, i):
    """coefficient i of [B][C][n] broadcast over NHWC"""
    return t[:, None, None, :, i].double()


def _stream_case(name, shape, dtype):
    """(operands, launch, exact outputs, approx outputs, reference(v) -> {output: float64 tensor, tolerance factor}) of one streaming pass"""
    from joligen_amd import _lib, ops

    L, dt, d = _lib.lib(), _code(dtype), dev()
    B, H, W, C = shape
    HW = H * W
    ab, pqr = _coefs(B, C, 9)
    abd, pqrd = ab.to(d), pqr.to(d)
    full, low = (B, H, W, C), (B, H // 2, W // 2, C)
    X = Operand(full, dtype, "in", 1, scale=1.3)
    st = ops._st

    def p(t):
        return t.data_ptr()

    def up(t):
        return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)

    def du_of(v, dy):
        return dy * _silu_grad(_bc(ab, 0) * v["x"] + _bc(ab, 1))

    if name == "gn_stats_ld":
        ops_ = {"x": X, "sums": Operand((B, 1, 1, 2 * C), torch.float32, "acc", unit=2)}
        run = lambda v: _lib.check(L.jg_gn_stats_ld(dt, p(v["x"]), _ld(v["x"]), p(v["sums"]), _ld(v["sums"]) // 2, B, HW, C, st()))
        ref = lambda v: {"sums": (torch.stack([v["x"].sum((1, 2)), (v["x"] ** 2).sum((1, 2))], -1).reshape(B, 1, 1, 2 * C), 1)}
        return ops_, run, [], {"sums": STATS_BOUND}, ref
    if name == "gn_apply_ld":
        ops_ = {"x": X, "y": Operand(full, dtype, "out")}
        run = lambda v: _lib.check(L.jg_gn_apply_ld(dt, p(v["x"]), _ld(v["x"]), p(abd), p(v["y"]), _ld(v["y"]), B, HW, C, SILU, st()))
        ref = lambda v: {"y": (F.silu(_bc(ab, 0) * v["x"] + _bc(ab, 1)), 1)}
        return ops_, run, ["y"], {}, ref
    if name == "gn_apply_add":
        ops_ = {"x": X, "add": Operand(full, dtype, "in", 2), "y": Operand(full, dtype, "out")}
        run = lambda v: _lib.check(L.jg_gn_apply_add(dt, p(v["x"]), _ld(v["x"]), p(abd), p(v["add"]), _ld(v["add"]), p(v["y"]), _ld(v["y"]), B, HW, C, SILU, st()))
        ref = lambda v: {"y": (F.silu(_bc(ab, 0) * v["x"] + _bc(ab, 1)) + v["add"], 1)}
        return ops_, run, ["y"], {}, ref
    if name == "gn_apply_pool":
        ops_ = {"x": X, "y": Operand(low, dtype, "out")}
        run = lambda v: _lib.check(L.jg_gn_apply_pool(dt, p(v["x"]), _ld(v["x"]), p(abd), p(v["y"]), _ld(v["y"]), B, H, W, C, SILU, 0.25, st()))
        ref = lambda v: {"y": (F.avg_pool2d(F.silu(_bc(ab, 0) * v["x"] + _bc(ab, 1)).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), 1)}
        return ops_, run, ["y"], {}, ref
    if name in ("gn_bwd_reduce_ld", "gn_bwd_reduce_ld_acc", "gn_bwd_reduce_up", "gn_bwd_reduce_up_acc"):
        is_up, acc = "_up" in name, name.endswith("_acc")
        ops_ = {"x": X, "dy": Operand(low if is_up else full, dtype, "in", 2), "red": Operand((B, 1, 1, 2 * C), torch.float32, "acc" if acc else "out")}
        fn = getattr(L, "jg_" + name)
        if is_up:
            run = lambda v: _lib.check(fn(dt, p(v["x"]), _ld(v["x"]), p(v["dy"]), _ld(v["dy"]), 0.25, p(abd), p(v["red"]), B, H, W, C, SILU, st()))
        else:
            run = lambda v: _lib.check(fn(dt, p(v["x"]), _ld(v["x"]), p(v["dy"]), _ld(v["dy"]), p(abd), p(v["red"]), B, HW, C, SILU, st()))

        def ref(v):
            du = du_of(v, 0.25 * up(v["dy"]) if is_up else v["dy"])
            return {"red": (torch.stack([du.sum((1, 2)), (du * v["x"]).sum((1, 2))], -1).reshape(B, 1, 1, 2 * C), 3)}
        return ops_, run, [], {"red": STATS_BOUND}, ref
    if name in ("gn_bwd_apply_ld", "gn_bwd_apply_up"):
        is_up = name.endswith("_up")
        ops_ = {"x": X, "dy": Operand(low if is_up else full, dtype, "in", 2), "dx": Operand(full, dtype, "out"),
                "add1": Operand(low if is_up else full, dtype, "in", 3), "add2": Operand(full, dtype, "in", 4)}
        if is_up:
            run = lambda v: _lib.check(L.jg_gn_bwd_apply_up(dt, p(v["x"]), _ld(v["x"]), p(v["dy"]), _ld(v["dy"]), 0.25, p(abd), p(pqrd), p(v["dx"]), _ld(v["dx"]),
                                                            p(v["add1"]), _ld(v["add1"]), S1, p(v["add2"]), _ld(v["add2"]), S2, B, H, W, C, SILU, st()))
        else:
            run = lambda v: _lib.check(L.jg_gn_bwd_apply_ld(dt, p(v["x"]), _ld(v["x"]), p(v["dy"]), _ld(v["dy"]), p(abd), p(pqrd), p(v["dx"]), _ld(v["dx"]),
                                                            p(v["add1"]), _ld(v["add1"]), S1, p(v["add2"]), _ld(v["add2"]), S2, B, HW, C, SILU, st()))

        def ref(v):
            du = du_of(v, 0.25 * up(v["dy"]) if is_up else v["dy"])
            a1 = up(v["add1"]) if is_up else v["add1"]
            return {"dx": (du * _bc(pqr, 0) + v["x"] * _bc(pqr, 1) + _bc(pqr, 2) + S1 * a1 + S2 * v["add2"], 3)}
        return ops_, run, ["dx"], {}, ref
    if name == "pool2x2_ld":
        ops_ = {"x": X, "y": Operand(low, dtype, "out")}
        run = lambda v: _lib.check(L.jg_pool2x2_ld(dt, p(v["x"]), _ld(v["x"]), p(v["y"]), _ld(v["y"]), B, H, W, C, 0.25, st()))
        ref = lambda v: {"y": (F.avg_pool2d(v["x"].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), 1)}
        return ops_, run, ["y"], {}, ref
    if name == "upsample2x_ld":
        ops_ = {"x": Operand(low, dtype, "in", 1), "y": Operand(full, dtype, "out")}
        run = lambda v: _lib.check(L.jg_upsample2x_ld(dt, p(v["x"]), _ld(v["x"]), p(v["y"]), _ld(v["y"]), B, H // 2, W // 2, C, 0.25, st()))
        ref = lambda v: {"y": (0.25 * up(v["x"]), 1)}
        return ops_, run, ["y"], {}, ref
    if name == "copy_channels":
        ops_ = {"x": X, "y": Operand(full, dtype, "out")}
        run = lambda v: _lib.check(L.jg_copy_channels(dt, p(v["x"]), _ld(v["x"]), 0, p(v["y"]), _ld(v["y"]), 0, B * HW, C, st()))
        ref = lambda v: {"y": (v["x"], 0)}           # 0: bit-exact
        return ops_, run, ["y"], {}, ref
    if name in ("channel_sum", "channel_sum_4096"):
        Bc = 16 if name.endswith("4096") else B      # >= 4096 pixels: the 16-byte-load form
        out0 = _rnd((1, 1, 1, C), torch.float32, 7)
        ops_ = {"x": Operand((Bc, H, W, C), dtype, "in", 1), "out": Operand((1, 1, 1, C), torch.float32, "acc", values=out0)}
        run = lambda v: _lib.check(L.jg_channel_sum(dt, p(v["x"]), _ld(v["x"]), p(v["out"]), Bc * HW, C, 0.5, st()))
        ref = lambda v: {"out": (out0.double() + 0.5 * v["x"].sum((0, 1, 2)).reshape(1, 1, 1, C), 1)}
        return ops_, run, [], {"out": STATS_BOUND}, ref
    if name == "bilinear_fwd":
        ops_ = {"x": Operand(low, dtype, "in", 1), "y": Operand(full, dtype, "out")}
        run = lambda v: _lib.check(L.jg_bilinear_fwd(dt, p(v["x"]), p(v["y"]), B, H // 2, W // 2, C, H, W, _ld(v["y"]), st()))
        ref = lambda v: {"y": (F.interpolate(v["x"].permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1), 1)}
        return ops_, run, ["y"], {}, ref
    if name == "bilinear_bwd":
        ops_ = {"dy": Operand(full, dtype, "in", 1), "dx": Operand(low, dtype, "out")}
        run = lambda v: _lib.check(L.jg_bilinear_bwd(dt, p(v["dy"]), p(v["dx"]), B, H // 2, W // 2, C, H, W, _ld(v["dy"]), st()))

        def ref(v):
            xr = torch.zeros(B, C, H // 2, W // 2, dtype=torch.float64, requires_grad=True)
            F.interpolate(xr, (H, W), mode="bilinear", align_corners=False).backward(v["dy"].permute(0, 3, 1, 2))
            return {"dx": (xr.grad.permute(0, 2, 3, 1), 1)}
        return ops_, run, ["dx"], {}, ref
    raise KeyError(name)


STREAM_PASSES = ["gn_stats_ld", "gn_apply_ld", "gn_apply_add", "gn_apply_pool", "gn_bwd_reduce_ld", "gn_bwd_reduce_ld_acc", "gn_bwd_reduce_up",
                 "gn_bwd_reduce_up_acc", "gn_bwd_apply_ld", "gn_bwd_apply_up", "pool2x2_ld", "upsample2x_ld", "copy_channels", "channel_sum",
                 "channel_sum_4096", "bilinear_fwd", "bilinear_bwd"]
# x / y of the bilinear passes and dx of its backward have no stride argument in the ABI: they stay contiguous
STREAM_FIXED = {"bilinear_fwd": ("x",), "bilinear_bwd": ("dx",), "channel_sum": ("out",), "channel_sum_4096": ("out",), "gn_bwd_reduce_ld": ("red",),
                "gn_bwd_reduce_ld_acc": ("red",), "gn_bwd_reduce_up": ("red",), "gn_bwd_reduce_up_acc": ("red",)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=["C64", "C192"])
@pytest.mark.parametrize("name", STREAM_PASSES)
def test_streaming_pass_on_channel_slices(name, shape, kind, dtype):
    operands, run, exact, approx, reference = _stream_case(name, shape, dtype)
    pair = _pair(run, operands, kind, fixed=STREAM_FIXED.get(name, ()))
    su.verify(pair, exact=exact, approx=approx)
    refs = reference({k: t.double().cpu() for k, t in pair.strided.items()})
    for out, (ref, factor) in refs.items():
        if factor == 0:
            assert torch.equal(pair.strided[out].double().cpu(), ref), f"{name} {out}: not a bit-exact copy"
        else:
            _close(pair.strided[out], ref, factor * TOL[dtype], f"{name} {out}")


# jg_gn_bwd_fused writes dx with plain stores, but from reductions its workgroups accumulate with fp32 atomics inside the same launch: two
# launches on the SAME contiguous operands already differ where a reduction's last bits flip a 16-bit rounding of dx, so bit-equality does
# not apply; dx is held to the bound of a re-ordered fp32 sum (STATS_BOUND, 1e-5) instead.  Measured run-to-run spread of dx on contiguous
# operands (these shapes, 8 launches each, largest pairwise norm-wise difference): fp16 1.0e-6 (4 elements), bf16 6.3e-8 (1 element);
# dgamma / dbeta 1.3e-7 -- all inside the borrowed bound, which therefore stays.


def _gn_one_launch_problem(C, form, up, dtype):
    """operands and launch of jg_gn_bwd_apply_fc / jg_gn_bwd_fused on real GroupNorm(32) + SiLU coefficients; launch appends (dgamma, dbeta)"""
    from joligen_amd import _lib, ops

    L, dt, d = _lib.lib(), _code(dtype), dev()
    B, H, W = 2, 16, 16
    HW, cpg = H * W, C // G
    g = torch.Generator().manual_seed(11)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    full, low = (B, H, W, C), (B, H // 2, W // 2, C)
    xv = (_rnd(full, torch.float32, 1) * 1.3 + 0.2).to(dtype)
    dyv = _rnd(low if up else full, dtype, 2)
    xf = xv.double()
    mean = xf.view(B, HW, G, cpg).mean(dim=(1, 3))
    rstd = (xf.view(B, HW, G, cpg).var(dim=(1, 3), unbiased=False) + 1e-5).rsqrt()
    a0 = rstd.repeat_interleave(cpg, 1) * gamma.double()
    b0 = beta.double() - mean.repeat_interleave(cpg, 1) * a0
    ab = torch.stack([a0, b0], -1).float().contiguous()
    mr = torch.stack([mean, rstd], -1).float().contiguous()
    dysc = 0.25 if up else 1.0
    # the reductions jg_gn_bwd_apply_fc reads, evaluated once on the host: both launches of a pair then see the same bits (the device
    # reduction passes, fp32 atomics, have their own rows in STREAM_PASSES)
    dyf = dysc * (dyv.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if up else dyv.double())
    du = dyf * _silu_grad(_bc(ab, 0) * xf + _bc(ab, 1))
    red_host = torch.stack([du.sum((1, 2)), (du * xf).sum((1, 2))], -1).float().contiguous()
    abd, mrd, gd, bd = ab.to(d), mr.to(d), gamma.to(d), beta.to(d)
    operands = {"x": Operand(full, dtype, "in", values=xv), "dy": Operand(low if up else full, dtype, "in", values=dyv), "dx": Operand(full, dtype, "out"),
                "add1": Operand(low if up else full, dtype, "in", 3), "add2": Operand(full, dtype, "in", 4)}
    grads = []

    def launch(v):
        dgamma, dbeta = torch.zeros(C, device=d), torch.zeros(C, device=d)
        p = lambda t: t.data_ptr()
        tail = (p(gd), p(bd), None, 0, p(mrd), p(dgamma), p(dbeta), None, 0, G, p(v["dx"]), _ld(v["dx"]), p(v["add1"]), _ld(v["add1"]), S1, p(v["add2"]),
                _ld(v["add2"]), S2, B, H, W, C, SILU, ops._st())
        if form == "fused":
            red = torch.zeros(B, C, 2, device=d)
            cnt = torch.zeros(B, 2, device=d, dtype=torch.int32)
            _lib.check(L.jg_gn_bwd_fused(dt, up, p(v["x"]), _ld(v["x"]), p(v["dy"]), _ld(v["dy"]), dysc, p(abd), p(red), p(cnt), p(ops.gn_status(d)), *tail),
                       "jg_gn_bwd_fused")
        else:
            red = red_host.to(d)
            _lib.check(L.jg_gn_bwd_apply_fc(dt, up, p(v["x"]), _ld(v["x"]), p(v["dy"]), _ld(v["dy"]), dysc, p(abd), p(red), *tail), "jg_gn_bwd_apply_fc")
        torch.cuda.synchronize()
        grads.append((dgamma.cpu(), dbeta.cpu()))

    return operands, launch, grads, gamma, beta


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
@pytest.mark.parametrize("up", [0, 1], ids=["full", "pooled"])
@pytest.mark.parametrize("form", ["fc", "fused"])
@pytest.mark.parametrize("C", [64, 192])
def test_gn_bwd_one_launch_forms_on_channel_slices(C, form, up, kind, dtype):
    """jg_gn_bwd_apply_fc and jg_gn_bwd_fused, both `up` values: x, dy, dx, add1 and add2 each on its own stride; against float64 autograd of
    SiLU(GroupNorm(x)) (through AvgPool2d for up = 1) plus the two addends; dgamma / dbeta as well."""
    from joligen_amd import ops

    operands, launch, grads, gamma, beta = _gn_one_launch_problem(C, form, up, dtype)
    pair = _pair(launch, operands, kind)
    ops.check_gn_status()
    if form == "fc":
        su.verify(pair, exact=["dx"])
    else:
        su.verify(pair, approx={"dx": STATS_BOUND})
    v = {k: t.double().cpu() for k, t in pair.strided.items()}
    xr = v["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.silu(F.group_norm(xr, G, gr, br, 1e-5))
    if up:
        y = F.avg_pool2d(y, 2)
    y.backward(v["dy"].permute(0, 3, 1, 2))
    a1 = v["add1"].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if up else v["add1"]
    want = xr.grad.permute(0, 2, 3, 1) + S1 * a1 + S2 * v["add2"]
    _close(pair.strided["dx"], want, 3 * TOL[dtype], f"{form} up={up} dx")
    for dgamma, dbeta in grads:
        _close(dgamma, gr.grad, 3 * TOL[dtype], "dgamma")
        _close(dbeta, br.grad, 3 * TOL[dtype], "dbeta")
    # fp32 atomics over the images in another order
    assert su.relerr(grads[1][0], grads[0][0]) < STATS_BOUND and su.relerr(grads[1][1], grads[0][1]) < STATS_BOUND
