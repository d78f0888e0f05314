"""Exact-integer tests of every convolution, input-gradient and weight-gradient kernel instance (tests/kernel_cases.py), and the first direct
test of jg_refresh_weights.

The tests that guard these kernels elsewhere compare with a float reference under ONE norm-wise bound (1e-3 fp16, 8e-3 bf16): one wrong
element among 131072, a tap dropped on a border row, a halo pixel mirrored from the wrong column, a K-step skipped at a tile edge or a split-K
slice overlapping its neighbour all stay below it (tests/test_exact_integer_host.py shows that on a CPU stand-in).  Here the operands are small
integers (kernel_cases.py: the recipe and its preconditions), so every product, every fp32 partial sum in any order, the epilogue and the
16-bit result are exact, and each launch is held to the float64 reference BIT FOR BIT, element by element, with no tolerance:
  1. y / dw / dbias / dx equal the reference rounded to the output type (strided_util.assert_bit_equal; it reports count and positions);
  2. canaries intact (NaN around inputs, bit patterns around outputs), outputs fully written, no NaN (strided_util.verify_once);
  3. fused statistics (sum y, sum y^2), summed over the slots in float64, equal the reference sums;
  4. stats_mode 1: (sum du, sum du gx) with integer (a, b) tables, act NONE / ReLU;
  5. split-K rows also run with JG_CONV_SPLITK 0: both equal the reference, hence each other.
Every launch runs under the row's tuning switches and jg_last_kernel() must name the row's instance.
"""
import pytest
import torch
import torch.nn.functional as F

import kernel_cases as kc
import strided_util as su
from kernel_cases import NSLOT
from strided_util import Operand

pytestmark = pytest.mark.gpu

DTYPES = kc.DTYPES
IDS = ["fp16", "bf16"]
ACT_NONE, ACT_RELU = 0, 2
ACTS = [ACT_NONE, ACT_RELU]
ACT_IDS = ["none", "relu"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _ld(v):
    assert v.stride(-1) == 1
    return v.stride(-2)


def _code(dtype):
    from joligen_amd import _lib

    return _lib.JG_F16 if dtype == torch.float16 else _lib.JG_BF16


def _once(launch, operands, tuning=None):
    return su.run_once(launch, operands, tuning=tuning, device=dev())


def _nhwc(ref_nchw):
    return ref_nchw.permute(0, 2, 3, 1)


def _act(u, act):
    return F.relu(u) if act == ACT_RELU else u


def _act_grad(u, act):
    return (u > 0).double() if act == ACT_RELU else torch.ones_like(u)


def _bc(t, i):
    """coefficient i of [B][C][n] broadcast over NHWC"""
    return t[:, None, None, :, i].double()


# ======================================================================================================================================
# jg_conv2d_nt: every row of the tables
# ======================================================================================================================================
def _conv_weights(case, dtype, prob):
    """device weights of the launch and their row stride: the 16-bit cast of the integer master weights, or their fold"""
    from joligen_amd import _lib, ops

    B, H, W, Cin, Cout, R, S, pad, stride = case.geo
    d, o = dev(), prob.o
    if o["x_mode"] == 2:
        wd = torch.empty((4, Cout, 2, 2, Cin), device=d, dtype=dtype)
        _lib.check(_lib.lib().jg_subpixel_fold(_code(dtype), prob.w.to(d).data_ptr(), wd.data_ptr(), Cout, Cin, ops._st()), "jg_subpixel_fold")
        return wd, 4 * Cin
    if o["y_mode"] == 2:
        # prob.w is the weight tensor in the sense of the launch, [Cout = C_in of the layer][3][3][Cin = C_out of the layer]: the flipped /
        # transposed copy of the forward layer's master weights, from which jg_subpixel_fold_pair writes the launch's weights (its outT)
        wf32 = prob.w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(d)         # [C_out][3][3][C_in]
        wf = torch.empty((4, Cin, 2, 2, Cout), device=d, dtype=dtype)
        wfT = torch.empty((4, Cout, 2, 2, Cin), device=d, dtype=dtype)
        _lib.check(_lib.lib().jg_subpixel_fold_pair(_code(dtype), wf32.data_ptr(), wf.data_ptr(), wfT.data_ptr(), Cin, Cout, ops._st()), "jg_subpixel_fold_pair")
        return wfT, 4 * Cin
    return prob.w.to(dtype).to(d), R * S * Cin


def _conv_operands(case, dtype, prob):
    B, Cout = case.geo[0], case.geo[4]
    xs, ys, rs = kc.conv_shapes(case)
    operands = {"x": Operand(xs, dtype, "in", values=prob.x), "y": Operand(ys, dtype, "out")}
    if prob.o["res"]:
        operands["res"] = Operand(rs, dtype, "in", values=prob.res)
    if prob.o["stats"]:
        operands["stats"] = Operand((B, NSLOT, 1, 2 * Cout), torch.float32, "acc", unit=2)
    return operands


def _conv_launcher(case, dtype, prob, gn_reduce=None):
    from joligen_amd import ops

    B, H, W, Cin, Cout, R, S, pad, stride = case.geo
    Ho, Wo = kc.conv_out_hw(H, W, R, S, pad, stride)
    o = prob.o
    wd, ldw = _conv_weights(case, dtype, prob)
    bd = None if prob.bias is None else prob.bias.to(dev())

    def launch(v):
        st = v.get("stats")
        ops.conv_nt(v["x"], wd, v["y"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo, ldx=_ld(v["x"]), ldw=ldw,
                    ldy=_ld(v["y"]), bias=bd, res=v.get("res"), ldres=_ld(v["res"]) if "res" in v else 0, alpha=kc.ALPHA, res_scale=kc.RES_SCALE,
                    stats=st, ldstats=_ld(st) // 2 if st is not None else 0, stats_slots=NSLOT if st is not None else 1, pad_mode=o["pad_mode"],
                    res_mode=o["res_mode"], x_mode=o["x_mode"], y_mode=o["y_mode"],
                    gn_reduce=None if gn_reduce is None else (v["gx"], _ld(v["gx"]), gn_reduce[0], gn_reduce[1]))

    return launch


def _stats_of(single, B, Cout):
    return single.views["stats"].double().cpu().sum(1).reshape(B, Cout, 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", kc.CONV_ROWS_ALL, ids=[c.id for c in kc.CONV_ROWS_ALL])
def test_conv_nt_exact(case, dtype):
    prob = kc.int_conv_problem(case)
    kc.check_conv_preconditions(case, prob)
    B, Cout = case.geo[0], case.geo[4]
    launch = _conv_launcher(case, dtype, prob)
    tunings = [dict(case.tune)]
    if case.inst.endswith("+splitK"):
        tunings.append(dict(case.tune, JG_CONV_SPLITK=0))
    for tune in tunings:
        one = _once(launch, _conv_operands(case, dtype, prob), tune)
        if tune.get("JG_CONV_SPLITK", 1) == 0:
            assert one.kernel.startswith("conv_nt_glds_kernel") and "splitK" not in one.kernel, one.kernel        # one slice (on whichever tile)
            su.verify_once(one)
        else:
            su.verify_once(one, kernel=case.inst)
        su.assert_bit_equal(one.views["y"], _nhwc(prob.ref), f"{case.id} y ({one.kernel})")
        if prob.o["stats"]:
            st = _stats_of(one, B, Cout)
            ref = prob.ref
            assert torch.equal(st[..., 0], ref.sum((2, 3))), f"{case.id}: fused sum y off by at most {float((st[..., 0] - ref.sum((2, 3))).abs().max())}"
            assert torch.equal(st[..., 1], (ref * ref).sum((2, 3))), \
                f"{case.id}: fused sum y^2 off by at most {float((st[..., 1] - (ref * ref).sum((2, 3))).abs().max())}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k,Cin,Cout,H,W", [(4, 64, 128, 32, 64), (3, 128, 64, 32, 32)], ids=["4x4", "3x3"])
def test_transposed_fold_conv_exact(k, Cin, Cout, H, W, dtype):
    """jg_transposed_fold + x_mode 2: the input gradient of a stride-2 convolution (kernel 4 / 3, padding 1; the first two PHASE_TCONV_CASES of
    test_gpu_0_ops.py) in the four-phase form, with bias and residual, against float64 autograd.  The fold is a rearrangement of the integer
    working weights: no arithmetic, exact."""
    from joligen_amd import _lib, ops

    B, d = 2, dev()
    p = kc.density(4 * Cout)                  # at most 2 x 2 taps of the strided kernel reach one input pixel
    w = kc.ternary((Cout, k, k, Cin), p, 181)                     # the strided convolution's weights [Cout][R][S][Cin]
    dy = kc.ternary((B, H // 2, W // 2, Cout), p, 182)
    bias, res = kc.integers((Cin,), -3, 3, 183), kc.integers((B, H, W, Cin), -4, 4, 184)
    xr = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double().permute(0, 3, 1, 2), None, 2, 1).backward(kc.nchw(dy))
    ref = kc.ALPHA * xr.grad.permute(0, 2, 3, 1) + bias.double() + kc.RES_SCALE * res.double()
    for dt in DTYPES:
        assert kc.representable(ref, dt)
    wT = w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(dtype).to(d)         # [Cin][R][S][Cout]: wT[n][R-1-r][S-1-s][c] = w[c][r][s][n]
    wf = torch.empty((4, Cin, 2, 2, Cout), device=d, dtype=dtype)
    _lib.check(_lib.lib().jg_transposed_fold(_code(dtype), wT.data_ptr(), wf.data_ptr(), Cin, Cout, k, k, 1, ops._st()), "jg_transposed_fold")
    bd = bias.to(d)
    operands = {"x": Operand((B, H // 2, W // 2, Cout), dtype, "in", values=dy), "y": Operand((B, H, W, Cin), dtype, "out"),
                "res": Operand((B, H, W, Cin), dtype, "in", values=res)}

    def launch(v):
        ops.conv_nt(v["x"], wf, v["y"], B=B, H=H, W=W, Cin=Cout, Cout=Cin, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=_ld(v["x"]), ldw=4 * Cout,
                    ldy=_ld(v["y"]), bias=bd, res=v["res"], ldres=_ld(v["res"]), alpha=kc.ALPHA, res_scale=kc.RES_SCALE, x_mode=2)

    one = _once(launch, operands)
    su.verify_once(one, kernel="conv3x3_halo_kernel<subpixel>")
    su.assert_bit_equal(one.views["y"], ref, "dx")


# stats_mode 1 (GroupNorm-backward reductions in the input-gradient epilogue).  conv3x3_p64_kernel does not take them: jg_conv_p64_try
# (csrc/conv_p64.hip) returns false for stats_mode != 0, so a launch with JG_PERSIST64 forced at a Cin == 64 shape is served by the halo-resident
# kernel -- asserted here, on the first forced P64 geometry -- next to a halo row of its own.
GN_REDUCE_ROWS = [
    kc.ConvCase("halo-cfg1-gn_reduce", "conv3x3_halo_kernel<128-wide,4 waves>", (2, 16, 16, 192, 256, 3, 3, 1, 1), {"JG_HALO_CFG": 1},
                dict(bias=False, res=False, stats=True)),
    kc.ConvCase("p64-forced-gn_reduce", "conv3x3_halo_kernel<64-wide>", (2, 32, 48, 64, 64, 3, 3, 1, 1), {"JG_PERSIST64": 2},
                dict(bias=False, res=False, stats=True)),
    # the generic kernel's LDS-transposed epilogue (a 1x1 below the streaming size; whole 128-pixel tiles per image)
    kc.ConvCase("glds128-gn_reduce", kc.G128, (2, 16, 16, 64, 128, 1, 1, 0, 1), {}, dict(bias=False, res=False, stats=True)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("act", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("case", GN_REDUCE_ROWS, ids=[c.id for c in GN_REDUCE_ROWS])
def test_conv_nt_gn_reduce_exact(case, act, dtype):
    """du = y * act'(a gx + b) with an integer (a, b) table in [-2, 2] and integer gx: (sum du, sum du gx) are sums of multiples of 0.5"""
    prob = kc.int_conv_problem(case)
    kc.check_conv_preconditions(case, prob)
    B, Cout = case.geo[0], case.geo[4]
    ys = kc.conv_shapes(case)[1]
    gx = kc.integers(ys, -2, 2, 121)
    ab = kc.integers((B, Cout, 2), -2, 2, 122)
    y = _nhwc(prob.ref)
    du = y * _act_grad(_bc(ab, 0) * gx.double() + _bc(ab, 1), act)
    want = torch.stack([du.sum((1, 2)), (du * gx.double()).sum((1, 2))], -1)
    assert float((2 * du.abs()).sum((1, 2)).max()) < kc.TWO24 and float((2 * (du * gx.double()).abs()).sum((1, 2)).max()) < kc.TWO24       # (ii)
    operands = _conv_operands(case, dtype, prob)
    operands["gx"] = Operand(ys, dtype, "in", values=gx)
    one = _once(_conv_launcher(case, dtype, prob, gn_reduce=(ab.to(dev()), act)), operands, case.tune)
    su.verify_once(one, kernel=case.inst)
    su.assert_bit_equal(one.views["y"], y, f"{case.id} y")
    st = _stats_of(one, B, Cout)
    assert torch.equal(st, want), f"{case.id}: (sum du, sum du gx) off by at most {float((st - want).abs().max())}"


# ======================================================================================================================================
# jg_conv2d_wgrad_tn and jg_conv2d_wgrad_tn_group
# ======================================================================================================================================
_WG_CACHE = {}


def _wgrad_problem(key, geo, o, seed=0):
    """(IntWgrad, dw reference, dbias reference), kept for the second dtype of the row"""
    if key not in _WG_CACHE:
        prob = kc.int_wgrad_problem(geo, o, seed)
        kc.check_wgrad_preconditions(key, prob)
        if len(_WG_CACHE) >= 3:
            _WG_CACHE.clear()
        _WG_CACHE[key] = (prob,) + kc.int_wgrad_reference(prob, geo)
    return _WG_CACHE[key]


def _wgrad_operands(prob, geo, dtype, tag=""):
    B, H, W, Cin, Cout, R, S, pad, stride = geo
    Ho, Wo = kc.conv_out_hw(H, W, R, S, pad, stride)
    real = prob.o.get("real_cout", Cout)
    return {f"dy{tag}": Operand((B, Ho, Wo, Cout), dtype, "in", values=prob.dy), f"x{tag}": Operand(tuple(prob.x.shape), dtype, "in", values=prob.x),
            f"dw{tag}": Operand((1, 1, real, R * S * Cin), torch.float32, "out" if prob.o.get("store") else "acc", values=prob.dw0),
            f"db{tag}": Operand((1, 1, 1, real), torch.float32, "acc", values=prob.db0)}


def _wgrad_call(v, prob, geo, splitk, tag="", defer=False):
    from joligen_amd import _lib, ops

    B, H, W, Cin, Cout, R, S, pad, stride = geo
    Ho, Wo = kc.conv_out_hw(H, W, R, S, pad, stride)
    o = prob.o
    store = bool(o.get("store"))
    ops.wgrad_tn(v[f"dy{tag}"], v[f"x{tag}"], v[f"dw{tag}"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo,
                 lddy=_ld(v[f"dy{tag}"]), ldx=_ld(v[f"x{tag}"]), lddw=R * S * Cin, dbias=None if store else v[f"db{tag}"], Cin_out=Cin,
                 Cout_out=o.get("real_cout", Cout), splitk=splitk, alpha=kc.ALPHA, out_mode=_lib.JG_OUT_STORE_F32 if store else _lib.JG_OUT_ATOMIC_F32,
                 dbias_scale=kc.DBIAS_SCALE, pad_mode=o.get("pad_mode", 0), x_mode=o.get("x_mode", 0), defer=defer)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", kc.WG_ROWS_ALL, ids=[c.id for c in kc.WG_ROWS_ALL])
def test_wgrad_tn_exact(case, dtype):
    """STORE rows are exact by plain stores, ATOMIC rows because every partial sum is a multiple of 0.5 below 2^24; dw and dbias start from
    non-zero integers the launch has to add to"""
    prob, ref_w, ref_b = _wgrad_problem(case.id, case.geo, kc.wgrad_opts(case))
    one = _once(lambda v: _wgrad_call(v, prob, case.geo, case.splitk), _wgrad_operands(prob, case.geo, dtype), case.tune)
    su.verify_once(one, kernel=case.inst)
    su.assert_bit_equal(one.views["dw"].reshape(ref_w.shape), ref_w, f"{case.id} dw")
    # a STORE launch takes no dbias: its start values stay
    su.assert_bit_equal(one.views["db"].reshape(1, -1), (prob.db0.double() if prob.o["store"] else ref_b).reshape(1, -1), f"{case.id} dbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wgrad_group_exact(dtype):
    """the three members of test_wgrad_group_on_channel_slices in one grouped launch, split-K 1, 2 and 3"""
    from joligen_amd import ops

    probs = [_wgrad_problem(f"group{i}", geo, {}, seed=10 * i) for i, geo in enumerate(kc.WG_GROUP_GEOS)]
    operands = {}
    for i, geo in enumerate(kc.WG_GROUP_GEOS):
        operands.update(_wgrad_operands(probs[i][0], geo, dtype, tag=str(i)))

    def launch(v):
        with ops.deferred_wgrads():
            for i, geo in enumerate(kc.WG_GROUP_GEOS):
                _wgrad_call(v, probs[i][0], geo, 1 + i, tag=str(i), defer=True)
            assert len(ops.WGRAD_DEFER) == 3         # all three ride in the grouped launch

    one = _once(launch, operands)
    su.verify_once(one)
    for i, (prob, ref_w, ref_b) in enumerate(probs):
        su.assert_bit_equal(one.views[f"dw{i}"].reshape(ref_w.shape), ref_w, f"member {i} dw")
        su.assert_bit_equal(one.views[f"db{i}"].reshape(1, -1), ref_b.reshape(1, -1), f"member {i} dbias")


# ======================================================================================================================================
# jg_conv1x1_gn_apply / jg_conv1x1_gn_bwd_apply: the streaming shape (1, 256, 256, 64 -> 128) and the reverse direction
# ======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("act", ACTS, ids=ACT_IDS)
def test_conv1x1_gn_apply_exact(act, dtype):
    from joligen_amd import ops

    B, H, W, Cin, Cout = 1, 256, 256, 64, 128
    d = dev()
    p = kc.density(Cin)
    x, w = kc.ternary((B, H, W, Cin), p, 131), kc.ternary((Cout, Cin), p, 132)
    bias = kc.integers((Cout,), -3, 3, 133)
    ab = kc.integers((B, Cin, 2), -2, 2, 134)
    want_y = kc.ALPHA * (x.double() @ w.double().t()) + bias.double()
    want_n = _act(_bc(ab, 0) * x.double() + _bc(ab, 1), act)
    for dt in DTYPES:
        assert kc.representable(want_y, dt) and kc.representable(want_n, dt)
    wd, bd, abd = w.to(dtype).to(d), bias.to(d), ab.to(d)
    operands = {"x": Operand((B, H, W, Cin), dtype, "in", values=x), "y": Operand((B, H, W, Cout), dtype, "out"), "yn": Operand((B, H, W, Cin), dtype, "out")}

    def launch(v):
        ok = ops.conv_nt(v["x"], wd, v["y"], B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldx=_ld(v["x"]), ldw=Cin,
                         ldy=_ld(v["y"]), bias=bd, alpha=kc.ALPHA, apply=(abd, v["yn"], _ld(v["yn"]), act))
        assert ok is not False

    one = _once(launch, operands)
    su.verify_once(one, kernel=kc.GN_APPLY_KERNEL)
    su.assert_bit_equal(one.views["y"], want_y, "y")
    su.assert_bit_equal(one.views["yn"], want_n, "y_norm")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("act", ACTS, ids=ACT_IDS)
def test_conv1x1_gn_bwd_apply_exact(act, dtype):
    """y = alpha dO W^T + du P + gx Q + R + scale1 add1 + scale2 add2, du = gdy act'(a gx + b): integer tables, scale1 = 2, scale2 = -1"""
    from joligen_amd import ops

    B, H, W, Cf, C = 1, 256, 256, 128, 64         # input gradient of a 1x1 convolution 64 -> 128
    d = dev()
    p = kc.density(Cf)
    dO, wT = kc.ternary((B, H, W, Cf), p, 141), kc.ternary((C, Cf), p, 142)
    gx, gdy = kc.integers((B, H, W, C), -2, 2, 143), kc.integers((B, H, W, C), -2, 2, 144)
    add1, add2 = kc.integers((B, H, W, C), -4, 4, 145), kc.integers((B, H, W, C), -4, 4, 146)
    ab, pqr = kc.integers((B, C, 2), -2, 2, 147), kc.integers((B, C, 3), -2, 2, 148)
    s1, s2 = 2.0, -1.0
    du = gdy.double() * _act_grad(_bc(ab, 0) * gx.double() + _bc(ab, 1), act)
    want = (du * _bc(pqr, 0) + gx.double() * _bc(pqr, 1) + _bc(pqr, 2) + s1 * add1.double() + s2 * add2.double()
            + kc.ALPHA * (dO.double() @ wT.double().t()))
    for dt in DTYPES:
        assert kc.representable(want, dt)
    wd, abd, pqrd = wT.to(dtype).to(d), ab.to(d), pqr.to(d)
    full = (B, H, W, C)
    operands = {"dO": Operand((B, H, W, Cf), dtype, "in", values=dO), "y": Operand(full, dtype, "out"), "gx": Operand(full, dtype, "in", values=gx),
                "gdy": Operand(full, dtype, "in", values=gdy), "add1": Operand(full, dtype, "in", values=add1), "add2": Operand(full, dtype, "in", values=add2)}

    def launch(v):
        ok = ops.conv_nt(v["dO"], wd, v["y"], B=B, H=H, W=W, Cin=Cf, Cout=C, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldx=_ld(v["dO"]), ldw=Cf,
                         ldy=_ld(v["y"]), alpha=kc.ALPHA, gn_bwd_apply=(v["gx"], v["gdy"], abd, pqrd, v["add1"], s1, v["add2"], s2, act))
        assert ok is not False

    one = _once(launch, operands)
    su.verify_once(one, kernel=kc.GN_BWD_APPLY_KERNEL)
    su.assert_bit_equal(one.views["y"], want, "y")


# ======================================================================================================================================
# jg_reflect_dgrad_border, jg_conv_dgrad_gather, jg_tapsum7 / jg_tapspread7
# ======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (2, 48, 16, 192, 128)], ids=lambda s: "x".join(map(str, s)))
def test_reflect_dgrad_border_exact(shape, dtype):
    """dx enters holding the zero-padded input gradient and leaves as exactly what float64 autograd of F.pad(reflect) + conv2d gives.  A ring
    pixel sums up to four folded contributions: the density of the four-output rows (12 / sqrt(K))"""
    from joligen_amd import _lib, ops

    B, H, W, Cin, Cout = shape
    d = dev()
    p = kc.density(9 * Cout, four_outputs=True)
    w = kc.ternary((Cout, Cin, 3, 3), p, 151)
    dy = kc.ternary((B, H, W, Cout), p, 152)
    grads = []
    for reflect in (False, True):
        xr = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
        xin = F.pad(xr, (1, 1, 1, 1), mode="reflect") if reflect else xr
        F.conv2d(xin, w.double(), None, 1, 0 if reflect else 1).backward(kc.nchw(dy))
        grads.append(xr.grad.permute(0, 2, 3, 1))
    dx0, ref = grads
    for dt in DTYPES:
        assert kc.representable(dx0, dt) and kc.representable(ref, dt)
    wT = w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(dtype).to(d)         # [Cin][3][3][Cout], flipped / transposed
    ws = torch.empty(_lib.lib().jg_reflect_dgrad_border_ws_floats(B, H, W, Cin), device=d, dtype=torch.float32)
    operands = {"dy": Operand((B, H, W, Cout), dtype, "in", values=dy), "dx": Operand((B, H, W, Cin), dtype, "acc", values=dx0)}

    def launch(v):
        _lib.check(_lib.lib().jg_reflect_dgrad_border(_code(dtype), v["dy"].data_ptr(), _ld(v["dy"]), wT.data_ptr(), v["dx"].data_ptr(), _ld(v["dx"]),
                                                      ws.data_ptr(), B, H, W, Cout, Cin, 1.0, ops._st()), "jg_reflect_dgrad_border")
        return _lib.lib().jg_last_kernel().decode()

    one = _once(launch, operands)
    su.verify_once(one)
    assert one.ret == kc.REFLECT_RING_KERNEL, one.ret
    assert not torch.equal(ref, dx0)
    su.assert_bit_equal(one.views["dx"], ref, "dx")


IMAGE_DGRAD_CASES = [      # IMAGE_DGRAD_CASES of test_gpu_0_ops.py
    ("7x7-s4-p3", dict(k=7, stride=4, padding=3, Cout=32, H=32, W=48)),
    ("4x4-s2-p1", dict(k=4, stride=2, padding=1, Cout=64, H=16, W=24)),
    ("3x3-s2-p1", dict(k=3, stride=2, padding=1, Cout=32, H=18, W=14)),
    ("7x7-s4-p3-ragged", dict(k=7, stride=4, padding=3, Cout=32, H=30, W=26)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", IMAGE_DGRAD_CASES, ids=[c[0] for c in IMAGE_DGRAD_CASES])
def test_conv_dgrad_gather_exact(case, dtype):
    """input gradient of a strided convolution onto an image (4 live channels of an 8-channel pixel): channels 4 .. 7 are exactly zero"""
    from joligen_amd import _lib, ops

    c = case[1]
    B, H, W, Cout, k, stride, pad = 2, c["H"], c["W"], c["Cout"], c["k"], c["stride"], c["padding"]
    Ho, Wo = kc.conv_out_hw(H, W, k, k, pad, stride)
    d = dev()
    p = kc.density(((k + stride - 1) // stride) ** 2 * Cout)            # ceil(k / s)^2 taps reach an input pixel
    w = kc.ternary((Cout, k, k, 8), p, 161)
    w[..., 4:] = 0
    dy = kc.ternary((B, Ho, Wo, Cout), p, 162)
    xr = torch.zeros(B, 8, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double().permute(0, 3, 1, 2), None, stride, pad).backward(kc.nchw(dy))
    ref = kc.ALPHA * xr.grad.permute(0, 2, 3, 1)
    assert float(ref[..., 4:].abs().max()) == 0.0 and float(ref[..., :4].abs().max()) > 0
    for dt in DTYPES:
        assert kc.representable(ref, dt)
    wd = w.to(dtype).to(d)
    operands = {"dy": Operand((B, Ho, Wo, Cout), dtype, "in", values=dy), "dx": Operand((B, H, W, 8), dtype, "out")}

    def launch(v):
        _lib.check(_lib.lib().jg_conv_dgrad_gather(_code(dtype), v["dy"].data_ptr(), wd.data_ptr(), v["dx"].data_ptr(), B, H, W, Ho, Wo, Cout, k, k,
                                                   stride, pad, kc.ALPHA, ops._st()), "jg_conv_dgrad_gather")

    one = _once(launch, operands)
    su.verify_once(one)
    su.assert_bit_equal(one.views["dx"], ref, "dx")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tapsum7_tapspread7_exact(dtype):
    """JG_ACT_NONE at (1, 32, 48): pure index sums.  Columns 28 .. 31 of z and channels 4 .. 7 of dout hold non-zero integers nobody may read"""
    from joligen_amd import _lib, ops

    B, H, W, Hz = 1, 32, 48, 40
    d = dev()
    z = kc.integers((B, H + 6, W, 32), -4, 4, 171)
    bias = kc.integers((8,), -3, 3, 172)
    want = torch.zeros(B, H, W, 8, dtype=torch.float64)
    for ky in range(7):
        want[..., :4] += z[:, ky:ky + H, :, ky * 4:ky * 4 + 4].double()
    want[..., :4] += bias[:4].double()
    dout = kc.integers((B, H, W, 8), -4, 4, 173)
    want_z = torch.zeros(B, Hz, W, 32, dtype=torch.float64)
    for ky in range(7):
        want_z[:, ky:ky + H, :, ky * 4:ky * 4 + 4] = dout[..., :4].double()
    want_zm = torch.zeros(B, H + 6, W + 12, 32, dtype=torch.float64)
    want_zm[:, :, 6:6 + W] = want_z[:, :H + 6]
    bd = bias.to(d)
    operands = {"z": Operand((B, H + 6, W, 32), dtype, "in", values=z), "out": Operand((B, H, W, 8), dtype, "out"),
                "dout": Operand((B, H, W, 8), dtype, "in", values=dout), "dz": Operand((B, Hz, W, 32), dtype, "out"),
                "dzm": Operand((B, H + 6, W + 12, 32), dtype, "out")}

    def launch(v):
        L, dt = _lib.lib(), _code(dtype)
        _lib.check(L.jg_tapsum7(dt, v["z"].data_ptr(), bd.data_ptr(), v["out"].data_ptr(), B, H, W, ACT_NONE, ops._st()), "jg_tapsum7")
        _lib.check(L.jg_tapspread7(dt, v["dout"].data_ptr(), None, v["dz"].data_ptr(), v["dzm"].data_ptr(), B, H, W, Hz, ACT_NONE, ops._st()), "jg_tapspread7")

    one = _once(launch, operands)
    su.verify_once(one)
    su.assert_bit_equal(one.views["out"], want, "tapsum7 out")
    su.assert_bit_equal(one.views["dz"], want_z, "tapspread7 dz")
    su.assert_bit_equal(one.views["dzm"], want_zm, "tapspread7 dzm")


# ======================================================================================================================================
# jg_refresh_weights
# ======================================================================================================================================
# (Cout, R * S, Cin, CoutPad, CinPad, transposed image wanted)
REFRESH_LAYERS = [
    (3, 49, 64, 8, 64, True),           # the head: Cout 3 -> 8
    (64, 16, 3, 64, 8, True),           # Cin 3 -> 8
    (316, 1, 256, 320, 256, True),      # ragged inside a 64 x 64 staging tile
    (192, 9, 72, 192, 72, True),        # neither a multiple of 64
    (328, 49, 320, 328, 320, True),     # 6 x 5 x 49 = 1470 staging tiles on the 1152 workgroups of a layer (csrc/optim.hip): the grid-stride trip
    (64, 9, 64, 64, 64, False),         # dstT_off < 0: no transposed image
]
REFRESH_GRID_X = 1152                   # dim3 grid(1152, nlayers) in jg_refresh_weights


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refresh_weights(dtype):
    """One launch over a descriptor table: w16 [CoutPad][RS][CinPad] = cast(p) padded with +0, w16T [CinPad][RS][CoutPad] its flipped /
    transposed image (w16T[ci][RS - 1 - rs][co] = w16[co][rs][ci]), both bit-equal to p.to(dtype) from randn masters (the cast rounds); every
    element outside the layers' regions -- the 8-element gaps between them, the region a skipped transpose would have had, the guards -- keeps
    its canary."""
    from joligen_amd import _lib, ops

    d = dev()
    assert max(-(-cop // 64) * -(-cip // 64) * rs for _, rs, _, cop, cip, _ in REFRESH_LAYERS) > REFRESH_GRID_X
    idt = torch.int16
    canary = su._patterns(dtype)[0]
    GAP = 8
    desc, masters, src, dst = [], [], 0, GAP
    for cout, rs, cin, cop, cip, tr in REFRESH_LAYERS:
        masters.append(torch.randn((cout, rs, cin), generator=torch.Generator().manual_seed(180 + len(desc))))
        desc.append([src, dst, dst if tr else -1, cout, rs, cin, cop, cip])
        src += cout * rs * cin
        dst += cop * rs * cip + GAP
    total = dst
    pbuf, pv = su.make_slice((1, 1, 1, src), torch.float32, 0, left=0, right=0, guard=3, role="in", values=torch.cat([m.reshape(-1) for m in masters]), device=d)
    wbuf, wv = su.make_slice((1, 1, 1, total), dtype, 0, left=0, right=0, guard=3, role="acc", device=d)
    tbuf, tv = su.make_slice((1, 1, 1, total), dtype, 0, left=0, right=0, guard=3, role="acc", device=d)
    for v in (wv, tv):
        v.view(idt).fill_(canary)                # the arenas themselves start as canary: what no layer owns must keep it
    want_w = torch.full((total,), canary, dtype=idt)
    want_t = want_w.clone()
    for (s0, d0, dT, cout, rs, cin, cop, cip), m in zip(desc, masters):
        w16 = torch.zeros((cop, rs, cip), dtype=dtype)
        w16[:cout, :, :cin] = m.to(dtype)
        want_w[d0:d0 + w16.numel()] = w16.reshape(-1).view(idt)
        if dT >= 0:
            want_t[dT:dT + w16.numel()] = w16.flip(1).permute(2, 1, 0).contiguous().reshape(-1).view(idt)
    descd = torch.tensor(desc, dtype=torch.int64, device=d)
    _lib.check(_lib.lib().jg_refresh_weights(_code(dtype), pv.data_ptr(), wv.data_ptr(), tv.data_ptr(), descd.data_ptr(), len(desc), ops._st()), "jg_refresh_weights")
    torch.cuda.synchronize()
    for buf in (pbuf, wbuf, tbuf):
        su.assert_canary_intact(buf)
    for name, got, want in (("w16", wv, want_w), ("w16T", tv, want_t)):
        bad = got.reshape(-1).cpu().view(idt) != want
        if bool(bad.any()):
            first = bad.nonzero()[:5, 0].tolist()
            owner = [max(i for i, dd in enumerate(desc) if dd[1] <= e) for e in first]
            raise AssertionError(f"{name}: {int(bad.sum())} of {total} elements differ; first (element, layer): {list(zip(first, owner))}")
