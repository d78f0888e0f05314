"""The tile walk of the two fused streaming 1x1 launches (csrc/conv1x1.hip: conv1x1_stream_runs_kernel): a wave owns a contiguous run of
16-pixel tiles and stages the per-image coefficients of jg_conv1x1_gn_apply / jg_conv1x1_gn_bwd_apply once per image the run touches; the
next image's rows wait in registers and are written to the wave's LDS slot at the boundary.
What can go wrong there is coefficients of the wrong image on the tiles next to an image boundary, a run that starts or ends mid-image,
a ring refill past the run's end, and a tile count the wave count does not divide -- so every case here uses per-image coefficients that
differ by O(1) from one image to the next (a wrong image on ONE tile of 16 pixels is then a gross error: 1 / 4096 of the elements off by
O(1) is 1.5e-2 norm-wise, against bounds of 1e-3 / 6e-3).

Two sets of shapes.  The first is the smallest the kernel takes (it refuses fewer than 65536 pixels):
  MANY    16 x 64 x 64     256 tiles per image
  RAGGED  3 x 160 x 144    1440 tiles per image, 4320 in all: no wave count the launcher picks divides it
  ONE     1 x 256 x 256    one image
At these the launcher (about 2048 workgroups per launch) hands a wave one to four tiles, and no run straddles an image: they check the
prologue, the one-tile run and the tail.  The boundary branch inside the tile loop, the coefficient prefetch and the steady-state refill need
runs LONGER than the ring (PF tiles) that STRADDLE images, which the launcher gives only above 131072 x (column groups) pixels.  The second
set is sized for that per instance, from the launcher's own formula (_run_layout restates it and every case asserts what it got):
  CROSS   B x 24 x 30      45 tiles per image (odd, so boundaries fall anywhere in a run), B = 92 ... 1001: runs of 2.5 - 5.5 tiles
  TINY    B x 4 x 8        2 tiles per image: every run crosses one or two boundaries (exact-integer cases)
Operands are drawn on the device, so the larger shapes cost milliseconds.
The bounds are those of test_gpu_0_ops.py (test_conv1x1_gn_apply_matches_the_two_passes, ..._gn_bwd_apply_matches_the_two_launch_form)
and the exact-integer recipe is that of test_gpu_23_exact_integer.py."""
import numpy as np
import pytest
import torch

import kernel_cases as kc

pytestmark = pytest.mark.gpu

DTYPES = kc.DTYPES
IDS = ["fp16", "bf16"]
NONE, SILU = 0, 1
MANY, RAGGED, ONE = (16, 64, 64), (3, 160, 144), (1, 256, 256)


def CROSS(B):
    return (B, 24, 30)


def TINY(B):
    return (B, 4, 8)


# (K, N) of the input-gradient launch, number of addends
GNB_CASES = [(MANY, 64, 128, 2), (MANY, 64, 192, 0), (MANY, 128, 256, 1), (MANY, 192, 64, 2), (MANY, 256, 512, 1),      # <4,2> <2,2> <4,4> <2,6> <2,8>
             (RAGGED, 128, 256, 2), (ONE, 64, 128, 0),
             # runs longer than the ring that straddle images, one case per fused instance: <4,2> <2,2> <2,4> <4,4> <2,6> <2,8>
             (CROSS(1001), 64, 128, 2), (CROSS(334), 64, 192, 0), (CROSS(212), 128, 192, 1), (CROSS(319), 128, 256, 2), (CROSS(455), 192, 64, 1),
             (CROSS(92), 256, 512, 1)]
# (Cin, Cout)
APPLY_CASES = [(MANY, 64, 128), (MANY, 128, 64), (MANY, 192, 64), (MANY, 256, 128), (RAGGED, 128, 64), (ONE, 128, 64),      # <4,2> <2,4> <2,6> <2,8>
               # <4,2> <2,2> <2,4> <2,6> <2,8>
               (CROSS(1001), 64, 128), (CROSS(334), 64, 192), (CROSS(637), 128, 64), (CROSS(455), 192, 64), (CROSS(228), 256, 128)]


def _instance(gnb, K, N):
    """<PAIRS, KS> of the fused launch, as dispatch_1x1 picks it"""
    ks, wide = K // 32, N % 128 == 0
    if ks == 2:
        return (4 if wide else 2), 2
    if ks == 4:
        return (4 if wide and gnb else 2), 4
    return 2, ks


def _run_layout(shape, gnb, K, N):
    """the runs launch_1x1_runs / conv1x1_stream_runs_kernel give this launch: grid (min(ceil(ntiles / 4), max(2048 / column groups, 64)),
    column groups), four waves per workgroup, wave w owns tiles [w ntiles / nwaves, (w + 1) ntiles / nwaves); the ring holds PF tiles.
    Returns (longest run, runs with an image boundary strictly inside, most boundaries inside one run, PF)."""
    B, H, W = shape
    pairs, ks = _instance(gnb, K, N)
    tpi, ntiles, ngroups = H * W // 16, B * H * W // 16, N // (pairs * 32)
    nwaves = 4 * min((ntiles + 3) // 4, max(2048 // ngroups, 64))
    t = np.arange(nwaves + 1, dtype=np.int64) * ntiles // nwaves
    t0, t1 = t[:-1], t[1:]
    inside = np.where(t1 > t0, (t1 - 1) // tpi - t0 // tpi, 0)       # image of the run's last tile - image of its first
    return int((t1 - t0).max()), int((inside > 0).sum()), int(inside.max()), (4 if ks <= 2 else 2 if ks <= 4 else 1)


def _check_layout(shape, gnb, K, N):
    """CROSS / TINY shapes: the launch really has runs longer than the ring, and more than PF of them straddle an image boundary"""
    longest, crossing, most, pf = _run_layout(shape, gnb, K, N)
    print(f"runs: longest {longest} tiles (ring {pf}), {crossing} straddle an image boundary, at most {most} boundaries in one")
    if shape[1:] in ((24, 30), (4, 8)):
        assert longest > pf and crossing > pf, (longest, crossing, pf)
    if shape[1:] == (4, 8):
        assert most >= 2, most


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def relerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _case_id(c):
    return "x".join(map(str, c[0])) + "-" + "-".join(map(str, c[1:]))


def _gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _per_image(B, device="cpu"):
    return torch.arange(B, dtype=torch.float32, device=device)[:, None]


def _ab(B, C, g):
    """scale and shift of image b: O(1) apart from those of image b - 1"""
    kw = dict(generator=g, device=g.device)
    i = _per_image(B, g.device)
    return torch.stack([(torch.rand(B, C, **kw) + 0.5) * (1 + i % 4), torch.randn(B, C, **kw) + i % 5], -1).contiguous()


def _pqr(B, C, g):
    kw = dict(generator=g, device=g.device)
    i = _per_image(B, g.device)
    return torch.stack([(torch.rand(B, C, **kw) + 0.5) * (1 + i % 3), 0.1 * torch.randn(B, C, **kw) + 0.5 * (i % 2),
                        0.1 * torch.randn(B, C, **kw) + i % 4], -1).contiguous()


def _bc(t, i):
    """coefficient i of [B][C][n] broadcast over NHWC"""
    return t[:, None, None, :, i]


def _conv(x, w, y, shape, cin, cout, **kw):
    from joligen_amd import ops

    B, H, W = shape
    kw.setdefault("ldx", x.stride(-2))
    kw.setdefault("ldy", y.stride(-2))
    ok = ops.conv_nt(x, w, y, B=B, H=H, W=W, Cin=cin, Cout=cout, R=1, S=1, pad=0, stride=1, Ho=H, Wo=W, ldw=cin, **kw)
    assert ok is not False
    return y


def _last_kernel():
    from joligen_amd import _lib

    return _lib.lib().jg_last_kernel().decode()


# ======================================================================================================================================
# jg_conv1x1_gn_apply, SiLU: against jg_conv2d_nt + jg_gn_apply_ld and an fp32 evaluation
# ======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", APPLY_CASES, ids=_case_id)
def test_gn_apply_runs_match_the_two_passes(case, dtype):
    from joligen_amd import _lib, ops

    shape, cin, cout = case
    B, H, W = shape
    d = dev()
    _check_layout(shape, False, cin, cout)
    g = _gen(cin * 3 + cout + B)
    kw = dict(generator=g, device=d)
    x = (torch.randn(B, H, W, cin, **kw) * 1.5).to(dtype)
    w = (torch.randn(cout, 1, 1, cin, **kw) * 0.1).to(dtype)
    bias = torch.randn(cout, **kw)
    ab = _ab(B, cin, g)
    y_ref = _conv(x, w, torch.empty(B, H, W, cout, device=d, dtype=dtype), shape, cin, cout, bias=bias)
    yn_ref = torch.empty_like(x)
    _lib.check(_lib.lib().jg_gn_apply_ld(ops._dt(x), x.data_ptr(), cin, ab.data_ptr(), yn_ref.data_ptr(), cin, B, H * W, cin, SILU, ops._st()))
    y, yn = torch.full_like(y_ref, float("nan")), torch.full_like(x, float("nan"))
    _conv(x, w, y, shape, cin, cout, bias=bias, apply=(ab, yn, cin, SILU))
    torch.cuda.synchronize()
    assert _last_kernel() == kc.GN_APPLY_KERNEL
    assert torch.equal(y, y_ref)                     # same MFMAs in the same order: bit for bit
    # the normalised activation: the same formula in two instruction streams; the last bit of the sigmoid flips the 16-bit rounding of a few
    bits, bits_ref = yn.view(torch.int16).int(), yn_ref.view(torch.int16).int()
    ne = bits != bits_ref
    print(f"y_norm: {float(ne.float().mean()):.3e} of the elements differ, worst {int((bits - bits_ref).abs().max())} ulp")
    assert float(ne.float().mean()) < 1e-4, float(ne.float().mean())
    assert int((bits - bits_ref).abs().max()) <= 1
    want = torch.nn.functional.silu(_bc(ab, 0) * x.float() + _bc(ab, 1))
    assert relerr(yn.float(), want) < (1e-3 if dtype == torch.float16 else 8e-3), relerr(yn.float(), want)


# ======================================================================================================================================
# jg_conv1x1_gn_bwd_apply, SiLU: against jg_gn_bwd_apply_ld + jg_conv2d_nt(res) and an fp32 evaluation
# ======================================================================================================================================
def _gnb_operands(shape, K, N, nadd, dtype, seed):
    B, H, W = shape
    g = _gen(seed)
    kw = dict(generator=g, device=g.device)
    t = dict(gx=(torch.randn(B, H, W, N, **kw) * 1.3).to(dtype), gdy=torch.randn(B, H, W, N, **kw).to(dtype),
             dO=torch.randn(B, H, W, K, **kw).to(dtype), wT=(torch.randn(N, 1, 1, K, **kw) * 0.1).to(dtype),
             ab=_ab(B, N, g), pqr=_pqr(B, N, g))
    for i in range(nadd):
        t[f"add{i + 1}"] = torch.randn(B, H, W, N, **kw).to(dtype)
    return t


def _gnb_fp32(t, s1, s2, alpha):
    """fp32 evaluation on the device of what both forms compute, from the 16-bit operands"""
    xf, ab, pqr = t["gx"].float(), t["ab"], t["pqr"]
    u = _bc(ab, 0) * xf + _bc(ab, 1)
    sg = torch.sigmoid(u)
    want = t["gdy"].float() * (sg * (1 + u * (1 - sg))) * _bc(pqr, 0) + xf * _bc(pqr, 1) + _bc(pqr, 2)
    if "add1" in t:
        want = want + s1 * t["add1"].float()
    if "add2" in t:
        want = want + s2 * t["add2"].float()
    K = t["dO"].shape[-1]
    return want + alpha * (t["dO"].float().reshape(-1, K) @ t["wT"].float().reshape(-1, K).t()).reshape(want.shape)


def _gnb_check(out, ref2, want, dtype):
    e_fused, e_two = relerr(out.float(), want), relerr(ref2.float(), want)
    print(f"relerr against fp32: fused {e_fused:.3e}, two launches {e_two:.3e}")
    assert e_fused < (1e-3 if dtype == torch.float16 else 6e-3), e_fused
    assert e_fused <= e_two * 1.05 + 1e-6, (e_fused, e_two)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", GNB_CASES, ids=_case_id)
def test_gn_bwd_apply_runs_match_the_two_launch_form(case, dtype):
    from joligen_amd import _lib, ops

    shape, K, N, nadd = case
    B, H, W = shape
    d = dev()
    _check_layout(shape, True, K, N)
    t = _gnb_operands(shape, K, N, nadd, dtype, K * 7 + N + B)
    a1, a2 = t.get("add1"), t.get("add2")
    s1, s2, alpha = 0.7, -1.3, 0.70710678
    dxg = torch.empty_like(t["gx"])
    _lib.check(_lib.lib().jg_gn_bwd_apply_ld(ops._dt(dxg), t["gx"].data_ptr(), N, t["gdy"].data_ptr(), N, t["ab"].data_ptr(), t["pqr"].data_ptr(),
                                             dxg.data_ptr(), N, ops._p(a1), N, s1, ops._p(a2), N, s2, B, H * W, N, SILU, ops._st()))
    ref2 = _conv(t["dO"], t["wT"], torch.empty_like(dxg), shape, K, N, alpha=alpha, res=dxg, ldres=N, res_scale=1.0)
    out = _conv(t["dO"], t["wT"], torch.full_like(dxg, float("nan")), shape, K, N, alpha=alpha,
                gn_bwd_apply=(t["gx"], t["gdy"], t["ab"], t["pqr"], a1, s1, a2, s2, SILU))
    torch.cuda.synchronize()
    assert _last_kernel() == kc.GN_BWD_APPLY_KERNEL
    _gnb_check(out, ref2, _gnb_fp32(t, s1, s2, alpha), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gn_bwd_apply_runs_on_channel_slices(dtype):
    """RAGGED, (128, 256), two addends: gx, gdy, both addends and the output are channel slices of wider buffers, each on its own stride.
    The outputs enter as NaN; the columns outside every slice hold a sentinel that must survive."""
    from joligen_amd import _lib, ops

    shape, K, N = RAGGED, 128, 256
    B, H, W = shape
    d = dev()
    SENT = 123.0
    t = _gnb_operands(shape, K, N, 2, dtype, 99)
    wide, v = {}, {}
    for i, name in enumerate(["gx", "gdy", "add1", "add2", "y"]):
        left, right = 64 * (1 + i % 3), 8 * (1 + i)
        wide[name] = torch.full((B, H, W, left + N + right), SENT, dtype=dtype, device=d)
        v[name] = wide[name][..., left:left + N]
        if name == "y":
            v[name].fill_(float("nan"))
        else:
            v[name].copy_(t[name])
    assert len({w_.shape[-1] for w_ in wide.values()}) == len(wide)
    s1, s2, alpha = 0.7, -1.3, 0.70710678
    dxg = torch.empty_like(t["gx"])
    _lib.check(_lib.lib().jg_gn_bwd_apply_ld(ops._dt(dxg), t["gx"].data_ptr(), N, t["gdy"].data_ptr(), N, t["ab"].data_ptr(), t["pqr"].data_ptr(),
                                             dxg.data_ptr(), N, ops._p(t["add1"]), N, s1, ops._p(t["add2"]), N, s2, B, H * W, N, SILU, ops._st()))
    ref2 = _conv(t["dO"], t["wT"], torch.empty_like(dxg), shape, K, N, alpha=alpha, res=dxg, ldres=N, res_scale=1.0)
    contig = _conv(t["dO"], t["wT"], torch.full_like(dxg, float("nan")), shape, K, N, alpha=alpha,
                   gn_bwd_apply=(t["gx"], t["gdy"], t["ab"], t["pqr"], t["add1"], s1, t["add2"], s2, SILU))
    _conv(t["dO"], t["wT"], v["y"], shape, K, N, alpha=alpha, gn_bwd_apply=(v["gx"], v["gdy"], t["ab"], t["pqr"], v["add1"], s1, v["add2"], s2, SILU))
    torch.cuda.synchronize()
    assert _last_kernel() == kc.GN_BWD_APPLY_KERNEL
    for name, w_ in wide.items():
        left = v[name].storage_offset() % w_.shape[-1]
        assert bool((w_[..., :left] == SENT).all()) and bool((w_[..., left + N:] == SENT).all()), f"sentinel columns of {name} were written"
    assert not bool(torch.isnan(v["y"].float()).any())
    assert torch.equal(v["y"], contig)               # only addresses differ
    _gnb_check(v["y"], ref2, _gnb_fp32(t, s1, s2, alpha), dtype)


# ======================================================================================================================================
# exact integers, act = none: every output equals the float64 evaluation (tests/test_gpu_23_exact_integer.py), image boundaries inside runs
# ======================================================================================================================================
def _ternary(shape, p, g):
    """kc.ternary drawn on the device: +1 / -1 with probability p / 2 each, else 0"""
    u = torch.rand(shape, generator=g, device=g.device)
    return (u < p / 2).float() - ((u >= p / 2) & (u < p)).float()


def _integers(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).float()


def _int_coefs(B, C, n, g):
    """integer coefficient rows [B][C][n] in -2 .. 4 whose image b is b % 3 above its draw: neighbouring images differ by O(1)"""
    return _integers((B, C, n), -2, 2, g) + (_per_image(B, g.device) % 3)[..., None]


# MANY: the issue's shape.  TINY: two tiles per image, every run crosses one or two boundaries; B from the launcher's wave count so that runs
# are longer than the ring: <2,4> 8192 waves x 3.5 tiles, <2,8> (two coefficient float4 per lane) 4096 x 3.5
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,cin,cout", [(MANY, 256, 128), (TINY(14333), 128, 64), (TINY(7169), 256, 128)], ids=["many-2,8", "tiny-2,4", "tiny-2,8"])
def test_gn_apply_runs_exact(shape, cin, cout, dtype):
    B, H, W = shape
    d = dev()
    _check_layout(shape, False, cin, cout)
    g = _gen(231)
    p = kc.density(cin)
    x, w = _ternary((B, H, W, cin), p, g), _ternary((cout, cin), p, g)
    bias, ab = _integers((cout,), -3, 3, g), _int_coefs(B, cin, 2, g)
    want_y = kc.ALPHA * (x.double() @ w.double().t()) + bias.double()
    want_n = _bc(ab, 0).double() * x.double() + _bc(ab, 1).double()
    for dt in DTYPES:
        assert kc.representable(want_y, dt) and kc.representable(want_n, dt)
    xd = x.to(dtype)
    y, yn = torch.full((B, H, W, cout), float("nan"), device=d, dtype=dtype), torch.full_like(xd, float("nan"))
    _conv(xd, w.to(dtype).view(cout, 1, 1, cin), y, shape, cin, cout, bias=bias, alpha=kc.ALPHA, apply=(ab, yn, cin, NONE))
    torch.cuda.synchronize()
    assert _last_kernel() == kc.GN_APPLY_KERNEL
    assert torch.equal(y, (want_y + 0.0).to(dtype)) and torch.equal(yn, (want_n + 0.0).to(dtype))


# TINY: <4,2> (two coefficient channels per lane) 8192 waves x 5.5 tiles, <2,8> 1024 waves x 4 tiles
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,K,N", [(MANY, 64, 128), (TINY(22528), 64, 128), (TINY(2070), 256, 512)], ids=["many-4,2", "tiny-4,2", "tiny-2,8"])
def test_gn_bwd_apply_runs_exact(shape, K, N, dtype):
    """scale1 = 2, scale2 = -1"""
    B, H, W = shape
    d = dev()
    _check_layout(shape, True, K, N)
    g = _gen(241)
    p = kc.density(K)
    dO, wT = _ternary((B, H, W, K), p, g), _ternary((N, K), p, g)
    gx, gdy = _integers((B, H, W, N), -2, 2, g), _integers((B, H, W, N), -2, 2, g)
    add1, add2 = _integers((B, H, W, N), -4, 4, g), _integers((B, H, W, N), -4, 4, g)
    ab, pqr = _int_coefs(B, N, 2, g), _int_coefs(B, N, 3, g)
    s1, s2 = 2.0, -1.0
    want = kc.ALPHA * (dO.double() @ wT.double().t())
    want += gdy.double() * _bc(pqr, 0).double()
    want += gx.double() * _bc(pqr, 1).double()
    want += _bc(pqr, 2).double() + s1 * add1.double() + s2 * add2.double()
    for dt in DTYPES:
        assert kc.representable(want, dt)
    c = lambda v: v.to(dtype)      # noqa: E731
    y = torch.full((B, H, W, N), float("nan"), device=d, dtype=dtype)
    _conv(c(dO), c(wT).view(N, 1, 1, K), y, shape, K, N, alpha=kc.ALPHA, gn_bwd_apply=(c(gx), c(gdy), ab, pqr, c(add1), s1, c(add2), s2, NONE))
    torch.cuda.synchronize()
    assert _last_kernel() == kc.GN_BWD_APPLY_KERNEL
    assert torch.equal(y, (want + 0.0).to(dtype))
