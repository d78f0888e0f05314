"""GPU tests of G_dropout / D_dropout: the three kernels of csrc/dropout.hip (jg_gn_apply_drop, jg_gn_bwd_reduce_drop, jg_gn_bwd_apply_drop)
on canary-guarded operands (tests/strided_util.py) against the float64 restatement of tests/dropout_ref.py; the drawn mask against the restated
Philox counter layout; the torch.ops surface; ResnetBlock / NLayerDiscriminator and three CUT steps against fixtures recorded from the
unmodified reference with its Dropout draws (tests/golden/dropout/, tests/tools/make_fixture_dropout.py); the three step drivers on drawn masks.

Bounds.  Kernels: the project's single-kernel bound 3e-3 (fp16) / 2e-2 (bf16) relative to the restatement (tests/test_gpu_4_segformer.py:16);
dropout multiplies by exactly 0 or 1 / keep and adds no rounding of its own.  Modules: TOL / TOL_DX / check_grads(3 * TOL) of
tests/test_gpu_3_cut.py:12-45, the bounds of the same modules without dropout.  Step: TOL_LOSS_FWD of tests/test_gpu_5_cutloss.py:293 on the
five losses and fake_B of every step and COS_UPDATE (:294) with parity_util.check_update / check_ema on the G / F / D updates and the EMA,
teacher-forced by the CPU oracle trainer with dropout (tests/dropout_oracle.py), as that file's test of the step without dropout is.
Drivers: the bound of tests/test_gpu_5_cutloss.py::test_cut_step_drivers_agree."""
import contextlib
import os
import random

import numpy as np
import pytest
import torch

import dropout_ref as R
import jg_oracle as O
import strided_util as su

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropout")
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
KTOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}            # tests/test_gpu_4_segformer.py:16
TOL = {torch.float16: 4e-3, torch.bfloat16: 3e-2}             # tests/test_gpu_3_cut.py:12
TOL_DX = {torch.float16: 0.12, torch.bfloat16: 0.35}          # tests/test_gpu_3_cut.py:16
TOL_LOSS_FWD = {torch.float16: 6e-3, torch.bfloat16: 4e-2}    # tests/test_gpu_5_cutloss.py:293
KEEP = 0.5
GUARD = 3
ACTS = {"relu": R.RELU, "lrelu": R.LRELU, "none": R.NONE, "silu": R.SILU}
# (B, H, W, C, left, right): one 16-byte group per pixel, odd HW, a ragged last block | a channel slice on pixel stride 32 | more 16-byte
# groups than jg_dropout_grid_cap(): the grid-stride loop of the two apply passes takes a second trip
S_SMALL, S_SLICE, S_BIG = (2, 5, 5, 8, 0, 0), (2, 9, 7, 24, 8, 0), (3, 96, 96, 320, 0, 0)


def load(name):
    return torch.load(os.path.join(DIR, name), weights_only=False)


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _act_id(name):
    from joligen_amd import _lib

    return {"relu": _lib.JG_ACT_RELU, "lrelu": _lib.JG_ACT_LRELU, "none": _lib.JG_ACT_NONE, "silu": _lib.JG_ACT_SILU}[name]


def _case(shape, dtype, norm, seed=0):
    """guarded operands on the GPU, the host copies of their values, and float32 tables ab (InstanceNorm of x) / pqr"""
    B, H, W, C, left, right = shape
    g = torch.Generator().manual_seed(seed)
    bufs, views = {}, {}
    for name, role in (("x", "in"), ("dy", "in"), ("y", "out"), ("dx", "out")):
        vals = None
        if role == "in":
            vals = torch.randn((B, H, W, C), generator=g) * (1.5 if name == "x" else 1.0) + (0.25 if name == "x" else 0.0)
        bufs[name], views[name] = su.make_slice((B, H, W, C), dtype, 0, left=left, right=right, guard=GUARD, role=role, values=vals, device=D0)
    x64 = views["x"].detach().double().cpu().numpy()
    dy64 = views["dy"].detach().double().cpu().numpy()
    ab = pqr = None
    if norm:
        mean, var = x64.mean(axis=(1, 2)), x64.var(axis=(1, 2))
        rstd = 1.0 / np.sqrt(var + 1e-5)
        ab = torch.tensor(np.stack((rstd, -mean * rstd), axis=-1), dtype=torch.float32)
        pqr = torch.stack((torch.tensor(rstd, dtype=torch.float32), torch.randn((B, C), generator=g) * 0.05, torch.randn((B, C), generator=g) * 0.05), dim=-1)
    u = torch.rand((B, C, H, W), generator=g)
    return bufs, views, x64, dy64, ab, pqr, u


def _ld(v):
    assert v.stride(-1) == 1
    return v.stride(-2)


def _launch_all(views, dtype, act, ab, pqr, red, u, key, stream, call, keep=KEEP):
    from joligen_amd import _lib, ops

    L, dt, st = _lib.lib(), ops._dt(views["x"]), ops._st()
    B, H, W, C = views["x"].shape
    p = lambda t: None if t is None else t.data_ptr()
    x, dy, y, dx = (views[k] for k in ("x", "dy", "y", "dx"))
    _lib.check(L.jg_gn_apply_drop(dt, p(x), _ld(x), p(ab), p(y), _ld(y), B, H, W, C, act, keep, p(u), p(key), stream, call, st), "jg_gn_apply_drop")
    if ab is not None:
        _lib.check(L.jg_gn_bwd_reduce_drop(dt, p(x), _ld(x), p(dy), _ld(dy), p(ab), p(red), B, H, W, C, act, keep, p(u), p(key), stream, call, st),
                   "jg_gn_bwd_reduce_drop")
    _lib.check(L.jg_gn_bwd_apply_drop(dt, p(x), _ld(x), p(dy), _ld(dy), p(ab), p(pqr), p(dx), _ld(dx), B, H, W, C, act, keep, p(u), p(key), stream,
                                      call, st), "jg_gn_bwd_apply_drop")
    torch.cuda.synchronize()


def _check_guards(bufs):
    for name, buf in bufs.items():
        su.assert_canary_intact(buf)
        if buf.spec.role == "out":
            su.assert_fully_written(buf)


def _kernel_case(shape, dtype, act, norm):
    bufs, views, x64, dy64, ab, pqr, u = _case(shape, dtype, norm)
    B, H, W, C = views["x"].shape
    abd, pqrd, ud = (None if t is None else t.to(D0) for t in (ab, pqr, u))
    red0 = torch.randn((B, C, 2), generator=torch.Generator().manual_seed(5))       # the reduce pass ACCUMULATES: a non-zero start
    red = red0.to(D0)
    _launch_all(views, dtype, _act_id(act), abd, pqrd, red, ud, None, 0, 0)
    _check_guards(bufs)
    m = R.mask(u.numpy(), KEEP)
    abn, pqrn = (None if t is None else t.numpy() for t in (ab, pqr))
    y, dx = views["y"].float().cpu(), views["dx"].float().cpu()
    assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(dx).any())
    tol = KTOL[dtype]
    e_y = relerr(y, R.apply_drop(x64, abn, ACTS[act], m, KEEP))
    e_dx = relerr(dx, R.bwd_apply_drop(x64, dy64, abn, pqrn, ACTS[act], m, KEEP))
    print(f"{shape} {dtype} {act} norm={norm}: y {e_y:.2e} dx {e_dx:.2e} (bound {tol:.0e})")
    assert e_y < tol and e_dx < tol, (e_y, e_dx)
    mt = torch.from_numpy(m)
    assert bool((y[~mt] == 0).all()), "a dropped element of y is not exactly 0"
    assert abs(float(mt.float().mean()) - KEEP) < 0.2
    if norm:
        e_red = relerr(red.cpu() - red0, R.bwd_reduce_drop(x64, dy64, abn, ACTS[act], m, KEEP))
        print(f"    red {e_red:.2e}")
        assert e_red < tol, e_red
    else:
        assert bool((dx[~mt] == 0).all()), "a dropped element of dx is not exactly 0"
        assert torch.equal(red.cpu(), red0)


@pytest.mark.parametrize("norm", [True, False], ids=["ab", "noab"])
@pytest.mark.parametrize("act", ["relu", "lrelu", "none"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [S_SMALL, S_SLICE], ids=["5x5x8", "9x7x24_ld32"])
def test_kernels_injected_u(shape, dtype, act, norm):
    _kernel_case(shape, dtype, act, norm)


@pytest.mark.parametrize("norm", [True, False], ids=["ab", "noab"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernels_silu(dtype, norm):
    """the fourth activation the entry points accept (the UNet's; no CUT network uses it behind a dropout)"""
    _kernel_case(S_SLICE, dtype, "silu", norm)


@pytest.mark.parametrize("dtype,act,norm", [(torch.bfloat16, "relu", True), (torch.float16, "lrelu", False)], ids=["bf16_relu_ab", "fp16_lrelu_noab"])
def test_kernels_beyond_the_grid_cap(dtype, act, norm):
    from joligen_amd import _lib

    B, H, W, C = S_BIG[:4]
    cap = int(_lib.lib().jg_dropout_grid_cap())
    assert cap < B * H * W * (C // 8) <= 2 * cap, cap          # the stride loop runs twice for some threads, once for the others
    _kernel_case(S_BIG, dtype, act, norm)


def _key(words=(0x1234ABCD, 0x8F1E2D3C)):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32, device=D0)


def _drawn(x, key, stream, call, dtype, ab=None):
    """(y, dx for an all-ones dy) of the act = none kernels with a drawn mask"""
    from joligen_amd import launch

    dy = torch.ones_like(x)
    y = launch.gn_apply_drop(x, ab, 0, KEEP, None, key, stream, call)
    dx = launch.gn_bwd_apply_drop(x, dy, None, None, 0, KEEP, None, key, stream, call)
    torch.cuda.synchronize()
    return y, dx


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_drawn_mask_is_the_restated_counter_layout(dtype):
    B, H, W, C = 2, 9, 7, 24
    g = torch.Generator().manual_seed(2)
    x = (torch.rand((B, H, W, C), generator=g) + 0.5).to(dtype).to(D0)           # no zeros
    key, stream, call = _key(), 5, 3
    y, dx = _drawn(x, key, stream, call, dtype)
    m = torch.from_numpy(R.mask(R.uniforms(key.cpu().numpy(), B, C, H, W, stream, call), KEEP))
    assert torch.equal(y.cpu() != 0, m), "forward mask differs from the restated Philox mask"
    assert torch.equal(dx.cpu() != 0, m), "backward mask differs from the forward mask"
    assert torch.equal(y.cpu()[m].float(), (x.cpu().float() * 2.0).to(dtype).float()[m]) and bool((dx.cpu()[m].float() == 2.0).all())
    # the reduce pass regenerates the same mask: with a = 1, b = 0, act none, dy = 1: red[..., 0] = (number kept) / keep
    from joligen_amd import launch

    ab = torch.tensor([1.0, 0.0], device=D0).repeat(B, C, 1).contiguous()
    red = torch.zeros((B, C, 2), device=D0)
    launch.gn_bwd_reduce_drop(x, torch.ones_like(x), ab, red, 0, KEEP, None, key, stream, call)
    assert torch.equal(red[..., 0].cpu(), m.float().sum(dim=(1, 2)) * 2.0)
    y2, dx2 = _drawn(x, key, stream, call, dtype)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    for other in (_drawn(x, key, stream, call + 1, dtype), _drawn(x, key, stream + 1, call, dtype), _drawn(x, _key((0x1234ABCC, 0x8F1E2D3C)), stream, call, dtype)):
        assert float(((other[0] != 0) != (y != 0)).float().mean()) > 0.4


def test_drawn_mask_kept_fraction():
    B, H, W, C = 4, 128, 128, 16
    n = B * H * W * C
    assert n >= 1_000_000
    x = torch.ones((B, H, W, C), device=D0, dtype=torch.bfloat16)
    y, _ = _drawn(x, _key(), 1, 0, torch.bfloat16)
    frac = float((y != 0).double().mean())
    assert abs(frac - KEEP) <= 4 * (KEEP * (1 - KEEP) / n) ** 0.5, frac


def test_bad_arguments_are_refused():
    from joligen_amd import ops

    x = torch.ones((2, 5, 5, 8), device=D0, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="dropout"):
        ops.activation_dropout(x, 0, 0.5)                                         # a draw without a key
    with pytest.raises(ValueError, match="dropout"):
        ops.activation_dropout(x, 0, 0.5, key=_key(), stream=1 << 16)
    with pytest.raises(ValueError, match="dropout"):
        ops.activation_dropout(x, 0, 0.0, key=_key())
    with pytest.raises(ValueError, match="dropout"):
        ops.group_norm(x, 8, keep=0.5, u=torch.rand(2, 8, 5, 4, device=D0))
    with pytest.raises(ValueError, match="addend"):
        ops.group_norm(x, 8, keep=0.5, key=_key(), add=x)


def test_torch_ops_opcheck_and_boundary():
    """schema, fake kernels and autograd registration of the new ops; `ops.group_norm(keep=)` / `ops.activation_dropout` under the boundary
    are the module graph's values (same launches), gradients included"""
    from joligen_amd import _lib, ops

    J = torch.ops.jg355
    B, H, W, C = S_SMALL[:4]
    g = torch.Generator().manual_seed(9)
    x = torch.randn((B, H, W, C), generator=g).to(torch.bfloat16).to(D0)
    dy = torch.randn((B, H, W, C), generator=g).to(torch.bfloat16).to(D0)
    u = torch.rand((B, C, H, W), generator=g).to(D0)
    key = _key()
    gamma, beta = torch.rand(C, generator=g).to(D0) + 0.5, torch.randn(C, generator=g).to(D0)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    relu = _lib.JG_ACT_RELU
    torch.library.opcheck(J.group_norm_act_drop.default, (x.clone().requires_grad_(True), None, None, None, C, relu, 1e-5, KEEP, u, None, 0, 0), test_utils=utils)
    torch.library.opcheck(J.group_norm_act_drop.default, (x.clone().requires_grad_(True), gamma, beta, None, 2, relu, 1e-5, KEEP, None, key, 3, 1), test_utils=utils)
    torch.library.opcheck(J.group_norm_act_drop_bwd.default, (x, dy, gamma, beta, None, 2, relu, 1e-5, KEEP, None, key, 3, 1), test_utils=utils[:2])
    torch.library.opcheck(J.act_drop.default, (x.clone().requires_grad_(True), relu, KEEP, u, None, 0, 0), test_utils=utils)
    torch.library.opcheck(J.act_drop.default, (x.clone().requires_grad_(True), relu, KEEP, None, key, 2, 0), test_utils=utils)
    torch.library.opcheck(J.act_drop_bwd.default, (x, dy, relu, KEEP, None, key, 2, 0), test_utils=utils[:2])
    for fn in (lambda t: ops.group_norm(t, C, None, None, None, relu, 1e-5, keep=KEEP, key=key, stream=4, call=2),
               lambda t: ops.activation_dropout(t, _lib.JG_ACT_LRELU, KEEP, u=u)):
        res = []
        for boundary in (False, True):
            xd = x.clone().requires_grad_(True)
            with (ops.torch_ops_boundary() if boundary else contextlib.nullcontext()):
                y = fn(xd)
                y.backward(dy)
            res.append((y.detach(), xd.grad))
        # the forward is the same launch on the same values; the backward of the functional op recomputes the statistics (fp32 atomics order)
        assert torch.equal(res[0][0], res[1][0]) and relerr(res[1][1], res[0][1]) < 1e-3
        assert bool((res[0][0] == 0).float().mean() > 0.3)


# ---- modules against the reference's fixtures ----------------------------------------------------------------------------------------------
def nchw(t, c):
    return t.permute(0, 3, 1, 2)[:, :c].float()


def check_grads(net, ref_checks, tol, dtype):
    """tests/test_gpu_3_cut.py:32-45"""
    bad = []
    for k, ref in ref_checks.items():
        v = dict(net.named_parameters())[k].grad.detach().float().cpu()
        mine = torch.stack([v.norm(), (v * O.projection_vector(k, v.shape)).sum()])
        floor = 0.0
        if k.endswith(".bias"):
            wk = k[:-4] + "weight"
            floor = 16 * (2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7) * float(ref_checks[wk][0])
        t = tol * float(ref[0]) + floor + 1e-6
        if abs(float(mine[0] - ref[0])) > t or abs(float(mine[1] - ref[1])) > 2 * t * max(1.0, v.numel() ** 0.5 / 4):
            bad.append((k, mine.tolist(), ref.tolist(), t))
    assert not bad, bad[:6]


def _inject(table, used):
    def rand(path, call, shape, device):
        u = table[(path, call)]
        assert tuple(u.shape) == tuple(shape), (path, call, tuple(u.shape), tuple(shape))
        used.add((path, call))
        return u.to(device)
    return rand


def _module_case(net, g, dtype, cin, cout, cpad):
    from joligen_amd import ops
    from joligen_amd.arena import ParamArena

    assert list(net.state_dict().keys()) == g["keys"]
    net.load_state_dict(O.synth_state_dict(net.state_dict(), seed=g["seed"]))
    d = torch.device(D0)
    if hasattr(net, "jg_finalize"):
        net.jg_finalize(d, dtype)
    else:
        net.arena = ParamArena(net, d, dtype, priority=())
        net.arena.ensure_fresh()
    net.train()
    table, used = {(p, c): u for p, c, u in g["u"]}, set()
    net.dropout_state.begin_step()
    net.dropout_rand = _inject(table, used)
    assert net.dropout_state.rand is net.dropout_rand
    x = ops.to_nhwc(g["x"].to(d), dtype, cpad).requires_grad_(True)
    out = net(x)
    assert used == set(table)
    e = relerr(nchw(out, cout), g["out"])
    out.backward(ops.to_nhwc(g["R"].to(d), dtype, out.shape[-1]))
    torch.cuda.synchronize()
    e_dx = relerr(nchw(x.grad, cin), g["dx"])
    print(f"{type(net).__name__} {dtype}: out {e:.2e} (bound {TOL[dtype]:.0e}) dx {e_dx:.2e} (bound {TOL_DX[dtype]})")
    assert e < TOL[dtype] and e_dx < TOL_DX[dtype], (e, e_dx)
    check_grads(net, g["grad_checks"], 3 * TOL[dtype], dtype)
    # eval(): no dropout, nothing drawn, nothing injected
    net.eval()
    net.dropout_rand = lambda *a: pytest.fail("eval() drew a dropout mask")
    with torch.no_grad():
        a, b = net(x.detach()), net(x.detach())
    assert torch.equal(a, b) and not torch.equal(a, out.detach())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_resnet_block_vs_reference_golden(dtype):
    from joligen_amd.modules.resnet_generator import ResnetBlock

    _module_case(ResnetBlock(16, "reflect", True, True), load("resblock.pt"), dtype, 16, 16, 16)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_patchgan_vs_reference_golden(dtype):
    from joligen_amd.modules.discriminators import NLayerDiscriminator

    _module_case(NLayerDiscriminator(3, ndf=16, n_layers=3, use_dropout=True), load("patchgan.pt"), dtype, 3, 1, 8)


# ---- the CUT step --------------------------------------------------------------------------------------------------------------------------
def build_cut_model(g, dtype, **extra):
    """tests/test_gpu_5_cutloss.py:258-268"""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    c, hp = g["cfg"], g["hp"]
    cfg = {"model_type": "cut", "G": {"netG": c.get("netG", "resnet"), "ngf": c["ngf"], "nblocks": c["n_blocks"]}, "D": {"netDs": ["basic"], "ndf": c["ndf"]},
           "alg": {"cut": {"nce_layers": c["nce_layers"], "num_patches": c["num_patches"], "nce_loss": c["nce_loss"]}},
           "data": {"crop_size": c["S"], "load_size": c["S"]},
           "train": {"batch_size": c["B"], "pool_size": c["pool"], "G_ema": True, "G_ema_beta": hp["ema_beta"], "G_lr": hp["lr_G"], "D_lr": hp["lr_D"]}}
    opt = opt_from_json(cfg, overrides={"jg_act_dtype": "fp16" if dtype == torch.float16 else "bf16", "gpu_ids": "0", **extra})
    return create_model(opt, 0)


class _Spy:
    """stands in for the loaded library: records the names of the entry points that are called"""

    def __init__(self, real):
        self.__dict__["real"], self.__dict__["called"] = real, set()

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self.real, name)


NEW_ENTRY_POINTS = {"jg_gn_apply_drop", "jg_gn_bwd_reduce_drop", "jg_gn_bwd_apply_drop"}


COS_UPDATE = {torch.float16: 0.80, torch.bfloat16: 0.55}       # tests/test_gpu_5_cutloss.py:294


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cut_steps_vs_reference_golden(dtype, monkeypatch):
    """tests/test_gpu_5_cutloss.py::test_cut_model_steps_vs_reference_golden for the fixture with G_dropout and D_dropout, same bounds: three
    optimize_parameters() under the sequential driver, TEACHER-FORCED by the CPU oracle trainer with dropout (tests/dropout_oracle.py, held to
    the fixture's losses and parameter checksums by tests/test_dropout_host.py and re-asserted here), the reference's Dropout draws injected
    on both sides by (module path, invocation).  Every step: the five losses and fake_B on identical weights (TOL_LOSS_FWD), the G / F / D
    parameter updates against the oracle's (PU.check_update, COS_UPDATE) and the EMA (PU.check_ema)."""
    import dropout_oracle as DO
    import parity_util as PU
    from joligen_amd import _lib
    from test_oracle_golden import ReplayRandom, cut_ids

    monkeypatch.setenv("JG_EARLY_D", "0")
    g = load("cutstep_dropout.pt")
    c = g["cfg"]
    dequant = lambda q: ((q.to(torch.float64) + 32768.5) / 65536.0).float()
    model = build_cut_model(g, dtype, G_dropout=True, D_dropout=True)
    assert model.g_dropout and model.d_dropout and not model._batched_nce() and not model._reuse_feats()
    s0 = g["steps"][0]
    model.data_dependent_initialize({"A": s0["A"], "B": s0["B"]})
    assert list(model.netG_A.state_dict().keys()) == g["keysG"]
    assert list(model.netD_B_basic.state_dict().keys()) == g["keysD"]
    assert list(model.netF.state_dict().keys()) == g["keysF"]
    draws = [d for s in g["steps"] for d in s["pool_draws"]]
    rng_ref = ReplayRandom(draws)
    tr = DO.trainer_for(g, rng_ref)
    rng = ReplayRandom(draws)
    model.set_pool_rng(rng)
    nl = len(c["nce_layers"].split(","))
    tol = TOL_LOSS_FWD[dtype]
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", spy)
    log = []
    for it, s in enumerate(g["steps"]):
        st = tr.state
        PU.force_state(model.netG_A, tr.G, {k: mv[0] for k, mv in st["G"].items()}, {k: mv[1] for k, mv in st["G"].items()}, tr.steps["G"], tr.ema)
        PU.force_state(model.netF, tr.Fp, {k: mv[0] for k, mv in st["F"].items()}, {k: mv[1] for k, mv in st["F"].items()}, tr.steps["F"])
        PU.force_state(model.netD_B_basic, tr.D, {k: mv[0] for k, mv in st["D"].items()}, {k: mv[1] for k, mv in st["D"].items()}, tr.steps["D"])
        before = {n: PU.snapshot(getattr(model, "net" + n)) for n in ("G_A", "F", "D_B_basic")}
        ref_before = {"G_A": {k: v.clone() for k, v in tr.G.items()}, "F": {k: v.clone() for k, v in tr.Fp.items()},
                      "D_B_basic": {k: v.clone() for k, v in tr.D.items()}}
        ema_before = None if tr.ema is None else {k: v.clone() for k, v in tr.ema.items()}
        ids_ab, ids_idt = cut_ids(s, nl, c["num_patches"])
        model.patch_ids_injection = lambda call, shapes, a=ids_ab, b=ids_idt: [i.to(D0) for i in (a if call == 0 else b)]
        table, used = {(p, n): dequant(q) for p, n, q in s["dropout"]}, set()
        model.dropout_rand = _inject(table, used)
        model.set_input({"A": s["A"], "B": s["B"]})
        model.optimize_parameters()
        torch.cuda.synchronize()
        assert model.step_driver == "sequential"
        assert used == set(table), sorted(set(table) - used)
        lo = tr.step(s["A"], s["B"], ids_ab, ids_idt, dropout=table)
        assert tr.used == set(table)
        losses = {k: float(v) for k, v in model.get_current_losses().items()}
        print(it, {rk: (round(losses[rk], 5), round(lo[ok], 5), round(s["losses"][rk], 5)) for ok, rk in (("G_tot", "G_tot"), ("D_tot", "D_tot"))})
        for ok, rk in (("G_tot", "G_tot"), ("G_GAN", "G_GAN_D_B_basic"), ("G_NCE", "G_NCE"), ("G_NCE_Y", "G_NCE_Y"), ("D_tot", "D_tot")):
            ref = s["losses"][rk]
            assert abs(lo[ok] - ref) <= 2e-4 * (1 + it) ** 2 * abs(ref) + 1e-5, ("oracle vs fixture", it, ok, lo[ok], ref)
            assert abs(losses[rk] - lo[ok]) <= tol * abs(lo[ok]) + 1e-4, (it, rk, losses[rk], lo[ok])
        fb = model.fake_B.permute(0, 3, 1, 2)[:, :3].float()
        assert relerr(fb, tr.fake_B) < tol, (it, relerr(fb, tr.fake_B))
        for n, ref_after, skip in (("G_A", tr.G, lambda k: k.endswith(".bias")), ("F", tr.Fp, lambda k: False),
                                   ("D_B_basic", tr.D, lambda k: k.endswith(".bias") and not k.startswith("model.0."))):
            after = PU.snapshot(getattr(model, "net" + n))
            PU.check_update(f"dropout {n} it{it}", before[n], after, ref_before[n], ref_after, COS_UPDATE[dtype], skip=skip, log=log)
            if n == "G_A":
                ema = {k: v.detach().float().cpu() for k, v in model.netG_A_ema.named_parameters()}
                PU.check_ema(f"ema it{it}", ema_before, ema, after, g["hp"]["ema_beta"], first=ema_before is None)
    print("\n".join(log))
    assert rng.i == len(rng.log) and rng_ref.i == len(rng_ref.log)
    assert NEW_ENTRY_POINTS <= spy.called


def test_dropout_off_is_the_step_of_before(monkeypatch):
    """with G_dropout / D_dropout off the model builds the state_dict keys of before and a step calls none of the new entry points"""
    from joligen_amd import _lib

    g = torch.load(os.path.join(os.path.dirname(DIR), "cutstep_patchnce.pt"), weights_only=False)
    model = build_cut_model(g, torch.bfloat16)
    assert not model.g_dropout and not model.d_dropout and not model._dropout_on and model._drop_key is None
    s0 = g["steps"][0]
    model.data_dependent_initialize({"A": s0["A"], "B": s0["B"]})
    assert list(model.netG_A.state_dict().keys()) == g["keysG"] and list(model.netD_B_basic.state_dict().keys()) == g["keysD"]
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", spy)
    for _ in range(2):
        model.set_input({"A": s0["A"], "B": s0["B"]})
        model.optimize_parameters()
    torch.cuda.synchronize()
    assert "jg_gn_apply" in spy.called and not (NEW_ENTRY_POINTS & spy.called), sorted(NEW_ENTRY_POINTS & spy.called)


_SMALL_CUT = {"model_type": "cut", "G": {"netG": "resnet", "ngf": 32, "nblocks": 2, "dropout": True}, "D": {"netDs": ["basic"], "ndf": 32, "dropout": True},
              "alg": {"cut": {"nce_layers": "0,4,8,10"}}, "data": {"crop_size": 64, "load_size": 64}}


def _run_driver(cfg, data, monkeypatch, early, graph, calls=7):
    """tests/test_gpu_5_cutloss.py:702-735, plus the Philox key of every step"""
    import warnings

    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    monkeypatch.setenv("JG_EARLY_D", "1" if early else "0")
    monkeypatch.setenv("JG_GRAPH_D", "1" if graph else "0")
    monkeypatch.setenv("JG_GRAPH_G", "1" if graph else "0")
    monkeypatch.delenv("JG_DBG_GRAPH_CANARY_FAIL", raising=False)
    torch.manual_seed(3)
    random.seed(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = create_model(opt_from_json(cfg, overrides={"jg_act_dtype": "bf16", "gpu_ids": "0"}), 0)
        assert m.g_dropout and m.d_dropout
        m.data_dependent_initialize(data)
        m.setup(m.opt)
        m.single_gpu()
        losses, keys = [], []
        for _ in range(calls):
            m.set_input(data)
            m.optimize_parameters()
            losses.append([float(getattr(m, "loss_D_GAN_" + dn)) for dn in m.discriminators_names] + [float(m.loss_G_tot)])
            keys.append(tuple(m._drop_key.tolist()))
    torch.cuda.synchronize()
    dropped = [str(w.message) for w in rec if "jg_graph_" in str(w.message)]
    m1 = {n: m._net(n).arena.m.detach().double().cpu() for n in m.model_names}
    return dict(losses=torch.tensor(losses, dtype=torch.float64), m1=m1, dropped=dropped, driver=m.step_driver, note=m.step_driver_note, keys=keys, model=m)


def test_step_drivers_agree_on_drawn_masks(monkeypatch):
    """tests/test_gpu_5_cutloss.py::test_cut_step_drivers_agree with G_dropout and D_dropout: same torch seed, masks drawn in the kernels; the
    sequential, early-D and graph drivers issue the same (key, stream, call) triples and agree to that test's bound (4 x the run-to-run floor
    + 2e-3).  The key changes every step, so no two steps share a mask; netG_A.eval() does not read the key."""
    import joligen_amd

    gen = torch.Generator().manual_seed(11)
    data = {"A": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1, "B": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1}
    cfg = dict(_SMALL_CUT, train={"batch_size": 2, "G_ema": True, "iter_size": 1, "pool_size": 0, "G_lr": 0.0, "D_lr": 0.0})
    a = _run_driver(cfg, data, monkeypatch, False, False)
    a2 = _run_driver(cfg, data, monkeypatch, False, False)
    b = _run_driver(cfg, data, monkeypatch, True, False)
    c = _run_driver(cfg, data, monkeypatch, True, True)
    assert a["driver"] == "sequential" and b["driver"] == "early", (a["driver"], b["driver"])
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert c["driver"] == "graph+graphG" and not c["dropped"], (c["driver"], c["note"], c["dropped"])
    assert len(set(a["keys"])) == len(a["keys"]), a["keys"]                      # a fresh key every step: no mask is repeated
    assert a["keys"] == a2["keys"] == b["keys"] == c["keys"], (a["keys"], b["keys"], c["keys"])
    la, pa = a["losses"], a["m1"]
    floor_l = float(((la - a2["losses"]).abs() / la.abs()).max())
    floor_p = max(float((pa[n] - a2["m1"][n]).norm() / pa[n].norm()) for n in pa)
    print("run-to-run floor: losses %.2e, first moments %.2e" % (floor_l, floor_p))
    for tag, r in (("early", b), ("graph", c)):
        l, p = r["losses"], r["m1"]
        assert torch.isfinite(l).all(), (tag, l)
        el = float(((l - la).abs() / la.abs()).max())
        print(tag, "losses %.2e" % el, {n: "%.2e" % float((p[n] - pa[n]).norm() / pa[n].norm()) for n in pa})
        assert el <= 4 * floor_l + 2e-3, (tag, el, floor_l)
        for n in pa:
            e = float((p[n] - pa[n]).norm() / pa[n].norm())
            assert e <= 4 * floor_p + 2e-3, (tag, n, e, floor_p)
    # eval(): the generator's output does not depend on the key -- no dropout entry point runs, and the output moves by no more than the fp32
    # atomics of the InstanceNorm statistics move it between any two runs (the single-kernel bound), where a training-mode pass moves by O(1)
    from joligen_amd import _lib

    m = a["model"]
    net = m.netG_A.eval()
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", spy)
    with torch.no_grad():
        o1 = net(m.real_A)
        m._drop_key.add_(12345)
        o2 = net(m.real_A)
        assert not (NEW_ENTRY_POINTS & spy.called) and "jg_gn_apply" in spy.called
        net.train()
        m.dropout_state.begin_step()
        o3 = net(m.real_A)
    assert "jg_gn_apply_drop" in spy.called
    e_eval, e_train = relerr(o2, o1), relerr(o3, o1)
    print("eval vs eval with another key %.2e, train vs eval %.2e" % (e_eval, e_train))
    assert e_eval < KTOL[torch.bfloat16] and e_train > 10 * KTOL[torch.bfloat16], (e_eval, e_train)
