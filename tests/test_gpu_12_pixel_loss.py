"""GPU tests of the paired / identity pixel losses of the CUT model: the fused kernel (`jg_pixel_loss`, `jg_pixel_loss_bwd`) against the
float64 restatement of tests/pixel_loss_ref.py on identical 16-bit inputs, its run-to-run bits, the argument checks, the torch.ops surface,
and `CUTModel` with alg_cut_supervised_loss / alg_cut_MSE_idt: step-0 losses against the fixtures recorded from the unmodified reference
(tests/golden/pixel_loss/), the batched form against the four-pass form, and the default (captured-graph) step driver."""
import os
import random
import warnings

import pytest
import torch

import jg_oracle as O
import pixel_loss_ref as R
from test_oracle_golden import ReplayRandom, cut_ids

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
PIX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixel_loss")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
CPAD = 8
# (M, S, C, H, W): one block; one valid channel; 960 pixels per image (no multiple of 256); several blocks plus a remainder;
# 1 / (M C H W) = 6.5e-6, below fp16's normal range; 76800 pixels per segment = 300 blocks, above the kernel's cap of 256 per segment, so
# that a thread makes more than one trip
SHAPES = [(1, 1, 3, 16, 16), (2, 2, 1, 8, 8), (3, 2, 3, 24, 40), (2, 2, 4, 72, 72), (2, 2, 3, 160, 160), (3, 2, 3, 160, 160)]
PAIRS = [(R.L1, R.L1), (R.MSE, R.L1), (R.OFF, R.L1), (R.L1, R.OFF)]
KERNEL_CASES = [(shape, modes) for shape in SHAPES for modes in (PAIRS if shape[1] == 2 else [(R.L1,), (R.MSE,)])]
LAMBDAS = (2.0, 0.5)
UPSTREAM = {torch.float16: 1024.0, torch.bfloat16: 1.0}           # fp16: the loss scale the model's upstream gradient carries
TOL_LOSS = 1e-5                                                   # fp32 hierarchical sum against float64 (the bound of jg_ect_loss)
TOL_KERNEL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}          # the project's single-kernel bound (README)
# forward-only tolerance of the losses of a CUT step at identical weights (test_gpu_5_cutloss.py::TOL_LOSS_FWD)
TOL_LOSS_FWD = {torch.float16: 6e-3, torch.bfloat16: 4e-2}


def kernel_inputs(shape, dtype, seed=7):
    """CPU tensors as jg_pixel_loss reads them: about 10 % of the elements of x equal y exactly, NaN in every pad channel of both"""
    M, S, C, H, W = shape
    g = torch.Generator().manual_seed(seed + M * 100 + H)
    y = torch.randn(M, H, W, CPAD, generator=g).to(dtype)
    x = torch.randn(S * M, H, W, CPAD, generator=g).to(dtype)
    tie = torch.rand(S * M, H, W, CPAD, generator=g) < 0.1
    x = torch.where(tie, y.repeat(S, 1, 1, 1), x)
    x[..., C:], y[..., C:] = float("nan"), float("nan")
    tie[..., C:] = False
    return x, y, tie


def launch(x, y, C, modes, lambdas, up):
    from joligen_amd import ops

    xd, yd = x.to(D0).requires_grad_(True), y.to(D0)
    loss = ops.pixel_loss(xd, yd, C, modes, lambdas)
    loss.backward(torch.full((len(modes),), up, device=D0))
    torch.cuda.synchronize()
    return loss.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape,modes", KERNEL_CASES, ids=lambda v: "x".join(map(str, v)))
def test_pixel_loss_kernel_vs_float64_restatement(shape, modes, dtype_name):
    dtype = DTYPES[dtype_name]
    M, S, C, H, W = shape
    x, y, tie = kernel_inputs(shape, dtype)
    lambdas, up = LAMBDAS[:S], UPSTREAM[dtype]
    loss, dx = launch(x, y, C, modes, lambdas, up)
    loss_ref = R.pixel_loss(x, y, C, modes, lambdas)
    dx_ref = R.pixel_grad(x, y, C, modes, lambdas, [up] * S)
    e_loss = [abs(float(a) - float(b)) / abs(float(b)) if float(b) != 0 else abs(float(a)) for a, b in zip(loss, loss_ref)]
    ulps = (R.ordered_bits(dx) - R.ordered_bits(dx_ref.to(dtype))).abs()
    e_norm = R.relerr(dx, dx_ref)
    print(f"pixel_loss {shape} {modes} {dtype_name}: loss {loss.tolist()} ref {loss_ref.tolist()} rel {['%.2e' % e for e in e_loss]}; dx max ulp "
          f"{int(ulps.max())} (elements off by one: {int((ulps == 1).sum())} of {ulps.numel()}), norm {e_norm:.2e}")
    assert loss.shape == (S,) and loss.dtype == torch.float32 and dx.dtype == dtype and dx.shape == x.shape
    assert torch.isfinite(loss).all() and torch.isfinite(dx).all()
    assert max(e_loss) < TOL_LOSS, (loss, loss_ref)
    assert int(ulps.max()) <= 1, int(ulps.max())
    assert e_norm < TOL_KERNEL[dtype], e_norm
    assert bool((dx[..., C:] == 0).all())                                    # pad channels
    for s, mode in enumerate(modes):
        seg = slice(s * M, (s + 1) * M)
        if mode == R.OFF:
            assert float(loss[s]) == 0.0 and bool((dx[seg] == 0).all())
        if mode == R.L1:                                                     # sign(0) = 0
            assert bool((dx[seg][tie[seg]] == 0).all()) and int(tie[seg].sum()) > 0
        if mode != R.OFF:
            assert float(dx[seg].abs().max()) > 0


def test_pixel_loss_same_bits_on_every_launch():
    """no atomics: losses and gradient are bit-identical run to run, and with JG_DETERMINISTIC on or off"""
    from joligen_amd import _lib

    shape = (2, 2, 4, 72, 72)
    x, y, _ = kernel_inputs(shape, torch.bfloat16)
    lib = _lib.lib()
    was = lib.jg_get_tuning(b"JG_DETERMINISTIC")
    runs = []
    try:
        for det in (0, 0, 1, 1, 0):
            lib.jg_set_tuning(b"JG_DETERMINISTIC", det)
            runs.append(launch(x, y, shape[2], (R.MSE, R.L1), LAMBDAS, 1.0))
    finally:
        lib.jg_set_tuning(b"JG_DETERMINISTIC", was)
    for loss, dx in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(dx, runs[0][1])


def test_pixel_loss_argument_checks():
    """the C entry points answer with an error code, the Python surface raises before any launch"""
    from joligen_amd import _lib, ops

    lib = _lib.lib()
    x, y, _ = kernel_inputs((2, 2, 3, 8, 8), torch.float16)
    x, y = x.to(D0), y.to(D0)
    ws, loss, dx, g = torch.empty(8, device=D0), torch.empty(2, device=D0), torch.empty_like(x), torch.ones(2, device=D0)

    def fwd(xp=x.data_ptr(), S=2, cpad=8, m0=1, m1=1, nws=8):
        return lib.jg_pixel_loss(0, xp, y.data_ptr(), ws.data_ptr(), nws, loss.data_ptr(), S, 2, 3, 8, 8, cpad, m0, m1, 1.0, 1.0, None)

    def bwd(dxp=dx.data_ptr(), S=2, cpad=8, m0=1, m1=1):
        return lib.jg_pixel_loss_bwd(0, x.data_ptr(), y.data_ptr(), g.data_ptr(), dxp, S, 2, 3, 8, 8, cpad, m0, m1, 1.0, 1.0, None)

    assert fwd() == _lib.JG_OK and bwd() == _lib.JG_OK
    assert fwd(cpad=16) == _lib.JG_ERR_UNSUPPORTED and bwd(cpad=16) == _lib.JG_ERR_UNSUPPORTED
    for kw in (dict(S=0), dict(S=3), dict(m0=3), dict(m1=-1)):
        assert fwd(**kw) == _lib.JG_ERR_BAD_ARG and bwd(**kw) == _lib.JG_ERR_BAD_ARG, kw
    assert fwd(xp=x.data_ptr() + 2) == _lib.JG_ERR_BAD_ARG and bwd(dxp=dx.data_ptr() + 2) == _lib.JG_ERR_BAD_ARG      # misaligned
    assert fwd(nws=1) == _lib.JG_ERR_BAD_ARG                                  # workspace too small for S * blocks partial sums
    torch.cuda.synchronize()
    wide = torch.zeros(4, 8, 8, 16, device=D0, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="jg_pixel_loss"):                  # Cpad = 16 is refused, not handled silently
        ops.pixel_loss(wide, wide[:2].contiguous(), 3, (1, 1), (1.0, 1.0))
    for bad, exc in (((x, y, 3, (1, 1, 1), (1.0, 1.0, 1.0)), ValueError), ((x, y, 3, (), ()), ValueError), ((x, y, 3, (1, 3), (1.0, 1.0)), ValueError),
                     ((x, y, 3, (1, 1), (1.0,)), ValueError), ((x, y, 3, (1,), (1.0,)), ValueError), ((x[:3], y, 3, (1, 1), (1.0, 1.0)), ValueError),
                     ((x, y, 9, (1, 1), (1.0, 1.0)), ValueError), ((x, y, 0, (1, 1), (1.0, 1.0)), ValueError),
                     ((x, y.bfloat16(), 3, (1, 1), (1.0, 1.0)), TypeError), ((x.float(), y.float(), 3, (1, 1), (1.0, 1.0)), TypeError),
                     ((x.permute(0, 2, 1, 3), y.permute(0, 2, 1, 3), 3, (1, 1), (1.0, 1.0)), TypeError),
                     ((x[:, :, :4], y, 3, (1, 1), (1.0, 1.0)), TypeError)):
        with pytest.raises(exc, match="pixel_loss|float16/bfloat16"):
            ops.pixel_loss(*bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pixel_loss(x.cpu(), y.cpu(), 3, (1, 1), (1.0, 1.0))


def test_pixel_loss_torch_ops_opcheck_and_boundary():
    """schema + fake kernel + autograd registration of torch.ops.jg355.pixel_loss / pixel_loss_bwd; `ops.pixel_loss` under the boundary is
    bit-equal to the ctypes path"""
    from joligen_amd import ops

    J = torch.ops.jg355
    for shape, modes in (((3, 2, 3, 24, 40), (R.MSE, R.L1)), ((3, 2, 3, 24, 40), (R.L1, R.OFF)), ((1, 1, 3, 16, 16), (R.L1,))):
        S, C = shape[1], shape[2]
        x, y, _ = kernel_inputs(shape, torch.bfloat16)
        lam = list(LAMBDAS[:S])
        xd, yd = x.to(D0).requires_grad_(True), y.to(D0)
        torch.library.opcheck(J.pixel_loss.default, (xd, yd, C, list(modes), lam), test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
        g = torch.full((S,), 0.5, device=D0)
        torch.library.opcheck(J.pixel_loss_bwd.default, (xd.detach(), yd, g, C, list(modes), lam), test_utils=("test_schema", "test_faketensor"))
        a = launch(x, y, C, modes, lam, 0.5)
        with ops.torch_ops_boundary():
            b = launch(x, y, C, modes, lam, 0.5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (shape, modes)
        assert torch.equal(J.pixel_loss(xd, yd, C, list(modes), lam).detach().cpu(), a[0])
        assert torch.equal(J.pixel_loss_bwd(xd.detach(), yd, g, C, list(modes), lam).cpu(), a[1])


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _build_from_fixture(g, dtype):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    c, hp = g["cfg"], g["hp"]
    cfg = {"model_type": "cut", "G": {"netG": "resnet", "ngf": c["ngf"], "nblocks": c["n_blocks"]}, "D": {"netDs": ["basic"], "ndf": c["ndf"]},
           "alg": {"cut": {"nce_layers": c["nce_layers"], "num_patches": c["num_patches"], "nce_loss": c["nce_loss"], "netF_nc": hp["netF_nc"],
                           "HDCE_gamma": hp["HDCE_gamma"], "lambda_SRC": hp["lambda_SRC"], "supervised_loss": hp["supervised_loss"],
                           "lambda_supervised": hp["lambda_supervised"], "MSE_idt": hp["MSE_idt"], "lambda_MSE_idt": hp["lambda_MSE_idt"]}},
           "data": {"crop_size": c["S"], "load_size": c["S"]},
           "train": {"batch_size": c["B"], "pool_size": c["pool"], "G_ema": True, "G_ema_beta": hp["ema_beta"], "G_lr": hp["lr_G"], "D_lr": hp["lr_D"]}}
    return create_model(opt_from_json(cfg, overrides={"jg_act_dtype": "fp16" if dtype == torch.float16 else "bf16", "gpu_ids": "0"}), 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ["l1_idt", "mse", "hdce_idt"])
def test_cut_model_pixel_loss_first_step_vs_reference_golden(name, dtype):
    """CUTModel from the configuration of the reference's step fixture: synthesised weights (seeds 0 / 1 / 3 as in the recipe), the recorded
    patch ids and pool draws; EVERY generator loss of step 0 (G_supervised and G_MSE_idt included) at the forward tolerance of the existing
    CUT step test.  hdce_idt passes only if the identity contrastive term runs with the hDCE weights."""
    g = torch.load(os.path.join(PIX_DIR, f"cutstep_{name}.pt"), weights_only=False)
    c, s = g["cfg"], g["steps"][0]
    model = _build_from_fixture(g, dtype)
    assert model.loss_names == g["loss_names"]
    model.data_dependent_initialize({"A": s["A"], "B": s["B"]})
    assert list(model.netG_A.state_dict().keys()) == g["keysG"] and list(model.netF.state_dict().keys()) == g["keysF"]
    assert list(model.netD_B_basic.state_dict().keys()) == g["keysD"]
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.netD_B_basic.load_state_dict(O.synth_state_dict(model.netD_B_basic.state_dict(), seed=1))
    model.netF.load_state_dict(O.synth_state_dict(model.netF.state_dict(), seed=3))
    model.set_pool_rng(ReplayRandom(s["pool_draws"]))
    nl = len(c["nce_layers"].split(","))
    ids_ab, ids_idt = cut_ids(s, nl, c["num_patches"])
    model.patch_ids_injection = lambda call, shapes: [i.to(D0) for i in (ids_ab if call == 0 else ids_idt)]
    model.set_input({"A": s["A"], "B": s["B"]})
    model.optimize_parameters()
    torch.cuda.synchronize()
    losses = {k: float(v) for k, v in model.get_current_losses().items()}
    tol = TOL_LOSS_FWD[dtype]
    checked = [n for n in g["loss_names"] if n.startswith("G_")]
    assert ("G_supervised" in checked) == (name != "hdce_idt") and ("G_MSE_idt" in checked) == (name != "mse")
    for n in checked:
        ref = s["losses"][n]
        print(name, n, losses[n], ref)
        assert abs(losses[n] - ref) <= tol * abs(ref) + 1e-4, (n, losses[n], ref)
    for n in ("supervised", "MSE_idt"):
        if "G_" + n in checked:
            assert getattr(model, "loss_G_" + n).is_cuda
    assert model.loss_G_SRC == 0.0 and "G_SRC" not in model.loss_names


_PIX_CUT = {"model_type": "cut", "G": {"netG": "resnet", "ngf": 32, "nblocks": 2}, "D": {"netDs": ["projected_d", "basic"], "ndf": 32, "proj_interp": 128},
            "alg": {"cut": {"nce_layers": "0,4,8", "nce_loss": "SRC_hDCE", "num_patches": 128, "HDCE_gamma": 0.5, "supervised_loss": ["L1"],
                            "lambda_supervised": 2.0, "MSE_idt": True, "lambda_MSE_idt": 0.5}}, "data": {"crop_size": 64, "load_size": 64},
            "train": {"batch_size": 2, "G_ema": True, "iter_size": 1, "pool_size": 0, "G_lr": 0.0, "D_lr": 0.0}}
_G_LOSSES = ["G_NCE", "G_NCE_Y", "G_supervised", "G_MSE_idt", "G_tot"]


def _run(monkeypatch, driver, batched, calls, pixel=True, other_last=False):
    """`calls` x optimize_parameters() from seed 3 (the setup of test_gpu_10_hdce.py::_run) at learning rate zero; driver "sequential" (the
    reference's order) or "default" (no switch set); `other_last`: the last call runs on another batch.  Returns the losses of every call
    (`_G_LOSSES` where they exist, then the D terms), Adam's first moments (a linear image of every gradient), the driver of every call and
    whether the pixel-loss attributes were device tensors after every call."""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    for var in ("JG_EARLY_D", "JG_GRAPH_D", "JG_GRAPH_G"):
        if driver == "sequential":
            monkeypatch.setenv(var, "0")
        else:
            monkeypatch.delenv(var, raising=False)
    monkeypatch.delenv("JG_DBG_GRAPH_CANARY_FAIL", raising=False)
    monkeypatch.setenv("JG_BATCHED_NCE", "1" if batched else "0")
    gen = torch.Generator().manual_seed(14)
    data = {"A": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1, "B": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1}
    other = {"A": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1, "B": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1}
    cfg = _PIX_CUT
    if not pixel:
        cfg = dict(cfg, alg={"cut": {k: v for k, v in cfg["alg"]["cut"].items() if k not in ("supervised_loss", "lambda_supervised", "MSE_idt", "lambda_MSE_idt")}})
    torch.manual_seed(3)
    random.seed(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = create_model(opt_from_json(cfg, overrides={"jg_act_dtype": "bf16", "gpu_ids": "0"}), 0)
        m.data_dependent_initialize(data)
        m.setup(m.opt)
        m.single_gpu()
        names = [n for n in _G_LOSSES if n in m.loss_names]
        losses, drivers, on_device = [], [], []
        for i in range(calls):
            m.set_input(other if other_last and i == calls - 1 else data)
            m.optimize_parameters()
            on_device.append(all(getattr(m, "loss_" + n).is_cuda for n in names if n in ("G_supervised", "G_MSE_idt")))
            losses.append([float(getattr(m, "loss_" + n)) for n in names] + [float(getattr(m, "loss_D_GAN_" + dn)) for dn in m.discriminators_names])
            drivers.append(m.step_driver)
    torch.cuda.synchronize()
    return dict(losses=torch.tensor(losses, dtype=torch.float64), names=names, m1={n: m._net(n).arena.m.detach().double().cpu() for n in m.model_names},
                driver=m.step_driver, drivers=drivers, on_device=on_device, note=m.step_driver_note,
                dropped=[str(w.message) for w in rec if "jg_graph_" in str(w.message)])


def test_cut_pixel_loss_batched_matches_the_four_pass_form(monkeypatch):
    """L1 supervised + identity loss with SRC_hDCE: the batched form (both contrastive terms weighted: wperiod = wcount = 1; the pixel terms
    from the shared helper) against the sequential four-pass computation: same seed, no injection; losses and Adam's first moments of
    G / F / D to 4 x the measured run-to-run floor of the four-pass form + 2e-3"""
    a = _run(monkeypatch, "sequential", False, 3)
    a2 = _run(monkeypatch, "sequential", False, 3)
    b = _run(monkeypatch, "sequential", True, 3)
    assert a["names"] == _G_LOSSES
    floor_l = float(((a["losses"] - a2["losses"]).abs() / a["losses"].abs()).max())
    floor_p = max(float((a["m1"][n] - a2["m1"][n]).norm() / a["m1"][n].norm()) for n in a["m1"])
    print("run-to-run floor of the four-pass form: losses %.2e, first moments %.2e" % (floor_l, floor_p))
    assert torch.isfinite(b["losses"]).all()
    e_l = float(((b["losses"] - a["losses"]).abs() / a["losses"].abs()).max())
    print("batched against four-pass: losses %.2e" % e_l)
    assert e_l <= 4 * floor_l + 2e-3, (b["losses"], a["losses"])
    for n in a["m1"]:
        e = float((b["m1"][n] - a["m1"][n]).norm() / a["m1"][n].norm())
        print("first moments of", n, "%.2e" % e)
        assert e <= 4 * floor_p + 2e-3, (n, e, floor_p)


def test_cut_pixel_loss_takes_the_default_step_driver(monkeypatch):
    """with no driver switch set the step runs on the captured graphs (the options are no reason to fall back), the losses of its first call
    agree with the sequential driver's at the forward tolerance, and the replayed graph publishes the new loss attributes: finite, on the
    device, and different after a replay on another batch"""
    import joligen_amd

    seq = _run(monkeypatch, "sequential", True, 1)
    r = _run(monkeypatch, "default", True, 7, other_last=True)
    assert seq["driver"] == "sequential"
    assert r["driver"] != "sequential", (r["driver"], r["note"])
    assert "pixel" not in r["note"] and "supervised" not in r["note"] and "MSE_idt" not in r["note"], r["note"]
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert r["drivers"][-2:] == ["graph+graphG"] * 2 and not r["dropped"], (r["drivers"], r["note"], r["dropped"])
    assert torch.isfinite(r["losses"]).all() and all(r["on_device"])
    l0, s0 = r["losses"][0], seq["losses"][0]
    assert float(((l0 - s0).abs() / s0.abs()).max()) <= TOL_LOSS_FWD[torch.bfloat16], (l0, s0)
    for n in ("G_supervised", "G_MSE_idt"):
        i = r["names"].index(n)
        same, moved = r["losses"][-3:-1, i], r["losses"][-1, i]
        print(n, "replays on one batch", same.tolist(), "then on another", float(moved))
        assert float(same[0]) > 0 and abs(float(same[0]) - float(same[1])) <= 1e-3 * float(same[0])      # learning rate 0: the same value again
        assert abs(float(moved) - float(same[1])) > 1e-3 * float(same[1]), (n, same, moved)


def test_cut_default_step_launches_no_pixel_loss(monkeypatch):
    """with both options off the helper launches nothing: a counter on ops.pixel_loss stays at 0 over two steps"""
    from joligen_amd import ops

    count = [0]
    real = ops.pixel_loss

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "pixel_loss", counted)
    r = _run(monkeypatch, "default", True, 2, pixel=False)
    assert r["names"] == ["G_NCE", "G_NCE_Y", "G_tot"] and torch.isfinite(r["losses"]).all()
    assert count[0] == 0
    r = _run(monkeypatch, "sequential", True, 1)      # (the counter does count when the options are on)
    assert count[0] == 1 and r["names"] == _G_LOSSES
