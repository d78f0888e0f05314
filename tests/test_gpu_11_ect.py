"""GPU tests of easy consistency tuning (cm_model, alg_ddpm_ft_mode = "ect"): the fused loss kernel (jg_ect_loss) against the float64
restatement of tests/ect_ref.py on identical 16-bit inputs, its run-to-run bits, the autograd and torch.ops surfaces, CMGenerator.forward
and 3 x optimize_parameters() against fixtures of the unmodified reference (tests/tools/make_fixture_ect.py -> tests/golden/ect/), and
one step at a shape where the halo kernels and flash attention are live."""
import os

import pytest
import torch

import ect_ref as R
import jg_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ECT_DIR = os.path.join(HERE, "golden", "ect")
# where the measured tables (floors, device errors, update cosines, gradient errors) go: JG_TEST_OUT, else test_out/ beside tests/
OUT_DIR = os.environ.get("JG_TEST_OUT") or os.path.join(os.path.dirname(HERE), "test_out")
CFGS = ["tiny_eff", "tiny_attn"]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
# (B, C, H, W) at Cpad = 8: one block; one channel; a pixel count (960) that is no multiple of the block; several blocks per sample plus
# a remainder (5184 = 20 * 256 + 64)
SHAPES = [(1, 3, 16, 16), (2, 1, 8, 8), (3, 3, 24, 40), (2, 4, 72, 72)]
CPAD = 8
TOL_KERNEL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}          # the project's single-kernel bound (README)
LAM, GRAD_SCALE = 1.5, 8.0


def load(name):
    return torch.load(os.path.join(ECT_DIR, name), weights_only=False)


def ordered_bits(x):
    """16-bit float -> integers in the order of the values (+0 and -0 both 0): neighbours differ by one"""
    b = x.cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def kernel_inputs(shape, dtype, mask_kind, seed=5):
    """CPU tensors as jg_ect_loss reads them.  dt spans 1e-3 .. 50; sample 0 has cs_c = 1, co_c = 0 (the r = 0 teacher); the pad channels of
    the UNet outputs hold values the kernel must not use; `label`: values 0 / 1 / 2, and the last sample all zero when there are two"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    Fn = torch.randn(B, H, W, CPAD, generator=g).to(dtype)
    Fc = torch.randn(B, H, W, CPAD, generator=g).to(dtype)
    noisy_n = torch.randn(B, C, H, W, generator=g)
    noisy_c = noisy_n + 0.3 * torch.randn(B, C, H, W, generator=g)
    t = torch.exp(torch.randn(B, generator=g) * R.P_STD + R.P_MEAN)
    dt = torch.logspace(-3, 1.69897, B) if B > 1 else torch.tensor([1e-3])
    r = torch.clamp(t - dt, min=0)
    r[0] = 0.0
    cs_n, co_n, cs_c, co_c = R.skip_train(t), R.out_train(t), R.skip_train(r), R.out_train(r)
    assert float(cs_c[0]) == 1.0 and float(co_c[0]) == 0.0
    mask = None
    if mask_kind != "none":
        mask = (torch.rand(B, 1, H, W, generator=g) < 0.6).long()
        if mask_kind == "label":
            mask = mask * torch.randint(1, 3, (B, 1, H, W), generator=g)
            assert int(mask.max()) == 2
            if B > 1:
                mask[B - 1] = 0
    return Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, dt


def launch(args):
    from joligen_amd import ops

    d = torch.device("cuda:0")
    dev = [None if a is None else a.to(d) for a in args]
    Fn = dev[0].requires_grad_(True)
    loss = ops.ect_loss(Fn, *dev[1:], lam=LAM, grad_scale=GRAD_SCALE)
    dFn = loss.grad_fn.saved_tensors[0]
    return loss, dFn, Fn, dev


@pytest.mark.parametrize("mask_kind", ["none", "binary", "label"])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ect_loss_kernel_vs_float64_restatement(shape, dtype_name, mask_kind):
    dtype = DTYPES[dtype_name]
    B, C, H, W = shape
    args = kernel_inputs(shape, dtype, mask_kind)
    loss, dFn, _, _ = launch(args)
    loss_ref, dFn_ref = R.ect_loss_nhwc(*args, c=R.ECT_C, lam=LAM, grad_scale=GRAD_SCALE)
    loss, dFn = float(loss.detach()), dFn.detach().cpu()
    mask = args[8]
    e_loss = abs(loss - float(loss_ref)) / abs(float(loss_ref)) if float(loss_ref) != 0 else abs(loss)
    ulps = (ordered_bits(dFn) - ordered_bits(dFn_ref.to(dtype))).abs()
    e_norm = R.relerr(dFn, dFn_ref)
    print(f"ect_loss {shape} {dtype_name} {mask_kind}: loss {loss:.6e} ref {float(loss_ref):.6e} rel {e_loss:.2e}; dFn max ulp {int(ulps.max())} "
          f"(elements off by one: {int((ulps == 1).sum())} of {ulps.numel()}), norm {e_norm:.2e}")
    assert torch.isfinite(dFn).all() and loss == loss
    assert e_loss < 1e-5, (loss, float(loss_ref))
    assert int(ulps.max()) <= 1, int(ulps.max())
    assert e_norm < TOL_KERNEL[dtype], e_norm
    assert bool((dFn[..., C:] == 0).all())                                   # pad channels
    if mask is not None:
        off = (mask == 0).permute(0, 2, 3, 1).expand(B, H, W, CPAD)
        assert bool((dFn[off] == 0).all())
        if mask_kind == "label" and B > 1:                                   # all-zero sample: loss_b = 0 and a zero gradient, not NaN
            assert bool((dFn[B - 1] == 0).all())
            keep = [a if (a is None or a.dim() == 0) else a[: B - 1] for a in args]
            loss_keep, _ = R.ect_loss_nhwc(*keep, c=R.ECT_C, lam=LAM, grad_scale=GRAD_SCALE)
            assert abs(loss - float(loss_keep) * (B - 1) / B) < 1e-5 * abs(loss)


def test_ect_loss_all_zero_mask_single_sample():
    """B = 1 with nothing inside the mask: S = 0, loss = (sqrt(c^2) - c) / dt = 0, gradient 0"""
    args = list(kernel_inputs((1, 3, 16, 16), torch.float16, "binary"))
    args[8] = torch.zeros_like(args[8])
    loss, dFn, _, _ = launch(args)
    assert abs(float(loss.detach())) < 1e-9 and bool((dFn == 0).all())


def test_ect_loss_same_bits_on_every_launch():
    """no atomics: loss and gradient are bit-identical run to run, and with JG_DETERMINISTIC on or off"""
    from joligen_amd import _lib

    args = kernel_inputs((2, 4, 72, 72), torch.bfloat16, "label")
    lib = _lib.lib()
    was = lib.jg_get_tuning(b"JG_DETERMINISTIC")
    runs = []
    try:
        for det in (0, 0, 1, 1, 0):
            lib.jg_set_tuning(b"JG_DETERMINISTIC", det)
            loss, dFn, _, _ = launch(args)
            runs.append((loss.detach().clone(), dFn.clone()))
    finally:
        lib.jg_set_tuning(b"JG_DETERMINISTIC", was)
    for loss, dFn in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(dFn, runs[0][1])


def test_ect_loss_argument_checks():
    from joligen_amd import _lib, ops

    args = kernel_inputs((2, 3, 8, 8), torch.float16, "none")
    _, _, _, dev = launch(args)
    wide = [torch.zeros(2, 8, 8, 16, device="cuda:0", dtype=torch.float16) for _ in range(2)]
    with pytest.raises(RuntimeError, match="jg_ect_loss"):                   # Cpad = 16 is refused, not handled silently
        ops.ect_loss(wide[0], wide[1], *dev[2:], lam=1.0, grad_scale=1.0)
    lib = _lib.lib()
    Fn, Fc, nn_, nc = dev[:4]
    v = dev[4:8] + [dev[9]]
    ws, loss, dFn = torch.empty(2, device="cuda:0"), torch.empty((), device="cuda:0"), torch.empty_like(Fn)
    call = lambda cpad, nws: lib.jg_ect_loss(0, Fn.data_ptr(), Fc.data_ptr(), nn_.data_ptr(), nc.data_ptr(), *[t.data_ptr() for t in v[:4]], None,
                                             v[4].data_ptr(), ws.data_ptr(), nws, loss.data_ptr(), dFn.data_ptr(), 2, 3, 8, 8, cpad, 1e-6, 1.0, 1.0, None)
    assert call(16, 2) == _lib.JG_ERR_UNSUPPORTED
    assert call(8, 1) == _lib.JG_ERR_BAD_ARG                                 # workspace too small for B * blocks partial sums
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ect_loss(*[None if a is None else a.cpu() for a in dev], lam=1.0, grad_scale=1.0)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_ect_loss_backward_scales_the_saved_gradient(dtype_name):
    """loss.backward(0.5): F_next.grad = 0.5 * the saved gradient to the rounding of axpby (one 16-bit rounding of an exact halving: the
    same bits unless the result is subnormal); F_cur receives none"""
    dtype = DTYPES[dtype_name]
    args = kernel_inputs((3, 3, 24, 40), dtype, "binary")
    from joligen_amd import ops

    d = torch.device("cuda:0")
    dev = [None if a is None else a.to(d) for a in args]
    Fn, Fc = dev[0].requires_grad_(True), dev[1].requires_grad_(True)
    loss = ops.ect_loss(Fn, Fc, *dev[2:], lam=LAM, grad_scale=GRAD_SCALE)
    dFn = loss.grad_fn.saved_tensors[0].clone()
    loss.backward(torch.tensor(0.5, device=d))
    assert Fc.grad is None
    want = (dFn.float() * 0.5).to(dtype)
    assert int((ordered_bits(Fn.grad) - ordered_bits(want)).abs().max()) <= 1
    assert R.relerr(Fn.grad, dFn.float() * 0.5) < 1e-3


def test_ect_loss_torch_op_opcheck():
    """schema + fake kernel + autograd registration of torch.ops.jg355.ect_loss; the op computes what the ctypes path computes"""
    from joligen_amd import ops

    J = torch.ops.jg355
    for mask_kind in ("none", "label"):
        args = kernel_inputs((2, 3, 24, 40), torch.bfloat16, mask_kind)
        loss, dFn, _, dev = launch(args)
        Fn = dev[0].detach().clone().requires_grad_(True)
        torch.library.opcheck(J.ect_loss.default, (Fn, *dev[1:], LAM, GRAD_SCALE),
                              test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
        l2, g2 = J.ect_loss(Fn, *dev[1:], LAM, GRAD_SCALE)
        assert torch.equal(l2.detach(), loss.detach()) and torch.equal(g2, dFn)
        l2.backward(torch.tensor(0.5, device=l2.device))
        assert R.relerr(Fn.grad, dFn.float() * 0.5) < 1e-3
        with ops.torch_ops_boundary():
            l3 = ops.ect_loss(Fn, *dev[1:], lam=LAM, grad_scale=GRAD_SCALE)
        assert torch.equal(l3.detach(), loss.detach())


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def make_model(c, dtype_name, hp=None, ft_mode="ect"):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(model_type="cm", G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"],
              G_unet_mha_attn_res=c["attn_res"], G_unet_mha_vit_efficient=c["efficient"], data_crop_size=c["S"],
              train_batch_size=c["B"], gpu_ids="0", jg_act_dtype=dtype_name, train_optim="adamw", train_G_ema=True,
              train_iter_size=1, checkpoints_dir="/tmp/jg_amd_ckpt/", name="ect", alg_ddpm_ft_mode=ft_mode)
    if hp:
        ov.update(train_G_lr=hp["lr"], train_beta1=hp["beta1"], train_beta2=hp["beta2"], train_optim_eps=hp["eps"],
                  train_optim_weight_decay=hp["weight_decay"], train_G_ema_beta=hp["ema_beta"], train_G_ema=hp["ema"],
                  alg_diffusion_lambda_G=hp["lambda_G"], train_optim=hp["optim"])
    opt = opt_from_json({}, ov)
    model = create_model(opt, 0)
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.setup(opt)
    model.single_gpu()
    return model


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("name", CFGS)
def test_ect_generator_vs_reference_golden(name, dtype_name):
    from test_gpu_2_cm import TOL_OUT, relerr

    g = load(f"ect_gen_{name}.pt")
    dtype = DTYPES[dtype_name]
    model = make_model(g["cfg"], dtype_name)
    assert model.total_t == g["total_t"] and model.ft_mode == "ect"
    d = torch.device("cuda:0")
    net = model.netG_A
    assert net.training and net.current_t == 0 and net.stage == 0
    with torch.no_grad():
        out = net(g["B"].to(d), g["total_t"], g["mask"].to(d), None, noise=g["noise"], rnd_normal=g["rnd_normal"])
    assert len(out) == 6 and net.current_t == g["cfg"]["B"]
    D_yt, D_yr, t_noisy_x, r_noisy_x, t, r = out
    assert relerr(t, g["t"]) < 1e-6 and relerr(r, g["r"]) < 1e-6
    assert torch.equal(r.cpu() == 0, g["r"] == 0) and bool((g["r"] == 0).any()) and bool((g["r"] > 0).any())
    assert relerr(t_noisy_x, g["t_noisy_x"]) < 1e-6 and relerr(r_noisy_x, g["r_noisy_x"]) < 1e-6
    keep = (g["mask"] == 0).expand_as(g["B"])                                # bit-exact mask semantics: unmasked pixels are copies of x
    assert torch.equal(t_noisy_x.cpu()[keep], g["B"][keep]) and torch.equal(r_noisy_x.cpu()[keep], g["B"][keep])
    z = (r == 0).cpu()
    assert torch.equal(D_yr.cpu()[z], r_noisy_x.cpu()[z])                    # r = 0: scalings (1, 0), the teacher returns its input
    e_t, e_r = relerr(D_yt, g["D_yt"]), relerr(D_yr, g["D_yr"])
    print(f"ect generator {name} {dtype_name}: D_yt {e_t:.2e} D_yr {e_r:.2e}")
    assert e_t < TOL_OUT[dtype] and e_r < TOL_OUT[dtype], (e_t, e_r)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("name", CFGS)
def test_ect_three_steps_vs_reference_golden(name, dtype_name):
    """3 x optimize_parameters() with the reference's recorded (noise, rnd_normal), TEACHER-FORCED by the CPU oracle (tests/parity_util.py;
    the oracle reproduces the fixture's loss of every iteration, re-asserted here).  Per iteration: the loss on identical weights, then the
    parameter / EMA update against the oracle's.  Loss bound: the larger of test_gpu_2_cm's TOL_LOSS_FWD and twice the floor measured here,
    the oracle with 16-bit storage between layers (O.activation_rounding) against itself in fp32 on the same weights and inputs."""
    import parity_util as PU
    from test_gpu_2_cm import COS_UPDATE, TOL_LOSS_FWD
    from test_oracle_golden import cm_cfg_of

    g = load(f"ect_step_{name}.pt")
    dtype = DTYPES[dtype_name]
    hp, cfg = g["hp"], cm_cfg_of(g["cfg"])
    model = make_model(g["cfg"], dtype_name, hp)
    assert model.group_G.backward_functions == ["compute_ect_loss"]
    net = model.netG_A
    sd0 = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    kw = dict(lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], weight_decay=hp["weight_decay"],
              ema_beta=hp["ema_beta"] if hp["ema"] else None, lambda_G=hp["lambda_G"], optim=hp["optim"])
    tr = R.OracleECTTrainer(sd0, cfg, g["total_t"], **kw)
    log = []
    for it, s in enumerate(g["steps"]):
        PU.force_state(net, {k: tr.P[k] for k in tr.param_names}, tr.m, tr.v, tr.step, tr.ema)
        before, ref_before = PU.snapshot(net), {k: tr.P[k].clone() for k in tr.param_names}
        ema_before = None if tr.ema is None else {k: v.clone() for k, v in tr.ema.items()}
        tr16 = R.OracleECTTrainer(tr.P, cfg, g["total_t"], **kw)
        tr16.grad_scale = model.loss_scale
        with O.activation_rounding(dtype):
            loss_16 = float(tr16.loss_and_grads(s["B"], s["mask"], s["noise"], s["rnd_normal"])[0])
        model.rng_injection = lambda b, s=s: (s["noise"], s["rnd_normal"])
        model.set_input({"A": s["A"], "B": s["B"], "B_label_mask": s["mask"], "A_img_paths": ["x"]})
        model.optimize_parameters()
        loss = float(torch.as_tensor(model.get_current_losses()["G_tot"]).detach())
        loss_ref = float(tr.optimize_parameters(s["B"], s["mask"], s["noise"], s["rnd_normal"]))
        assert abs(loss_ref - float(s["loss"])) < 2e-4 * abs(float(s["loss"])) + 1e-6
        floor, err = abs(loss_16 - loss_ref) / abs(loss_ref), abs(loss - loss_ref) / abs(loss_ref)
        bound = max(TOL_LOSS_FWD[dtype], 2.0 * floor)
        log.append(f"{name} {dtype_name} it{it}: loss {loss:.6f} oracle {loss_ref:.6f} device error {err:.3e} 16-bit-storage floor {floor:.3e} "
                   f"bound {bound:.3e} r {s['r'].tolist()}")
        print(log[-1])
        assert err < bound, (it, loss, loss_ref, floor)
        after = PU.snapshot(net)
        PU.check_update(f"{name} {dtype_name} it{it}", before, after, ref_before, {k: tr.P[k] for k in tr.param_names},
                        COS_UPDATE[dtype], log=log)
        if hp["ema"]:
            ema = {k: v.detach().float().cpu() for k, v in model.netG_A_ema.named_parameters()}
            PU.check_ema(f"ema it{it}", ema_before, ema, after, hp["ema_beta"], first=ema_before is None)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"update_agreement_ect_{name}_{dtype_name}.txt"), "w") as f:
        f.write("\n".join(log))
    B = g["cfg"]["B"]
    assert net.current_t == 3 * B and model.ect_state["cur_nimg"] == 3 * B and model.ect_state["cur_tick"] == 0
    model.compute_visuals(B)
    vis = model.get_current_visuals(B)
    assert len(vis) == B and list(vis[0].keys()) == [n + "0" for n in g["visual_names"]]
    assert list(vis[0].keys()) == ["gt_image_0", "y_t_0", "t_noisy_x_0", "r_noisy_x_0", "mask_0", "output_0"]
    test_vis = model.get_current_visuals(B, phase="test", test_name="t")
    assert test_vis and all("noisy" not in k for v in test_vis for k in v)


def test_ect_first_step_gradients_vs_oracle_halo_and_flash_attention():
    """64x64, ngf 64, B = 2 (halo kernels, fused statistics, flash attention live), a drawn rnd_normal with one r = 0 and one r > 0: loss and
    every weight gradient against the CPU oracle, bounded as in test_cm_c5_shape_first_step_gradients_vs_oracle by twice the rounding floor
    MEASURED on the same inputs (the oracle with 16-bit storage between layers)."""
    from test_gpu_2_cm import TOL_LOSS_FWD, relerr

    c = dict(ngf=64, mults=[1, 2], res_blocks=[1, 1], attn_res=[2], efficient=True, S=64, B=2)
    model = make_model(c, "fp16")
    net = model.netG_A
    sd = {k: (v.float().cpu().half().float() if (torch.is_floating_point(v) and v.dim() >= 3) else v.float().cpu()) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    cfg = O.UNetCfg(in_channel=3, inner_channel=64, out_channel=3, res_blocks=[1, 1], attn_res=[2], channel_mults=[1, 2], efficient=True,
                    cond_embed_dim=256)
    g = torch.Generator().manual_seed(9)
    Bimg = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).half().float()
    mask = torch.zeros(2, 1, 64, 64, dtype=torch.int64)
    mask[:, :, 10:40, 20:50] = 1
    A = Bimg * (1 - mask) + torch.randn(Bimg.shape, generator=g).half().float() * mask
    seed = 3
    while True:                                                              # the first seed whose draw takes both branches
        gd = torch.Generator().manual_seed(seed)
        rnd_normal = torch.randn(2, generator=gd)
        r = R.t_to_r((rnd_normal * R.P_STD + R.P_MEAN).exp())
        if bool((r == 0).any()) and bool((r > 0).any()):
            break
        seed += 1
    noise = torch.randn(Bimg.shape, generator=gd)
    tr = R.OracleECTTrainer(sd, cfg, model.total_t)
    loss_ref, grads, _ = tr.loss_and_grads(Bimg, mask, noise, rnd_normal)
    tr16 = R.OracleECTTrainer(sd, cfg, model.total_t)
    tr16.grad_scale = model.loss_scale
    with O.activation_rounding(torch.float16):
        loss_16, grads16, _ = tr16.loss_and_grads(Bimg, mask, noise, rnd_normal)
    model.rng_injection = lambda b: (noise, rnd_normal)
    model.set_input({"A": A, "B": Bimg, "B_label_mask": mask})
    net.arena.g.zero_()
    model.compute_ect_loss()
    model.loss_G_tot.backward()
    torch.cuda.synchronize()
    loss_ref, loss_16, loss = float(loss_ref), float(loss_16), float(model.loss_G_tot)
    floor_l, err_l = abs(loss_16 - loss_ref) / abs(loss_ref), abs(loss - loss_ref) / abs(loss_ref)
    scale = model.loss_scale
    mine_e, floor_e = [], []
    for k, p in net.named_parameters():
        if (k.endswith(".weight") and p.dim() >= 2) and float(grads[k].norm()) > 1e-12:
            mine_e.append((relerr(p.grad.detach().float().cpu() / scale, grads[k]), k))
            floor_e.append(relerr(grads16[k], grads[k]))
    mine_e.sort(reverse=True)
    floor_e.sort(reverse=True)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, "grad_table_ect_64_fp16.txt"), "w") as f:
        f.write(f"# seed {seed} r {r.tolist()} loss {loss:.6f} oracle {loss_ref:.6f} device error {err_l:.3e} floor {floor_l:.3e}\n")
        f.write(f"# rounding floor (oracle, 16-bit storage): worst {floor_e[0]:.3e} median {floor_e[len(floor_e) // 2]:.3e}\n")
        f.write("\n".join(f"{e:10.3e} {k}" for e, k in mine_e))
    print(f"ect 64x64: loss error {err_l:.3e} floor {floor_l:.3e}; gradients worst {mine_e[0][0]:.3e} (floor {floor_e[0]:.3e}) median "
          f"{mine_e[len(mine_e) // 2][0]:.3e} (floor {floor_e[len(floor_e) // 2]:.3e})")
    assert err_l < max(TOL_LOSS_FWD[torch.float16], 2.0 * floor_l), (loss, loss_ref, floor_l)
    assert mine_e[0][0] <= max(2.0 * floor_e[0], 2e-2), (mine_e[:5], floor_e[:3])
    assert mine_e[len(mine_e) // 2][0] <= max(1.5 * floor_e[len(floor_e) // 2], 5e-3), (mine_e[len(mine_e) // 2], floor_e[len(floor_e) // 2])


def test_example_cm_json_with_ect_runs_a_training_window(tmp_path):
    """examples/example_cm_noglasses2glasses.json (tests/golden/examples/: a verbatim copy, settings only) with alg_ddpm_ft_mode = "ect"
    constructs, and one accumulation window of its own train_iter_size runs through optimize_parameters(): finite losses, the weights move
    at the window boundary, the counters advance"""
    import math

    from bench import synth_batch
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(output_display_type=["none"], output_print_freq=10 ** 9, checkpoints_dir=str(tmp_path), gpu_ids="0", train_metrics_list=[],
              jg_act_dtype="bf16", name="ect_e2e", data_crop_size=64, data_load_size=64, train_batch_size=2, alg_ddpm_ft_mode="ect")
    opt = opt_from_json(os.path.join(HERE, "golden", "examples", "example_cm_noglasses2glasses.json"), ov)
    assert opt.model_type == "cm" and opt.alg_ddpm_ft_mode == "ect" and opt.train_iter_size == 16
    model = create_model(opt, 0)
    model.setup(opt)
    model.single_gpu()
    data = synth_batch(2, 64, 3, torch.device("cuda:0"))
    torch.manual_seed(0)
    net = model._net("G_A")
    start = float(net.arena.p.double().sum())
    for j in range(opt.train_iter_size):
        model.set_input(data)
        model.optimize_parameters()
        assert (float(net.arena.p.double().sum()) != start) == (j == opt.train_iter_size - 1), j
    losses = {k: float(v) for k, v in model.get_current_losses().items()}
    assert losses and all(math.isfinite(v) for v in losses.values()) and all(v > 0 for k, v in losses.items() if k.startswith("G_tot")), losses
    assert net.current_t == 32 and model.ect_state["cur_nimg"] == 32 and net.stage == 0


def test_cm_mode_keeps_its_loss_group():
    c = dict(ngf=32, mults=[1, 2], res_blocks=[1, 1], attn_res=[16], efficient=True, S=16, B=2)
    model = make_model(c, "bf16", ft_mode="cm")
    assert model.ft_mode == "cm" and model.group_G.backward_functions == ["compute_cm_loss"] and not hasattr(model, "ect_state")
    assert model.gen_visual_names == ["gt_image_", "y_t_", "next_noisy_x_", "current_noisy_x_", "mask_", "output_"]
    with pytest.raises(NotImplementedError, match="alg_ddpm_ft_mode"):
        make_model(c, "bf16", ft_mode="other")
