"""GPU tests of cm_gan (consistency training with discriminators): the fused seam kernels (jg_cm_gan_head / jg_cm_gan_head_bwd) against
ops.cm_loss on the same inputs and against the float64 restatement of tests/cm_gan_ref.py, their run-to-run bits, the autograd and torch.ops
surfaces; 3 x CMGanModel.optimize_parameters() against fixtures of the unmodified reference (tests/tools/make_fixture_cm_gan.py ->
tests/golden/cm_gan/), the routing of the discriminator's gradient into the UNet at a shape where the halo kernels and flash attention are
live, and the reference's example configuration over one accumulation window."""
import math
import os

import pytest
import torch

import cm_gan_ref as R
import jg_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "cm_gan")
EXAMPLE = os.path.join(HERE, "golden", "examples", "example_cm_gan_noglasses2glasses.json")
# where the measured tables (floors, device errors, update cosines, gradient errors) go: JG_TEST_OUT, else test_out/ beside tests/
OUT_DIR = os.environ.get("JG_TEST_OUT") or os.path.join(os.path.dirname(HERE), "test_out")
CFGS = ["tiny_eff", "tiny_attn"]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -24, torch.bfloat16: -133}             # exponent of the smallest subnormal
# the shapes of test_gpu_11_ect.py: one block; one channel; a pixel count (960) that is no multiple of the block; several blocks plus a remainder
SHAPES = [(1, 3, 16, 16), (2, 1, 8, 8), (3, 3, 24, 40), (2, 4, 72, 72)]
CPAD = 8
LAM, GRAD_SCALE = 1.5, 8.0
D0 = "cuda:0"


def load(name):
    return torch.load(os.path.join(DIR, name), weights_only=False)


def ordered_bits(x):
    """16-bit float -> integers in the order of the values (+0 and -0 both 0): neighbours differ by one"""
    b = x.cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def ulp16(x, dtype):
    """the spacing of `dtype` at |x| (float64 in, float64 out)"""
    _, e = torch.frexp(x.abs().double())
    return torch.pow(2.0, torch.clamp(e.double() - 1 - MANT[dtype], min=MIN_EXP[dtype]))


def kernel_inputs(shape, dtype, mask_kind, seed=5):
    """CPU tensors as jg_cm_gan_head reads them: the scalings of the consistency schedule at drawn noise levels, loss weights over three
    decades; the pad channels of the UNet outputs hold values the kernel must not use; `label`: values 0 / 1 / 2, and the last sample all
    zero when there are two.  Nothing but the mask depends on `mask_kind`."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    Fn = torch.randn(B, H, W, CPAD, generator=g).to(dtype)
    Fc = torch.randn(B, H, W, CPAD, generator=g).to(dtype)
    noisy_n = torch.randn(B, C, H, W, generator=g)
    noisy_c = noisy_n + 0.3 * torch.randn(B, C, H, W, generator=g)
    sig_n = torch.exp(torch.randn(B, generator=g) * 2.0 - 1.1) + 0.002
    sig_c = sig_n * 0.8
    cs_n, co_n, cs_c, co_c = O.cm_skip_scaling(sig_n), O.cm_output_scaling(sig_n), O.cm_skip_scaling(sig_c), O.cm_output_scaling(sig_c)
    w = torch.logspace(-1, 2, B) if B > 1 else torch.tensor([3.0])
    gm = torch.Generator().manual_seed(seed + 1)
    mask = None
    if mask_kind != "none":
        mask = (torch.rand(B, 1, H, W, generator=gm) < 0.6).long()
        if mask_kind == "label":
            mask = mask * torch.randint(1, 3, (B, 1, H, W), generator=gm)
            assert int(mask.max()) == 2
            if B > 1:
                mask[B - 1] = 0
    return Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w


def to_dev(args):
    return [None if a is None else a.to(D0) for a in args]


def launch(args):
    """(loss, pred, the saved dFn_cm, F_next leaf, device arguments) of ops.cm_gan_head"""
    from joligen_amd import ops

    dev = to_dev(args)
    Fn = dev[0].requires_grad_(True)
    loss, pred = ops.cm_gan_head(Fn, *dev[1:], lam=LAM, grad_scale=GRAD_SCALE)
    return loss, pred, loss.grad_fn.saved_tensors[0], Fn, dev


def launch_cm_loss(args):
    from joligen_amd import ops

    dev = to_dev(args)
    loss = ops.cm_loss(dev[0].requires_grad_(True), *dev[1:], lam=LAM, grad_scale=GRAD_SCALE)
    return loss, loss.grad_fn.saved_tensors[0]


class deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from joligen_amd import _lib

        self.lib = _lib.lib()
        self.was = self.lib.jg_get_tuning(b"JG_DETERMINISTIC")
        self.lib.jg_set_tuning(b"JG_DETERMINISTIC", self.on)

    def __exit__(self, *a):
        self.lib.jg_set_tuning(b"JG_DETERMINISTIC", self.was)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["none", "binary", "label"])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_forward_vs_cm_loss_and_float64_restatement(shape, dtype_name, mask_kind):
    dtype = DTYPES[dtype_name]
    B, C, H, W = shape
    args = kernel_inputs(shape, dtype, mask_kind)
    loss_ref, pred_ref, _ = R.head_nhwc(*args, lam=LAM, grad_scale=GRAD_SCALE)
    with deterministic(0):
        loss, pred, dFn, _, _ = launch(args)
        _, dFn_cm = launch_cm_loss(args)
    with deterministic(1):
        loss_d, pred_d, dFn_d, _, _ = launch(args)
        loss_cm_d, dFn_cm_d = launch_cm_loss(args)
    loss, loss_d, pred, pred_d = loss.detach(), loss_d.detach(), pred.detach(), pred_d.detach()
    e_loss = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
    ulps = (ordered_bits(pred) - ordered_bits(pred_ref.to(dtype))).abs()
    print(f"cm_gan_head {shape} {dtype_name} {mask_kind}: loss {float(loss):.6e} ref {float(loss_ref):.6e} rel {e_loss:.2e}; deterministic "
          f"{float(loss_d):.9e} cm_loss {float(loss_cm_d):.9e}; pred max ulp {int(ulps.max())} (off by one: {int((ulps == 1).sum())} of {ulps.numel()})")
    assert torch.equal(dFn, dFn_cm) and torch.equal(dFn_d, dFn_cm_d) and torch.equal(dFn, dFn_d)      # element-wise, the same arithmetic
    assert torch.equal(loss_d, loss_cm_d.detach())                                                              # one workgroup, the same order
    assert e_loss < 1e-5 and abs(float(loss_d) - float(loss_ref)) < 1e-5 * abs(float(loss_ref)), (float(loss), float(loss_d), float(loss_ref))
    assert int(ulps.max()) <= 1 and torch.equal(pred, pred_d)
    assert bool((pred[..., C:] == 0).all()) and bool((dFn[..., C:] == 0).all())                        # pad channels exactly 0
    assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(dFn).all())


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pred_does_not_depend_on_the_mask(shape, dtype_name):
    preds = [launch(kernel_inputs(shape, DTYPES[dtype_name], k))[1] for k in ("none", "binary", "label")]
    assert torch.equal(preds[0], preds[1]) and torch.equal(preds[0], preds[2])


@pytest.mark.parametrize("mask_kind", ["none", "binary", "label"])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_backward_combines_both_gradients(shape, dtype_name, mask_kind):
    """|dF - ref| <= 1 ulp16(ref) + 2^-22 (|g dFn_cm| + |co_n dpred|): one 16-bit rounding of an fp32 sum of two fp32 products (each product
    and the sum carry 2^-24 relative: the cancellation floor); random dpred with garbage in its pad channels, g = 0.5"""
    dtype = DTYPES[dtype_name]
    B, C, H, W = shape
    args = kernel_inputs(shape, dtype, mask_kind)
    loss, pred, dFn, Fn, dev = launch(args)
    gd = torch.Generator().manual_seed(11)
    dpred = (torch.randn(B, H, W, CPAD, generator=gd) * 1e-2).to(dtype)
    g = torch.tensor(0.5, device=D0)
    torch.autograd.backward([loss, pred], [g, dpred.to(D0)])
    ref, mag = R.head_bwd(dFn.cpu(), dpred, 0.5, args[5], C)
    got = Fn.grad.cpu().double()
    excess = ((got - ref).abs() - ulp16(ref, dtype) - 2.0 ** -22 * mag).max()
    print(f"cm_gan_head_bwd {shape} {dtype_name} {mask_kind}: max |dF - ref| {float((got - ref).abs().max()):.3e}, over the bound by {float(excess):.3e}")
    assert float(excess) <= 0.0
    assert bool((got[..., C:] == 0).all()) and bool(torch.isfinite(got).all())
    assert float((got[..., :C] - 0.5 * dFn.cpu().double()[..., :C]).abs().max()) > 0          # the second term arrived


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_head_backward_without_a_gan_branch_is_the_axpby_path(dtype_name):
    from joligen_amd import ops

    args = kernel_inputs((3, 3, 24, 40), DTYPES[dtype_name], "binary")
    loss, pred, dFn, Fn, dev = launch(args)
    g = torch.tensor(0.5, device=D0)
    loss.backward(g)
    assert torch.equal(Fn.grad, ops.axpby(dFn, 1.0, alpha_dev=g))
    # only pred used: co_n * dpred alone
    loss, pred, dFn, Fn, dev = launch(args)
    dpred = torch.ones_like(pred)
    pred.backward(dpred)
    ref, _ = R.head_bwd(dFn.cpu(), dpred.cpu(), 0.0, args[5], 3)
    assert int((ordered_bits(Fn.grad) - ordered_bits(ref.to(DTYPES[dtype_name]))).abs().max()) <= 1


def test_same_bits_on_every_launch():
    """gradient, pred and the backward: the same bits always; the loss: the same bits with JG_DETERMINISTIC on"""
    args = kernel_inputs((2, 4, 72, 72), torch.bfloat16, "label")
    dpred = torch.randn(2, 72, 72, CPAD, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(D0)
    runs = []
    for det in (1, 1, 0, 0, 1):
        with deterministic(det):
            loss, pred, dFn, Fn, _ = launch(args)
            torch.autograd.backward([loss, pred], [torch.tensor(0.5, device=D0), dpred])
            runs.append((det, loss.detach().clone(), pred.detach().clone(), dFn.clone(), Fn.grad.clone()))
    for det, loss, pred, dFn, dF in runs[1:]:
        assert torch.equal(pred, runs[0][2]) and torch.equal(dFn, runs[0][3]) and torch.equal(dF, runs[0][4])
        if det:
            assert torch.equal(loss, runs[0][1])


def test_argument_checks():
    from joligen_amd import _lib, ops

    args = kernel_inputs((2, 3, 8, 8), torch.float16, "none")
    _, _, _, _, dev = launch(args)
    wide = [torch.zeros(2, 8, 8, 16, device=D0, dtype=torch.float16) for _ in range(2)]
    with pytest.raises(RuntimeError, match="jg_cm_gan_head"):                # Cpad = 16 is refused, not handled silently
        ops.cm_gan_head(wide[0], wide[1], *dev[2:], lam=1.0, grad_scale=1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cm_gan_head(*[None if a is None else a.cpu() for a in dev], lam=1.0, grad_scale=1.0)
    with pytest.raises(ValueError, match="per-sample"):
        ops.cm_gan_head(*dev[:4], dev[4][:1], *dev[5:], lam=1.0, grad_scale=1.0)
    lib = _lib.lib()
    Fn, Fc, nn_, nc = [t.detach() for t in dev[:4]]
    v = dev[4:8] + [dev[9]]
    loss, dFn, pred = torch.zeros((), device=D0), torch.empty_like(Fn), torch.empty_like(Fn)

    def fwd(cpad, fn_ptr=Fn.data_ptr(), pred_ptr=pred.data_ptr()):
        return lib.jg_cm_gan_head(0, fn_ptr, Fc.data_ptr(), nn_.data_ptr(), nc.data_ptr(), *[t.data_ptr() for t in v[:4]], None, v[4].data_ptr(),
                                  loss.data_ptr(), dFn.data_ptr(), pred_ptr, 2, 3, 8, 8, cpad, 0.01, 1.0, 1.0, None)

    def bwd(cpad, a_ptr=dFn.data_ptr(), d_ptr=pred.data_ptr(), g_ptr=loss.data_ptr()):
        return lib.jg_cm_gan_head_bwd(0, a_ptr, d_ptr, g_ptr, v[1].data_ptr(), Fn.data_ptr(), 2, 3, 8, 8, cpad, None)

    assert fwd(16) == _lib.JG_ERR_UNSUPPORTED and bwd(16) == _lib.JG_ERR_UNSUPPORTED
    assert fwd(8, fn_ptr=Fn.data_ptr() + 2) == _lib.JG_ERR_BAD_ARG and fwd(8, pred_ptr=None) == _lib.JG_ERR_BAD_ARG      # misaligned / null
    assert bwd(8, d_ptr=pred.data_ptr() + 8) == _lib.JG_ERR_BAD_ARG and bwd(8, g_ptr=None) == _lib.JG_ERR_BAD_ARG
    assert fwd(8) == _lib.JG_OK and bwd(8) == _lib.JG_OK and bwd(8, d_ptr=None) == _lib.JG_OK
    torch.cuda.synchronize()


def test_torch_op_opcheck():
    """schema + fake kernel + autograd registration of torch.ops.jg355.cm_gan_head; the op computes what the ctypes path computes"""
    from joligen_amd import ops

    J = torch.ops.jg355
    for mask_kind in ("none", "label"):
        args = kernel_inputs((2, 3, 24, 40), torch.bfloat16, mask_kind)
        with deterministic(1):
            loss, pred, dFn, Fn0, dev = launch(args)
            dpred = torch.randn_like(pred) * 1e-2
            g = torch.tensor(0.5, device=D0)
            torch.autograd.backward([loss, pred], [g, dpred])
            Fn = dev[0].detach().clone().requires_grad_(True)
            torch.library.opcheck(J.cm_gan_head.default, (Fn, *[d.detach() if d is not None else None for d in dev[1:]], LAM, GRAD_SCALE),
                                  test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
            l2, p2, g2 = J.cm_gan_head(Fn, *dev[1:], LAM, GRAD_SCALE)
            assert torch.equal(l2.detach(), loss.detach()) and torch.equal(p2.detach(), pred.detach()) and torch.equal(g2, dFn)
            torch.autograd.backward([l2, p2], [g, dpred])
            assert torch.equal(Fn.grad, Fn0.grad)
            Fn3 = dev[0].detach().clone().requires_grad_(True)
            with ops.torch_ops_boundary():
                l3, p3 = ops.cm_gan_head(Fn3, *dev[1:], lam=LAM, grad_scale=GRAD_SCALE)
            assert torch.equal(l3.detach(), loss.detach()) and torch.equal(p3.detach(), pred.detach())
            torch.autograd.backward([l3, p3], [g, dpred])
            assert torch.equal(Fn3.grad, Fn0.grad)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def make_model(c, dtype_name, hp=None, task="inpainting", d_scale=1.0, ndf=16, **extra):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(model_type="cm_gan", G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"],
              G_unet_mha_attn_res=c["attn_res"], G_unet_mha_vit_efficient=c["efficient"], data_crop_size=c["S"],
              train_batch_size=c["B"], gpu_ids="0", jg_act_dtype=dtype_name, train_optim="adamw", train_G_ema=True,
              train_iter_size=1, checkpoints_dir="/tmp/jg_amd_ckpt/", name="cm_gan", D_netDs=["basic"], D_ndf=ndf, D_n_layers=3,
              alg_diffusion_task=task)
    if hp:
        ov.update(train_G_lr=hp["lr_G"], train_D_lr=hp["lr_D"], train_beta1=hp["beta1"], train_beta2=hp["beta2"], train_optim_eps=hp["eps"],
                  train_optim_weight_decay=hp["weight_decay"], train_G_ema_beta=hp["ema_beta"], train_G_ema=hp["ema"],
                  alg_diffusion_lambda_G=hp["lambda_G"], train_optim=hp["optim"], train_pool_size=hp["pool_size"], D_ndf=hp["D_ndf"],
                  D_n_layers=hp["D_n_layers"], train_gan_mode=hp["gan_mode"])
    ov.update(extra)
    opt = opt_from_json({}, ov)
    model = create_model(opt, 0)
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    sdD = O.synth_state_dict(model.netD_B_basic.state_dict(), seed=1)
    model.netD_B_basic.load_state_dict({k: v * d_scale if k.endswith("weight") else v for k, v in sdD.items()})
    model.setup(opt)
    model.single_gpu()
    return model


def cpu_sd(net):
    return {k: v.detach().float().cpu() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("name", CFGS)
def test_cm_gan_three_steps_vs_reference_golden(name, dtype_name):
    """3 x optimize_parameters() with the reference's recorded (noise, timesteps), TEACHER-FORCED by the CPU oracle (tests/parity_util.py; the
    oracle reproduces the fixture's losses of every iteration, re-asserted here).  Per iteration: every loss on identical weights, then the
    parameter updates of G and D and the EMA against the oracle's.  Loss bound: the larger of the project's bound (TOL_LOSS_FWD of
    test_gpu_2_cm for G_cm / G_tot, of test_gpu_5_cutloss for the GAN terms) and twice the floor measured here, the oracle with 16-bit storage
    between layers (O.activation_rounding) against itself in fp32 on the same weights and inputs."""
    import parity_util as PU
    import test_gpu_2_cm as T2
    import test_gpu_5_cutloss as T5

    g = load(f"cm_gan_step_{name}.pt")
    dtype = DTYPES[dtype_name]
    hp, cfg = g["hp"], R.cfg_of(g["cfg"])
    model = make_model(g["cfg"], dtype_name, hp)
    assert model.model_names == g["model_names"] and model.loss_names == g["loss_names"] and model.loss_functions_G == g["loss_functions_G"]
    for grp, rec in zip(model.networks_groups, g["groups"]):
        assert {k: getattr(grp, k) for k in rec if k != "optimizer"} == {k: v for k, v in rec.items() if k != "optimizer"}
    assert model.group_D.optimizer == ["optimizer_D_B_basic"] and model.optimizer_D is model.optimizer_D_B_basic
    assert model.opt.alg_gan_lambda == hp["gan_lambda"] == 0.01 and model.total_t == g["total_t"]
    assert model.loss_scale == (1024.0 if dtype == torch.float16 else 1.0)
    netG, netD = model.netG_A, model.netD_B_basic
    kw = dict(lr_G=hp["lr_G"], lr_D=hp["lr_D"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], weight_decay=hp["weight_decay"],
              ema_beta=hp["ema_beta"] if hp["ema"] else None, lambda_G=hp["lambda_G"], optim=hp["optim"], gan_lambda=hp["gan_lambda"],
              n_layers=hp["D_n_layers"], pool_size=hp["pool_size"])
    tr = R.OracleCMGanTrainer(cpu_sd(netG), cpu_sd(netD), cfg, g["total_t"], **kw)
    tol = dict(G_cm=T2.TOL_LOSS_FWD[dtype], G_tot=T2.TOL_LOSS_FWD[dtype], G_GAN_D_B_basic=T5.TOL_LOSS_FWD[dtype], D_GAN_D_B_basic=T5.TOL_LOSS_FWD[dtype])
    log = []
    for it, s in enumerate(g["steps"]):
        mask = s["mask"].long()
        PU.force_state(netG, {k: tr.P[k] for k in tr.param_names}, tr.m, tr.v, tr.step, tr.ema)
        PU.force_state(netD, tr.D, tr.mD, tr.vD, tr.stepD)
        before = {n: PU.snapshot(net) for n, net in (("G", netG), ("D", netD))}
        ref_before = dict(G={k: tr.P[k].clone() for k in tr.param_names}, D={k: v.clone() for k, v in tr.D.items()})
        ema_before = None if tr.ema is None else {k: v.clone() for k, v in tr.ema.items()}
        tr16 = R.OracleCMGanTrainer(tr.P, tr.D, cfg, g["total_t"], **kw)
        tr16.current_t, tr16.grad_scale = tr.current_t, model.loss_scale
        with O.activation_rounding(dtype):
            l16, _, fake16 = tr16.g_loss_and_grads(s["B"], mask, s["noise"], s["timesteps"])
            l16["D_GAN_D_B_basic"] = tr16.d_loss_and_grads(s["B"], fake16)[0]
        model.rng_injection = lambda b, s=s: (s["noise"], s["timesteps"])
        model.set_input({"A": s["A"], "B": s["B"], "B_label_mask": mask, "A_img_paths": ["x"]})
        model.optimize_parameters()
        losses = {k: float(torch.as_tensor(v).detach()) for k, v in model.get_current_losses().items()}
        ref = {k: float(v) for k, v in tr.optimize_parameters(s["B"], mask, s["noise"], s["timesteps"]).items()}
        for k, v in s["losses"].items():
            assert abs(ref[k] - float(v)) < 2e-4 * abs(float(v)) + 1e-6, (it, k, ref[k], float(v))
        for k, project in tol.items():
            floor, err = abs(float(l16[k]) - ref[k]) / abs(ref[k]), abs(losses[k] - ref[k]) / abs(ref[k])
            bound = max(project, 2.0 * floor)
            log.append(f"{name} {dtype_name} it{it} {k}: {losses[k]:.6f} oracle {ref[k]:.6f} device error {err:.3e} 16-bit-storage floor {floor:.3e} "
                       f"bound {bound:.3e}")
            print(log[-1])
            assert err < bound, (it, k, losses[k], ref[k], floor)
        assert abs(losses["G_tot"] - (losses["G_cm"] + losses["G_GAN_D_B_basic"])) <= 2.0 ** -22 * abs(losses["G_tot"])
        assert losses["D_tot"] == losses["D_GAN_D_B_basic"]
        after = {n: PU.snapshot(net) for n, net in (("G", netG), ("D", netD))}
        PU.check_update(f"{name} {dtype_name} it{it} G", before["G"], after["G"], ref_before["G"], {k: tr.P[k] for k in tr.param_names},
                        T2.COS_UPDATE[dtype], log=log)
        PU.check_update(f"{name} {dtype_name} it{it} D", before["D"], after["D"], ref_before["D"], tr.D, T5.COS_UPDATE[dtype], log=log)
        if hp["ema"]:
            ema = {k: v.detach().float().cpu() for k, v in model.netG_A_ema.named_parameters()}
            PU.check_ema(f"ema it{it}", ema_before, ema, after["G"], hp["ema_beta"], first=ema_before is None)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"update_agreement_cm_gan_{name}_{dtype_name}.txt"), "w") as f:
        f.write("\n".join(log))
    B = g["cfg"]["B"]
    assert netG.current_t == 3 * B and len(model.fake_B_pool) == 3 * B
    model.compute_visuals(B)
    vis = model.get_current_visuals(B)
    assert len(vis) == B and list(vis[0].keys()) == [n + "0" for n in g["gen_visual_names"]]


def test_cm_gan_pix2pix_step_vs_reference_golden():
    """the pix2pix task (conditioning image = A, no mask) of the reference's cm_gan: the first recorded step, fp16, losses as above"""
    import test_gpu_2_cm as T2
    import test_gpu_5_cutloss as T5

    g = load("cm_gan_step_pix2pix_tiny_eff.pt")
    assert g["task"] == "pix2pix"
    hp, cfg, dtype = g["hp"], R.cfg_of(g["cfg"], "pix2pix"), torch.float16
    model = make_model(g["cfg"], "fp16", hp, task="pix2pix")
    kw = dict(lr_G=hp["lr_G"], lr_D=hp["lr_D"], lambda_G=hp["lambda_G"], optim=hp["optim"], n_layers=hp["D_n_layers"], task="pix2pix")
    sdG, sdD = cpu_sd(model.netG_A), cpu_sd(model.netD_B_basic)
    s = g["steps"][0]
    tr, tr16 = R.OracleCMGanTrainer(sdG, sdD, cfg, g["total_t"], **kw), R.OracleCMGanTrainer(sdG, sdD, cfg, g["total_t"], **kw)
    tr16.grad_scale = model.loss_scale
    with O.activation_rounding(dtype):
        l16, _, fake16 = tr16.g_loss_and_grads(s["B"], None, s["noise"], s["timesteps"], y_cond=s["A"])
        l16["D_GAN_D_B_basic"] = tr16.d_loss_and_grads(s["B"], fake16)[0]
    model.rng_injection = lambda b: (s["noise"], s["timesteps"])
    model.set_input({"A": s["A"], "B": s["B"], "A_img_paths": ["x"]})
    model.optimize_parameters()
    losses = {k: float(torch.as_tensor(v).detach()) for k, v in model.get_current_losses().items()}
    ref = {k: float(v) for k, v in tr.optimize_parameters(s["B"], None, s["noise"], s["timesteps"], y_cond=s["A"]).items()}
    for k, project in dict(G_cm=T2.TOL_LOSS_FWD[dtype], G_tot=T2.TOL_LOSS_FWD[dtype], G_GAN_D_B_basic=T5.TOL_LOSS_FWD[dtype],
                           D_GAN_D_B_basic=T5.TOL_LOSS_FWD[dtype]).items():
        assert abs(ref[k] - float(s["losses"][k])) < 2e-4 * abs(float(s["losses"][k])) + 1e-6
        floor, err = abs(float(l16[k]) - ref[k]) / abs(ref[k]), abs(losses[k] - ref[k]) / abs(ref[k])
        print(f"pix2pix {k}: {losses[k]:.6f} oracle {ref[k]:.6f} device error {err:.3e} floor {floor:.3e}")
        assert err < max(project, 2.0 * floor), (k, losses[k], ref[k], floor)


# the scale of the discriminator's synthetic weights in the routing test.  Checked on the CPU when the test was written (oracle, the test's
# inputs, D_ndf 64): with the GAN term's gradient cut the UNet's weight gradients differ from the full ones by 0.88 (worst tensor; median
# 0.75) at scale 1 and by 1.0 at scale 4 and 16 -- at alg_gan_lambda = 0.01 the discriminator's gradient already dominates the consistency
# term's -- against a 16-bit-storage floor of 0.093 (worst; median 0.071), i.e. a bound of 0.19.  Scale 1 is enough.
ROUTING_D_SCALE = 1.0


def test_discriminator_gradient_reaches_every_unet_weight():
    """64x64, ngf 64, B = 2, fp16 (halo kernels, fused statistics, flash attention live): every UNet weight gradient of compute_cm_gan_loss
    against the CPU oracle, bounded as in the ECT test by the rounding floor MEASURED on the same inputs (the oracle with 16-bit storage
    between layers): worst <= max(2 floor, 2e-2), median <= max(1.5 floor, 5e-3).  The same step with the GAN term's gradient cut (fake_B
    detached) must give gradients that differ from the full ones by more than that bound on at least one tensor -- in the oracle (the premise:
    it holds by the choice of ROUTING_D_SCALE, checked on the CPU when the test was written) and on the device (the claim)."""
    import test_gpu_2_cm as T2

    c = dict(ngf=64, mults=[1, 2], res_blocks=[1, 1], attn_res=[2], efficient=True, S=64, B=2)
    model = make_model(c, "fp16", d_scale=ROUTING_D_SCALE, ndf=64)
    netG, netD = model.netG_A, model.netD_B_basic
    r16 = lambda sd: {k: (v.half().float() if (torch.is_floating_point(v) and v.dim() >= 3) else v) for k, v in sd.items()}
    sdG, sdD = r16(cpu_sd(netG)), r16(cpu_sd(netD))
    netG.load_state_dict(sdG)
    netD.load_state_dict(sdD)
    cfg = R.cfg_of(c)
    g = torch.Generator().manual_seed(9)
    Bimg = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).half().float()
    mask = torch.zeros(2, 1, 64, 64, dtype=torch.int64)
    mask[:, :, 10:40, 20:50] = 1
    A = Bimg * (1 - mask) + torch.randn(Bimg.shape, generator=g).half().float() * mask
    sig = O.cm_karras_schedule(O.cm_improved_timesteps_schedule(0, model.total_t))
    noise, timesteps = O.cm_draw_step_randomness(torch.Generator().manual_seed(3), Bimg, sig)

    def oracle(gan_scale=1.0, rounding=False):
        tr = R.OracleCMGanTrainer(sdG, sdD, cfg, model.total_t)
        tr.gan_scale = gan_scale
        if rounding:
            tr.grad_scale = model.loss_scale
            with O.activation_rounding(torch.float16):
                return tr.g_loss_and_grads(Bimg, mask, noise, timesteps)
        return tr.g_loss_and_grads(Bimg, mask, noise, timesteps)

    L, grads, _ = oracle()
    _, grads_cut, _ = oracle(gan_scale=0.0)
    L16, grads16, _ = oracle(rounding=True)

    def device(cut):
        model.rng_injection = lambda b: (noise, timesteps)
        model.set_input({"A": A, "B": Bimg, "B_label_mask": mask})
        model._group_flags(model.group_G)
        netG.current_t = 0
        netG.arena.g.zero_()
        orig = model.compute_G_loss_GAN
        if cut:
            def gan_cut():
                model.fake_B = model.fake_B.detach()
                orig()
            model.compute_G_loss_GAN = gan_cut
        try:
            model.compute_cm_gan_loss()
        finally:
            model.compute_G_loss_GAN = orig
        model.loss_G_tot.backward()
        torch.cuda.synchronize()
        return ({k: float(getattr(model, "loss_" + k).detach()) for k in ("G_tot", "G_cm", "G_GAN_D_B_basic")},
                {k: p.grad.detach().float().cpu() / model.loss_scale for k, p in netG.named_parameters()})

    loss_dev, gdev = device(cut=False)
    loss_dev_cut, gdev_cut = device(cut=True)
    keys = [k for k, p in netG.named_parameters() if k.endswith(".weight") and p.dim() >= 2 and float(grads[k].norm()) > 1e-12]
    mine = sorted(((R.relerr(gdev[k], grads[k]), k) for k in keys), reverse=True)
    floor = sorted((R.relerr(grads16[k], grads[k]) for k in keys), reverse=True)
    mid = len(keys) // 2
    bound_worst, bound_median = max(2.0 * floor[0], 2e-2), max(1.5 * floor[mid], 5e-3)
    sep_oracle = sorted(((R.relerr(grads_cut[k], grads[k]), k) for k in keys), reverse=True)
    sep_device = sorted(((R.relerr(gdev_cut[k], gdev[k]), k) for k in keys), reverse=True)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, "grad_table_cm_gan_64_fp16.txt"), "w") as f:
        f.write(f"# device losses {loss_dev} oracle { {k: float(v) for k, v in L.items()} } 16-bit-storage oracle { {k: float(v) for k, v in L16.items()} }\n")
        f.write(f"# rounding floor (oracle, 16-bit storage): worst {floor[0]:.3e} median {floor[mid]:.3e}; bounds worst {bound_worst:.3e} median {bound_median:.3e}\n")
        f.write(f"# GAN gradient cut vs full: oracle worst {sep_oracle[0][0]:.3e} ({sep_oracle[0][1]}), device worst {sep_device[0][0]:.3e} ({sep_device[0][1]})\n")
        f.write("\n".join(f"{e:10.3e} {k}" for e, k in mine))
    print(f"cm_gan 64x64: gradients worst {mine[0][0]:.3e} (floor {floor[0]:.3e}) median {mine[mid][0]:.3e} (floor {floor[mid]:.3e}); GAN cut vs full: "
          f"oracle {sep_oracle[0][0]:.3e} device {sep_device[0][0]:.3e}; losses {loss_dev}")
    for k in ("G_cm", "G_tot", "G_GAN_D_B_basic"):
        fl, err = abs(float(L16[k]) - float(L[k])) / abs(float(L[k])), abs(loss_dev[k] - float(L[k])) / abs(float(L[k]))
        assert err < max(T2.TOL_LOSS_FWD[torch.float16], 2.0 * fl), (k, loss_dev[k], float(L[k]), fl)
    assert mine[0][0] <= bound_worst, (mine[:5], floor[:3])
    assert mine[mid][0] <= bound_median, (mine[mid], floor[mid])
    assert sep_oracle[0][0] > bound_worst, ("the premise: ROUTING_D_SCALE too small for the GAN gradient to show", sep_oracle[:3], bound_worst)
    assert sep_device[0][0] > bound_worst, ("the discriminator's gradient does not arrive in the UNet", sep_device[:3], bound_worst)
    # the cut changes the gradient, not the values: the two device runs agree to their run-to-run noise (fp16 storage, atomics: < 2^-10)
    assert abs(loss_dev_cut["G_tot"] - loss_dev["G_tot"]) < 2.0 ** -10 * abs(loss_dev["G_tot"]), (loss_dev_cut, loss_dev)


def test_example_cm_gan_json_runs_a_training_window(tmp_path):
    """examples/example_cm_gan_noglasses2glasses.json (tests/golden/examples/: a verbatim copy, settings only) constructs with both of its
    discriminators (the projector on its random-initialised backbone), crop 64, B = 2; one accumulation window of its own train_iter_size
    runs: finite losses, G and both D move only at the window boundary, the counters advance, the visuals carry the cm names.
    The pool: compute_D_loss queries it once per discriminator (base_gan_model.py:341-419), so every iteration offers 2 x B images."""
    from bench import synth_batch
    from joligen_amd.models import create_model
    from joligen_amd.models.cm_gan_model import CMGanModel
    from joligen_amd.options import opt_from_json

    ov = dict(output_display_type=["none"], output_print_freq=10 ** 9, checkpoints_dir=str(tmp_path), gpu_ids="0", train_metrics_list=[],
              jg_act_dtype="bf16", name="cm_gan_e2e", data_crop_size=64, data_load_size=64, train_batch_size=2,
              D_proj_interp=128)
    # D_proj_interp: the example's own -1 feeds the projector the crop.  At 64 x 64 its deepest map is 4 x 4, below the heads' end_sz = 8:
    # SingleDisc then builds no DownBlock and its last convolution expects CHANNEL_DICT[8] = 512 channels on a 256-channel map, here as in
    # the reference (discriminator.py:13-77).  128 is the smallest input whose four maps are all >= 8; the CUT model test of
    # test_gpu_6_projd (test_cut_model_with_projected_and_basic_discriminators) sets the same value at crop 64.  The example's -1 is
    # therefore not exercised at this crop; at its own crop of 128 the two settings are the same network.
    opt = opt_from_json(EXAMPLE, ov)
    assert opt.model_type == "cm_gan" and opt.train_iter_size == 16 and opt.D_netDs == ["projected_d", "basic"]
    model = create_model(opt, 0)
    assert isinstance(model, CMGanModel) and model.opt.alg_gan_lambda == 0.01
    assert model.model_names == ["G_A", "D_B_projected_d", "D_B_basic"]
    assert [n.replace("_avg", "") for n in model.loss_names] == ["G_tot", "G_cm", "G_GAN_D_B_projected_d", "G_GAN_D_B_basic", "D_tot",
                                                                 "D_GAN_D_B_projected_d", "D_GAN_D_B_basic"]
    assert model.D_B_projected_d_loss_calculator.gan_mode == "projected" and model.D_B_basic_loss_calculator.gan_mode == "lsgan"
    model.setup(opt)
    model.single_gpu()
    data = synth_batch(2, 64, 3, torch.device(D0))
    torch.manual_seed(0)
    nets = {n: model._net(n) for n in model.model_names}
    trainable = lambda net: torch.cat([p.detach().double().flatten() for k, p in net.named_parameters() if not k.startswith("freeze")]).sum()
    start = {n: float(trainable(net)) for n, net in nets.items()}
    frozen0 = {k: p.detach().clone() for k, p in nets["D_B_projected_d"].named_parameters() if k.startswith("freeze")}
    W, B, nD = opt.train_iter_size, 2, 2
    for j in range(W):
        model.set_input(data)
        model.optimize_parameters()
        for n, net in nets.items():
            assert (float(trainable(net)) != start[n]) == (j == W - 1), (n, j)
        assert len(model.fake_B_pool) == min(opt.train_pool_size, nD * B * (j + 1)), j
    losses = {k: float(v) for k, v in model.get_current_losses().items()}
    assert len(losses) == 7 and all(math.isfinite(v) for v in losses.values()), losses
    assert abs(losses["G_tot_avg"] - losses["G_cm_avg"] - losses["G_GAN_D_B_projected_d_avg"] - losses["G_GAN_D_B_basic_avg"]) < 1e-4 * abs(losses["G_tot_avg"]) + 1e-6
    assert nets["G_A"].current_t == W * B
    assert all(torch.equal(p.detach(), frozen0[k]) for k, p in nets["D_B_projected_d"].named_parameters() if k in frozen0)
    assert tuple(model.fake_B.shape) == (B, 64, 64, 8) and model.fake_B.dtype == torch.bfloat16
    model.compute_visuals(B)
    vis = model.get_current_visuals(B)
    assert len(vis) == B and list(vis[0].keys()) == ["gt_image_0", "y_t_0", "next_noisy_x_0", "current_noisy_x_0", "mask_0", "output_0"]
    with pytest.raises(NotImplementedError, match="more than one GPU"):
        model.parallelize(0)


def test_cm_is_unchanged_and_refusals():
    from joligen_amd.models import create_model
    from joligen_amd.models.cm_gan_model import CMGanModel
    from joligen_amd.models.cm_model import CMModel
    from joligen_amd.options import opt_from_json

    c = dict(ngf=32, mults=[1, 2], res_blocks=[1, 1], attn_res=[16], efficient=True, S=32, B=2)
    ov = dict(G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"], G_unet_mha_attn_res=c["attn_res"],
              G_unet_mha_vit_efficient=True, data_crop_size=c["S"], train_batch_size=c["B"], gpu_ids="0", train_G_ema=True, name="cm_gan")
    cm = create_model(opt_from_json({}, dict(ov, model_type="cm")), 0)
    assert type(cm) is CMModel and cm.group_G.backward_functions == ["compute_cm_loss"] and cm.loss_names == ["G_tot"]
    assert cm.model_names == ["G_A"] and len(cm.networks_groups) == 1 and not hasattr(cm, "discriminators_names")
    gan = create_model(opt_from_json({}, dict(ov, model_type="cm_gan", D_netDs=["basic"], D_ndf=16)), 0)
    assert type(gan) is CMGanModel and gan.group_G.backward_functions == ["compute_cm_gan_loss"] and gan.group_G.forward_functions == []
    assert gan.loss_names == ["G_tot", "G_cm", "G_GAN_D_B_basic", "D_tot", "D_GAN_D_B_basic"] and gan.optimizers == [gan.optimizer_G, gan.optimizer_D]
    for bad, match in ((dict(alg_ddpm_ft_mode="ect"), "unpacks 7 values"), (dict(D_netDs=["vision_aided"]), "D_netDs"), (dict(dataaug_APA=True), "dataaug_APA")):
        with pytest.raises(NotImplementedError, match=match):
            create_model(opt_from_json({}, {**ov, "model_type": "cm_gan", "D_netDs": ["basic"], **bad}), 0)
