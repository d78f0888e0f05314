"""Generate tests/golden/cm_gan/*.pt from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY): cm_gan_model (consistency training
with discriminators), built from examples/example_cm_gan_noglasses2glasses.json with the overrides, weights, batches and seeds of
oracle/make_golden_cm.py, D_netDs = ["basic"], D_ndf = 16, D_n_layers = 3, crop 32 (the smallest crop the 3-layer PatchGAN trains at).
  * cm_gan_step_<cfg>.pt      : 3 x CMGanModel.optimize_parameters(): per step the batch, the recorded (noise, timesteps), the five losses
                                and the projections (jg_oracle.projection_vector) and norms of the updated G, EMA-of-G and D parameters,
                                as [n, 2] tensors in the order of `g_shapes` / `d_shapes`.  No weights: both networks are loaded from
                                jg_oracle.synth_state_dict (seed 0 for G, seed 1 for D).
  * cm_gan_step_pix2pix_tiny_eff.pt : the same with alg_diffusion_task = "pix2pix" (the conditioning image is `A`).
  * cm_gan_head.pt            : CMGanModel.compute_cm_gan_loss itself, netG_A replaced by a stand-in that returns prepared (pred, target,
                                ..., loss_weights, ...) and the discriminator by a fixed linear functional of fake_B: the loss values and
                                d(loss_G_tot)/d(pred) without a mask, with a 0/1 mask, and with a label mask (value 2, one sample all zero).
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_cm_gan.py [output directory]"""
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden_cm as MG  # noqa: E402  (installs ref_shim)
import ref_shim  # noqa: E402

import torch  # noqa: E402

O = MG.O
S_GAN = 32                # InstanceNorm of the 3-layer PatchGAN needs more than one value per plane: 32 is the smallest crop
D_OVERRIDES = dict(netDs=["basic"], ndf=16, n_layers=3)
LOSSES = ["G_tot", "G_cm", "G_GAN_D_B_basic", "D_tot", "D_GAN_D_B_basic"]
EXAMPLE = "examples/example_cm_gan_noglasses2glasses.json"


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def build_opt(c, task="inpainting"):
    """the option builder of oracle/make_golden_cm.py pointed at the cm_gan example"""
    from options.train_options import TrainOptions
    import train as ref_train

    cfg = json.load(open(os.path.join(ref_shim.REFERENCE_ROOT, EXAMPLE)))
    cfg["data"]["crop_size"] = cfg["data"]["load_size"] = c["S"]
    cfg["train"]["batch_size"] = c["B"]
    cfg["train"]["iter_size"] = 1
    cfg["gpu_ids"] = "-1"
    cfg["G"].update(ngf=c["ngf"], unet_mha_channel_mults=c["mults"], unet_mha_res_blocks=c["res_blocks"], unet_mha_attn_res=c["attn_res"],
                    unet_mha_vit_efficient=c["efficient"])
    cfg["D"].update(D_OVERRIDES)
    cfg["alg"]["diffusion"]["task"] = task
    cfg["output"]["display"]["type"] = ["none"]
    cfg["checkpoints_dir"] = os.path.join(tempfile.gettempdir(), "jg_golden_ckpt") + "/"
    cfg["dataroot"] = os.path.join(tempfile.gettempdir(), "nodata")
    opt = TrainOptions().parse_json(cfg, save_config=False)
    opt.use_cuda = False
    opt.optim = ref_train.optim
    opt.jg_dir = ref_shim.REFERENCE_ROOT
    opt.total_iters = 0
    opt.num_test_images = 0
    return opt


def cm_gan_model(c, task="inpainting"):
    from models import create_model

    opt = build_opt(c, task)
    assert opt.model_type == "cm_gan", opt.model_type
    assert not hasattr(opt, "alg_gan_lambda") or opt.alg_gan_lambda != 0.01     # set by CMGanModel.__init__, whatever was parsed
    torch.manual_seed(0)
    with quiet():
        model = create_model(opt, 0)
        model.setup(opt)
    model.use_temporal = False
    assert model.opt.alg_gan_lambda == 0.01
    return opt, model


def proj(named):
    """[n, 2] (l2 norm, projection on jg_oracle.projection_vector) in the order of `named`"""
    rows = [MG.checks({k: v})[k] for k, v in named]
    return torch.stack(rows)


def group_fields(g):
    return {k: getattr(g, k) for k in ("networks_to_optimize", "forward_functions", "backward_functions", "loss_names_list", "optimizer",
                                       "loss_backward", "networks_to_ema")}


def step_fixture(out, name, c, task="inpainting"):
    c = dict(c, S=S_GAN)
    opt, model = cm_gan_model(c, task)
    netG, netD = model.netG_A, model.netD_B_basic
    g_sd, d_sd = netG.state_dict(), netD.state_dict()
    netG.load_state_dict(O.synth_state_dict(g_sd, seed=0))
    netD.load_state_dict(O.synth_state_dict(d_sd, seed=1))
    # neither network has buffers: the rows of g_proj / ema_proj / d_proj follow the keys of g_shapes / d_shapes
    assert [k for k, _ in netG.named_parameters()] == list(g_sd) and [k for k, _ in netD.named_parameters()] == list(d_sd)
    assert model.model_names == ["G_A", "D_B_basic"] and model.loss_names == LOSSES, (model.model_names, model.loss_names)
    B, S, total_t = c["B"], c["S"], model.total_t
    netG.current_t = 0
    steps, cur_t = [], 0
    for it in range(3):
        data = MG.synth_batch(B, S, seed=4321 + it)
        sig = O.cm_karras_schedule(O.cm_improved_timesteps_schedule(cur_t, total_t))
        noise, timesteps = O.cm_draw_step_randomness(torch.Generator().manual_seed(2000 + it), data["B"], sig)
        model.set_input(data)
        torch.manual_seed(2000 + it)
        with quiet():
            model.optimize_parameters()
        cur_t += B
        m = torch.clamp(data["B_label_mask"], 0, 1) if task == "inpainting" else None
        chk = data["B"] + sig[timesteps + 1].view(-1, 1, 1, 1) * noise
        if m is not None:
            chk = chk * m + (1 - m) * data["B"]
        assert torch.allclose(model.next_noisy_x, chk), "draw order differs from cm_draw_step_randomness"
        losses = {k: torch.as_tensor(v).detach().clone().float() for k, v in model.get_current_losses().items()}
        assert list(losses) == LOSSES
        rec = dict(A=data["A"], B=data["B"], mask=data["B_label_mask"].to(torch.uint8), noise=noise, timesteps=timesteps, losses=losses,
                   g_proj=proj(netG.named_parameters()), ema_proj=proj(model.netG_A_ema.named_parameters()), d_proj=proj(netD.named_parameters()))
        steps.append(rec)
        print(name, task, "step", it, {k: float(v) for k, v in losses.items()})
    assert len(model.fake_B_pool.images) == 3 * B            # below train_pool_size: the pool returned its input, no host draws
    hp = dict(lr_G=opt.train_G_lr, lr_D=opt.train_D_lr, beta1=opt.train_beta1, beta2=opt.train_beta2, eps=opt.train_optim_eps,
              weight_decay=opt.train_optim_weight_decay, ema_beta=opt.train_G_ema_beta, lambda_G=opt.alg_diffusion_lambda_G,
              optim=opt.train_optim, ema=bool(opt.train_G_ema), gan_lambda=model.opt.alg_gan_lambda, gan_mode=opt.train_gan_mode,
              pool_size=opt.train_pool_size, D_ndf=opt.D_ndf, D_n_layers=opt.D_n_layers)
    fname = f"cm_gan_step_{name}.pt" if task == "inpainting" else f"cm_gan_step_{task}_{name}.pt"
    torch.save(dict(cfg=c, task=task, hp=hp, total_t=total_t, steps=steps, g_shapes={k: tuple(v.shape) for k, v in g_sd.items()},      # in state_dict order
                    d_shapes={k: tuple(v.shape) for k, v in d_sd.items()},
                    model_names=list(model.model_names), loss_names=list(model.loss_names), groups=[group_fields(g) for g in model.networks_groups],
                    loss_functions_G=list(model.loss_functions_G), gen_visual_names=list(model.gen_visual_names)), os.path.join(out, fname))
    return model


def head_fixture(out, model):
    B, C, S = 3, 3, 16
    g = torch.Generator().manual_seed(91)
    target = torch.randn(B, C, S, S, generator=g)
    pred0 = target + torch.randn(B, C, S, S, generator=g) * torch.tensor([1.0, 0.05, 1e-3]).view(B, 1, 1, 1)
    loss_weights = torch.tensor([0.7, 12.0, 300.0]).view(B, 1, 1, 1)
    wd = torch.randn(1, C, S, S, generator=g) * 0.2          # the discriminator stand-in: one linear functional of the image + a bias
    bd = 0.3
    m01 = torch.zeros(B, 1, S, S, dtype=torch.int64)
    m01[:, :, 3:12, 2:9] = 1
    mlabel = m01.clone()
    mlabel[0, :, 5:8, 4:7] = 2
    mlabel[1] = 0
    model.netD_B_basic = lambda x: (x * wd).sum(dim=(1, 2, 3)).view(-1, 1) / (C * S) + bd
    recs = {}
    for name, mask in (("none", None), ("binary", m01), ("label", mlabel)):
        pred = pred0.clone().requires_grad_(True)
        model.netG_A = lambda y_0, total_t, m, y_cond, pred=pred: (pred, target, 11, None, loss_weights, y_0, y_0)
        model.gt_image, model.cond_image, model.mask = target, None, mask
        model.real_B = target
        model.compute_cm_gan_loss()
        (dpred,) = torch.autograd.grad(model.loss_G_tot, [pred])
        assert model.fake_B is pred and torch.isfinite(dpred).all()
        recs[name] = dict(mask=mask, G_tot=model.loss_G_tot.detach().clone(), G_cm=model.loss_G_cm.clone(),
                          G_GAN=model.loss_G_GAN_D_B_basic.detach().clone(), dpred=dpred.clone())
        print("cm_gan_head", name, float(recs[name]["G_cm"]), float(recs[name]["G_GAN"]), float(recs[name]["G_tot"]))
    torch.save(dict(pred=pred0, target=target, loss_weights=loss_weights, wd=wd, bd=bd, lambda_G=model.opt.alg_diffusion_lambda_G,
                    gan_lambda=model.opt.alg_gan_lambda, cases=recs), os.path.join(out, "cm_gan_head.pt"))


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    for name, c in MG.TINY.items():
        model = step_fixture(out, name, c)
    step_fixture(out, "tiny_eff", MG.TINY["tiny_eff"], task="pix2pix")
    head_fixture(out, model)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "cm_gan"))
