"""Generate tests/golden/ect/*.pt from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY): cm_model with alg_ddpm_ft_mode = "ect"
(easy consistency tuning), in the tiny configurations and with the option set, weights and batches of oracle/make_golden_cm.py.
  * ect_fn.pt          : CMGenerator.t_to_r_sigmoid on a fixed vector of t (values either side of the r = 0 thresholds) for stages 0, 1, 3,
                         and skip_scaling_train / output_scaling_train on the same vector;
  * ect_loss.pt        : CMModel.compute_ect_loss itself, its netG_A replaced by a stand-in that returns prepared (pred, target, ..., t, r):
                         loss and d loss / d pred without a mask, with a 0/1 mask, and with a label mask (value 2, one sample all zero);
  * ect_gen_<cfg>.pt   : CMGenerator.forward in training mode with its two draws recorded (randn(B), then randn_like(x));
  * ect_step_<cfg>.pt  : 3 x CMModel.optimize_parameters() with the recipe's seeds 2000 + it.
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_ect.py [output directory]"""
import contextlib
import io
import math
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden_cm as MG  # noqa: E402  (installs ref_shim)

import torch  # noqa: E402

O = MG.O
LN7, LN53 = math.log(7.0), math.log(5.0 / 3.0)        # r = 0 below these at stage 0 / stage 1 (k = 8, b = 1, q = 2)
T_VECTOR = [1e-3, 0.05, 0.4, LN53 - 1e-3, LN53 + 1e-3, 0.6, 1.0, 1.9, LN7 - 1e-3, LN7 + 1e-3, 2.0, 3.0, 10.0, 50.0, 80.0]
STAGES = [0, 1, 3]
GEN_SEED0 = 55           # the first seed from here on whose draws give one r = 0 and one r > 0


def quiet():
    return contextlib.redirect_stdout(io.StringIO())      # the reference prints t and r at every step


def ect_model(c):
    from models import create_model

    opt = MG.build_opt(c)
    opt.alg_ddpm_ft_mode = "ect"
    assert opt.model_type == "cm", opt.model_type
    torch.manual_seed(0)
    with quiet():
        model = create_model(opt, 0)
        model.setup(opt)
    model.use_temporal = False
    assert model.ft_mode == "ect" and model.group_G.backward_functions == ["compute_ect_loss"]
    return opt, model


def draws(seed, x):
    """the two draws of the ECT branch in its order, from the default generator"""
    torch.manual_seed(seed)
    rnd_normal = torch.randn(x.shape[0])
    noise = torch.randn(x.shape, dtype=x.dtype)
    return rnd_normal, noise


def t_r(netG, rnd_normal):
    t = (rnd_normal * netG.P_std + netG.P_mean).exp()
    return t, netG.t_to_r(netG.k, netG.b, netG.q, t, netG.stage)


def fn_fixture(out, netG):
    from models.modules import cm_generator as RG

    t = torch.tensor(T_VECTOR, dtype=torch.float32)
    rec = dict(t=t, k=netG.k, b=netG.b, q=netG.q, sigma_data=netG.sigma_data, sigma_min=netG.sigma_min, P_mean=netG.P_mean, P_std=netG.P_std,
               double_ticks=netG.double_ticks, r={s: netG.t_to_r_sigmoid(netG.k, netG.b, netG.q, t, s) for s in STAGES},
               skip_scaling_train=RG.skip_scaling_train(t, netG.sigma_data, netG.sigma_min),
               output_scaling_train=RG.output_scaling_train(t, netG.sigma_data, netG.sigma_min))
    assert (rec["r"][0] == 0).any() and (rec["r"][0] > 0).any() and (rec["r"][1] == 0).any() and (rec["r"][3] > 0).all()
    torch.save(rec, os.path.join(out, "ect_fn.pt"))


def loss_fixture(out, model):
    B, C, S = 3, 3, 16
    g = torch.Generator().manual_seed(77)
    target = torch.randn(B, C, S, S, generator=g)
    pred0 = target + torch.randn(B, C, S, S, generator=g) * torch.tensor([1.0, 0.05, 1e-3]).view(B, 1, 1, 1)
    t = torch.tensor([0.3, 2.5, 40.0])
    r = torch.tensor([0.0, 0.8, 30.0])
    m01 = torch.zeros(B, 1, S, S, dtype=torch.int64)
    m01[:, :, 3:12, 2:9] = 1
    mlabel = m01.clone()
    mlabel[0, :, 5:8, 4:7] = 2
    mlabel[1] = 0
    recs = {}
    for name, mask in (("none", None), ("binary", m01), ("label", mlabel)):
        pred = pred0.clone().requires_grad_(True)
        model.netG_A = lambda y_0, total_t, m, y_cond, pred=pred: (pred, target, y_0, y_0, t, r)
        model.gt_image, model.cond_image, model.mask = target, None, mask
        model.compute_ect_loss()
        (dpred,) = torch.autograd.grad(model.loss_G_tot, [pred])
        assert torch.isfinite(dpred).all()
        recs[name] = dict(mask=mask, loss=model.loss_G_tot.detach().clone(), dpred=dpred.clone())
        print("ect_loss", name, float(model.loss_G_tot.detach()))
    torch.save(dict(pred=pred0, target=target, t=t, r=r, c=model.c, lambda_G=model.opt.alg_diffusion_lambda_G, cases=recs),
               os.path.join(out, "ect_loss.pt"))


def model_fixtures(out):
    fn_done = False
    for name, c in MG.TINY.items():
        opt, model = ect_model(c)
        netG = model.netG_A
        ref_sd = netG.state_dict()
        netG.load_state_dict(O.synth_state_dict(ref_sd, seed=0))
        assert netG.training
        if not fn_done:
            fn_fixture(out, netG)
            fn_done = True
        B, S = c["B"], c["S"]
        total_t = model.total_t

        # ---- CMGenerator.forward (training mode) with pinned randomness ----
        data = MG.synth_batch(B, S, seed=4321)
        y_0, mask = data["B"], data["B_label_mask"]
        seed = GEN_SEED0
        while True:
            rnd_normal, noise = draws(seed, y_0)
            t, r = t_r(netG, rnd_normal)
            if (r == 0).any() and (r > 0).any():
                break
            seed += 1
        netG.current_t = 0
        torch.manual_seed(seed)
        with torch.no_grad(), quiet():
            D_yt, D_yr, t_noisy_x, r_noisy_x, t_out, r_out = netG(y_0, total_t, mask, None)
        assert torch.equal(t_out, t) and torch.equal(r_out, r), "draw order differs from draws()"
        m = torch.clamp(mask, min=0.0, max=1.0)
        assert torch.equal(t_noisy_x, (y_0 + t.view(-1, 1, 1, 1) * noise) * m + (1 - m) * y_0), "draw order differs from draws()"
        assert netG.current_t == B
        torch.save(dict(cfg=c, total_t=total_t, seed=seed, B=y_0, mask=mask, noise=noise, rnd_normal=rnd_normal, t=t, r=r, D_yt=D_yt, D_yr=D_yr,
                        t_noisy_x=t_noisy_x, r_noisy_x=r_noisy_x), os.path.join(out, f"ect_gen_{name}.pt"))
        print(name, "generator seed", seed, "t", t.tolist(), "r", r.tolist())

        # ---- 3 full optimize_parameters() steps ----
        netG.current_t = 0
        steps = []
        for it in range(3):
            data = MG.synth_batch(B, S, seed=4321 + it)
            rnd_normal, noise = draws(2000 + it, data["B"])
            t, r = t_r(netG, rnd_normal)
            model.set_input(data)
            torch.manual_seed(2000 + it)
            with quiet():
                model.optimize_parameters()
            loss = model.get_current_losses()["G_tot"].detach().clone()
            rec = dict(A=data["A"], B=data["B"], mask=data["B_label_mask"], noise=noise, rnd_normal=rnd_normal, t=t, r=r, loss=loss)
            if it in (0, 2):
                rec["param_checks"] = MG.checks(dict(model.netG_A.named_parameters()))
                rec["ema_checks"] = MG.checks(dict(model.netG_A_ema.named_parameters()))
            steps.append(rec)
            print(name, "step", it, "loss", float(loss), "r", r.tolist())
        allr = torch.cat([s["r"] for s in steps])
        assert (allr == 0).any() and (allr > 0).any(), "the recorded steps must take both the r = 0 and the r > 0 branch"
        assert netG.current_t == 3 * B and model.cur_nimg == 3 * B and model.cur_tick == 0 and netG.stage == 0
        hp = dict(lr=opt.train_G_lr, beta1=opt.train_beta1, beta2=opt.train_beta2, eps=opt.train_optim_eps,
                  weight_decay=opt.train_optim_weight_decay, ema_beta=opt.train_G_ema_beta, lambda_G=opt.alg_diffusion_lambda_G,
                  optim=opt.train_optim, ema=bool(opt.train_G_ema), c=model.c, kimg_per_tick=model.kimg_per_tick)
        torch.save(dict(cfg=c, hp=hp, total_t=total_t, steps=steps, keys=list(ref_sd.keys()), shapes={k: tuple(v.shape) for k, v in ref_sd.items()},
                        visual_names=list(model.gen_visual_names)), os.path.join(out, f"ect_step_{name}.pt"))
    return model


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    model = model_fixtures(out)
    loss_fixture(out, model)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ect"))
