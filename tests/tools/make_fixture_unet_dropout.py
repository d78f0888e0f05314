"""Generate tests/golden/unet_dropout/ from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * palette_step_tiny_eff.pt : 3 x PaletteModel.optimize_parameters() of the `tiny_eff` recipe of oracle/make_golden.py with G_dropout = 0.25
    (a float, as the reference's own tests pass it; keep * 65536 is an integer).  It stores what palette_step_tiny_eff.pt stores and, per
    step, under "dropout" the list of (module path below netG_A, invocation of that module within the step, shape [B, C, H, W], mask) in
    invocation order.  The mask is (u < keep), bit-packed (numpy.packbits over the flattened [B, C, H, W]): the result depends on nothing else
    of the draw.  Tests inject u = 0 for a kept element and u = 1 for a dropped one (tests/unet_dropout_oracle.py).
  * cm_step_tiny_eff.pt : the same for cm_model in mode "cm" (the `tiny_eff` recipe of oracle/make_golden_cm.py, what cm_step_tiny_eff.pt
    stores): every Dropout is invoked twice per step, by the student (invocation 0) and by the no-grad teacher (invocation 1).
  * resblock_{plain,down,up_eff,up_noeff}.pt : one reference ResBlock each (RESBLOCKS below: 32 -> 64 channels with the 1x1 skip; a down
    block; the up block of the efficient UNet, convolution in front of the upsample; the plain up block) with dropout = 0.25, GroupNorm 32,
    use_scale_shift_norm: input, emb, state_dict keys / shapes (the weights are jg_oracle.synth_state_dict of them, seed 0), the mask of
    `out_layers.2`, output, the gradients of input and emb and parameter-gradient checksums for a seeded grad_output.
Only torch.nn.functional.dropout is wrapped, as in make_fixture_dropout.py: it draws u = torch.rand(x.shape) on a generator of its own (the
default generator's order, which the step's t / u / noise come from, is untouched), records the mask and returns x * (u < keep) / keep --
nn.Dropout's definition with the draw made visible.  The reference is imported at run time through oracle/ref_shim.py; nothing of its text is
here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_unet_dropout.py [output directory]"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as MG  # noqa: E402  (installs ref_shim)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import jg_oracle as O  # noqa: E402

P_DROP = 0.25
REAL_RAND = torch.rand


class DropoutRecorder:
    """torch.nn.functional.dropout with its draw recorded; `watch(net, prefix)` names the Dropout modules by forward pre-hooks"""

    def __init__(self, seed):
        self.g, self.log, self.path, self.real = torch.Generator().manual_seed(seed), [], None, F.dropout

    def dropout(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        u = REAL_RAND(x.shape, generator=self.g)
        self.log.append((self.path, (u < 1.0 - p).clone()))
        return x * (u < 1.0 - p).to(x.dtype) / (1.0 - p)

    def watch(self, net, prefix=""):
        for name, m in net.named_modules():
            if isinstance(m, nn.Dropout):
                m.register_forward_pre_hook(lambda mod, inp, path=prefix + name: setattr(self, "path", path))

    def __enter__(self):
        F.dropout = self.dropout
        return self

    def __exit__(self, *a):
        F.dropout = self.real


def pack(mask):
    return torch.from_numpy(np.packbits(mask.reshape(-1).numpy().astype(np.uint8)))


def numbered(log):
    seen, out = {}, []
    for path, m in log:
        out.append((path, seen.get(path, 0), tuple(m.shape), pack(m)))
        seen[path] = seen.get(path, 0) + 1
    return out


# name -> (channels, out_channel, up, down, efficient, input H, W): odd / non-square low resolutions, every path of the block around the mask
RESBLOCKS = {"plain": (32, 64, False, False, False, 8, 6), "down": (64, 64, False, True, True, 8, 6),
             "up_eff": (64, 64, True, False, True, 4, 3), "up_noeff": (64, 64, True, False, False, 4, 3)}
EMB = 32


def resblocks(out):
    from models.modules.unet_generator_attn.unet_generator_attn import ResBlock

    for i, (name, (cin, cout, up, down, eff, H, W)) in enumerate(RESBLOCKS.items()):
        net = ResBlock(cin, EMB, P_DROP, "groupnorm32", out_channel=cout, use_scale_shift_norm=True, up=up, down=down, efficient=eff)
        sd = O.synth_state_dict(net.state_dict(), seed=0)
        net.load_state_dict(sd)
        net.train()
        g = torch.Generator().manual_seed(100 + i)
        x = torch.randn(2, cin, H, W, generator=g).requires_grad_(True)
        emb = torch.randn(2, EMB, generator=g).requires_grad_(True)
        with DropoutRecorder(61 + i) as rec:
            rec.watch(net)
            y = net(x, emb)
        R = torch.randn(y.shape, generator=g)
        y.backward(R)
        (entry,) = numbered(rec.log)
        torch.save(dict(cfg=dict(channels=cin, out_channel=cout, up=up, down=down, efficient=eff, emb_channels=EMB, p=P_DROP), x=x.detach(),
                        emb=emb.detach(), keys=list(sd.keys()), shapes={k: tuple(v.shape) for k, v in sd.items()}, seed=0, dropout=[entry],
                        out=y.detach(), R=R, dx=x.grad.clone(), demb=emb.grad.clone(),
                        grad_checks=MG.checks({k: p.grad for k, p in net.named_parameters()})), os.path.join(out, f"resblock_{name}.pt"))
        print("resblock", name, tuple(x.shape), "->", tuple(y.shape), entry[:3])


def palette_step(out, name="tiny_eff"):
    from models import create_model

    c = MG.TINY[name]
    opt = MG.build_opt(c)
    opt.G_dropout = P_DROP
    torch.manual_seed(0)
    model = create_model(opt, 0)
    model.setup(opt)
    model.use_temporal = False
    netG = model.netG_A
    ref_sd = netG.state_dict()
    netG.load_state_dict(O.synth_state_dict(ref_sd, seed=0))
    rec = DropoutRecorder(53)
    rec.watch(netG)
    live = [n for n, m in netG.named_modules() if isinstance(m, nn.Dropout) and m.p > 0]
    assert live and all(m.p in (0.0, P_DROP) for m in netG.modules() if isinstance(m, nn.Dropout)), live
    steps = []
    with rec:
        for it in range(3):
            data = MG.synth_batch(c["B"], c["S"], seed=1234 + it)
            gen = torch.Generator().manual_seed(1000 + it)
            t, u, noise = O.draw_step_randomness(gen, data["B"], 2000)
            n0 = len(rec.log)
            model.set_input(data)
            torch.manual_seed(1000 + it)
            model.optimize_parameters()
            loss = model.get_current_losses()["G_tot"].detach().clone()
            step = dict(A=data["A"], B=data["B"], mask=data["B_label_mask"], t=t, u=u, noise=noise, loss=loss, dropout=numbered(rec.log[n0:]))
            if it in (0, 2):
                step["param_checks"] = MG.checks(dict(netG.named_parameters()))
                step["ema_checks"] = MG.checks(dict(model.netG_A_ema.named_parameters()))
            steps.append(step)
            print(name, "step", it, "loss", float(loss), [(p, k, s) for p, k, s, _ in step["dropout"]])
    hp = dict(lr=opt.train_G_lr, beta1=opt.train_beta1, beta2=opt.train_beta2, eps=opt.train_optim_eps, weight_decay=opt.train_optim_weight_decay,
              ema_beta=opt.train_G_ema_beta, lambda_G=opt.alg_diffusion_lambda_G, optim=opt.train_optim, G_dropout=P_DROP)
    names = list(dict(netG.named_parameters()).keys())
    sample = {k: dict(netG.named_parameters())[k].detach().flatten()[:8].clone() for k in names[:: max(1, len(names) // 12)]}
    torch.save(dict(cfg=c, hp=hp, steps=steps, param_sample=sample, keys=list(ref_sd.keys()), shapes={k: tuple(v.shape) for k, v in ref_sd.items()},
                    live=live), os.path.join(out, f"palette_step_{name}.pt"))


def cm_step(out, name="tiny_eff"):
    import make_golden_cm as MC
    from models import create_model

    c = MC.TINY[name]
    opt = MC.build_opt(c)
    assert opt.model_type == "cm" and opt.alg_ddpm_ft_mode == "cm", (opt.model_type, opt.alg_ddpm_ft_mode)
    opt.G_dropout = P_DROP
    torch.manual_seed(0)
    model = create_model(opt, 0)
    model.setup(opt)
    model.use_temporal = False
    netG = model.netG_A
    ref_sd = netG.state_dict()
    netG.load_state_dict(O.synth_state_dict(ref_sd, seed=0))
    rec = DropoutRecorder(59)
    rec.watch(netG)
    live = [n for n, m in netG.named_modules() if isinstance(m, nn.Dropout) and m.p > 0]
    assert live, "the reference's cm UNet has no Dropout with a rate"
    B, S, total_t = c["B"], c["S"], model.total_t
    netG.current_t = 0
    steps, cur_t = [], 0
    with rec:
        for it in range(3):
            data = MG.synth_batch(B, S, seed=4321 + it)
            sig = O.cm_karras_schedule(O.cm_improved_timesteps_schedule(cur_t, total_t))
            noise, timesteps = O.cm_draw_step_randomness(torch.Generator().manual_seed(2000 + it), data["B"], sig)
            n0 = len(rec.log)
            model.set_input(data)
            torch.manual_seed(2000 + it)
            model.optimize_parameters()
            cur_t += B
            loss = model.get_current_losses()["G_tot"].detach().clone()
            step = dict(A=data["A"], B=data["B"], mask=data["B_label_mask"], noise=noise, timesteps=timesteps, loss=loss, dropout=numbered(rec.log[n0:]))
            if it in (0, 2):
                step["param_checks"] = MG.checks(dict(netG.named_parameters()))
                step["ema_checks"] = MG.checks(dict(model.netG_A_ema.named_parameters()))
            steps.append(step)
            print("cm", name, "step", it, "loss", float(loss), [(p, k, s) for p, k, s, _ in step["dropout"]])
    hp = dict(lr=opt.train_G_lr, beta1=opt.train_beta1, beta2=opt.train_beta2, eps=opt.train_optim_eps, weight_decay=opt.train_optim_weight_decay,
              ema_beta=opt.train_G_ema_beta, lambda_G=opt.alg_diffusion_lambda_G, optim=opt.train_optim, ema=bool(opt.train_G_ema), G_dropout=P_DROP)
    torch.save(dict(cfg=c, hp=hp, total_t=total_t, steps=steps, keys=list(ref_sd.keys()), shapes={k: tuple(v.shape) for k, v in ref_sd.items()},
                    live=live), os.path.join(out, f"cm_step_{name}.pt"))


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    resblocks(out)
    palette_step(out)
    cm_step(out)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "unet_dropout"))
