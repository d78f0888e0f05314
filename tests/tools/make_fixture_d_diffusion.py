"""Generate tests/golden/d_diffusion/ from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * diffusion_fn.pt : the reference `Diffusion` (models/modules/projected_d/diffusion.py) on its own.
      tables  : for p in {0, 0.37, 1} as float32 and for p whose p * 64 / p * 495 lies on a .5 tie in float32: T, n, alphas_bar_sqrt,
                one_minus_alphas_bar_sqrt and t_epl after update_T();
      forward : Diffusion.forward on four maps with np.random.choice and torch.randn_like wrapped to record t and the noise (before the
                multiplication by noise_std), the state it ran on and its outputs;
      updates : sequences of DiscriminatorGANLoss.update with loss_D_real above, below and equal to 0.9 and at both clamps: p (float32), T
                and n after every call.
  * projd_diffusion.pt : the recipe of oracle/make_golden_projd.py (stand-in backbone, synthetic weights) with diffusion_aug=True and p = 0.37
      at interp 128, B = 1: compute_loss_D, its parameter gradients, compute_loss_G, dfake, the recorded draws of the three forwards, the state the
      forwards ran on and (p, T, n) after `update`.  Asserted here: |loss_D_real - 0.9| >= 0.05, so that 16-bit rounding cannot flip the
      sign in a replay.
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_d_diffusion.py [output directory]"""
import importlib.machinery
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
try:
    import scipy.signal  # noqa: F401  (imported, never used, by the reference's diffusion.py)
except ImportError:
    for name in ("scipy", "scipy.signal"):
        mod = types.ModuleType(name)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, loader=None, is_package=True)
        mod.__path__ = []
        sys.modules[name] = mod

import numpy as np  # noqa: E402
import torch  # noqa: E402

import jg_oracle as O  # noqa: E402
from make_golden import checks  # noqa: E402

WIDTHS = (24, 40, 112, 320)
LOSS_MARGIN = 0.05


class Recorder:
    """wraps np.random.choice and torch.randn_like while active; `t` / `z`: the draws in call order"""

    def __init__(self):
        self.t, self.z = [], []

    def __enter__(self):
        self.real_choice, self.real_randn_like = np.random.choice, torch.randn_like

        def choice(*a, **k):
            r = self.real_choice(*a, **k)
            self.t.append(torch.from_numpy(np.asarray(r).copy()).to(torch.int32))
            return r

        def randn_like(x, **k):
            r = self.real_randn_like(x, **k)
            self.z.append(r.clone())
            return r

        np.random.choice, torch.randn_like = choice, randn_like
        return self

    def __exit__(self, *a):
        np.random.choice, torch.randn_like = self.real_choice, self.real_randn_like


def state_of(d):
    t_epl = torch.from_numpy(np.asarray(d.t_epl).copy()).to(torch.int32)
    return dict(p=torch.tensor(float(d.p), dtype=torch.float64), T=int(d.num_timesteps), n=int((t_epl != 0).sum()), a=d.alphas_bar_sqrt.clone(),
                b=d.one_minus_alphas_bar_sqrt.clone(), t_epl=t_epl)


def find_tie(scale):
    """a float32 p in (0, 1) whose float32 product p * scale is m + 0.5 exactly, with m even and with m odd (round half to even goes both ways)"""
    out = []
    for want_odd in (False, True):
        for m in range(3, int(scale) - 1):
            if (m % 2 == 1) != want_odd:
                continue
            p = np.float32((m + 0.5) / scale)
            if float(np.float32(p * np.float32(scale))) == m + 0.5:
                out.append(p)
                break
    return out


def fn_fixture(out):
    from models.modules.loss import DiscriminatorGANLoss
    from models.modules.projected_d.diffusion import Diffusion

    np.random.seed(1234)
    torch.manual_seed(4321)
    ps = [np.float32(0.0), np.float32(0.37), np.float32(1.0)] + find_tie(64.0) + find_tie(495.0)
    tables = []
    for p in ps:
        d = Diffusion(t_min=5, t_max=500, beta_start=1e-4, beta_end=1e-2)
        d.p = p
        d.update_T()
        st = state_of(d)
        st["p64"], st["p495"] = float(np.float32(p * np.float32(64))), float(np.float32(p * np.float32(495)))
        tables.append(st)
    # forward on four maps (B = 3, the lite0 widths at 8x8 .. 1x1) at p = 0.37
    d = Diffusion(t_min=5, t_max=500, beta_start=1e-4, beta_end=1e-2)
    d.p = np.float32(0.37)
    d.update_T()
    xs = [torch.randn(3, c, s, s) for c, s in zip(WIDTHS, (8, 4, 2, 1))]
    with Recorder() as rec:
        outs = [d(x, noise_std=0.5) for x in xs]
    forward = dict(state=state_of(d), noise_std=0.5, xs=xs, outs=[o.clone() for o in outs], t=[t.reshape(x.shape[0], x.shape[1]) for t, x in zip(rec.t, xs)],
                   z=rec.z)
    assert len(rec.t) == len(rec.z) == 4
    # update sequences: a stub discriminator that carries the reference's Diffusion where the calculator looks for it
    updates = []
    for B, every, losses in ((1000, 50, [0.5, 1.2, 0.9, 1.5, 2.0, 0.3, 0.9, 0.1, 0.2, 0.95]),
                             (3, 7, [1.0, 1.0, 0.2, 1.3, 0.9, 0.9001, 0.8999, 1.0, 1.0, 1.0, 0.0, 2.0]),
                             (16, 4, [1.1] * 6)):
        netD = types.SimpleNamespace(freeze_feature_network=types.SimpleNamespace(diffusion=Diffusion(t_min=5, t_max=500, beta_start=1e-4, beta_end=1e-2)))
        calc = DiscriminatorGANLoss(netD, torch.device("cpu"), 0.0, 0.6, B, 50, 4, False, "projected", False, True, every)
        seq = []
        for i, lv in enumerate(losses):
            calc.loss_D_real = torch.tensor(lv, dtype=torch.float32)
            calc.update(i * every)              # niter % every == 0 < B: every call updates
            dd = netD.freeze_feature_network.diffusion
            assert np.asarray(dd.p).dtype == np.float32
            st = state_of(dd)
            seq.append(dict(loss=calc.loss_D_real.clone(), p=torch.tensor(float(dd.p), dtype=torch.float32), T=st["T"], n=st["n"]))
        updates.append(dict(B=B, every=every, steps=seq))
    torch.save(dict(tables=tables, forward=forward, updates=updates), os.path.join(out, "diffusion_fn.pt"))
    print("tables:", [(float(t["p"]), t["T"], t["n"], t["p64"], t["p495"]) for t in tables])
    print("updates:", [[(round(float(s["p"]), 5), s["T"], s["n"]) for s in u["steps"]] for u in updates])


def projd_fixture(out):
    import timm

    from joligen_amd.modules.projected_d import StandInEfficientNet

    timm.create_model = lambda *a, **k: StandInEfficientNet()
    from models.modules.loss import DiscriminatorGANLoss
    from models.modules.projected_d.discriminator import ProjectedDiscriminator

    S, interp, B, every = 64, 128, 1, 4      # interp 128: the smallest the four mini-discriminators accept; B = 1: the three forwards' noise stays under the file-size limit
    torch.manual_seed(0)
    np.random.seed(99)
    netD = ProjectedDiscriminator("efficientnet", interp=interp, img_size=S, diffusion_aug=True)
    ref_sd = netD.state_dict()
    netD.load_state_dict(O.synth_state_dict(ref_sd, seed=5))
    netD.train()
    dif = netD.freeze_feature_network.diffusion
    dif.p = np.float32(0.37)
    dif.update_T()
    state = state_of(dif)
    g = torch.Generator().manual_seed(77)
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    fake = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    lossf = DiscriminatorGANLoss(netD=netD, device=torch.device("cpu"), dataaug_APA_p=0, dataaug_APA_target=0.6, train_batch_size=B,
                                 dataaug_APA_nimg=50, dataaug_APA_every=4, dataaug_D_label_smooth=False, train_gan_mode="projected",
                                 dataaug_APA=False, dataaug_D_diffusion=True, dataaug_D_diffusion_every=every)
    for p in netD.discriminator.parameters():
        p.requires_grad_(True)
    with Recorder() as rec:
        loss_D = lossf.compute_loss_D(netD, real, fake, None)
        pred_real = lossf.pred_real.detach().clone()
        loss_D.backward()
        grads = {k: p.grad.detach().clone() for k, p in netD.named_parameters() if p.grad is not None}
        sd_mid = {k: v.clone() for k, v in netD.state_dict().items() if k.endswith("weight_u") or k.endswith("weight_v")}
        fk = fake.clone().requires_grad_(True)
        loss_G = lossf.compute_loss_G(netD, real, fk)
        loss_G.backward()
    assert len(rec.t) == len(rec.z) == 12
    loss_D_real = lossf.loss_D_real.detach().clone()
    assert abs(float(loss_D_real) - 0.9) >= LOSS_MARGIN, float(loss_D_real)
    feat_hw = [interp // s for s in (4, 8, 16, 32)]
    draws = [dict(t=[rec.t[4 * f + l].reshape(B, WIDTHS[l]) for l in range(4)], z=[rec.z[4 * f + l] for l in range(4)]) for f in range(3)]
    for dr in draws:
        for l in range(4):
            assert tuple(dr["z"][l].shape) == (B, WIDTHS[l], feat_hw[l], feat_hw[l])
    lossf.update(0)
    after = state_of(dif)
    torch.save(dict(cfg=dict(S=S, interp=interp, B=B, every=every), keys=list(ref_sd.keys()), shapes={k: tuple(v.shape) for k, v in ref_sd.items()},
                    real=real, fake=fake, pred_real=pred_real, loss_D=loss_D.detach(), loss_D_real=loss_D_real, grad_checks=checks(grads),
                    uv_mid=checks(sd_mid), loss_G=loss_G.detach(), dfake=fk.grad.detach().clone(), state=state, draws=draws,
                    after=dict(p=torch.tensor(float(after["p"]), dtype=torch.float32), T=after["T"], n=after["n"])),
               os.path.join(out, "projd_diffusion.pt"))
    print("projd_diffusion: loss_D", float(loss_D), "loss_D_real", float(loss_D_real), "loss_G", float(loss_G), "state", state["T"], state["n"],
          "after", float(after["p"]), after["T"], after["n"])


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    fn_fixture(out)
    projd_fixture(out)
    sizes = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    print("bytes:", sizes)
    assert all(v < 1_000_000 for v in sizes.values()), sizes


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "d_diffusion"))
