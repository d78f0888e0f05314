"""Generate tests/golden/d_aug/ from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * cutstep_{noise,apa,noise_apa}.pt : 4 x CUTModel.optimize_parameters() with dataaug_D_noise = 0.1 and / or dataaug_APA (p = 0.5, every = 2,
    nimg = 1) -- the `patchnce` step configuration of oracle/make_golden_cutstep.py at B = 2, pool = 2, recorded by that recipe's own loop.
    Beside what the recipe records, every step carries under "d_aug": the torch.normal draws of util.gaussian (`noise`: fake first, then real;
    each is sigma * z), the torch.rand draws of the APA flags (`u`), the flags (u < p before the step), p before the step and (p, adjust, s)
    after the calculator's update, and get_current_APA_prob().  `pool_draws` is the recipe's record of python's `random`, which
    includes the draws of ImagePool.get_random.
  * apa_fn.pt : DiscriminatorGANLoss.adaptive_pseudo_augmentation and update_adaptive_pseudo_augmentation_p on their own: inputs and outputs
    for predictions of both layouts ([B, 1, h, w] logit maps, [B, N] projected logits), the clamps at 0 and 1 and s == target (adjust = 0).
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.  Asserted here: every |s - target| of the step
fixtures is at least 0.05, so that a 16-bit sign flip of a near-zero logit cannot change `adjust` in a test that replays them.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_d_aug.py [output directory]"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
_argv, sys.argv = sys.argv, sys.argv[:1]          # make_golden_cutstep reads its own selection from sys.argv at import
import make_golden_cutstep as MG  # noqa: E402  (installs ref_shim)

sys.argv = _argv
import torch  # noqa: E402

import make_golden_segformer as MS  # noqa: E402

BASE = dict(MG.STEP_CFGS["patchnce"], B=2, pool=2, iters=4)
NOISE = dict(dataaug_D_noise=0.1)
APA = dict(dataaug_APA=True, dataaug_APA_p=0.5, dataaug_APA_every=2, dataaug_APA_nimg=1)
CASES = {"noise": NOISE, "apa": APA, "noise_apa": dict(NOISE, **APA)}
HP = ("dataaug_D_noise", "dataaug_APA", "dataaug_APA_p", "dataaug_APA_target", "dataaug_APA_every", "dataaug_APA_nimg")
S_MARGIN = 0.05


def _plain(v):
    return bool(v) if isinstance(v, bool) else int(v) if isinstance(v, int) else float(v)


def step_fixture(out, name, override):
    import models

    real_build_opt, real_create, real_normal, real_rec_rand = MG.build_opt, models.create_model, torch.normal, MS.Recorder.rand
    seen, steps, cur = {}, [], {}

    def build_opt(c):
        opt = real_build_opt(c)
        for k, v in override.items():
            setattr(opt, k, v)
        seen["opt"] = opt
        return opt

    def normal(*a, **k):
        n = real_normal(*a, **k)
        cur.setdefault("noise", []).append(n.clone())
        return n

    def rec_rand(self, *shape, **kw):
        u = real_rec_rand(self, *shape, **kw)
        if u.dim() == 4 and tuple(u.shape[1:]) == (1, 1, 1):      # the flags' draw (DropPath draws do not occur with the resnet generator)
            cur.setdefault("u", []).append(u.reshape(-1).clone())
        return u

    def create_model(opt, rank):
        model = real_create(opt, rank)
        calcs = [getattr(model, "D_" + dn + "_loss_calculator") for dn in model.discriminators_names]
        step = model.optimize_parameters

        def optimize_parameters():
            cur.clear()
            p_before = [float(c.adaptive_pseudo_augmentation_p) for c in calcs]
            step()
            rec = dict(noise=list(cur.get("noise", [])), u=list(cur.get("u", [])), p_before=p_before)
            if opt.dataaug_APA:
                rec["flags"] = [(u < p).to(torch.int32) for u, p in zip(rec["u"], p_before)]
                rec["p"] = [torch.as_tensor(c.adaptive_pseudo_augmentation_p, dtype=torch.float32).detach().reshape(()).clone() for c in calcs]
                rec["adjust"] = [torch.as_tensor(c.adjust, dtype=torch.float32).detach().reshape(()).clone() for c in calcs]
                rec["s"] = [c.pred_real.detach().sign().mean().reshape(()).clone() for c in calcs]
                rec["APA_prob"] = dict(model.get_current_APA_prob())
                for c, f, s, a in zip(calcs, rec["flags"], rec["s"], rec["adjust"]):
                    updated = model.niter % opt.dataaug_APA_every < opt.train_batch_size
                    assert not updated or float(torch.sign(s - opt.dataaug_APA_target)) == float(a), (name, float(s), float(a))
                    assert abs(float(s) - opt.dataaug_APA_target) >= S_MARGIN, (name, float(s))
                    base = model.real_B_noisy if opt.dataaug_D_noise > 0 else model.real_B
                    for b in range(f.numel()):      # the substituted batch the calculator saw agrees with the recorded flags
                        assert torch.equal(c.real[b], model.APA_img[b] if bool(f[b]) else base[b]), (name, b)
            steps.append(rec)

        model.optimize_parameters = optimize_parameters
        return model

    keep = MG.STEP_CFGS, MG.OUT, MG.ONLY
    MG.STEP_CFGS, MG.OUT, MG.ONLY, MG.build_opt = {name: BASE}, out, [], build_opt
    models.create_model, torch.normal, MS.Recorder.rand = create_model, normal, rec_rand
    try:
        MG.step_fixtures()
    finally:
        (MG.STEP_CFGS, MG.OUT, MG.ONLY), MG.build_opt = keep, real_build_opt
        models.create_model, torch.normal, MS.Recorder.rand = real_create, real_normal, real_rec_rand
    path = os.path.join(out, f"cutstep_{name}.pt")
    g = torch.load(path, weights_only=False)
    assert len(steps) == len(g["steps"]) == BASE["iters"]
    for s, rec in zip(g["steps"], steps):
        s["d_aug"] = rec
    for k in HP:
        g["hp"][k] = _plain(getattr(seen["opt"], k))
    torch.save(g, path)
    print(name, "p:", [[round(float(p), 4) for p in r.get("p", [])] for r in steps], "flags:", [[f.tolist() for f in r.get("flags", [])] for r in steps])


def apa_fn_fixture(out):
    from models.modules.loss import DiscriminatorGANLoss

    def calc(p, target=0.6, B=2, nimg=1, every=2):
        return DiscriminatorGANLoss(None, torch.device("cpu"), p, target, B, nimg, every, False, "lsgan", True, False, 4)

    g = torch.Generator().manual_seed(11)
    updates = []
    # (layout, prediction, p, target, B, nimg, every)
    maps = lambda B, h, w, shift: torch.randn(B, 1, h, w, generator=g) + shift
    flat = lambda B, N, shift: torch.randn(B, N, generator=g) + shift
    half = torch.ones(2, 8)
    half[:, :2] = -1.0          # 12 positive, 4 negative: s = 0.5 exactly
    cases = [("map", maps(2, 6, 6, 1.5), 0.5, 0.6, 2, 1, 2), ("map", maps(2, 6, 6, -1.5), 0.5, 0.6, 2, 1, 2), ("map", maps(3, 5, 7, 0.2), 0.25, 0.6, 3, 50, 4),
                ("flat", flat(2, 40, 2.0), 0.3, 0.6, 2, 50, 4), ("flat", flat(4, 33, -0.5), 0.0, 0.6, 4, 50, 4),
                ("map", maps(2, 6, 6, -2.0), 0.001, 0.6, 2, 1, 2),          # p + lambda < 0: clamped at 0 (p * 0)
                ("flat", flat(2, 40, 3.0), 0.999, 0.6, 2, 1, 2),            # p + lambda > 1: clamped at 1
                ("map", maps(2, 6, 6, 3.0), 1.0, 0.6, 2, 1, 2), ("flat", flat(2, 40, -3.0), 0.0, 0.6, 2, 1, 2),
                ("flat", half, 0.4, 0.5, 2, 1, 2),                          # s == target: adjust = 0, p unchanged
                ("flat", torch.cat((torch.zeros(2, 4), flat(2, 12, 1.0)), dim=1), 0.4, 0.6, 2, 7, 3)]      # exact zeros count for neither sign
    for layout, pred, p, target, B, nimg, every in cases:
        c = calc(p, target, B, nimg, every)
        c.pred_real = pred.clone()
        c.update_adaptive_pseudo_augmentation_p()
        updates.append(dict(layout=layout, pred=pred, p0=p, target=target, B=B, nimg=nimg, every=every, s=pred.sign().mean().reshape(()).clone(),
                            p=torch.as_tensor(c.adaptive_pseudo_augmentation_p, dtype=torch.float32).detach().reshape(()).clone(),
                            adjust=torch.as_tensor(c.adjust, dtype=torch.float32).detach().reshape(()).clone()))
    selects = []
    real_rand = torch.rand
    for B, p in ((4, 0.5), (3, 0.0), (3, 1.0), (5, 0.3)):
        real, fake = torch.randn(B, 3, 5, 7, generator=g), torch.randn(B, 3, 5, 7, generator=g)
        log = []

        def rand(*a, **k):
            k.pop("device", None)
            u = real_rand(*a, generator=g, **k)
            log.append(u.clone())
            return u

        torch.rand = rand
        try:
            c = calc(p)
            outp = c.adaptive_pseudo_augmentation(real, fake)
        finally:
            torch.rand = real_rand
        selects.append(dict(real=real, fake=fake, p=p, u=log[0].reshape(-1), out=outp.clone()))
    torch.save(dict(updates=updates, selects=selects), os.path.join(out, "apa_fn.pt"))
    print("apa_fn:", [(float(u["s"]), float(u["adjust"]), float(u["p"])) for u in updates])


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    for name, override in CASES.items():
        step_fixture(out, name, override)
    apa_fn_fixture(out)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "d_aug"))
