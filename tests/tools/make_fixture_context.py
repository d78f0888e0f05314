"""Generate tests/golden/context/ from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * cutstep_{c5,c5_noise_apa,c8}.pt : 4 x CUTModel.optimize_parameters() with data_online_context_pixels = 5 / 5 (+ dataaug_D_noise = 0.1 and
    dataaug_APA: p = 0.5, every = 2, nimg = 1) / 8 -- the `patchnce` step configuration of oracle/make_golden_cutstep.py at B = 2, pool = 2,
    crop 32, recorded by that recipe's own loop with its batches generated at 32 + 2 c.  With c = 5 the PatchGAN sees 42 x 42 images and its
    second stride-2 layer an odd 21 x 21 map; with c = 8 every map is even.
    Beside what the recipe records, every step carries under "d_aug" what tests/tools/make_fixture_d_aug.py records (the torch.normal draws of
    util.gaussian -- fake first, then real, each sigma * z at the FRAMED size --, the torch.rand draws of the APA flags, the flags, p before and
    (p, adjust, s) after the update, get_current_APA_prob()); step 0 carries `fake_B_with_context`; the file carries the option value under
    hp["data_online_context_pixels"] and the reference's `context_visual_names`.  `pool_draws` includes the draws of ImagePool.get_random.
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.  Asserted here: every |s - target| is at least
0.05 (a 16-bit sign flip of a near-zero logit cannot change `adjust` in a test that replays the fixture), and the recorded frame: inside the
window fake_B_with_context is fake_B, outside it real_A_with_context (= the batch's A).
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_context.py [output directory [case ...]]"""
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
NOISE_APA = dict(dataaug_D_noise=0.1, dataaug_APA=True, dataaug_APA_p=0.5, dataaug_APA_every=2, dataaug_APA_nimg=1)
CASES = {"c5": dict(data_online_context_pixels=5), "c5_noise_apa": dict(NOISE_APA, data_online_context_pixels=5), "c8": dict(data_online_context_pixels=8)}
HP = ("data_online_context_pixels", "dataaug_D_noise", "dataaug_APA", "dataaug_APA_p", "dataaug_APA_target", "dataaug_APA_every", "dataaug_APA_nimg")
S_MARGIN = 0.05


def _plain(v):
    return bool(v) if isinstance(v, bool) else int(v) if isinstance(v, int) else float(v)


def step_fixture(out, name, override):
    import models

    c = override["data_online_context_pixels"]
    real_build_opt, real_create, real_normal, real_rec_rand, real_batch = MG.build_opt, models.create_model, torch.normal, MS.Recorder.rand, MG.batch
    seen, steps, cur = {}, [], {}

    def build_opt(cfg):
        opt = real_build_opt(cfg)
        for k, v in override.items():
            setattr(opt, k, v)
        seen["opt"] = opt
        return opt

    def batch(B, S, seed, rand=MG.REAL_RAND):      # the loader's images: the crop plus c pixels on every side
        return real_batch(B, S + 2 * c, seed, rand)

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
        seen["model"] = model
        calcs = [getattr(model, "D_" + dn + "_loss_calculator") for dn in model.discriminators_names]
        step = model.optimize_parameters

        def optimize_parameters():
            cur.clear()
            p_before = [float(cc.adaptive_pseudo_augmentation_p) for cc in calcs]
            step()
            S = opt.data_crop_size
            fwc = model.fake_B_with_context.detach()
            assert tuple(fwc.shape[2:]) == (S + 2 * c, S + 2 * c) and tuple(model.fake_B.shape[2:]) == (S, S), (fwc.shape, model.fake_B.shape)
            assert torch.equal(fwc[:, :, c:-c, c:-c], model.fake_B.detach())
            ring = torch.ones_like(fwc, dtype=torch.bool)
            ring[:, :, c:-c, c:-c] = False
            assert torch.equal(fwc[ring], model.real_A_with_context[ring])
            rec = dict(noise=list(cur.get("noise", [])), u=list(cur.get("u", [])), p_before=p_before)
            if not steps:
                rec["fake_B_with_context"] = fwc.clone()
            if opt.dataaug_APA:
                rec["flags"] = [(u < p).to(torch.int32) for u, p in zip(rec["u"], p_before)]
                rec["p"] = [torch.as_tensor(cc.adaptive_pseudo_augmentation_p, dtype=torch.float32).detach().reshape(()).clone() for cc in calcs]
                rec["adjust"] = [torch.as_tensor(cc.adjust, dtype=torch.float32).detach().reshape(()).clone() for cc in calcs]
                rec["s"] = [cc.pred_real.detach().sign().mean().reshape(()).clone() for cc in calcs]
                rec["APA_prob"] = dict(model.get_current_APA_prob())
                for cc, f, s, a in zip(calcs, rec["flags"], rec["s"], rec["adjust"]):
                    updated = model.niter % opt.dataaug_APA_every < opt.train_batch_size
                    assert not updated or float(torch.sign(s - opt.dataaug_APA_target)) == float(a), (name, float(s), float(a))
                    assert abs(float(s) - opt.dataaug_APA_target) >= S_MARGIN, (name, float(s))
                    base = model.real_B_with_context_noisy if opt.dataaug_D_noise > 0 else model.real_B_with_context
                    assert tuple(model.APA_img.shape) == tuple(base.shape)
                    for b in range(f.numel()):      # the substituted batch the calculator saw agrees with the recorded flags
                        assert torch.equal(cc.real[b], model.APA_img[b] if bool(f[b]) else base[b]), (name, b)
            steps.append(rec)

        model.optimize_parameters = optimize_parameters
        return model

    keep = MG.STEP_CFGS, MG.OUT, MG.ONLY
    MG.STEP_CFGS, MG.OUT, MG.ONLY, MG.build_opt, MG.batch = {name: BASE}, out, [], build_opt, batch
    models.create_model, torch.normal, MS.Recorder.rand = create_model, normal, rec_rand
    try:
        MG.step_fixtures()
    finally:
        (MG.STEP_CFGS, MG.OUT, MG.ONLY), MG.build_opt, MG.batch = keep, real_build_opt, real_batch
        models.create_model, torch.normal, MS.Recorder.rand = real_create, real_normal, real_rec_rand
    path = os.path.join(out, f"cutstep_{name}.pt")
    g = torch.load(path, weights_only=False)
    assert len(steps) == len(g["steps"]) == BASE["iters"]
    for s, rec in zip(g["steps"], steps):
        s["d_aug"] = rec
    for k in HP:
        g["hp"][k] = _plain(getattr(seen["opt"], k))
    g["context_visual_names"] = list(seen["model"].context_visual_names)
    torch.save(g, path)
    print(name, "p:", [[round(float(p), 4) for p in r.get("p", [])] for r in steps], "flags:", [[f.tolist() for f in r.get("flags", [])] for r in steps])


def main(out, only=()):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    for name, override in CASES.items():
        if only and name not in only:
            continue
        step_fixture(out, name, override)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "context"), sys.argv[2:])
