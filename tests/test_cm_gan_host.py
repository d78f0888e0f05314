"""Host-side tests of cm_gan (consistency training with discriminators): the float64 restatement of tests/cm_gan_ref.py (the yardstick of the
GPU kernel tests) against the reference's own compute_cm_gan_loss, the CPU oracle of the whole step against the losses and parameter
projections recorded from the unmodified reference (tests/tools/make_fixture_cm_gan.py -> tests/golden/cm_gan/), the option checks and
names of the model, and the regeneration of the fixtures."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import cm_gan_ref as R
import jg_oracle as O
import ref_shim

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "cm_gan")
STEP_FILES = ["cm_gan_step_tiny_eff.pt", "cm_gan_step_tiny_attn.pt", "cm_gan_step_pix2pix_tiny_eff.pt"]
FILES = ["cm_gan_head.pt"] + STEP_FILES
EXAMPLE = os.path.join(HERE, "golden", "examples", "example_cm_gan_noglasses2glasses.json")
LOSSES = ["G_tot", "G_cm", "G_GAN_D_B_basic", "D_tot", "D_GAN_D_B_basic"]
# |projection - recorded| / recorded norm of a parameter tensor after each of the 3 steps.  Measured when the fixtures were made
# (tests/tools/make_fixture_cm_gan.py, then this oracle on the same machine): 0 for every tensor of G, EMA and D in all three files -- the
# oracle replays the reference bit for bit there.  The bound leaves room for another summation order of the fp32 CPU kernels (a
# projection is one dot product: a few fp32 eps of the norm); the recorded steps move the projections by 1e-3 of the norm (median).
TOL_PROJ = 1e-6


def load(name):
    return torch.load(os.path.join(DIR, name), weights_only=False)


def stand_in_D(g):
    C, S = g["pred"].shape[1], g["pred"].shape[2]
    wd = g["wd"].double()
    return lambda x: (x * wd).sum(dim=(1, 2, 3)).view(-1, 1) / (C * S) + g["bd"]


def test_restatement_reproduces_the_reference_head():
    """loss values 1e-6 relative, d(loss_G_tot)/d(pred) 1e-5, without a mask, with a 0/1 mask, and with a label mask (value 2, one sample all
    zero); the NHWC restatement of the two kernels (head_nhwc + head_bwd) gives the same numbers as autograd through the restated loss"""
    g = load("cm_gan_head.pt")
    assert set(g["cases"]) == {"none", "binary", "label"} and g["gan_lambda"] == R.GAN_LAMBDA == 0.01
    D = stand_in_D(g)
    B, C, S, _ = g["pred"].shape
    w = g["loss_weights"].double()
    for name, rec in g["cases"].items():
        mask = rec["mask"]
        pred = g["pred"].double().requires_grad_(True)
        tot, G_cm, (G_GAN,) = R.cm_gan_loss(pred, g["target"].double(), None if mask is None else mask.double(), w, [D], g["lambda_G"], g["gan_lambda"])
        (auto,) = torch.autograd.grad(tot, [pred])
        errs = [abs(float(a) - float(b)) / abs(float(b)) for a, b in ((tot.detach(), rec["G_tot"]), (G_cm, rec["G_cm"]), (G_GAN.detach(), rec["G_GAN"]))]
        e_grad = R.relerr(auto, rec["dpred"])
        # the kernels' formulation: pred = 0 * x + 1 * F_next in NHWC with 8 channels, the GAN gradient arriving as dpred
        nhwc = lambda t: torch.cat((t.permute(0, 2, 3, 1), torch.zeros(B, S, S, 8 - C, dtype=t.dtype)), dim=-1)
        zero, one, x0 = torch.zeros(B), torch.ones(B), torch.zeros(B, C, S, S)
        loss_k, pred_k, dFn_cm = R.head_nhwc(nhwc(g["pred"].double()), nhwc(g["target"].double()), x0, x0, zero, one, zero, one, mask, w.flatten(),
                                             lam=g["lambda_G"])
        p2 = g["pred"].double().requires_grad_(True)
        (dgan,) = torch.autograd.grad(g["gan_lambda"] * O.lsgan(D(p2), 1.0), [p2])
        dF, _ = R.head_bwd(dFn_cm, nhwc(dgan), 1.0, one, C)
        e_k = [abs(float(loss_k) - float(rec["G_cm"])) / abs(float(rec["G_cm"])), R.relerr(pred_k[..., :C].permute(0, 3, 1, 2), g["pred"]),
               R.relerr(dF[..., :C].permute(0, 3, 1, 2), rec["dpred"])]
        print(name, "losses %s grad %.2e; kernel formulation: loss %.2e pred %.2e grad %.2e" % (["%.2e" % e for e in errs], e_grad, *e_k))
        assert max(errs) < 1e-6 and e_grad < 1e-5, (name, errs, e_grad)
        assert e_k[0] < 1e-6 and e_k[1] == 0.0 and e_k[2] < 1e-5, (name, e_k)
        assert bool((dF[..., C:] == 0).all()) and bool((pred_k[..., C:] == 0).all())
        assert abs(float(rec["G_tot"]) - float(rec["G_cm"]) - float(rec["G_GAN"])) < 1e-7       # loss_G_tot is NOT reset before the GAN term
    none, lab = g["cases"]["none"], g["cases"]["label"]
    assert int(lab["mask"].max()) == 2 and bool((lab["mask"][1] == 0).all())
    assert torch.equal(none["G_GAN"], lab["G_GAN"])                 # fake_B is the full prediction: the mask does not reach the GAN term
    off = (lab["mask"] == 0).expand_as(lab["dpred"])
    assert bool((lab["dpred"][off] != 0).all())                     # outside the mask only the discriminator's gradient arrives


def make_trainer(g):
    hp = g["hp"]
    sdG = O.synth_state_dict({k: torch.zeros(s) for k, s in g["g_shapes"].items()}, seed=0)
    sdD = O.synth_state_dict({k: torch.zeros(s) for k, s in g["d_shapes"].items()}, seed=1)
    return R.OracleCMGanTrainer(sdG, sdD, R.cfg_of(g["cfg"], g["task"]), g["total_t"], lr_G=hp["lr_G"], lr_D=hp["lr_D"], beta1=hp["beta1"],
                                beta2=hp["beta2"], eps=hp["eps"], weight_decay=hp["weight_decay"], ema_beta=hp["ema_beta"] if hp["ema"] else None,
                                lambda_G=hp["lambda_G"], optim=hp["optim"], gan_lambda=hp["gan_lambda"], n_layers=hp["D_n_layers"],
                                pool_size=hp["pool_size"], task=g["task"])


def projections(P, names):
    return torch.stack([torch.stack([P[k].norm(), (P[k] * O.projection_vector(k, P[k].shape)).sum()]) for k in names])


@pytest.mark.parametrize("fname", STEP_FILES)
def test_oracle_trainer_reproduces_the_recorded_steps(fname):
    """every recorded loss of the three iterations within 2e-4 |loss| + 1e-6 (the bound of the ECT step test), and the projections of the
    updated G, EMA-of-G and D parameters within TOL_PROJ of the recorded ones"""
    g = load(fname)
    assert g["model_names"] == ["G_A", "D_B_basic"] and g["loss_names"] == LOSSES and g["hp"]["gan_lambda"] == 0.01
    assert g["cfg"]["S"] == 32 and g["cfg"]["B"] == 2 and g["hp"]["D_ndf"] == 16 and g["hp"]["D_n_layers"] == 3
    tr = make_trainer(g)
    gn, dn = list(g["g_shapes"]), list(g["d_shapes"])
    for it, s in enumerate(g["steps"]):
        L = tr.optimize_parameters(s["B"], s["mask"].long(), s["noise"], s["timesteps"], y_cond=s["A"] if g["task"] == "pix2pix" else None)
        assert list(s["losses"]) == LOSSES
        for k, v in s["losses"].items():
            assert abs(float(L[k]) - float(v)) < 2e-4 * abs(float(v)) + 1e-6, (it, k, float(L[k]), float(v))
        assert abs(float(s["losses"]["G_tot"]) - float(s["losses"]["G_cm"]) - float(s["losses"]["G_GAN_D_B_basic"])) < 1e-7
        for tag, mine, ref in (("G", projections(tr.P, gn), s["g_proj"]), ("ema", projections(tr.ema, gn), s["ema_proj"]),
                               ("D", projections(tr.D, dn), s["d_proj"])):
            err = float(((mine[:, 1] - ref[:, 1]).abs() / ref[:, 0]).max())
            print(fname, it, tag, "projection error / norm: max %.3e" % err)
            assert err < TOL_PROJ, (it, tag, err)
    assert tr.current_t == 3 * g["cfg"]["B"] and len(tr.pool.images) == 3 * g["cfg"]["B"]      # the pool was below its size: no host draws


def test_recorded_names_and_groups():
    from joligen_amd.models.cm_gan_model import cm_gan_loss_names

    g = load("cm_gan_step_tiny_eff.pt")
    G, D = g["groups"]
    assert G["forward_functions"] == [] and G["backward_functions"] == ["compute_cm_gan_loss"] and G["optimizer"] == ["optimizer_G"]
    assert G["loss_backward"] == ["loss_G_tot"] and G["networks_to_ema"] == ["G_A"] and G["networks_to_optimize"] == ["G_A"]
    assert D["forward_functions"] is None and D["backward_functions"] == ["compute_D_loss"] and D["optimizer"] == ["optimizer_D"]
    assert D["loss_backward"] == ["loss_D_tot"] and D["networks_to_optimize"] == ["D_B_basic"]
    assert g["loss_functions_G"] == ["compute_G_loss_GAN"]
    assert g["gen_visual_names"] == ["gt_image_", "y_t_", "next_noisy_x_", "current_noisy_x_", "mask_", "output_"]
    names_G, names_D = cm_gan_loss_names(["D_B_basic"])
    assert names_G + names_D == g["loss_names"]
    assert cm_gan_loss_names(["D_B_projected_d", "D_B_basic"]) == (["G_tot", "G_cm", "G_GAN_D_B_projected_d", "G_GAN_D_B_basic"],
                                                                   ["D_tot", "D_GAN_D_B_projected_d", "D_GAN_D_B_basic"])


def test_option_checks_need_no_device():
    from joligen_amd.models.cm_gan_model import GAN_LAMBDA, check_cm_gan_options
    from joligen_amd.options import opt_from_json

    opt = SimpleNamespace()
    assert check_cm_gan_options(opt) == ["D_B_projected_d", "D_B_basic"] and opt.alg_gan_lambda == GAN_LAMBDA == 0.01
    opt = SimpleNamespace(D_netDs=["basic"], alg_gan_lambda=1.0)
    assert check_cm_gan_options(opt) == ["D_B_basic"] and opt.alg_gan_lambda == 0.01       # forced, whatever the config says
    with pytest.raises(NotImplementedError, match="unpacks 7 values"):
        check_cm_gan_options(SimpleNamespace(alg_ddpm_ft_mode="ect"))
    for bad in (["vision_aided"], ["basic", "temporal"], ["depth"], ["mask"], []):
        with pytest.raises(NotImplementedError, match="D_netDs"):
            check_cm_gan_options(SimpleNamespace(D_netDs=bad))
    for flag in ("dataaug_APA", "dataaug_D_diffusion", "train_semantic_mask", "train_semantic_cls", "train_mask_out_mask",
                 "train_temporal_criterion"):
        with pytest.raises(NotImplementedError, match=flag):
            check_cm_gan_options(SimpleNamespace(**{flag: True}))
    with pytest.raises(NotImplementedError, match="dataaug_D_noise"):
        check_cm_gan_options(SimpleNamespace(dataaug_D_noise=0.1))
    # options the PatchGAN built here would ignore, and an output wider than the head's one 8-channel vector per pixel
    for bad, match in ((dict(D_dropout=True), "D_dropout"), (dict(D_spectral=True), "D_spectral"), (dict(D_norm="batch"), "D_norm"),
                       (dict(model_output_nc=9), "model_output_nc")):
        with pytest.raises(NotImplementedError, match=match):
            check_cm_gan_options(SimpleNamespace(**bad))
    assert check_cm_gan_options(SimpleNamespace(D_dropout=False, D_spectral=False, D_norm="instance", model_output_nc=8)) == ["D_B_projected_d", "D_B_basic"]
    # the example parses with both of its discriminators; the other model types parse what they parsed before
    ex = opt_from_json(EXAMPLE, {"gpu_ids": "0"})
    assert ex.model_type == "cm_gan" and ex.D_netDs == ["projected_d", "basic"] and ex.train_gan_mode == "lsgan" and ex.train_iter_size == 16
    assert check_cm_gan_options(ex) == ["D_B_projected_d", "D_B_basic"] and ex.alg_gan_lambda == 0.01
    bare = opt_from_json({}, {"gpu_ids": "0", "model_type": "cm_gan"})
    assert bare.D_netDs == ["projected_d", "basic"] and bare.D_ndf == 64 and bare.D_n_layers == 3
    for mt in ("palette", "cm", "cut"):
        o = opt_from_json({}, {"gpu_ids": "0", "model_type": mt})
        assert not hasattr(o, "D_netDs") and not hasattr(o, "train_gan_mode") and not hasattr(o, "dataaug_APA")


def test_example_json_is_a_settings_file():
    import json

    cfg = json.load(open(EXAMPLE))
    assert cfg["model_type"] == "cm_gan" and cfg["D"]["netDs"] == ["projected_d", "basic"] and cfg["alg"]["gan"] == {}


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "models")),
                    reason="the reference tree is only present in the build container")
def test_cm_gan_fixtures_regenerate(tmp_path):
    """every fixture is an output of the unmodified reference: the recipe writes them again, bit for bit; none is larger than the largest
    file under tests/golden/ect/"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(HERE, "tools", "make_fixture_cm_gan.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert sorted(os.listdir(tmp_path)) == sorted(FILES) == sorted(os.listdir(DIR))
    ect = os.path.join(HERE, "golden", "ect")
    limit = max(os.path.getsize(os.path.join(ect, f)) for f in os.listdir(ect))
    for f in FILES:
        assert open(os.path.join(tmp_path, f), "rb").read() == open(os.path.join(DIR, f), "rb").read(), f
        assert os.path.getsize(os.path.join(DIR, f)) <= limit, (f, limit)
    ref_example = os.path.join(ref_shim.REFERENCE_ROOT, "examples", os.path.basename(EXAMPLE))
    assert open(ref_example, "rb").read() == open(EXAMPLE, "rb").read()
