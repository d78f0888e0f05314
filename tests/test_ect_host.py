"""Host-side tests of easy consistency tuning (cm_model, alg_ddpm_ft_mode = "ect"): the t -> r map and the training scalings against
values recorded from the unmodified reference (tests/tools/make_fixture_ect.py -> tests/golden/ect/), the tick / stage schedule, the
option check, the float64 restatement of tests/ect_ref.py (the yardstick of the GPU kernel test) against the reference's own
compute_ect_loss, the CPU oracle of the step against the recorded losses, and the regeneration of the fixtures."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import ect_ref as R
import ref_shim
from joligen_amd.models.cm_model import ect_tick
from joligen_amd.modules.cm_generator import check_ft_mode, output_scaling_train, skip_scaling_train, t_to_r_sigmoid

HERE = os.path.dirname(os.path.abspath(__file__))
ECT_DIR = os.path.join(HERE, "golden", "ect")
FILES = ["ect_fn.pt", "ect_loss.pt"] + [f"ect_{k}_{c}.pt" for k in ("gen", "step") for c in ("tiny_eff", "tiny_attn")]


def load(name):
    return torch.load(os.path.join(ECT_DIR, name), weights_only=False)


def ulp_close(a, b):
    """equal, or one fp32 unit in the last place apart"""
    return bool((a == b).logical_or(a == torch.nextafter(b, a)).all())


def test_t_to_r_and_train_scalings_vs_reference():
    g = load("ect_fn.pt")
    t = g["t"]
    assert float(t.min()) < 0.51 < 1.9459 < float(t.max())
    for stage, r_ref in g["r"].items():
        r = t_to_r_sigmoid(g["k"], g["b"], g["q"], t, stage)
        assert torch.equal(r == 0, r_ref == 0), stage                   # the same samples take the r = 0 branch
        assert ulp_close(r, r_ref), (stage, r, r_ref)
        assert ulp_close(R.t_to_r(t, stage), r_ref)
    assert (g["r"][0] == 0).sum() > (g["r"][1] == 0).sum() > (g["r"][3] == 0).sum() == 0
    assert ulp_close(skip_scaling_train(t, g["sigma_data"], g["sigma_min"]), g["skip_scaling_train"])
    assert ulp_close(output_scaling_train(t, g["sigma_data"], g["sigma_min"]), g["output_scaling_train"])
    zero = torch.zeros(3)
    assert torch.equal(skip_scaling_train(zero), torch.ones(3)) and torch.equal(output_scaling_train(zero), zero)   # r = 0: D_yr is x itself


def test_tick_and_stage_schedule():
    from joligen_amd.modules.cm_generator import CMGenerator

    class Net:                                                          # the fields update_stage works on, without a UNet
        stage, q, double_ticks, ratio = 0, 2.0, 1000, 0.5
        update_stage = CMGenerator.update_stage

    net = Net()
    st = dict(cur_tick=0, cur_nimg=0, tick_start_nimg=0, kimg_per_tick=50)
    assert ect_tick(st, 49_999, net) is False and st["cur_tick"] == 0 and st["cur_nimg"] == 49_999
    assert ect_tick(st, 1, net) is True and st["cur_tick"] == 1 and st["tick_start_nimg"] == 50_000 and net.stage == 0
    assert ect_tick(st, 49_999, net) is False and ect_tick(st, 2, net) is True and st["cur_tick"] == 2 and st["tick_start_nimg"] == 100_001
    net.update_stage(999)
    assert net.stage == 0 and net.ratio == 0.5
    net.update_stage(1000)
    assert net.stage == 1 and net.ratio == 0.75
    net.update_stage(3500)
    assert net.stage == 3 and net.ratio == 1 - 1 / 16
    net.update_stage(1200)                                              # never goes down
    assert net.stage == 3 and net.ratio == 1 - 1 / 16
    st = dict(cur_tick=999, cur_nimg=0, tick_start_nimg=0, kimg_per_tick=50)
    net2 = Net()
    assert ect_tick(st, 50_000, net2) and net2.stage == 1


def test_ft_mode_option_check():
    assert check_ft_mode(SimpleNamespace()) == "cm"
    assert check_ft_mode(SimpleNamespace(alg_ddpm_ft_mode="cm")) == "cm" and check_ft_mode(SimpleNamespace(alg_ddpm_ft_mode="ect")) == "ect"
    for bad in ("ECT", "", "ecm", None):
        with pytest.raises(NotImplementedError, match="alg_ddpm_ft_mode"):
            check_ft_mode(SimpleNamespace(alg_ddpm_ft_mode=bad))
    from joligen_amd.options import opt_from_json

    assert opt_from_json({}, {"gpu_ids": "0"}).alg_ddpm_ft_mode == "cm"
    assert opt_from_json({}, {"gpu_ids": "0", "alg_ddpm_ft_mode": "ect"}).alg_ddpm_ft_mode == "ect"


def test_restatement_reproduces_the_reference_loss():
    """loss 1e-6 relative, gradient 1e-5, for the mask absent, 0/1, and a label mask with a value of 2 and one sample all zero; the
    closed-form gradient is also what autograd gives for the restated loss"""
    g = load("ect_loss.pt")
    assert set(g["cases"]) == {"none", "binary", "label"} and g["c"] == R.ECT_C
    dt = (g["t"] - g["r"]).double()
    for name, rec in g["cases"].items():
        mask = rec["mask"]
        pred = g["pred"].double().requires_grad_(True)
        loss = R.ect_loss(pred, g["target"].double(), None if mask is None else mask.double(), dt, g["c"], g["lambda_G"])
        (auto,) = torch.autograd.grad(loss, [pred])
        grad = R.ect_grad(pred.detach(), g["target"].double(), mask, dt, g["c"], g["lambda_G"])
        e_loss = abs(float(loss.detach()) - float(rec["loss"])) / abs(float(rec["loss"]))
        e_grad, e_auto = R.relerr(grad, rec["dpred"]), R.relerr(grad, auto)
        print(name, "loss %.2e grad %.2e closed form vs autograd %.2e" % (e_loss, e_grad, e_auto))
        assert e_loss < 1e-6 and e_grad < 1e-5 and e_auto < 1e-12, (name, e_loss, e_grad, e_auto)
        if mask is not None:
            assert bool((grad[(mask == 0).expand_as(grad)] == 0).all())
    lab = g["cases"]["label"]
    assert int(lab["mask"].max()) == 2 and bool((lab["mask"][1] == 0).all())
    assert bool((lab["dpred"][1] == 0).all()) and bool(torch.isfinite(lab["dpred"]).all())     # all-zero mask: loss_b = 0, no NaN


@pytest.mark.parametrize("name", ["tiny_eff", "tiny_attn"])
def test_oracle_trainer_reproduces_the_recorded_steps(name):
    from test_oracle_golden import cm_cfg_of

    g = load(f"ect_step_{name}.pt")
    hp = g["hp"]
    assert g["visual_names"] == ["gt_image_", "y_t_", "t_noisy_x_", "r_noisy_x_", "mask_", "output_"]
    allr = torch.cat([s["r"] for s in g["steps"]])
    assert bool((allr == 0).any()) and bool((allr > 0).any())
    sd = {k: torch.zeros(g["shapes"][k]) for k in g["keys"]}
    import jg_oracle as O

    tr = R.OracleECTTrainer(O.synth_state_dict(sd, seed=0), cm_cfg_of(g["cfg"]), g["total_t"], lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"],
                            eps=hp["eps"], weight_decay=hp["weight_decay"], ema_beta=hp["ema_beta"] if hp["ema"] else None,
                            lambda_G=hp["lambda_G"], optim=hp["optim"])
    for it, s in enumerate(g["steps"]):
        loss = float(tr.optimize_parameters(s["B"], s["mask"], s["noise"], s["rnd_normal"]))
        print(name, it, loss, float(s["loss"]))
        assert abs(loss - float(s["loss"])) < 2e-4 * abs(float(s["loss"])) + 1e-6, (it, loss, float(s["loss"]))
    assert tr.current_t == 3 * g["cfg"]["B"]


def test_generator_fixture_layout():
    for name in ("tiny_eff", "tiny_attn"):
        g = load(f"ect_gen_{name}.pt")
        assert bool((g["r"] == 0).any()) and bool((g["r"] > 0).any())
        z = g["r"] == 0
        assert torch.equal(g["D_yr"][z], g["r_noisy_x"][z]) and torch.equal(g["r_noisy_x"][z], g["B"][z])    # r = 0: the teacher returns x


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "models")),
                    reason="the reference tree is only present in the build container")
def test_ect_fixtures_regenerate(tmp_path):
    """every fixture is an output of the unmodified reference: the recipe writes them again, bit for bit"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(HERE, "tools", "make_fixture_ect.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert sorted(os.listdir(tmp_path)) == sorted(FILES) == sorted(os.listdir(ECT_DIR))
    for f in FILES:
        assert open(os.path.join(tmp_path, f), "rb").read() == open(os.path.join(ECT_DIR, f), "rb").read(), f
        assert os.path.getsize(os.path.join(ECT_DIR, f)) < 1 << 20
