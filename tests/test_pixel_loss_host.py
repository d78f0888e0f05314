"""Host-side tests of the paired / identity pixel losses of the CUT model: the float64 restatement of tests/pixel_loss_ref.py against
torch.nn.L1Loss / MSELoss, the option checks and loss names of the model, and the fixtures recorded from the unmodified reference
(tests/tools/make_fixture_pixel_loss.py -> tests/golden/pixel_loss/)."""
import os
import subprocess
import sys

import pytest
import torch

import pixel_loss_ref as R
import ref_shim

HERE = os.path.dirname(os.path.abspath(__file__))
PIX_DIR = os.path.join(HERE, "golden", "pixel_loss")
FIXTURES = ["l1_idt", "mse", "hdce_idt"]


def _load(name):
    return torch.load(os.path.join(PIX_DIR, f"cutstep_{name}.pt"), weights_only=False)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("modes", [(R.L1, R.L1), (R.MSE, R.L1), (R.OFF, R.L1), (R.L1, R.OFF), (R.L1,), (R.MSE,)], ids=str)
def test_restatement_is_torch_l1_mse_in_float64(modes, dtype):
    """losses and the closed-form gradient against nn.L1Loss / nn.MSELoss and their autograd on the valid channels, NaN in the pad channels,
    exact ties (x == y) included"""
    S, M, C, H, W = len(modes), 2, 3, 6, 10
    g = torch.Generator().manual_seed(3)
    y = torch.randn(M, H, W, 8, generator=g).to(dtype)
    x = torch.randn(S * M, H, W, 8, generator=g).to(dtype)
    tie = torch.rand(S * M, H, W, 8, generator=g) < 0.1
    x = torch.where(tie, y.repeat(S, 1, 1, 1), x)
    x[..., C:], y[..., C:] = float("nan"), float("nan")
    lambdas, up = (2.0, 0.5)[:S], torch.tensor([1.5, -3.0][:S], dtype=torch.float64)
    xv = x.double()[..., :C].clone().requires_grad_(True)
    crit = {R.L1: torch.nn.L1Loss(), R.MSE: torch.nn.MSELoss()}
    want = torch.stack([torch.zeros((), dtype=torch.float64) if m == R.OFF else lam * crit[m](xv[s * M:(s + 1) * M], y.double()[..., :C])
                        for s, (m, lam) in enumerate(zip(modes, lambdas))])
    got = R.pixel_loss(x, y, C, modes, lambdas)
    assert torch.isfinite(got).all() and torch.allclose(got, want.detach(), rtol=1e-12, atol=0)
    dx = R.pixel_grad(x, y, C, modes, lambdas, up)
    dwant = torch.autograd.grad((want * up).sum(), xv)[0] if any(m != R.OFF for m in modes) else torch.zeros_like(xv)
    assert torch.allclose(dx[..., :C], dwant, rtol=1e-12, atol=0) and bool((dx[..., C:] == 0).all())
    assert bool((dx[..., :C][tie[..., :C] & torch.tensor([m == R.L1 for m in modes]).repeat_interleave(M).view(-1, 1, 1, 1)] == 0).all())
    for s, m in enumerate(modes):
        if m == R.OFF:
            assert float(got[s]) == 0.0 and bool((dx[s * M:(s + 1) * M] == 0).all())


def test_ordered_bits_counts_neighbours():
    for dtype in (torch.float16, torch.bfloat16):
        b = R.ordered_bits(torch.tensor([1.0, -1.0, 0.0, -0.0], dtype=dtype))
        assert int(b[2]) == 0 and int(b[3]) == 0 and int(b[0]) == -int(b[1]) > 0
        pair = torch.tensor([0x3C00, 0x3C01, -0x7FFF, 0x0001], dtype=torch.int16).view(dtype)      # neighbours; -tiny and +tiny
        b = R.ordered_bits(pair)
        assert int(b[1] - b[0]) == 1 and int(b[3] - b[2]) == 2


def _opt(**cut):
    from joligen_amd.options import opt_from_json

    return opt_from_json({"model_type": "cut", "alg": {"cut": cut}}, {"gpu_ids": "0"})


def test_pixel_loss_option_checks():
    from joligen_amd import ops
    from joligen_amd.models.cut_model import CUT_DEFAULTS, check_pixel_loss_options

    assert CUT_DEFAULTS["alg_cut_lambda_supervised"] == 1.0 and CUT_DEFAULTS["alg_cut_lambda_MSE_idt"] == 1.0
    assert (ops.PIXEL_OFF, ops.PIXEL_L1, ops.PIXEL_MSE) == (R.OFF, R.L1, R.MSE)
    assert check_pixel_loss_options(_opt()) == (R.OFF, R.OFF)
    assert check_pixel_loss_options(_opt(supervised_loss=["L1"])) == (R.L1, R.OFF)
    assert check_pixel_loss_options(_opt(supervised_loss=["MSE"])) == (R.MSE, R.OFF)
    assert check_pixel_loss_options(_opt(supervised_loss=["L1", "MSE"])) == (R.MSE, R.OFF)      # the reference's if / elif: MSE first
    assert check_pixel_loss_options(_opt(supervised_loss=["MSE", "L1"])) == (R.MSE, R.OFF)
    assert check_pixel_loss_options(_opt(MSE_idt=True)) == (R.OFF, R.L1)                        # an L1 loss despite the name
    assert check_pixel_loss_options(_opt(MSE_idt=True, lambda_MSE_idt=0.0)) == (R.OFF, R.OFF)
    assert check_pixel_loss_options(_opt(supervised_loss=["L1"], MSE_idt=True, lambda_MSE_idt=0.5)) == (R.L1, R.L1)
    for bad in (["LPIPS"], ["DISTS"], ["L1", "LPIPS"], ["MSE", "DISTS"]):
        with pytest.raises(NotImplementedError, match="supervised_loss"):
            check_pixel_loss_options(_opt(supervised_loss=bad))
    with pytest.raises(ValueError, match="nce_idt"):
        check_pixel_loss_options(_opt(MSE_idt=True, nce_idt=False))
    assert check_pixel_loss_options(_opt(supervised_loss=["L1"], nce_idt=False)) == (R.L1, R.OFF)


def test_cut_loss_names_default_is_unchanged():
    from joligen_amd.models.cut_model import cut_loss_names

    assert cut_loss_names(_opt(), ["D_B_basic"]) == ["G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic"]
    assert cut_loss_names(_opt(nce_idt=False), ["D_B_projected_d", "D_B_basic"]) == ["G_tot", "G_NCE", "G_GAN_D_B_projected_d", "G_GAN_D_B_basic"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_layout_names_and_total(name):
    """the file loads and is small; cut_loss_names gives the reference's loss_names; G_tot of step 0 is the reference's sum
    (NCE + NCE_Y) / 2 + MSE_idt + supervised + GAN of the other recorded losses"""
    from joligen_amd.models.cut_model import check_nce_options, check_pixel_loss_options, cut_loss_names

    assert os.path.getsize(os.path.join(PIX_DIR, f"cutstep_{name}.pt")) < 1 << 20
    g = _load(name)
    c, hp = g["cfg"], g["hp"]
    assert c["B"] == 2 and c["iters"] == 2 and len(g["steps"]) == 2
    want = {"l1_idt": dict(supervised_loss=["L1"], lambda_supervised=2.0, MSE_idt=True, lambda_MSE_idt=0.5, nce="patchnce"),
            "mse": dict(supervised_loss=["MSE"], lambda_supervised=10.0, MSE_idt=False, nce="patchnce"),
            "hdce_idt": dict(supervised_loss=[""], MSE_idt=True, lambda_MSE_idt=1.0, netF_nc=32, nce="SRC_hDCE")}[name]
    assert c["nce_loss"] == want.pop("nce")
    for k, v in want.items():
        assert hp[k] == v, (k, hp[k], v)
    opt = _opt(supervised_loss=hp["supervised_loss"], MSE_idt=hp["MSE_idt"], lambda_MSE_idt=hp["lambda_MSE_idt"], nce_loss=c["nce_loss"])
    check_nce_options(opt)
    check_pixel_loss_options(opt)
    names_G = cut_loss_names(opt, ["D_B_basic"])
    assert names_G + ["D_tot", "D_GAN_D_B_basic"] == g["loss_names"]
    assert "G_SRC" not in g["loss_names"]
    if name == "l1_idt":
        assert g["loss_names"] == ["G_tot", "G_NCE", "G_supervised", "G_NCE_Y", "G_MSE_idt", "G_GAN_D_B_basic", "D_tot", "D_GAN_D_B_basic"]
    for s in g["steps"]:
        assert set(g["loss_names"]) <= set(s["losses"])
    l = g["steps"][0]["losses"]
    total = (l["G_NCE"] + l["G_NCE_Y"]) * 0.5 + l.get("G_MSE_idt", 0.0) + l.get("G_supervised", 0.0) + l["G_GAN_D_B_basic"]
    assert abs(total - l["G_tot"]) <= 1e-5, (total, l["G_tot"])
    assert (("G_supervised" in l) == bool([s for s in hp["supervised_loss"] if s])) and (("G_MSE_idt" in l) == hp["MSE_idt"])


def test_fixture_pixel_terms_are_the_restatement():
    """the recorded G_supervised / G_MSE_idt of step 0 are the restatement on the recorded images (fake_B is stored; fp32 reference)"""
    for name, mode in (("l1_idt", R.L1), ("mse", R.MSE)):
        g = _load(name)
        s = g["steps"][0]
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
        got = R.pixel_loss(nhwc(s["fake_B"]), nhwc(s["B"]), 3, (mode,), (g["hp"]["lambda_supervised"],))
        assert abs(float(got[0]) - s["losses"]["G_supervised"]) <= 1e-5 * abs(s["losses"]["G_supervised"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "models")),
                    reason="the reference tree is only present in the build container")
def test_pixel_loss_fixtures_regenerate(tmp_path):
    """the fixtures are outputs of the unmodified reference: the recipe writes them again, bit for bit"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(HERE, "tools", "make_fixture_pixel_loss.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    for name in FIXTURES:
        f = f"cutstep_{name}.pt"
        assert open(os.path.join(tmp_path, f), "rb").read() == open(os.path.join(PIX_DIR, f), "rb").read(), f
