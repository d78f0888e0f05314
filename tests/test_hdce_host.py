"""Host-side tests of the SRC_hDCE loss: the restatement of tests/hdce_ref.py against fixtures recorded from the unmodified reference
(tests/tools/make_fixture_hdce.py -> tests/golden/hdce/), the regeneration of those fixtures, and the option checks of the CUT model."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

import hdce_ref as R
import ref_shim

HERE = os.path.dirname(os.path.abspath(__file__))
HDCE_DIR = os.path.join(HERE, "golden", "hdce")


def _records():
    return torch.load(os.path.join(HDCE_DIR, "hdce_loss.pt"), weights_only=False)["records"]


def test_restatement_reproduces_the_reference_fixture():
    """weights of SRC_Loss (off the diagonal: the reference's diagonal is the softmax of -10 and is never used), PatchHDCELoss per-patch
    loss with the weights and with weight=None, and dq / dk of both under the recorded row weighting"""
    recs = _records()
    assert {(r["case"], r["T"], r["gamma"]) for r in recs} == {(c, T, g) for c in ("per_image", "all_negatives") for T, g in ((0.07, 1.0), (0.2, 0.1))}
    for r in recs:
        nimg, P = r["nimg"], r["q"].shape[0] // r["nimg"]
        assert P == r["D"], "the reference's diagonal mask is eye(feature width)"
        off = ~torch.eye(P, dtype=torch.bool)[None].expand(nimg, P, P)
        w = R.hdce_weights(r["k"], nimg, r["gamma"])
        e = R.relerr(w[off], r["weights"][off])
        print(r["case"], r["T"], r["gamma"], "weights %.2e" % e)
        assert e < 1e-5, e
        for tag, wcount in (("weighted", 1), ("unweighted", 0)):
            q, k = r["q"].clone().requires_grad_(True), r["k"].clone().requires_grad_(True)
            loss = R.hdce_loss(q, k, nimg, r["T"], r["gamma"], 1, wcount)
            dq, dk = torch.autograd.grad((loss * r["row_weight"]).sum(), [q, k])
            ref = r[tag]
            errs = R.relerr(loss, ref["loss"]), R.relerr(dq, ref["dq"]), R.relerr(dk, ref["dk"])
            print(r["case"], r["T"], r["gamma"], tag, "loss %.2e dq %.2e dk %.2e" % errs)
            assert errs[0] < 1e-6 and errs[1] < 2e-6 and errs[2] < 2e-6, (r["case"], r["T"], r["gamma"], tag, errs)
        assert R.relerr(r["weighted"]["loss"], r["unweighted"]["loss"]) > 1e-2      # the two modes are different losses


def test_step_fixture_layout():
    g = torch.load(os.path.join(HDCE_DIR, "cutstep_hdce.pt"), weights_only=False)
    c = g["cfg"]
    assert c["nce_loss"] == "SRC_hDCE" and c["B"] == 2 and c["iters"] == 3 and len(g["steps"]) == 3
    assert c["num_patches"] == g["hp"]["netF_nc"] == 32 and g["hp"]["HDCE_gamma"] == 1.0
    assert "G_SRC" not in g["loss_names"]
    for s in g["steps"]:
        assert {"G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic", "D_tot"} <= set(s["losses"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "models")),
                    reason="the reference tree is only present in the build container")
def test_hdce_fixtures_regenerate(tmp_path):
    """both fixtures are outputs of the unmodified reference: the recipe writes them again, bit for bit"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(HERE, "tools", "make_fixture_hdce.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    for f in ("hdce_loss.pt", "cutstep_hdce.pt"):
        assert open(os.path.join(tmp_path, f), "rb").read() == open(os.path.join(HDCE_DIR, f), "rb").read(), f
        assert os.path.getsize(os.path.join(HDCE_DIR, f)) < 1 << 20


def test_cut_option_checks():
    from joligen_amd.models.cut_model import CUT_DEFAULTS, check_nce_options
    from joligen_amd.options import opt_from_json

    assert CUT_DEFAULTS["alg_cut_HDCE_gamma"] == 1.0 and CUT_DEFAULTS["alg_cut_HDCE_gamma_min"] == 1.0

    def opt(**cut):
        return opt_from_json({"model_type": "cut", "alg": {"cut": cut}}, {"gpu_ids": "0"})

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert check_nce_options(opt(nce_loss="SRC_hDCE")) is True
        assert check_nce_options(opt(nce_loss="SRC_hDCE", HDCE_gamma=0.1)) is True
        assert check_nce_options(opt(nce_loss="monce")) is False and check_nce_options(opt()) is False
    for gamma in (0.0, -1.0):
        with pytest.raises(ValueError, match="gamma"):
            check_nce_options(opt(nce_loss="SRC_hDCE", HDCE_gamma=gamma))
    for loss in ("monce", "patchnce"):
        with pytest.raises(NotImplementedError, match="lambda_SRC"):
            check_nce_options(opt(nce_loss=loss, lambda_SRC=0.05))
    with pytest.warns(UserWarning, match="does not enter the update"):
        assert check_nce_options(opt(nce_loss="SRC_hDCE", lambda_SRC=0.05)) is True
    with pytest.raises(NotImplementedError):
        check_nce_options(opt(nce_loss="other"))
