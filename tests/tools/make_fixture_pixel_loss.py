"""Generate tests/golden/pixel_loss/cutstep_{l1_idt,mse,hdce_idt}.pt from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
N x CUTModel.optimize_parameters() with the paired / identity pixel losses of compute_G_loss_cut -- the `patchnce` step configuration of
oracle/make_golden_cutstep.py at B = 2, two iterations, recorded by that recipe's own loop:
  * l1_idt   : alg_cut_supervised_loss = ["L1"], lambda_supervised = 2, alg_cut_MSE_idt with lambda_MSE_idt = 0.5;
  * mse      : alg_cut_supervised_loss = ["MSE"], lambda_supervised = 10;
  * hdce_idt : alg_cut_nce_loss = "SRC_hDCE" (alg_cut_netF_nc = num_patches = 32, as in make_fixture_hdce.py) with alg_cut_MSE_idt: the
               identity contrastive term runs with the hDCE weights too.
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_pixel_loss.py [output directory]"""
import os
import tempfile
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
_argv, sys.argv = sys.argv, sys.argv[:1]          # make_golden_cutstep reads its own selection from sys.argv at import
import make_golden_cutstep as MG  # noqa: E402  (installs ref_shim)

sys.argv = _argv
import torch  # noqa: E402

BASE = dict(MG.STEP_CFGS["patchnce"], B=2, iters=2)
CASES = {      # name: (step configuration, options set on the parsed opt)
    "l1_idt": (BASE, dict(alg_cut_supervised_loss=["L1"], alg_cut_lambda_supervised=2.0, alg_cut_MSE_idt=True, alg_cut_lambda_MSE_idt=0.5)),
    "mse": (BASE, dict(alg_cut_supervised_loss=["MSE"], alg_cut_lambda_supervised=10.0)),
    "hdce_idt": (dict(BASE, nce_loss="SRC_hDCE"), dict(alg_cut_netF_nc=32, alg_cut_MSE_idt=True)),
}
HP = ("supervised_loss", "lambda_supervised", "MSE_idt", "lambda_MSE_idt", "HDCE_gamma", "netF_nc", "lambda_SRC")


def step_fixture(out, name, cfg, override):
    real_build_opt = MG.build_opt
    seen = {}

    def build_opt(c):
        opt = real_build_opt(c)
        for k, v in override.items():
            setattr(opt, k, v)
        seen["opt"] = opt
        return opt

    keep = MG.STEP_CFGS, MG.OUT, MG.ONLY
    MG.STEP_CFGS, MG.OUT, MG.ONLY, MG.build_opt = {name: cfg}, out, [], build_opt
    try:
        MG.step_fixtures()
    finally:
        (MG.STEP_CFGS, MG.OUT, MG.ONLY), MG.build_opt = keep, real_build_opt
    # the recipe's `hp` record has no slot for the options of these losses: append them (plain values)
    path = os.path.join(out, f"cutstep_{name}.pt")
    g = torch.load(path, weights_only=False)
    opt = seen["opt"]
    for k in HP:
        v = getattr(opt, "alg_cut_" + k)
        g["hp"][k] = list(v) if isinstance(v, (list, tuple)) else bool(v) if isinstance(v, bool) else int(v) if isinstance(v, int) else float(v)
    torch.save(g, path)


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    for name, (cfg, override) in CASES.items():
        step_fixture(out, name, cfg, override)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pixel_loss"))
