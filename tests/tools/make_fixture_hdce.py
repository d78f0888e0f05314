"""Generate tests/golden/hdce/hdce_loss.pt and cutstep_hdce.pt from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * hdce_loss.pt    : SRC_Loss weights (models/modules/NCE/SRC.py, only_weight=True), PatchHDCELoss per-patch loss with those weights and with
                      weight=None (NCE/hDCE.py), and dq / dk of both under a seeded random row weighting, on seeded L2-normalised q, k;
  * cutstep_hdce.pt : N x CUTModel.optimize_parameters() with alg_cut_nce_loss = "SRC_hDCE" -- the `patchnce` step configuration of
                      oracle/make_golden_cutstep.py at B = 2 and alg_cut_netF_nc = num_patches = 32 (SRC_Loss builds its diagonal mask as
                      eye(feature width): the reference runs only where the patch count equals it), recorded by that recipe's own loop.
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_hdce.py [output directory]"""
import os
import tempfile
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
_argv, sys.argv = sys.argv, sys.argv[:1]          # make_golden_cutstep reads its own selection from sys.argv at import
import make_golden_cutstep as MG  # noqa: E402  (installs ref_shim)

sys.argv = _argv
import torch  # noqa: E402

LOSS_CASES = {      # name: (B, P, D, all negatives from the minibatch); B * P == D there, P == D otherwise
    "per_image": (2, 32, 32, False),
    "all_negatives": (2, 16, 32, True),
}
T_GAMMA = [(0.07, 1.0), (0.2, 0.1)]
STEP_CFG = dict(MG.STEP_CFGS["patchnce"], B=2, iters=3, nce_loss="SRC_hDCE")
NETF_NC = 32


def loss_fixture(out):
    from models.modules.NCE.SRC import SRC_Loss
    from models.modules.NCE.hDCE import PatchHDCELoss

    recs = []
    for name, (B, P, D, allneg) in LOSS_CASES.items():
        g = torch.Generator().manual_seed(21)
        k = torch.nn.functional.normalize(torch.randn(B * P, D, generator=g))
        q = torch.nn.functional.normalize(k + 0.5 * torch.randn(B * P, D, generator=g))
        r = torch.rand(B * P, generator=g)
        for T, gamma in T_GAMMA:
            opt = SimpleNamespace(alg_cut_nce_includes_all_negatives_from_minibatch=allneg, alg_cut_nce_T=T, alg_cut_num_patches=P,
                                  alg_cut_HDCE_gamma=gamma, alg_cut_HDCE_gamma_min=gamma, train_batch_size=B)
            _, w = SRC_Loss(opt)(q, k, only_weight=True)
            rec = dict(case=name, B=B, P=P, D=D, all_negatives=allneg, nimg=1 if allneg else B, T=T, gamma=gamma, q=q.clone(), k=k.clone(),
                       row_weight=r.clone(), weights=w.detach().clone())
            for tag, weight in (("weighted", w), ("unweighted", None)):
                qr, kr = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
                loss = PatchHDCELoss(opt)(feat_q=qr, feat_k=kr, current_batch=B, weight=None if weight is None else weight.clone())
                dq, dk = torch.autograd.grad((loss * r).sum(), [qr, kr])
                rec[tag] = dict(loss=loss.detach().clone(), dq=dq.clone(), dk=dk.clone())
            recs.append(rec)
            print("hdce_loss", name, T, gamma, float(rec["weighted"]["loss"].mean()), float(rec["unweighted"]["loss"].mean()))
    torch.save(dict(records=recs), os.path.join(out, "hdce_loss.pt"))


def step_fixture(out):
    real_build_opt = MG.build_opt
    seen = {}

    def build_opt(c):
        opt = real_build_opt(c)
        opt.alg_cut_netF_nc = NETF_NC
        seen["opt"] = opt
        return opt

    keep = MG.STEP_CFGS, MG.OUT, MG.ONLY
    MG.STEP_CFGS, MG.OUT, MG.ONLY, MG.build_opt = {"hdce": STEP_CFG}, out, [], build_opt
    try:
        MG.step_fixtures()
    finally:
        (MG.STEP_CFGS, MG.OUT, MG.ONLY), MG.build_opt = keep, real_build_opt
    # the recipe's `hp` record has no slot for the two options this loss adds: append them (plain values)
    path = os.path.join(out, "cutstep_hdce.pt")
    g = torch.load(path, weights_only=False)
    opt = seen["opt"]
    g["hp"].update(HDCE_gamma=float(opt.alg_cut_HDCE_gamma), netF_nc=int(opt.alg_cut_netF_nc), lambda_SRC=float(opt.alg_cut_lambda_SRC))
    torch.save(g, path)


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    loss_fixture(out)
    step_fixture(out)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "hdce"))
