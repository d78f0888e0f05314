"""GPU tests of the SRC_hDCE contrastive loss: the fused kernel (`jg_nce_hdce`) against the plain-torch restatement of tests/hdce_ref.py on
identical fp32 inputs and against the fixture recorded from the unmodified reference (tests/golden/hdce/hdce_loss.pt), the torch.ops boundary,
and `CUTModel` with alg_cut_nce_loss = "SRC_hDCE": step-0 losses against the reference's step fixture, the batched form against the four-pass
form, and the default (captured-graph) step driver."""
import os
import random
import warnings

import pytest
import torch

import hdce_ref as R
import jg_oracle as O
from test_oracle_golden import ReplayRandom, cut_ids

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
HDCE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdce")

# the bounds of test_gpu_5_cutloss.py::test_patch_nce_vs_oracle (fp32 kernel against fp32 torch on the same inputs)
TOL_LOSS, TOL_GRAD = 2e-5, 2e-4
# forward-only tolerance of the losses of a CUT step at identical weights (test_gpu_5_cutloss.py::TOL_LOSS_FWD)
TOL_LOSS_FWD = {torch.float16: 6e-3, torch.bfloat16: 4e-2}

SHAPES = [(1, 5, 8), (3, 48, 32), (2, 64, 64), (2, 256, 256), (1, 320, 64), (2, 1, 16)]
T_GAMMA = [(0.07, 1.0), (0.2, 0.1)]
MODES = [(1, 1), (1, 0), (2, 1)]      # (wperiod, wcount): all weighted, none, alternating (needs two problems)
KERNEL_CASES = [(*shape, T, gamma, *mode) for shape in SHAPES for T, gamma in T_GAMMA for mode in MODES if mode != (2, 1) or shape[0] >= 2]


def _inputs(nimg, P, D):
    g = torch.Generator().manual_seed(nimg * 1000 + P)
    k = torch.nn.functional.normalize(torch.randn(nimg * P, D, generator=g))
    q = torch.nn.functional.normalize(k + 0.5 * torch.randn(nimg * P, D, generator=g))
    return q, k, torch.rand(nimg * P, generator=g)


def _restated(q, k, r, nimg, T, gamma, wperiod, wcount):
    """loss, dq, dk of the restatement in the dtype of q"""
    qr, kr = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    loss = R.hdce_loss(qr, kr, nimg, T, gamma, wperiod, wcount)
    dq, dk = torch.autograd.grad((loss * r).sum(), [qr, kr])
    return loss.detach(), dq, dk


def _bounds(ref32, ref64, gamma):
    """loss / gradient bounds; at gamma = 0.1 (weights exp(10 x)) the larger of the fixed bound and 4 x the error of the fp32 restatement
    against its own float64 run -- never anything measured on the kernel"""
    b = [TOL_LOSS, TOL_GRAD, TOL_GRAD]
    if gamma == 0.1:
        b = [max(t, 4 * R.relerr(a, c)) for t, a, c in zip(b, ref32, ref64)]
    return b


def _kernel(q, k, r, nimg, T, gamma, wperiod, wcount):
    from joligen_amd import ops

    qd, kd = q.to(D0).requires_grad_(True), k.to(D0).requires_grad_(True)
    loss = ops.patch_hdce_loss(qd, kd, nimg, T, gamma, wperiod, wcount)
    (loss * r.to(D0)).sum().backward()
    torch.cuda.synchronize()
    return loss.detach(), qd.grad, kd.grad


@pytest.mark.parametrize("nimg,P,D,T,gamma,wperiod,wcount", KERNEL_CASES)
def test_hdce_kernel_vs_restatement(nimg, P, D, T, gamma, wperiod, wcount):
    """same fp32 inputs on both sides: per-patch loss, dq, and dk through the negatives under a random row weighting; rows not a multiple of
    the 4 per block, P below / at / above one wave and above the register-resident 256, P % 64 != 0, P = 1 (no negatives)"""
    q, k, r = _inputs(nimg, P, D)
    ref = _restated(q, k, r, nimg, T, gamma, wperiod, wcount)
    ref64 = _restated(q.double(), k.double(), r.double(), nimg, T, gamma, wperiod, wcount)
    got = _kernel(q, k, r, nimg, T, gamma, wperiod, wcount)
    bounds = _bounds(ref, ref64, gamma)
    errs = [R.relerr(a, b) for a, b in zip(got, ref)]
    print("loss %.2e dq %.2e dk %.2e" % tuple(errs), "bounds", bounds)
    assert all(torch.isfinite(t).all() for t in got)
    for e, b, what in zip(errs, bounds, ("loss", "dq", "dk")):
        assert e < b, (what, e, b)
    if wperiod == 2:      # the unweighted problems of a mixed batch are the w == 1 loss, the weighted ones the weighted loss
        ones = _restated(q, k, r, nimg, T, gamma, 1, 0)
        full = _restated(q, k, r, nimg, T, gamma, 1, 1)
        rows = R.weighted_problems(nimg, wperiod, wcount).repeat_interleave(P)
        for g_, o_, f_, b in zip(got, ones, full, bounds):
            assert R.relerr(g_.cpu()[~rows], o_[~rows]) < b and R.relerr(g_.cpu()[rows], f_[rows]) < b


@pytest.mark.parametrize("gamma", [1.0, 0.1])
@pytest.mark.parametrize("nimg,P,D", SHAPES)
def test_hdce_weights_vs_restatement(nimg, P, D, gamma):
    """the optional W output: off-diagonal weights against the restatement (a forward value: the loss bound), zero diagonal"""
    from joligen_amd import ops

    _, k, _ = _inputs(nimg, P, D)
    W = ops.hdce_weights(k.to(D0), nimg, gamma).cpu()
    ref, ref64 = R.hdce_weights(k, nimg, gamma), R.hdce_weights(k.double(), nimg, gamma)
    assert W.shape == (nimg, P, P) and torch.equal(torch.diagonal(W, dim1=1, dim2=2), torch.zeros(nimg, P))
    bound = max(TOL_LOSS, 4 * R.relerr(ref, ref64)) if gamma == 0.1 else TOL_LOSS
    e = R.relerr(W, ref)
    print("weights %.2e bound %.2e" % (e, bound))
    assert e < bound, (e, bound)
    if P > 1:
        assert float(W.max()) <= 1.0 + 1e-6 and abs(float(W.amax(dim=2).min()) - 1.0) < 1e-6      # every row's largest weight is 1


def test_hdce_bit_reproducible():
    q, k, r = _inputs(3, 48, 32)
    a = _kernel(q, k, r, 3, 0.07, 0.5, 2, 1)
    b = _kernel(q, k, r, 3, 0.07, 0.5, 2, 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_hdce_unweighted_problems_never_read_the_gram_matrix():
    """C ABI directly: with wcount = 0 a Gram matrix full of NaN changes nothing against G = NULL; in a mixed batch the NaN-filled slices of the
    unweighted problems change nothing either"""
    from joligen_amd import _lib, ops

    nimg, P, D, T, gamma = 4, 48, 32, 0.07, 0.5
    q, k, r = (t.to(D0) for t in _inputs(nimg, P, D))
    S = torch.empty(nimg, P, P, device=D0)
    G = torch.empty(nimg, P, P, device=D0)
    ops.sgemm(q, k, S, P, P, D, (D, 1), (D, 1), (P, 1), nimg, (P * D, P * D, P * P))
    ops.sgemm(k, k, G, P, P, D, (D, 1), (D, 1), (P, 1), nimg, (P * D, P * D, P * P))
    L = _lib.lib()

    def run(Gm, wperiod, wcount):
        stats, loss = torch.empty(3, nimg * P, device=D0), torch.empty(nimg * P, device=D0)
        dS, gpos = torch.empty_like(S), torch.empty(nimg * P, device=D0)
        gp = None if Gm is None else Gm.data_ptr()
        _lib.check(L.jg_nce_hdce(S.data_ptr(), gp, stats.data_ptr(), loss.data_ptr(), None, None, None, None, nimg, P, T, gamma, wperiod, wcount,
                                 ops._st()), "fwd")
        _lib.check(L.jg_nce_hdce(S.data_ptr(), gp, stats.data_ptr(), None, dS.data_ptr(), gpos.data_ptr(), r.data_ptr(), None, nimg, P, T, gamma,
                                 wperiod, wcount, ops._st()), "bwd")
        torch.cuda.synchronize()
        return loss, dS, gpos

    nan = torch.full_like(G, float("nan"))
    for x, y in zip(run(None, 1, 0), run(nan, 1, 0)):
        assert torch.isfinite(y).all() and torch.equal(x, y)
    mixed = G.clone()
    mixed[1::2] = float("nan")          # wperiod 2, wcount 1: problems 1 and 3 are unweighted
    for x, y in zip(run(G, 2, 1), run(mixed, 2, 1)):
        assert torch.isfinite(y).all() and torch.equal(x, y)
    # argument checks of the entry point
    z = torch.empty(8, device=D0)
    assert L.jg_nce_hdce(S.data_ptr(), None, z.data_ptr(), z.data_ptr(), None, None, None, None, nimg, P, T, gamma, 1, 1, ops._st()) == _lib.JG_ERR_BAD_ARG
    assert L.jg_nce_hdce(S.data_ptr(), G.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, None, None, nimg, P, T, 0.0, 1, 1, ops._st()) == _lib.JG_ERR_BAD_ARG
    assert L.jg_nce_hdce(S.data_ptr(), G.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, None, None, nimg, P, T, gamma, 1, 2, ops._st()) == _lib.JG_ERR_BAD_ARG


def test_hdce_kernel_vs_reference_fixture():
    """the kernel against the unmodified reference's SRC_Loss + PatchHDCELoss directly (P == D, where the reference runs)"""
    from joligen_amd import ops

    for rec in torch.load(os.path.join(HDCE_DIR, "hdce_loss.pt"), weights_only=False)["records"]:
        nimg, T, gamma = rec["nimg"], rec["T"], rec["gamma"]
        q, k, r = rec["q"], rec["k"], rec["row_weight"]
        P = q.shape[0] // nimg
        off = ~torch.eye(P, dtype=torch.bool)[None].expand(nimg, P, P)
        W = ops.hdce_weights(k.to(D0), nimg, gamma).cpu()
        wb = max(TOL_LOSS, 4 * R.relerr(R.hdce_weights(k, nimg, gamma), R.hdce_weights(k.double(), nimg, gamma))) if gamma == 0.1 else TOL_LOSS
        assert R.relerr(W[off], rec["weights"][off]) < wb, (rec["case"], R.relerr(W[off], rec["weights"][off]), wb)
        for tag, wcount in (("weighted", 1), ("unweighted", 0)):
            ref = rec[tag]
            got = _kernel(q, k, r, nimg, T, gamma, 1, wcount)
            bounds = _bounds(_restated(q, k, r, nimg, T, gamma, 1, wcount), _restated(q.double(), k.double(), r.double(), nimg, T, gamma, 1, wcount), gamma)
            errs = [R.relerr(a, b) for a, b in zip(got, (ref["loss"], ref["dq"], ref["dk"]))]
            print(rec["case"], T, gamma, tag, "loss %.2e dq %.2e dk %.2e" % tuple(errs))
            for e, b, what in zip(errs, bounds, ("loss", "dq", "dk")):
                assert e < b, (rec["case"], T, gamma, tag, what, e, b)


def test_hdce_torch_ops_boundary():
    """schema + fake kernel + autograd registration of torch.ops.jg355.patch_hdce; the boundary computes what the ctypes path computes"""
    from joligen_amd import ops

    chk = ("test_schema", "test_faketensor", "test_autograd_registration")
    J = torch.ops.jg355
    for nimg, wperiod, wcount in ((4, 2, 1), (2, 1, 1), (2, 1, 0), (3, 4, 2)):
        q, k, r = _inputs(nimg, 24, 48)
        qd, kd = q.to(D0).requires_grad_(True), k.to(D0).requires_grad_(True)
        torch.library.opcheck(J.patch_hdce.default, (qd, kd, nimg, 0.07, 0.5, wperiod, wcount), test_utils=chk)
        a = _kernel(q, k, r, nimg, 0.07, 0.5, wperiod, wcount)
        with ops.torch_ops_boundary():
            b = _kernel(q, k, r, nimg, 0.07, 0.5, wperiod, wcount)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (nimg, wperiod, wcount)
        loss = J.patch_hdce(qd, kd, nimg, 0.07, 0.5, wperiod, wcount)[0]
        assert torch.equal(loss.detach(), a[0])


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _build_from_fixture(g, dtype):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    c, hp = g["cfg"], g["hp"]
    cfg = {"model_type": "cut", "G": {"netG": "resnet", "ngf": c["ngf"], "nblocks": c["n_blocks"]}, "D": {"netDs": ["basic"], "ndf": c["ndf"]},
           "alg": {"cut": {"nce_layers": c["nce_layers"], "num_patches": c["num_patches"], "nce_loss": c["nce_loss"], "netF_nc": hp["netF_nc"],
                           "HDCE_gamma": hp["HDCE_gamma"], "lambda_SRC": hp["lambda_SRC"]}},
           "data": {"crop_size": c["S"], "load_size": c["S"]},
           "train": {"batch_size": c["B"], "pool_size": c["pool"], "G_ema": True, "G_ema_beta": hp["ema_beta"], "G_lr": hp["lr_G"], "D_lr": hp["lr_D"]}}
    return create_model(opt_from_json(cfg, overrides={"jg_act_dtype": "fp16" if dtype == torch.float16 else "bf16", "gpu_ids": "0"}), 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_cut_model_hdce_first_step_vs_reference_golden(dtype):
    """CUTModel with alg_cut_nce_loss = "SRC_hDCE" from the configuration of the reference's step fixture: synthesised weights (seeds 0 / 1 / 3
    as in the recipe), the recorded patch ids and pool draws; the generator losses of step 0 at the forward tolerance of the existing CUT step
    test, and loss_G_SRC == 0.0 (the reference's JSD term never enters the update)"""
    g = torch.load(os.path.join(HDCE_DIR, "cutstep_hdce.pt"), weights_only=False)
    c, s = g["cfg"], g["steps"][0]
    model = _build_from_fixture(g, dtype)
    model.data_dependent_initialize({"A": s["A"], "B": s["B"]})
    assert list(model.netG_A.state_dict().keys()) == g["keysG"] and list(model.netF.state_dict().keys()) == g["keysF"]
    assert list(model.netD_B_basic.state_dict().keys()) == g["keysD"]
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.netD_B_basic.load_state_dict(O.synth_state_dict(model.netD_B_basic.state_dict(), seed=1))
    model.netF.load_state_dict(O.synth_state_dict(model.netF.state_dict(), seed=3))
    model.set_pool_rng(ReplayRandom(s["pool_draws"]))
    nl = len(c["nce_layers"].split(","))
    ids_ab, ids_idt = cut_ids(s, nl, c["num_patches"])
    model.patch_ids_injection = lambda call, shapes: [i.to(D0) for i in (ids_ab if call == 0 else ids_idt)]
    model.set_input({"A": s["A"], "B": s["B"]})
    model.optimize_parameters()
    torch.cuda.synchronize()
    losses = {k: float(v) for k, v in model.get_current_losses().items()}
    tol = TOL_LOSS_FWD[dtype]
    for name in ("G_NCE", "G_NCE_Y", "G_GAN_D_B_basic", "G_tot"):
        ref = s["losses"][name]
        print(name, losses[name], ref)
        assert abs(losses[name] - ref) <= tol * abs(ref) + 1e-4, (name, losses[name], ref)
    assert model.loss_G_SRC == 0.0 and "G_SRC" not in model.loss_names


_HDCE_CUT = {"model_type": "cut", "G": {"netG": "resnet", "ngf": 32, "nblocks": 2}, "D": {"netDs": ["projected_d", "basic"], "ndf": 32, "proj_interp": 128},
             "alg": {"cut": {"nce_layers": "0,4,8", "nce_loss": "SRC_hDCE", "num_patches": 128, "HDCE_gamma": 0.5}}, "data": {"crop_size": 64, "load_size": 64},
             "train": {"batch_size": 2, "G_ema": True, "iter_size": 1, "pool_size": 0, "G_lr": 0.0, "D_lr": 0.0}}


def _run(monkeypatch, driver, batched, calls):
    """`calls` x optimize_parameters() from seed 3 (the RNG handling of test_gpu_5_cutloss.py::_run_cut_driver) at learning rate zero; driver
    "sequential" (the reference's order) or "default" (no switch set).  Returns the losses of every call (G_NCE, G_NCE_Y, G_tot, D terms),
    Adam's first moments (a linear image of every gradient) and the driver that ran the last call."""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    for var in ("JG_EARLY_D", "JG_GRAPH_D", "JG_GRAPH_G"):
        if driver == "sequential":
            monkeypatch.setenv(var, "0")
        else:
            monkeypatch.delenv(var, raising=False)
    monkeypatch.delenv("JG_DBG_GRAPH_CANARY_FAIL", raising=False)
    monkeypatch.setenv("JG_BATCHED_NCE", "1" if batched else "0")
    gen = torch.Generator().manual_seed(14)
    data = {"A": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1, "B": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1}
    torch.manual_seed(3)
    random.seed(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = create_model(opt_from_json(_HDCE_CUT, overrides={"jg_act_dtype": "bf16", "gpu_ids": "0"}), 0)
        m.data_dependent_initialize(data)
        m.setup(m.opt)
        m.single_gpu()
        losses = []
        for _ in range(calls):
            m.set_input(data)
            m.optimize_parameters()
            losses.append([float(m.loss_G_NCE), float(m.loss_G_NCE_Y), float(m.loss_G_tot)] + [float(getattr(m, "loss_D_GAN_" + dn)) for dn in m.discriminators_names])
    torch.cuda.synchronize()
    return dict(losses=torch.tensor(losses, dtype=torch.float64), m1={n: m._net(n).arena.m.detach().double().cpu() for n in m.model_names},
                driver=m.step_driver, note=m.step_driver_note, dropped=[str(w.message) for w in rec if "jg_graph_" in str(w.message)])


def test_cut_hdce_batched_matches_the_four_pass_form(monkeypatch):
    """both contrastive terms of every layer in one launch set ([layer][term][B] problems, wperiod = 2 B, wcount = B) against the sequential
    four-pass computation (per-layer criteria, NCE term weighted, identity term not): same seed, no injection, per-image negatives; losses
    and Adam's first moments of G / F / D to the bound of test_gpu_5_cutloss.py::test_cut_batched_nce_matches_the_four_pass_form"""
    a = _run(monkeypatch, "sequential", False, 5)
    a2 = _run(monkeypatch, "sequential", False, 5)
    b = _run(monkeypatch, "sequential", True, 5)
    floor_l = float(((a["losses"] - a2["losses"]).abs() / a["losses"].abs()).max())
    floor_p = max(float((a["m1"][n] - a2["m1"][n]).norm() / a["m1"][n].norm()) for n in a["m1"])
    print("run-to-run floor of the four-pass form: losses %.2e, first moments %.2e" % (floor_l, floor_p))
    assert torch.isfinite(b["losses"]).all()
    assert float(((b["losses"] - a["losses"]).abs() / a["losses"].abs()).max()) <= 4 * floor_l + 2e-3, (b["losses"], a["losses"])
    for n in a["m1"]:
        e = float((b["m1"][n] - a["m1"][n]).norm() / a["m1"][n].norm())
        assert e <= 4 * floor_p + 2e-3, (n, e, floor_p)


def test_cut_hdce_takes_the_default_step_driver(monkeypatch):
    """with no driver switch set the step runs on the captured graphs where the other losses do (the loss is no reason to fall back), and the
    losses of its first call agree with the sequential driver's at the forward tolerance"""
    import joligen_amd

    seq = _run(monkeypatch, "sequential", True, 1)
    r = _run(monkeypatch, "default", True, 7)
    assert seq["driver"] == "sequential"
    assert r["driver"] != "sequential", (r["driver"], r["note"])
    assert "hDCE" not in r["note"] and "nce_loss" not in r["note"], r["note"]
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert r["driver"] == "graph+graphG" and not r["dropped"], (r["driver"], r["note"], r["dropped"])
    assert torch.isfinite(r["losses"]).all()
    l0, s0 = r["losses"][0], seq["losses"][0]
    assert float(((l0 - s0).abs() / s0.abs()).max()) <= TOL_LOSS_FWD[torch.bfloat16], (l0, s0)
