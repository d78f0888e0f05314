"""Generate tests/golden/sem_cls/ from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * cls_fn.pt : models/modules/classifiers.Classifier (ndf = 8) on its own, with synthesised weights (oracle/jg_oracle.synth_state_dict, seed 4):
    10 classes at crop 16 / B = 3 and crop 32 / B = 2 (CrossEntropyLoss), 1 class at crop 16 / B = 3 (MSELoss and L1Loss).  Per case: the state
    dict, the input, the train-mode logits of the first call, the buffers after one and after two calls, the loss against recorded targets, its
    gradient with respect to the input and to every parameter, and the eval-mode logits (with the buffers after two calls).
  * cutstep_cls_{closed,open,open_B}.pt : 3 x CUTModel.optimize_parameters() with train_semantic_cls (cls_nf = 8, 10 classes) -- the
    `patchnce` step configuration of oracle/make_golden_cutstep.py at B = 2, pool = 2 (its crop, 32, is a power of two), recorded by that
    recipe's own loop with labels added to its batches.  `closed`: as constructed (no loss_CLS yet, then a cross entropy near ln 10 against the
    threshold 1.0); `open`: loss_CLS preset to 0.5 before step 0, the state of a resumed run; `open_B`: the same with train_sem_cls_B.
    Beside what the recipe records every step carries under "cls": the labels, the gate and the loss_CLS it read, the classifier's buffers after
    the step, gt_pred_cls_A / pfB and the logits they were taken from.
The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.  Asserted here: |loss_CLS - threshold| >= 0.05 at
every gate read (a 16-bit rounding cannot flip a gate in a test that replays the fixture), and at least half of the recorded rows have a
top-two logit gap above twice 4e-2 of the largest logit magnitude of their batch (the forward tolerance in bf16 lets each of two logits move by
that much): the rows whose argmax a replaying test can compare.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_sem_cls.py [output directory]"""
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
_argv, sys.argv = sys.argv, sys.argv[:1]          # make_golden_cutstep reads its own selection from sys.argv at import
import make_golden_cutstep as MG  # noqa: E402  (installs ref_shim)

sys.argv = _argv
import torch  # noqa: E402

import jg_oracle as O  # noqa: E402
import ref_shim  # noqa: E402

BASE = dict(MG.STEP_CFGS["patchnce"], B=2, pool=2, iters=3)
SEM = dict(train_semantic_cls=True, cls_nf=8, cls_semantic_nclasses=10)
CASES = {"closed": dict(SEM), "open": dict(SEM), "open_B": dict(SEM, train_sem_cls_B=True)}
PRESET = {"open": 0.5, "open_B": 0.5}
HP = ("train_semantic_cls", "cls_nf", "cls_semantic_nclasses", "f_s_semantic_threshold", "train_sem_cls_lambda", "train_sem_lr_f_s",
      "train_sem_cls_B", "train_cls_regression", "train_cls_l1_regression")
CLS_SEED = 4
GATE_MARGIN = 0.05
GAP = 4e-2
NCLASSES = 10


def labels(B, seed, dom):
    g = torch.Generator().manual_seed(7000 + seed * 2 + (dom == "B"))
    return torch.randint(0, NCLASSES, (B,), generator=g)


def _plain(v):
    return bool(v) if isinstance(v, bool) else int(v) if isinstance(v, int) else float(v)


def cls_fn_fixture(out):
    from models.modules.classifiers import Classifier

    cases = []
    for crop, B, n in ((16, 3, 10), (32, 2, 10), (16, 3, 1)):
        g = torch.Generator().manual_seed(40 + crop + n)
        net = Classifier(3, 8, n, crop)
        sd = O.synth_state_dict(net.state_dict(), seed=CLS_SEED)
        net.load_state_dict(sd)
        net.train()
        x = (torch.rand(B, 3, crop, crop, generator=g) * 2 - 1).requires_grad_(True)
        logits = net(x)
        bufs1 = {k: v.clone() for k, v in net.named_buffers()}
        params = dict(net.named_parameters())
        rec = dict(crop=crop, B=B, nclasses=n, ndf=8, state_dict={k: v.clone() for k, v in sd.items()}, x=x.detach().clone(), logits=logits.detach().clone(),
                   buffers1=bufs1, losses={})
        if n > 1:
            target = torch.randint(0, n, (B,), generator=g)
            crits = {"CE": torch.nn.CrossEntropyLoss()}
            rec["argmax"] = logits.max(1)[1].clone()
        else:
            target = torch.randn(B, generator=g)
            crits = {"MSE": torch.nn.MSELoss(), "L1": torch.nn.L1Loss()}
        rec["target"] = target.clone()
        for name, crit in crits.items():
            loss = crit(logits if n > 1 else logits.squeeze(1), target)
            grads = torch.autograd.grad(loss, [x] + list(params.values()), retain_graph=True)
            rec["losses"][name] = dict(loss=loss.detach().clone(), dx=grads[0].clone(), dparams={k: gr.clone() for k, gr in zip(params, grads[1:])})
        with torch.no_grad():
            net(x)
            rec["buffers2"] = {k: v.clone() for k, v in net.named_buffers()}
            net.eval()
            rec["logits_eval"] = net(x).clone()
        cases.append(rec)
        print("cls_fn", crop, B, n, {k: float(v["loss"]) for k, v in rec["losses"].items()}, [k for k in sd if "running" in k or "tracked" in k])
    torch.save(dict(cases=cases, seed=CLS_SEED), os.path.join(out, "cls_fn.pt"))


def step_fixture(out, name, override):
    import models

    real_build_opt, real_create, real_batch = MG.build_opt, models.create_model, MG.batch
    seen, steps = {}, []

    def build_opt(c):
        opt = real_build_opt(c)
        for k, v in override.items():
            setattr(opt, k, v)
        seen["opt"] = opt
        return opt

    def batch(B, S, seed, *a, **k):
        d = real_batch(B, S, seed, *a, **k)
        d["A_label_cls"], d["B_label_cls"] = labels(B, seed, "A"), labels(B, seed, "B")
        return d

    def create_model(opt, rank):
        model = real_create(opt, rank)
        seen["model"] = model
        ddi, step, set_input = model.data_dependent_initialize, model.optimize_parameters, model.set_input
        cur = {}

        def data_dependent_initialize(data):
            ddi(data)
            model.netCLS.load_state_dict(O.synth_state_dict(model.netCLS.state_dict(), seed=CLS_SEED))
            seen["sdCLS"] = {k: v.clone() for k, v in model.netCLS.state_dict().items()}
            if name in PRESET:
                model.loss_CLS = torch.tensor(PRESET[name])

        def set_input_rec(data):
            cur["data"] = data
            set_input(data)

        def optimize_parameters():
            thr = opt.f_s_semantic_threshold
            before = float(model.loss_CLS) if hasattr(model, "loss_CLS") else None
            assert before is None or abs(before - thr) >= GATE_MARGIN, (name, before)
            step()
            d = cur["data"]
            steps.append(dict(label_A=d["A_label_cls"].clone(), label_B=d["B_label_cls"].clone(), gate=bool(before is not None and not before > thr),
                              loss_CLS_before=before, buffers={k: v.clone() for k, v in model.netCLS.named_buffers()},
                              gt_pred_cls_A=model.gt_pred_cls_A.clone(), pfB=model.pfB.clone(), pred_cls_real_A=model.pred_cls_real_A.detach().clone(),
                              pred_cls_fake_B=model.pred_cls_fake_B.detach().clone()))

        model.data_dependent_initialize, model.optimize_parameters, model.set_input = data_dependent_initialize, optimize_parameters, set_input_rec
        return model

    keep = MG.STEP_CFGS, MG.OUT, MG.ONLY
    MG.STEP_CFGS, MG.OUT, MG.ONLY, MG.build_opt, MG.batch = {"cls_" + name: BASE}, out, [], build_opt, batch
    models.create_model = create_model
    try:
        MG.step_fixtures()
    finally:
        (MG.STEP_CFGS, MG.OUT, MG.ONLY), MG.build_opt, MG.batch = keep, real_build_opt, real_batch
        models.create_model = real_create
    path = os.path.join(out, f"cutstep_cls_{name}.pt")
    g = torch.load(path, weights_only=False)
    assert len(steps) == len(g["steps"]) == BASE["iters"]
    rows = wide = 0
    for s, rec in zip(g["steps"], steps):
        s["cls"] = rec
        for lg in (rec["pred_cls_real_A"], rec["pred_cls_fake_B"]):
            top = lg.topk(2, dim=1).values
            rows += lg.shape[0]
            wide += int(((top[:, 0] - top[:, 1]) > 2 * GAP * float(lg.abs().max())).sum())
    assert 2 * wide >= rows, (name, wide, rows)
    for k in HP:
        g["hp"][k] = _plain(getattr(seen["opt"], k))
    g["hp"]["preset_loss_CLS"] = PRESET.get(name)
    g["keysCLS"] = list(seen["sdCLS"].keys())
    g["shapesCLS"] = {k: tuple(v.shape) for k, v in seen["sdCLS"].items()}
    g["cls_seed"] = CLS_SEED
    torch.save(g, path)
    print(name, "gates:", [r["gate"] for r in steps], "loss_CLS read:", [r["loss_CLS_before"] for r in steps], "G_sem_cls_AB:",
          [s["losses"].get("G_sem_cls_AB") for s in g["steps"]], "CLS:", [s["losses"].get("CLS") for s in g["steps"]], "wide rows", wide, "of", rows)


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    ex = os.path.join(os.path.dirname(out), "examples")
    os.makedirs(ex, exist_ok=True)
    shutil.copyfile(os.path.join(ref_shim.REFERENCE_ROOT, "examples", "example_gan_mnist2USPS.json"), os.path.join(ex, "example_gan_mnist2USPS.json"))
    os.chdir(tempfile.gettempdir())
    cls_fn_fixture(out)
    for name, override in CASES.items():
        step_fixture(out, name, override)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sem_cls"))
