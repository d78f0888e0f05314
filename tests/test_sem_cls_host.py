"""Host-side tests of train_semantic_cls (no GPU): the option checks, the loss-name order against the reference's step fixture, the
mnist2USPS example through opt_from_json, and the float restatement of tests/sem_cls_ref.py against the reference's own classifier
(tests/golden/sem_cls/cls_fn.pt)."""
import os
from types import SimpleNamespace

import pytest
import torch

import sem_cls_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "sem_cls")
EXAMPLE = os.path.join(HERE, "golden", "examples", "example_gan_mnist2USPS.json")
TOL_LOSS = 1e-5      # the project's bound for the same sums taken in another order (fp32)


def _opt(**kw):
    return SimpleNamespace(**dict(dict(train_semantic_cls=True, data_crop_size=32, model_input_nc=3, model_output_nc=3, cls_semantic_nclasses=10), **kw))


def test_check_sem_cls_options_accepts_and_raises():
    from joligen_amd.models.cut_model import check_sem_cls_options
    from joligen_amd.options import SEM_CLS_DEFAULTS

    off = SimpleNamespace()
    assert check_sem_cls_options(off) == "off"
    assert {k: getattr(off, k) for k in SEM_CLS_DEFAULTS} == SEM_CLS_DEFAULTS
    assert (off.cls_nf, off.f_s_semantic_threshold, off.train_sem_cls_lambda, off.train_sem_lr_f_s, off.train_sem_cls_template) == (64, 1.0, 1.0, 2e-4, "basic")
    assert not any(getattr(off, k) for k in ("train_sem_cls_B", "train_sem_cls_pretrained", "train_cls_regression", "train_cls_l1_regression",
                                             "train_sem_idt", "train_sem_net_output", "train_sem_use_label_B"))
    # off: nothing else is looked at
    assert check_sem_cls_options(SimpleNamespace(train_semantic_cls=False, data_crop_size=100, train_sem_idt=True, train_sem_cls_template="vgg")) == "off"
    assert check_sem_cls_options(_opt()) == "CE"
    assert check_sem_cls_options(_opt(cls_semantic_nclasses=1, train_cls_regression=True)) == "MSE"
    assert check_sem_cls_options(_opt(cls_semantic_nclasses=1, train_cls_regression=True, train_cls_l1_regression=True)) == "L1"
    assert check_sem_cls_options(_opt(train_cls_l1_regression=True)) == "CE"          # read only in regression mode, as in the reference
    for size in (8, 16, 128, 1024):
        assert check_sem_cls_options(_opt(data_crop_size=size)) == "CE"
    # accepted and ignored: they do not reach the training step of the reference
    assert check_sem_cls_options(_opt(train_sem_use_label_B=True, cls_class_weights=[1.0, 2.0], cls_all_classes_as_one=True, cls_dropout=True,
                                      train_sem_cls_B=True, train_sem_net_output=True, cls_semantic_threshold=0.1)) == "CE"
    for tpl in ("vgg", "resnet18", "efficientnet_b0"):
        with pytest.raises(NotImplementedError, match="train_sem_cls_template"):
            check_sem_cls_options(_opt(train_sem_cls_template=tpl))
    with pytest.raises(NotImplementedError, match="reference cannot run it either"):
        check_sem_cls_options(_opt(train_sem_idt=True))
    for size in (4, 12, 100, 286, 0):
        with pytest.raises(ValueError, match="power of two"):
            check_sem_cls_options(_opt(data_crop_size=size))
    with pytest.raises(ValueError, match="model_input_nc"):
        check_sem_cls_options(_opt(model_input_nc=1))
    with pytest.raises(ValueError, match="train_cls_regression"):
        check_sem_cls_options(_opt(train_cls_regression=True))
    for n in (0, -3):
        with pytest.raises(ValueError, match="cls_semantic_nclasses"):
            check_sem_cls_options(_opt(cls_semantic_nclasses=n))


def test_loss_names_follow_the_reference():
    from joligen_amd.models.cut_model import cut_all_loss_names, cut_loss_names

    for name in ("closed", "open", "open_B"):
        g = torch.load(os.path.join(DIR, f"cutstep_cls_{name}.pt"), weights_only=False)
        opt = SimpleNamespace(train_semantic_cls=True, alg_cut_nce_idt=True)
        assert cut_all_loss_names(opt, ["D_B_basic"]) == g["loss_names"]
        assert g["loss_names"][-2:] == ["G_sem_cls_AB", "CLS"] and g["loss_names"].count("G_sem_cls_AB") == 1
    assert cut_loss_names(opt, ["D_B_basic"]) == ["G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic", "G_sem_cls_AB"]
    # option off: what it was
    off = SimpleNamespace(alg_cut_nce_idt=True)
    assert cut_loss_names(off, ["D_B_basic"]) == ["G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic"]
    assert cut_all_loss_names(off, ["D_B_basic"]) == ["G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic", "D_tot", "D_GAN_D_B_basic"]
    old = torch.load(os.path.join(HERE, "golden", "cutstep_patchnce.pt"), weights_only=False)
    assert cut_all_loss_names(off, ["D_B_basic"]) == old["loss_names"]


def test_example_mnist2usps_parses():
    from joligen_amd.models.cut_model import check_d_aug_options, check_sem_cls_options
    from joligen_amd.options import opt_from_json

    ex = opt_from_json(EXAMPLE, {"gpu_ids": "0"})
    assert ex.model_type == "cut" and ex.G_netG == "mobile_resnet_attn" and ex.train_semantic_cls is True
    assert ex.cls_semantic_nclasses == 10 and ex.dataaug_D_noise == 0.001 and ex.train_iter_size == 2 and ex.data_crop_size == 128
    assert check_sem_cls_options(ex) == "CE" and check_d_aug_options(ex) == (0.001, False)
    assert ex.train_sem_lr_f_s == 0.0002 and ex.cls_nf == 64 and ex.train_sem_cls_template == "basic"
    # a config (or an override) that names its generator keeps it; the other model types keep their default
    assert opt_from_json({"model_type": "cut", "G": {"netG": "resnet"}}, {"gpu_ids": "0"}).G_netG == "resnet"
    assert opt_from_json({"model_type": "cut"}, {"gpu_ids": "0", "G_netG": "segformer_attn_conv"}).G_netG == "segformer_attn_conv"
    assert opt_from_json({"model_type": "cut"}, {"gpu_ids": "0"}).G_netG == "mobile_resnet_attn"
    assert opt_from_json({}, {"gpu_ids": "0"}).G_netG == "unet_mha" and opt_from_json({"model_type": "cm"}, {"gpu_ids": "0"}).G_netG == "unet_mha"


def test_cm_gan_still_refuses_the_flag():
    from joligen_amd.models.cm_gan_model import check_cm_gan_options

    with pytest.raises(NotImplementedError, match="train_semantic_cls"):
        check_cm_gan_options(SimpleNamespace(train_semantic_cls=True))


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_restatement_reproduces_the_reference_classifier():
    """cls_fn.pt in fp32: logits, loss, input and parameter gradients, the running statistics after one and two train-mode calls and the
    eval-mode logits at TOL_LOSS; num_batches_tracked and the argmaxes exactly.  (The running statistics are floating-point sums taken in another
    order than the reference's BatchNorm kernel takes them: TOL_LOSS is the bound for exactly that; the integer buffer is exact.)"""
    cases = torch.load(os.path.join(DIR, "cls_fn.pt"), weights_only=False)["cases"]
    assert [(c["crop"], c["B"], c["nclasses"]) for c in cases] == [(16, 3, 10), (32, 2, 10), (16, 3, 1)]
    for c in cases:
        keys = list(c["state_dict"])
        nbn = sum(k.endswith("running_mean") for k in keys)
        assert nbn == {16: 1, 32: 2}[c["crop"]] and keys[-4:] == ["after_linear.0.weight", "after_linear.0.bias", "after_linear.1.weight", "after_linear.1.bias"]
        sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in c["state_dict"].items()}
        x = c["x"].clone().requires_grad_(True)
        logits, b1 = R.classifier_forward(sd, x, training=True)
        assert _rel(logits, c["logits"]) <= TOL_LOSS
        for k, v in c["buffers1"].items():
            key = "before_linear." + k.split("before_linear.")[-1]
            if k.endswith("num_batches_tracked"):
                assert int(b1[key]) == int(v) == 1
            else:
                assert _rel(b1[key], v) <= TOL_LOSS, k
        params = [k for k in sd if sd[k].requires_grad]
        for lname, rec in c["losses"].items():
            mode = {"CE": R.CE, "MSE": R.MSE, "L1": R.L1}[lname]
            loss, dlogits, arg, gate = R.cls_loss(logits, c["target"], mode)
            assert gate and abs(float(loss) - float(rec["loss"])) <= TOL_LOSS * abs(float(rec["loss"]))
            if mode == R.CE:
                assert torch.equal(arg, c["argmax"])
            grads = torch.autograd.grad(logits, [x] + [sd[k] for k in params], grad_outputs=dlogits.to(logits.dtype), retain_graph=True)
            assert _rel(grads[0], rec["dx"]) <= TOL_LOSS
            if c["crop"] == 16:      # even size, unpadded stride 2: the last row and column belong to no window
                assert bool((rec["dx"][:, :, -1, :] == 0).all()) and bool((rec["dx"][:, :, :, -1] == 0).all())
                assert bool((grads[0][:, :, -1, :] == 0).all()) and bool((grads[0][:, :, :, -1] == 0).all())
            for k, gr in zip(params, grads[1:]):
                if k in R.bias_before_batchnorm(sd):
                    # BatchNorm on batch statistics removes the channel mean: this gradient is exactly zero in real arithmetic and rounding
                    # noise on both sides -- bounded against the scale of the same convolution's weight gradient, not against itself
                    scale = float(rec["dparams"][k.replace(".bias", ".weight")].abs().max())
                    assert float(gr.abs().max()) <= TOL_LOSS * scale and float(rec["dparams"][k].abs().max()) <= TOL_LOSS * scale, (lname, k)
                    continue
                assert _rel(gr, rec["dparams"][k]) <= TOL_LOSS, (lname, k)
        sd2 = dict(sd, **b1)
        with torch.no_grad():
            _, b2 = R.classifier_forward(sd2, c["x"], training=True)
            for k, v in c["buffers2"].items():
                if k.endswith("num_batches_tracked"):
                    assert int(b2[k]) == int(v) == 2
                else:
                    assert _rel(b2[k], v) <= TOL_LOSS, k
            ev, b3 = R.classifier_forward(dict(sd, **b2), c["x"], training=False)
            assert _rel(ev, c["logits_eval"]) <= TOL_LOSS
            assert all(torch.equal(b3[k], b2[k]) for k in b2)


def test_restatement_gate_and_bad_labels():
    x = torch.tensor([[0.5, 2.0, 2.0, -1.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    t = torch.tensor([1, 4, 0])
    loss, d, arg, gate = R.cls_loss(x, t, R.CE, lam=0.5)
    assert gate and torch.isnan(loss) and arg.tolist() == [1, 0, 0] and bool((d[1] == 0).all()) and bool(torch.isfinite(d).all())
    want = torch.nn.functional.cross_entropy(x[[0, 2]].double(), t[[0, 2]], reduction="sum") * 0.5 / 3
    ok, d_ok, _, _ = R.cls_loss(x[[0, 2]], t[[0, 2]], R.CE, lam=0.5 * 2 / 3)
    assert abs(float(ok) - float(want)) <= 1e-12 and torch.allclose(d_ok, d[[0, 2]], atol=1e-15)
    for prev, open_ in ((0.5, True), (1.0, True), (1.5, False), (float("inf"), False), (float("nan"), True)):
        loss, d, _, gate = R.cls_loss(x, torch.tensor([1, 2, 0]), R.CE, prev=prev, threshold=1.0)
        assert gate is open_ and (float(loss) > 0) is open_ and bool((d != 0).any()) is open_
    with pytest.raises(ValueError):
        R.cls_loss(x, torch.zeros(3), R.MSE)
