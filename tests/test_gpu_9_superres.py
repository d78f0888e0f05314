"""GPU: the palette model's super_resolution task (reference models/palette_model.py:120-130, 364-366, 546-548, 838-844).

The conditioning image is the ground truth resized to S / scale and back with torchvision's anti-aliased bilinear Resize; here that is
one kernel (jg_lowres_roundtrip_f32).  Checked: the kernel against torch's CPU `F.interpolate` pair, the torch.ops entry, the model
plumbing, bit-equality of the whole step and of the samplers with the pix2pix path on the same conditioning image, the CPU oracle's
loss, the reference's shipped example through the train loop, and the torch.ops boundary."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import jg_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DF2K = os.path.join(ROOT, "tests", "golden", "examples", "example_ddpm_df2kost.json")
TINY = dict(ngf=32, mults=[1, 2], res_blocks=[1, 1], attn_res=[16], efficient=True, S=32, B=2)      # the smoke() configuration
TOL_LOSS_FWD = {"fp16": 5e-3, "bf16": 3e-2}      # the palette step's loss against the oracle (tests/test_gpu_1_model.py)

CASES = [(2, 3, 32, 32, 2), (2, 3, 64, 64, 4), (1, 3, 40, 40, 1.7), (1, 3, 96, 96, 2.5), (2, 3, 32, 32, 8), (1, 1, 32, 32, 1),
         (1, 2, 48, 80, 2), (2, 3, 256, 256, 4)]
_REF = {}


def cpu_roundtrip(x, scale):
    """the reference's transform_hr(transform_lr(x)) on the CPU in fp32"""
    H, W = x.shape[-2:]
    lo = F.interpolate(x, size=(int(H / scale), int(W / scale)), mode="bilinear", antialias=True, align_corners=False)
    return F.interpolate(lo, size=(H, W), mode="bilinear", antialias=True, align_corners=False)


def case_data(case):
    """(input, CPU round trip) of a case: computed once, shared, never modified"""
    if case not in _REF:
        B, C, H, W, scale = case
        x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(H * 131 + W)) * 2 - 1
        _REF[case] = (x, cpu_roundtrip(x, scale))
    return _REF[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_lowres_roundtrip_kernel_vs_cpu_interpolate(case):
    """max |delta| <= 1e-5 against the CPU F.interpolate pair: four passes of at most 17 fp32 taps on values in [-1, 1] give about 4e-6
    at most, the bound doubles that.  Two calls are bit-identical, and the floats around the output are not written."""
    from joligen_amd import ops

    B, C, H, W, scale = case
    x, ref = case_data(case)
    xd = x.cuda()
    n, pad = x.numel(), 4096                      # a multiple of 4 floats: the output keeps the 16-byte alignment of its vector stores
    buf = torch.full((n + 2 * pad,), 777.0, device="cuda")
    out = buf[pad:pad + n].view(B, C, H, W)
    y = ops.lowres_roundtrip(xd, scale, out=out)
    y2 = ops.lowres_roundtrip(xd, scale)
    torch.cuda.synchronize()
    err = float((y.cpu() - ref).abs().max())
    print(f"lowres_roundtrip {case}: max |delta| vs CPU F.interpolate = {err:.3e}")
    assert err <= 1e-5, (case, err)
    assert torch.equal(y, y2)
    assert bool((buf[:pad] == 777.0).all()) and bool((buf[pad + n:] == 777.0).all())
    assert torch.equal(xd.cpu(), x)
    if scale == 1:
        assert float((y.cpu() - x).abs().max()) <= 1e-6


def test_lowres_roundtrip_unaligned_and_odd_width():
    """the scalar path: a width that is no multiple of 4, and an output that starts off a 16-byte boundary"""
    from joligen_amd import ops

    for (B, C, H, W, scale), shift in (((1, 2, 30, 37, 2.2), 0), ((1, 2, 32, 32, 2), 1)):
        x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1
        buf = torch.full((x.numel() + 64,), 777.0, device="cuda")
        out = buf[32 + shift:32 + shift + x.numel()].view(B, C, H, W)
        y = ops.lowres_roundtrip(x.cuda(), scale, out=out)
        err = float((y.cpu() - cpu_roundtrip(x, scale)).abs().max())
        assert err <= 1e-5, (W, shift, err)
        assert bool((buf[:32 + shift] == 777.0).all()) and bool((buf[32 + shift + x.numel():] == 777.0).all())


def test_lowres_roundtrip_argument_checks():
    from joligen_amd import ops

    x = torch.zeros(1, 1, 32, 32, device="cuda")
    with pytest.raises(ValueError):
        ops.lowres_roundtrip(x, 0.5)
    with pytest.raises(ValueError):
        ops.lowres_roundtrip(x, 64)
    with pytest.raises(TypeError):
        ops.lowres_roundtrip(x.half(), 2)
    with pytest.raises(RuntimeError):
        ops.lowres_roundtrip(x.cpu(), 2)


def test_lowres_roundtrip_torch_op_opcheck():
    from joligen_amd import ops  # noqa: F401  (registers torch.ops.jg355.*)

    x = torch.rand(2, 3, 40, 40, device="cuda") * 2 - 1
    torch.library.opcheck(torch.ops.jg355.lowres_roundtrip, (x, 23, 23), test_utils=("test_schema", "test_faketensor"))
    y = torch.ops.jg355.lowres_roundtrip(x, 23, 23)
    assert torch.equal(y, ops.lowres_roundtrip(x, (23, 23)))
    with ops.torch_ops_boundary():
        assert torch.equal(ops.lowres_roundtrip(x, (23, 23)), y)


def make_model(dtype_name, c=TINY, **extra):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"], G_unet_mha_attn_res=c["attn_res"],
              G_unet_mha_vit_efficient=c["efficient"], data_crop_size=c["S"], train_batch_size=c["B"], gpu_ids="0", train_optim="adamw",
              train_G_ema=True, jg_act_dtype=dtype_name, checkpoints_dir="/tmp/jg_amd_ckpt/", name="t_sr")
    ov.update(extra)
    opt = opt_from_json({}, ov)
    model = create_model(opt, 0)
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.setup(opt)
    model.single_gpu()
    return model


def tiny_image():
    return torch.rand(TINY["B"], 3, TINY["S"], TINY["S"], generator=torch.Generator().manual_seed(1)) * 2 - 1


def test_super_resolution_model_plumbing():
    model = make_model("fp16", alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=2)
    assert model.opt.alg_diffusion_cond_image_creation == "low_res" and model.data_crop_size_low_res == 16      # palette_model.py:120-124
    x = tiny_image()
    model.set_input({"A": x})
    assert torch.equal(model.gt_image.cpu(), x) and model.mask is None and model.cls is None
    err = float((model.cond_image.cpu() - cpu_roundtrip(x, 2)).abs().max())
    assert err <= 1e-5, err
    assert model.real_A is model.cond_image and model.real_B is model.gt_image and model.batch_size == TINY["B"]
    assert model.gen_visual_names == ["gt_image_", "cond_image_", "output_"]
    assert model.visual_names[0] == ["gt_image_0", "cond_image_0", "output_0"]
    with pytest.raises(ValueError):
        make_model("fp16", alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=0.5)
    with pytest.raises(ValueError):
        make_model("fp16", alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=64)
    with pytest.raises(NotImplementedError):       # refused at construction: 4096 / 64 needs 129 taps
        make_model("fp16", alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=64, data_crop_size=4096)


def test_super_resolution_step_and_samplers_equal_pix2pix_on_the_same_conditioning():
    """super_resolution on {"A": x} and pix2pix on {"A": cond_image, "B": x} are the same computation after set_input: with the same
    weights and draws, in deterministic mode, two optimizer steps leave torch.equal losses and parameters, and both samplers return
    torch.equal images"""
    from joligen_amd import _lib

    x = tiny_image()
    S, B, T = TINY["S"], TINY["B"], 8
    draws = [O.draw_step_randomness(torch.Generator().manual_seed(20 + i), x, 2000) for i in range(2)]
    gn = torch.Generator().manual_seed(7)
    noises = [torch.randn(B, 3, S, S, generator=gn) for _ in range(T)]
    prev = _lib.set_tuning("JG_DETERMINISTIC", 1)
    try:
        sr = make_model("fp16", alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=2, G_diff_n_timestep_test=T)
        px = make_model("fp16", alg_diffusion_task="pix2pix", G_diff_n_timestep_test=T)
        for i in range(2):
            for m in (sr, px):
                m.rng_injection = lambda b, i=i: draws[i]
            sr.set_input({"A": x})
            px.set_input({"A": sr.cond_image, "B": x})
            sr.optimize_parameters()
            px.optimize_parameters()
            torch.cuda.synchronize()
            assert torch.equal(sr.loss_G_tot, px.loss_G_tot), (i, float(sr.loss_G_tot), float(px.loss_G_tot))
            assert torch.equal(sr.netG_A.arena.p, px.netG_A.arena.p), i
        assert math.isfinite(float(sr.loss_G_tot)) and float(sr.loss_G_tot) > 0
        for method in ("ddpm", "ddim"):
            outs = []
            for m in (sr, px):
                m.sample_num, m.sampling_noises = 2, noises
                m._net("G_A").set_new_sampling_method(method)
                torch.manual_seed(3)                 # the samplers start from a device draw
                m.inference(2)
                outs.append(m.output.clone())
            torch.cuda.synchronize()
            assert tuple(outs[0].shape) == (2, 3, S, S) and bool(torch.isfinite(outs[0]).all())
            assert torch.equal(outs[0], outs[1]), method
        vis = sr.get_current_visuals(2)
        assert list(vis[1].keys()) == ["gt_image_1", "cond_image_1", "output_1"]
    finally:
        _lib.set_tuning("JG_DETERMINISTIC", prev)


@pytest.mark.parametrize("dtype_name", ["fp16", "bf16"])
def test_super_resolution_step_vs_oracle(dtype_name):
    """one teacher-forced step: the oracle trainer is given the CPU round trip as y_cond (as smoke() gives it the inpainting pair)"""
    model = make_model(dtype_name, alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=2)
    x = tiny_image()
    t, u, noise = O.draw_step_randomness(torch.Generator().manual_seed(2), x, 2000)
    cfg = O.UNetCfg(in_channel=6, inner_channel=TINY["ngf"], res_blocks=TINY["res_blocks"], attn_res=TINY["attn_res"],
                    channel_mults=TINY["mults"], efficient=True)
    tr = O.OraclePaletteTrainer({k: v.float().cpu() for k, v in model.netG_A.state_dict().items()}, cfg)
    loss_ref = float(tr.optimize_parameters(x, cpu_roundtrip(x, 2), None, noise, t, u))
    model.rng_injection = lambda b: (t, u, noise)
    model.set_input({"A": x})
    model.optimize_parameters()
    loss = float(model.get_current_losses()["G_tot"])
    print(f"super_resolution step {dtype_name}: loss {loss:.6f}, oracle {loss_ref:.6f}")
    assert abs(loss - loss_ref) <= TOL_LOSS_FWD[dtype_name] * abs(loss_ref), (loss, loss_ref)


def test_example_ddpm_df2kost_json_through_the_train_loop(tmp_path):
    """the reference's shipped super-resolution example (scale 4) as tests/test_gpu_7_train_loop.py drives the other examples"""
    from test_gpu_7_train_loop import _appendix_c, _loop
    from joligen_amd.options import opt_from_json

    ov = _appendix_c(tmp_path, name="df2kost_e2e", data_crop_size=64, data_load_size=64, train_batch_size=2)
    opt = opt_from_json(DF2K, ov)
    assert opt.alg_diffusion_task == "super_resolution" and opt.alg_diffusion_super_resolution_scale == 4.0 and opt.train_iter_size == 1
    data = {"A": torch.rand(2, 3, 64, 64, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1, "A_img_paths": ["x"] * 2}
    torch.manual_seed(0)
    model, losses = _loop(opt, data, 2)
    assert model.data_crop_size_low_res == 16 and tuple(model.cond_image.shape) == (2, 3, 64, 64)
    assert all(math.isfinite(v) for l in losses for v in l.values()) and "G_tot" in losses[0]
    model.save_networks("latest")
    lr0 = model.optimizers[0].param_groups[0]["lr"]
    model.update_learning_rate()
    assert model.optimizers[0].param_groups[0]["lr"] <= lr0
    sd = torch.load(os.path.join(str(tmp_path), "df2kost_e2e", "latest_net_G_A.pth"), map_location="cpu")
    assert tuple(sd["denoise_fn.model.input_blocks.0.0.weight"].shape) == (64, 6, 3, 3)


def test_super_resolution_step_through_torch_ops():
    """under ops.torch_ops_boundary() set_input calls torch.ops.jg355.lowres_roundtrip and the step runs on the op graph.  In
    deterministic mode the conditioning image and the loss are torch.equal with the ctypes run on the same (module-by-module) graph --
    the forward is the same kernels on the same bits; the backward of the op graph groups its sums differently
    (tests/test_gpu_1_model.py::test_palette_step_is_bit_reproducible_in_deterministic_mode), so the first moments agree to fp32
    rounding (1e-6 of their norm), not to the bit"""
    from joligen_amd import _lib, ops

    x = tiny_image()
    draw = O.draw_step_randomness(torch.Generator().manual_seed(2), x, 2000)
    prev = _lib.set_tuning("JG_DETERMINISTIC", 1)
    try:
        res = []
        for boundary in (False, True):
            model = make_model("fp16", alg_diffusion_task="super_resolution", alg_diffusion_super_resolution_scale=2)
            model.netG_A.denoise_fn.model.jg_fused = False
            model.rng_injection = lambda b: draw
            if boundary:
                with ops.torch_ops_boundary():
                    model.set_input({"A": x})
                    model.optimize_parameters()
            else:
                model.set_input({"A": x})
                model.optimize_parameters()
            torch.cuda.synchronize()
            res.append((model.cond_image.clone(), model.loss_G_tot.detach().clone(), model.netG_A.arena.m.clone(), model.netG_A.arena.p.clone()))
    finally:
        _lib.set_tuning("JG_DETERMINISTIC", prev)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (float(res[0][1]), float(res[1][1]))
    e = float((res[0][2].double() - res[1][2].double()).norm() / res[0][2].double().norm())
    print(f"torch.ops vs ctypes first moments: {e:.3e}; parameters after the step torch.equal: {torch.equal(res[0][3], res[1][3])}")
    assert e < 1e-6, e
