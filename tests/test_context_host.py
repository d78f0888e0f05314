"""Host-side tests of data_online_context_pixels of the CUT model: the torch restatement (tests/context_ref.py) against a literal evaluation of
the reference's F.pad + mask * ctx, the option checks, the C ABI declarations and their binding, and the fixtures recorded from the unmodified
reference (tests/tools/make_fixture_context.py -> tests/golden/context/)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import context_ref as R
import ref_shim  # noqa: F401  (the reference's path, for the regeneration test)

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "context")
FIXTURES = {"c5": (5, False), "c5_noise_apa": (5, True), "c8": (8, False)}      # name -> (c, dataaug_D_noise + dataaug_APA)
SHAPES = [(2, 8, 1, 3), (1, 5, 3, 1), (3, 16, 5, 4), (2, 32, 8, 8)]              # (B, S, c, C)
KEY = (0x1234ABCD, 0x0F1E2D3C)


def _load(name):
    return torch.load(os.path.join(DIR, f"cutstep_{name}.pt"), weights_only=False)


def _nhwc(x, cpad=8):
    out = torch.zeros(x.shape[0], x.shape[2], x.shape[3], cpad, dtype=x.dtype)
    out[..., :x.shape[1]] = x.permute(0, 2, 3, 1)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_is_the_reference_expression(shape):
    """split = the loader's image and its centre; frame = F.pad(inner, c) + mask_context * ctx, value for value (float64: the sum with an exact
    zero changes nothing); the adjoint = what autograd gives the literal expression: the window for inner, nothing from the frame"""
    B, S, c, C = shape
    g = torch.Generator().manual_seed(3 + S)
    x = torch.rand(B, C, S + 2 * c, S + 2 * c, generator=g) * 2 - 1
    for dtype in (torch.float16, torch.bfloat16):
        ctx, crop = R.split(x, c, dtype)
        assert tuple(ctx.shape) == (B, S + 2 * c, S + 2 * c, 8) and tuple(crop.shape) == (B, S, S, 8)
        assert torch.equal(ctx[..., :C], x.permute(0, 2, 3, 1).to(dtype)) and bool((ctx[..., C:] == 0).all())
        assert torch.equal(crop[..., :C], x[:, :, c:-c, c:-c].permute(0, 2, 3, 1).to(dtype)) and bool((crop[..., C:] == 0).all())
    inner = (torch.rand(B, C, S, S, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    ctx = x.double().requires_grad_(True)
    lit = R.frame_literal(inner, ctx, c)
    mine = R.frame(_nhwc(inner.detach()), _nhwc(ctx.detach()), c, C)
    assert torch.equal(mine[..., :C], lit.detach().permute(0, 2, 3, 1)) and bool((mine[..., C:] == 0).all())
    assert torch.equal(lit.detach()[:, :, c:-c, c:-c], inner.detach())
    m = R.mask_context(B, C, S + 2 * c, S + 2 * c, c)
    assert float(m.sum()) == B * C * ((S + 2 * c) ** 2 - S * S) and torch.equal(lit.detach() * m, ctx.detach() * m)
    dout = torch.randn(lit.shape, generator=g, dtype=torch.float64)
    d_inner, d_ctx = torch.autograd.grad(lit, [inner, ctx], dout)
    assert torch.equal(R.frame_grad(_nhwc(dout), c)[..., :C], d_inner.permute(0, 2, 3, 1))
    assert torch.equal(d_ctx, dout * m)                                          # the frame's gradient goes to the (detached) surroundings only
    # the noise covers the WHOLE framed image, drawn on its own grid
    z = R.drawn_z(KEY, B, C, S + 2 * c, S + 2 * c, call=0)
    n = R.noisy(mine, C, 0.1, z)
    assert tuple(z.shape) == (B, C, S + 2 * c, S + 2 * c) and bool((n[..., C:] == 0).all())
    assert torch.allclose(n[..., :C] - mine[..., :C], float(torch.tensor(0.1, dtype=torch.float32)) * z.permute(0, 2, 3, 1), rtol=0, atol=1e-15)
    assert not torch.equal(R.drawn_z(KEY, B, C, S + 2 * c, S + 2 * c, call=1), z)


def test_select_differs_from_the_expression_only_for_non_finite_surroundings():
    """why the kernel writes the select: 0 * inf under the window would poison the crop in the multiply-add form"""
    inner, ctx = torch.ones(1, 1, 2, 2, dtype=torch.float64), torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    ctx[0, 0, 1, 1] = float("inf")
    assert torch.isnan(R.frame_literal(inner, ctx, 1)[0, 0, 1, 1])
    assert bool((R.frame(_nhwc(inner), _nhwc(ctx), 1, 1)[:, 1:3, 1:3, 0] == 1).all())


def _opt(over=None, **cut):
    from joligen_amd.options import opt_from_json

    return opt_from_json({"model_type": "cut", "alg": {"cut": cut}}, dict({"gpu_ids": "0"}, **(over or {})))


def test_context_option_checks():
    from joligen_amd.models.cm_gan_model import check_cm_gan_options
    from joligen_amd.models.cut_model import CONTEXT_VISUAL_NAMES, check_context_discriminators, check_context_options, cut_all_loss_names

    assert _opt().data_online_context_pixels == 0 and check_context_options(_opt()) == 0
    o = SimpleNamespace()
    assert check_context_options(o) == 0 and o.data_online_context_pixels == 0       # the default is filled in
    assert check_context_options(_opt({"data_online_context_pixels": 10})) == 10
    assert _opt_json_reads_the_option() == 7
    for bad in (-1, 2.5, "3", True, None):
        with pytest.raises(ValueError, match="data_online_context_pixels.*integer >= 0"):
            check_context_options(SimpleNamespace(data_online_context_pixels=bad))
    with pytest.raises(ValueError, match="model_input_nc=1 must equal model_output_nc=3"):
        check_context_options(SimpleNamespace(data_online_context_pixels=4, model_input_nc=1, model_output_nc=3))
    assert check_context_options(SimpleNamespace(data_online_context_pixels=0, model_input_nc=1, model_output_nc=3)) == 0      # off: nothing to frame
    # projected discriminators: resized to D_proj_interp, or built for the framed size
    check_context_discriminators(SimpleNamespace(data_crop_size=64, D_netDs=["projected_d", "basic"], D_proj_interp=128), 5)
    check_context_discriminators(SimpleNamespace(data_crop_size=64, D_netDs=["projected_d"], D_proj_interp=-1), 16)
    check_context_discriminators(SimpleNamespace(data_crop_size=33, D_netDs=["basic"]), 5)
    check_context_discriminators(SimpleNamespace(data_crop_size=50, D_netDs=["projected_d"], D_proj_interp=-1), 0)
    with pytest.raises(NotImplementedError, match="framed size 74 is not a multiple of 32"):
        check_context_discriminators(SimpleNamespace(data_crop_size=64, D_netDs=["projected_d"], D_proj_interp=-1), 5)
    # neither the loss names nor their order change; the visual names are the reference's
    assert cut_all_loss_names(_opt({"data_online_context_pixels": 5}), ["D_B_basic"]) == cut_all_loss_names(_opt(), ["D_B_basic"])
    assert CONTEXT_VISUAL_NAMES == ["real_A_with_context_vis", "real_B_with_context_vis", "fake_B_with_context_vis", "mask_context_vis"]
    with pytest.raises(NotImplementedError, match="data_online_context_pixels.*cm_gan"):
        check_cm_gan_options(SimpleNamespace(data_online_context_pixels=4))
    check_cm_gan_options(SimpleNamespace(data_online_context_pixels=0))


def _opt_json_reads_the_option():
    from joligen_amd.options import opt_from_json

    return opt_from_json({"model_type": "cut", "data": {"online_context_pixels": 7}}, {"gpu_ids": "0"}).data_online_context_pixels


def test_header_declares_and_lib_binds_the_entry_points():
    """include/jg355.h is the one statement of the ABI: both entry points are declared there, parsed into typed signatures, and exported by
    the built library"""
    import ctypes

    from joligen_amd import _lib

    text = open(_lib.HEADER).read()
    for name, nargs in (("jg_context_split", 11), ("jg_context_frame", 17)):
        assert f"int {name}(" in text
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs and _lib.RESTYPES[name] is ctypes.c_int32
    sig = _lib.SIGNATURES["jg_context_frame"]
    assert sig[5] is ctypes.c_float and sig[8] is ctypes.c_uint32 and sig[9] is ctypes.c_uint32 and sig[1] is ctypes.c_void_p
    assert "context.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "context.hip"))
    L = _lib.lib()
    for name in ("jg_context_split", "jg_context_frame"):
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
    # the argument checks answer before any launch: no device is needed to see them
    assert L.jg_context_split(0, None, None, None, 1, 3, 10, 10, 1, 8, None) == _lib.JG_ERR_BAD_ARG
    assert L.jg_context_frame(0, None, None, None, None, 0.0, None, None, 0, 0, 1, 10, 10, 1, 3, 8, None) == _lib.JG_ERR_BAD_ARG
    assert L.jg_context_frame(7, None, None, None, None, 0.0, None, None, 0, 0, 1, 10, 10, 1, 3, 8, None) == _lib.JG_ERR_UNSUPPORTED


def test_python_surfaces_exist_and_refuse_cpu_tensors():
    from joligen_amd import launch, ops

    assert callable(launch.context_split) and callable(launch.context_frame)
    assert hasattr(torch.ops.jg355, "context_split") and hasattr(torch.ops.jg355, "context_frame")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.context_split(torch.zeros(1, 3, 6, 6), 1, torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.context_frame(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16), torch.zeros(1, 6, 6, 8, dtype=torch.bfloat16), 1, 3)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_layout_names_and_frame(name):
    from joligen_amd.models.cut_model import CONTEXT_VISUAL_NAMES, cut_all_loss_names

    c, aug = FIXTURES[name]
    assert os.path.getsize(os.path.join(DIR, f"cutstep_{name}.pt")) < 1 << 20
    g = _load(name)
    cfg, hp = g["cfg"], g["hp"]
    S = cfg["S"]
    assert (cfg["B"], S, cfg["pool"], cfg["iters"], cfg["nce_loss"]) == (2, 32, 2, 4, "patchnce") and len(g["steps"]) == 4
    assert hp["data_online_context_pixels"] == c and hp["dataaug_D_noise"] == (0.1 if aug else 0.0) and hp["dataaug_APA"] is aug
    assert g["loss_names"] == cut_all_loss_names(_opt({"data_online_context_pixels": c}), ["D_B_basic"])
    assert g["context_visual_names"] == CONTEXT_VISUAL_NAMES
    for it, s in enumerate(g["steps"]):
        d = s["d_aug"]
        assert tuple(s["A"].shape) == tuple(s["B"].shape) == (2, 3, S + 2 * c, S + 2 * c) and tuple(s["fake_B"].shape) == (2, 3, S, S)
        assert len(d["noise"]) == (2 if aug else 0) and all(tuple(n.shape) == (2, 3, S + 2 * c, S + 2 * c) for n in d["noise"])      # framed noise
        assert len(d["u"]) == (1 if aug else 0) and ("fake_B_with_context" in d) == (it == 0)
    # the recorded frame against the restatement: inside fake_B, outside the batch's A, value for value (fp32 in the reference)
    s0 = g["steps"][0]
    want = R.frame(_nhwc(s0["fake_B"]), _nhwc(s0["A"]), c, 3)
    assert torch.equal(_nhwc(s0["d_aug"]["fake_B_with_context"]), want)
    if aug:
        flags = [f for s in g["steps"] for f in s["d_aug"]["flags"][0].tolist()]
        assert any(flags) and not all(flags)
        assert all(abs(float(s["d_aug"]["s"][0]) - hp["dataaug_APA_target"]) >= 0.05 for s in g["steps"])


def test_nearest_resize_of_the_visuals_is_the_default_interpolate():
    """the *_vis images are F.interpolate(x, size=crop) with its default mode: nearest"""
    x = torch.arange(2 * 3 * 10 * 10, dtype=torch.float32).reshape(2, 3, 10, 10)
    assert torch.equal(F.interpolate(x, size=(6, 6)), F.interpolate(x, size=(6, 6), mode="nearest"))
    m = F.interpolate(R.mask_context(1, 3, 10, 10, 2, dtype=torch.float32), size=(6, 6))[:, 0]
    assert tuple(m.shape) == (1, 6, 6) and float(m[0, 0, 0]) == 1.0 and float(m[0, 3, 3]) == 0.0


def test_context_fixture_regenerates(tmp_path):
    """the fixtures are outputs of the unmodified reference: the recipe writes the augmented one again, bit for bit"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(HERE, "tools", "make_fixture_context.py"), str(tmp_path), "c5_noise_apa"], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    assert os.listdir(tmp_path) == ["cutstep_c5_noise_apa.pt"] and sorted(os.listdir(DIR)) == sorted(f"cutstep_{n}.pt" for n in FIXTURES)
    assert open(os.path.join(tmp_path, "cutstep_c5_noise_apa.pt"), "rb").read() == open(os.path.join(DIR, "cutstep_c5_noise_apa.pt"), "rb").read()
