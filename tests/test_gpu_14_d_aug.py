"""GPU tests of dataaug_D_noise / adaptive pseudo augmentation (APA) of the CUT model: the fused kernels (`jg_d_aug`, `jg_apa_update`) against
the restatement of tests/d_aug_ref.py, the in-kernel Philox / Box-Muller generator, the argument checks, the torch.ops surface, and `CUTModel`
with the options on: against the step fixtures recorded from the unmodified reference (tests/golden/d_aug/), under the three step drivers,
and with the options off (no launch)."""
import contextlib
import ctypes
import os
import random
import warnings

import numpy as np
import pytest
import torch

import d_aug_ref as R
import jg_oracle as O
from pixel_loss_ref import ordered_bits
from test_d_aug_host import KEY, N_SHAPE, normal_statistics
from test_oracle_golden import ReplayRandom, cut_ids

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "d_aug")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
CPAD = 8
# (B, H, W, C): one pixel; a tail that fills no vector group of a block; C = 1 (the MNIST example); per-sample flags with B > 1 over several blocks
SHAPES = [(1, 1, 1, 3), (2, 5, 7, 3), (3, 32, 32, 1), (2, 64, 64, 3)]
MODES = ["noise", "select", "both", "sigma0"]
SIGMA = 0.1
# forward-only tolerance of the losses of a CUT step at identical weights (test_gpu_5_cutloss.py::TOL_LOSS_FWD)
TOL_LOSS_FWD = {torch.float16: 6e-3, torch.bfloat16: 4e-2}
# In-kernel generator against the float64 restatement on the same uniforms, |device - restatement| / max(1, |restatement|) with the device's
# draw stored as fp16 (src = 0, sigma = 1).  Measured on an MI355X at N = 4 * 3 * 256 * 256: see DESIGN.md 23 (the storage rounding, half an fp16
# unit = 2^-11 = 4.9e-4 relative, is the whole of it); the bound is four times the measured maximum, capped at 1e-3.
GEN_MEASURED = 4.871e-4
GEN_BOUND = min(4 * GEN_MEASURED, 1e-3)


def _key(words=KEY):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy()).to(D0)


def kernel_inputs(shape, dtype, seed=5):
    """CPU tensors as jg_d_aug reads them: NaN in every padding channel of src and alt; z fp32 [B, C, H, W]; u with flags on both sides of p = 0.5"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed + 10 * B + H)
    src, alt = (torch.randn(B, H, W, CPAD, generator=g).to(dtype) for _ in range(2))
    src[..., C:], alt[..., C:] = float("nan"), float("nan")
    z = torch.randn(B, C, H, W, generator=g)
    u = torch.tensor([0.25, 0.75, 0.4999][:B])
    return src, alt, z, u


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_d_aug_kernel_vs_float64_restatement(shape, mode, dtype_name):
    from joligen_amd import ops

    dtype = DTYPES[dtype_name]
    B, H, W, C = shape
    src, alt, z, u = kernel_inputs(shape, dtype)
    sigma = SIGMA if mode in ("noise", "both") else 0.0
    sel = mode != "noise"
    p = torch.tensor([0.5], device=D0)
    kw = dict(alts=[alt.to(D0)], ps=[p], us=[u.to(D0)]) if sel else {}
    (out,), flags = ops.d_aug(src.to(D0), C, sigma, z=z.to(D0) if sigma else None, **kw)
    torch.cuda.synchronize()
    out = out.cpu()
    ref, rflags = R.d_aug(src.double().numpy(), C, sigma, z=z.numpy(), alt=alt.double().numpy() if sel else None, u=u.numpy(), p=0.5)
    ref16 = torch.from_numpy(ref).to(dtype)
    ulps = (ordered_bits(out[..., :C]) - ordered_bits(ref16[..., :C])).abs()
    print(f"d_aug {shape} {mode} {dtype_name}: max ulp {int(ulps.max())}, off by one {int((ulps == 1).sum())} of {ulps.numel()}, flags {rflags.tolist()}")
    assert out.dtype == dtype and out.shape == src.shape and torch.isfinite(out).all()
    assert int(ulps.max()) <= 1
    assert bool((out[..., C:].view(torch.int16) == 0).all())                     # padding channels: +0
    if sel:
        assert flags.cpu().tolist() == [rflags.tolist()] and rflags.tolist() == [1, 0, 1][:B]
        for b in range(B):
            if rflags[b]:                                                        # flagged rows: alt bit for bit
                assert torch.equal(out[b, ..., :C].view(torch.int16), alt[b, ..., :C].view(torch.int16))
    else:
        assert flags is None
    if sigma == 0.0:                                                             # unflagged rows at sigma = 0: src bit for bit
        for b in range(B):
            if not rflags[b]:
                assert torch.equal(out[b, ..., :C].view(torch.int16), src[b, ..., :C].view(torch.int16))
    else:
        assert not torch.equal(out[..., :C], src[..., :C])


def test_d_aug_several_targets_share_src_and_noise():
    """one launch, three targets: the unflagged rows of all of them are the same src + sigma z; each target follows its own flags and alt"""
    from joligen_amd import ops

    shape = (3, 32, 32, 1)
    src, alt, z, _ = kernel_inputs(shape, torch.bfloat16)
    alts = [alt.to(D0), (alt * 2).to(D0), (alt * 3).to(D0)]
    us = [torch.tensor(v, device=D0) for v in ([0.1, 0.9, 0.9], [0.9, 0.1, 0.9], [0.9, 0.9, 0.9])]
    ps = [torch.tensor([0.5], device=D0), torch.tensor([0.5], device=D0), torch.tensor([1.0], device=D0)]
    outs, flags = ops.d_aug(src.to(D0), 1, SIGMA, z=z.to(D0), alts=alts, ps=ps, us=us)
    (plain,), _ = ops.d_aug(src.to(D0), 1, SIGMA, z=z.to(D0))
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [[1, 0, 0], [0, 1, 0], [1, 1, 1]]
    for d in range(3):
        for b in range(3):
            want = alts[d][b] if flags[d, b] else plain[b]
            assert torch.equal(outs[d][b, ..., :1], want[..., :1]), (d, b)
    with pytest.raises(ValueError, match="d_aug"):
        ops.d_aug(src.to(D0), 1, alts=[alt.to(D0)] * 5, ps=ps[:1] * 5, us=us[:1] * 5)


def test_d_aug_generator_matches_the_restatement_and_is_normal():
    from joligen_amd import ops

    B, C, H, W = N_SHAPE
    src = torch.zeros(B, H, W, CPAD, device=D0, dtype=torch.float16)
    nchw = lambda t: t[..., :C].permute(0, 3, 1, 2).double().cpu().numpy()
    (a,), _ = ops.d_aug(src, C, 1.0, key=_key(), call=0)
    (a2,), _ = ops.d_aug(src, C, 1.0, key=_key(), call=0)
    (b,), _ = ops.d_aug(src, C, 1.0, key=_key((KEY[0] + 1, KEY[1])), call=0)
    (c,), _ = ops.d_aug(src, C, 1.0, key=_key(), call=0, noise_stream=1)
    torch.cuda.synchronize()
    assert torch.equal(a, a2) and not torch.equal(a, b) and not torch.equal(a, c)          # same key: same bits; another key / stream: other draws
    z, ref = nchw(a), R.normals(KEY, B, C, H, W, stream=0, call=0)
    dev = float((np.abs(z - ref) / np.maximum(1.0, np.abs(ref))).max())
    ref16 = torch.from_numpy(ref).to(torch.float16)
    # in units of the storage type, where such a unit (>= 2^-16 at |z| >= 2^-6) is far above the fp32 error of the device's log / sincos
    # (2 pi u carries 2^-24 * 2 pi = 4e-7 of angle, times a radius below 6): the device's value is the restatement's or its neighbour
    ulps = (ordered_bits(a[..., :C].permute(0, 3, 1, 2).contiguous()) - ordered_bits(ref16)).abs()[torch.from_numpy(np.abs(ref) >= 2.0 ** -6)]
    print(f"in-kernel generator against the float64 restatement: max relative deviation {dev:.3e} (bound {GEN_BOUND:.1e}); fp16 units: max "
          f"{int(ulps.max())}, off by one {int((ulps == 1).sum())} of {ulps.numel()}; largest |z| {np.abs(z).max():.3f}")
    assert dev <= GEN_BOUND, dev
    assert int(ulps.max()) <= 1 and int((ulps == 1).sum()) <= ulps.numel() // 20            # the device's fp32 log / sincos move a rounding now and then
    for what, val, bound in normal_statistics(z, nchw(c)):
        print(f"device draws, {what}: {val:.3e} (bound {bound:.3e})")
        assert val <= bound, (what, val, bound)
    assert bool((a[..., C:] == 0).all())


def test_d_aug_drawn_flags_equal_the_restatement():
    from joligen_amd import ops

    B = 256
    src = torch.zeros(B, 2, 2, CPAD, device=D0, dtype=torch.bfloat16)
    alt = torch.ones_like(src)
    for call, p in ((0, 0.5), (1, 0.484), (3, 0.0), (4, 1.0)):
        ps = [torch.tensor([p], device=D0)] * 2
        outs, flags = ops.d_aug(src, 3, alts=[alt, alt], ps=ps, key=_key(), call=call, streams=[1, 2])
        _, again = ops.d_aug(src, 3, alts=[alt, alt], ps=ps, key=_key(), call=call, streams=[1, 2])
        torch.cuda.synchronize()
        for d, stream in enumerate((1, 2)):
            want = (np.float32(R.flag_uniforms(KEY, B, stream, call)) < np.float32(p)).astype(np.int32)
            assert flags[d].cpu().numpy().tolist() == want.tolist(), (call, p, stream)
            assert torch.equal(outs[d][:, 0, 0, 0].float().cpu(), torch.from_numpy(want).float())
        assert torch.equal(flags, again)
        if 0 < p < 1:
            assert not torch.equal(flags[0], flags[1])                             # one stream id per discriminator: independent flags


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_apa_update_equals_the_reference_bit_for_bit(dtype_name):
    """apa_fn.pt: p, adjust and s of the reference's update, for PatchGAN logit maps (channel 0 of an NHWC tensor padded to 8 channels; the other
    channels hold values of the OTHER sign), for projected logits (every element) and for the first B rows of a batched real / fake prediction"""
    from joligen_amd import ops

    dtype = DTYPES[dtype_name]
    ups = torch.load(os.path.join(DIR, "apa_fn.pt"), weights_only=False)["updates"]
    assert {c["layout"] for c in ups} == {"map", "flat"} and any(float(c["adjust"]) == 0 for c in ups)
    for c in ups:
        pred = c["pred"].to(dtype)
        assert torch.equal(pred.float().sign(), c["pred"].sign())                  # the 16-bit copy keeps every sign
        if c["layout"] == "map":
            x = (-pred.permute(0, 2, 3, 1)).repeat(1, 1, 1, CPAD).contiguous()
            x[..., 0] = pred[:, 0]
            preds = [(x.to(D0), True)]
        else:
            both = torch.cat((pred, -pred), dim=0).to(D0)                          # [real | fake] rows of the batched discriminator pass
            preds = [(pred.to(D0), False), (both[: pred.shape[0]], False)]
        for x, channel0 in preds:
            state = torch.tensor([c["p0"], 7.0, 7.0], device=D0)
            ops.apa_update(x, state, c["target"], c["B"] * c["every"], c["nimg"] * 1000, channel0=channel0)
            torch.cuda.synchronize()
            got = state.cpu()
            for i, k in enumerate(("p", "adjust", "s")):
                assert got[i].numpy().tobytes() == c[k].to(torch.float32).numpy().tobytes(), (c["layout"], c["p0"], k, float(got[i]), float(c[k]))


def test_d_aug_argument_checks():
    """the C entry points answer with an error code before any launch (the outputs keep their sentinel); the Python surface raises"""
    from joligen_amd import _lib, ops

    lib = _lib.lib()
    B, H, W = 2, 4, 4
    src = torch.ones(B, H, W, CPAD, device=D0, dtype=torch.float16)
    alt, out = torch.ones_like(src) * 2, torch.full_like(src, 5.0)
    p, flags = torch.tensor([0.5], device=D0), torch.full((1, B), 9, device=D0, dtype=torch.int32)
    u, z, key = torch.tensor([0.1, 0.9], device=D0), torch.zeros(B, 3, H, W, device=D0), _key()
    arr = lambda *ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    sid = (ctypes.c_uint32 * 1)(1)

    def call(srcp=src.data_ptr(), outs=arr(out.data_ptr()), alts=arr(alt.data_ptr()), ps=arr(p.data_ptr()), fl=arr(flags.data_ptr()), us=arr(u.data_ptr()),
             sigma=0.1, zp=z.data_ptr(), keyp=None, C=3, cpad=CPAD, nd=1, dtype=0, noise_stream=0, ids=sid):
        return lib.jg_d_aug(dtype, srcp, nd, alts, ps, outs, fl, us, ids, sigma, zp, keyp, noise_stream, 0, B, H, W, C, cpad, None)

    bad = [dict(C=9), dict(cpad=12), dict(srcp=None), dict(outs=None), dict(outs=arr(None)), dict(ps=None), dict(ps=arr(None)), dict(fl=None),
           dict(nd=0), dict(nd=5), dict(dtype=2), dict(C=0), dict(zp=None), dict(us=None), dict(srcp=src.data_ptr() + 2),
           dict(outs=arr(out.data_ptr() + 2)), dict(outs=arr(src.data_ptr())), dict(outs=arr(alt.data_ptr())), dict(sigma=float("nan")),
           dict(us=None, keyp=key.data_ptr(), zp=None, noise_stream=1),      # drawn flags on the noise's stream
           dict(us=None, keyp=key.data_ptr(), ids=(ctypes.c_uint32 * 1)(1 << 16)), dict(noise_stream=1 << 16)]
    for kw in bad:
        assert call(**kw) == _lib.JG_ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((flags == 9).all())                  # nothing was launched
    assert call() == _lib.JG_OK and call(us=None, keyp=key.data_ptr()) == _lib.JG_OK and call(alts=None, ps=None, fl=None, us=None, ids=None) == _lib.JG_OK
    torch.cuda.synchronize()
    pred, st = torch.ones(4, 8, device=D0, dtype=torch.bfloat16), torch.tensor([0.5, 9.0, 9.0], device=D0)
    sp = st.data_ptr()

    def upd(predp=pred.data_ptr(), n=32, stride=1, pp=sp, ap=sp + 4, s_p=sp + 8, target=0.6, num=4.0, den=1000.0, dtype=1):
        return lib.jg_apa_update(dtype, predp, n, stride, pp, ap, s_p, target, num, den, None)

    for kw in (dict(predp=None), dict(pp=None), dict(ap=None), dict(s_p=None), dict(n=0), dict(stride=0), dict(den=0.0), dict(num=-1.0),
               dict(target=float("nan")), dict(dtype=3)):
        assert upd(**kw) == _lib.JG_ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0.5, 9.0, 9.0]
    assert upd() == _lib.JG_OK
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [float(v) for v in R.apa_update(np.ones(32), 0.5, 0.6, 4.0, 1000.0)]
    # the Python surface
    for args, kw, exc in (((src, 9), {}, ValueError), ((src, 3, 0.1), dict(z=z.double()), TypeError), ((src, 3, 0.1), dict(z=z[:1]), TypeError),
                          ((src, 3), dict(alts=[alt]), ValueError), ((src, 3), dict(alts=[alt.bfloat16()], ps=[p]), TypeError),
                          ((src, 3), dict(alts=[alt], ps=[p], us=[u[:1]]), TypeError), ((src, 3), dict(ps=[p]), ValueError),
                          ((src, 3), dict(outs=[out[:1]]), TypeError), ((src, 3, 0.1), dict(z=z, key=key.float()), TypeError)):
        with pytest.raises(exc, match="d_aug"):
            ops.d_aug(*args, **kw)
    with pytest.raises(RuntimeError, match="jg_d_aug"):                           # noise without z and without a key
        ops.d_aug(src, 3, 0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.d_aug(src.cpu(), 3)
    with pytest.raises(TypeError, match="apa_update"):
        ops.apa_update(pred, st.double(), 0.6, 4, 1000)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.apa_update(pred.cpu(), st, 0.6, 4, 1000)


def test_d_aug_torch_ops_opcheck_and_boundary():
    """schema + fake kernels of torch.ops.jg355.d_aug / apa_update; `ops.d_aug` / `ops.apa_update` under the boundary are bit-equal to the ctypes path"""
    from joligen_amd import ops

    J = torch.ops.jg355
    shape = (2, 5, 7, 3)
    src, alt, z, u = kernel_inputs(shape, torch.bfloat16)
    src, alt, z, u, p, key = src.to(D0), alt.to(D0), z.to(D0), u.to(D0), torch.tensor([0.5], device=D0), _key()
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(J.d_aug.default, (src, [alt], [p], [u], [1], 3, SIGMA, z, None, 0, 0), test_utils=utils)
    torch.library.opcheck(J.d_aug.default, (src, [], [], [], [], 3, SIGMA, None, key, 0, 1), test_utils=utils)
    torch.library.opcheck(J.d_aug.default, (src, [alt, alt], [p, p], [], [1, 2], 3, 0.0, None, key, 0, 1), test_utils=utils)
    pred = torch.randn(2, 6, 6, CPAD).bfloat16().to(D0)
    torch.library.opcheck(J.apa_update.default, (pred, torch.tensor([0.5, 0.0, 0.0], device=D0), 72, 8, 0.6, 4.0, 1000.0), test_utils=utils)
    for kw in (dict(z=z), dict(key=key, call=1), dict(z=z, alts=[alt], ps=[p], us=[u]), dict(key=key, alts=[alt, alt], ps=[p, p], call=2)):
        sigma = SIGMA if ("z" in kw or "call" in kw) else 0.0
        a, fa = ops.d_aug(src, 3, sigma, **kw)
        with ops.torch_ops_boundary():
            b, fb = ops.d_aug(src, 3, sigma, **kw)
            outs = [torch.empty_like(src) for _ in a]
            c, _ = ops.d_aug(src, 3, sigma, outs=outs, **kw)
        assert all(torch.equal(x[..., :3], y[..., :3]) and torch.equal(x, w) for x, y, w in zip(a, b, c)) and all(o is w for o, w in zip(outs, c))
        assert (fa is None and fb is None) or torch.equal(fa, fb)
    sa, sb = torch.tensor([0.5, 0.0, 0.0], device=D0), torch.tensor([0.5, 0.0, 0.0], device=D0)
    ops.apa_update(pred, sa, 0.6, 4, 1000, channel0=True)
    with ops.torch_ops_boundary():
        ops.apa_update(pred, sb, 0.6, 4, 1000, channel0=True)
    assert torch.equal(sa, sb) and float(sa[1]) != 0.0


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _build_from_fixture(g, dtype, **over):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    c, hp = g["cfg"], g["hp"]
    cfg = {"model_type": "cut", "G": {"netG": "resnet", "ngf": c["ngf"], "nblocks": c["n_blocks"]}, "D": {"netDs": ["basic"], "ndf": c["ndf"]},
           "alg": {"cut": {"nce_layers": c["nce_layers"], "num_patches": c["num_patches"], "nce_loss": c["nce_loss"]}},
           "dataaug": {"D_noise": hp["dataaug_D_noise"], "APA": hp["dataaug_APA"], "APA_p": hp["dataaug_APA_p"], "APA_target": hp["dataaug_APA_target"],
                       "APA_every": hp["dataaug_APA_every"], "APA_nimg": hp["dataaug_APA_nimg"]},
           "data": {"crop_size": c["S"], "load_size": c["S"]},
           "train": {"batch_size": c["B"], "pool_size": c["pool"], "G_ema": True, "G_ema_beta": hp["ema_beta"], "G_lr": hp["lr_G"], "D_lr": hp["lr_D"]}}
    return create_model(opt_from_json(cfg, overrides=dict({"jg_act_dtype": "fp16" if dtype == torch.float16 else "bf16", "gpu_ids": "0"}, **over)), 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ["noise", "apa", "noise_apa"])
def test_cut_model_d_aug_vs_reference_golden(name, dtype):
    """CUTModel from the configuration of the reference's step fixture, synthesised weights (seeds 0 / 1 / 3 as in the recipe), with the recorded
    patch ids, pool draws (get_random's included), torch.normal and torch.rand draws injected: every loss of step 0 (the D losses included) at
    the forward tolerance of the existing CUT step test; over all four steps the flags, the trajectory of p bit for bit, adjust,
    get_current_APA_prob() and fake_B_noisy - fake_B = sigma z to one unit of the storage type."""
    g = torch.load(os.path.join(DIR, f"cutstep_{name}.pt"), weights_only=False)
    c, hp = g["cfg"], g["hp"]
    sigma, apa = hp["dataaug_D_noise"], hp["dataaug_APA"]
    model = _build_from_fixture(g, dtype, jg_early_D=False)
    assert model.loss_names == g["loss_names"]
    s0 = g["steps"][0]
    model.data_dependent_initialize({"A": s0["A"], "B": s0["B"]})
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.netD_B_basic.load_state_dict(O.synth_state_dict(model.netD_B_basic.state_dict(), seed=1))
    model.netF.load_state_dict(O.synth_state_dict(model.netF.state_dict(), seed=3))
    calc = model.D_B_basic_loss_calculator
    nl, tol = len(c["nce_layers"].split(",")), TOL_LOSS_FWD[dtype]
    for it, s in enumerate(g["steps"]):
        d = s["d_aug"]
        draws = {("z_fake", 0): d["noise"][0] / sigma, ("z_real", 0): d["noise"][1] / sigma} if sigma else {}
        if apa:
            draws[("u", 0)] = d["u"][0]
        model.d_aug_injection = lambda kind, i, draws=draws: draws[(kind, i)].to(D0).contiguous()
        model.set_pool_rng(ReplayRandom(s["pool_draws"]))
        ids_ab, ids_idt = cut_ids(s, nl, c["num_patches"])
        model.patch_ids_injection = lambda call, shapes, a=ids_ab, b=ids_idt: [i.to(D0) for i in (a if call == 0 else b)]
        model.set_input({"A": s["A"], "B": s["B"]})
        model.optimize_parameters()
        torch.cuda.synchronize()
        assert model.step_driver == "sequential" and model.fake_B_pool.rng.i == len(s["pool_draws"])      # every recorded draw consumed, in order
        if it == 0:
            losses = {k: float(v) for k, v in model.get_current_losses().items()}
            for n in g["loss_names"]:
                ref = s["losses"][n]
                print(name, n, losses[n], ref)
                assert abs(losses[n] - ref) <= tol * abs(ref) + 1e-4, (n, losses[n], ref)
        if sigma:
            fb = model.fake_B.detach()[..., :3].double().cpu()
            want = (fb + d["noise"][0].permute(0, 2, 3, 1).double()).to(dtype)
            ulps = (ordered_bits(model.fake_B_noisy[..., :3].contiguous()) - ordered_bits(want.contiguous())).abs()
            assert int(ulps.max()) <= 1, (it, int(ulps.max()))
            assert bool((model.fake_B_noisy[..., 3:] == 0).all())
        if apa:
            assert calc.apa_flags.cpu().tolist() == d["flags"][0].tolist(), (it, calc.apa_flags.tolist(), d["flags"][0].tolist())
            state = calc.apa_state.cpu()
            print(name, it, "p", float(state[0]), "adjust", float(state[1]), "s", float(state[2]), "reference s", float(d["s"][0]))
            assert state[0].numpy().tobytes() == d["p"][0].numpy().tobytes(), (it, float(state[0]), float(d["p"][0]))
            assert float(state[1]) == float(d["adjust"][0])
            assert model.get_current_APA_prob() == d["APA_prob"]
            assert tuple(model.APA_img.shape) == tuple(model.real_B.shape)
        else:
            assert model.get_current_APA_prob() == {"APA_p": 0.0, "APA_adjust": 0.0}


_CUT = {"model_type": "cut", "G": {"netG": "resnet", "ngf": 32, "nblocks": 2}, "D": {"netDs": ["projected_d", "basic"], "ndf": 32, "proj_interp": 128},
        "alg": {"cut": {"nce_layers": "0,4,8", "nce_loss": "patchnce", "num_patches": 128}}, "data": {"crop_size": 64, "load_size": 64},
        "dataaug": {"D_noise": 0.1, "APA": True, "APA_p": 0.5, "APA_every": 1, "APA_nimg": 1},
        "train": {"batch_size": 2, "G_ema": True, "iter_size": 1, "pool_size": 4, "G_lr": 0.0, "D_lr": 0.0}}


def _run(monkeypatch, driver, calls, on=True, inject=True, boundary_last=False, seen=None):
    """`calls` x optimize_parameters() on one batch at learning rate zero with both options on (`on`), projected + PatchGAN discriminators;
    driver "sequential" or "default" (no switch set); `inject`: the same z / u draws for every run (seeded per step), else drawn in the kernels.
    Returns per call the GAN losses of both groups (independent of the patch ids, which the drivers draw differently), the APA state of every
    discriminator, its flags, and the driver."""
    from joligen_amd import ops
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    for var in ("JG_EARLY_D", "JG_GRAPH_D", "JG_GRAPH_G"):
        if driver == "sequential":
            monkeypatch.setenv(var, "0")
        else:
            monkeypatch.delenv(var, raising=False)
    monkeypatch.delenv("JG_DBG_GRAPH_CANARY_FAIL", raising=False)
    gen = torch.Generator().manual_seed(14)
    data = {"A": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1, "B": torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1}
    cfg = _CUT if on else {k: v for k, v in _CUT.items() if k != "dataaug"}
    torch.manual_seed(3)
    random.seed(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = create_model(opt_from_json(cfg, overrides={"jg_act_dtype": "bf16", "gpu_ids": "0"}), 0)
        m.data_dependent_initialize(data)
        m.setup(m.opt)
        m.single_gpu()
        names = ["G_GAN_" + dn for dn in m.discriminators_names] + ["D_GAN_" + dn for dn in m.discriminators_names]
        calcs = [getattr(m, dn + "_loss_calculator") for dn in m.discriminators_names]
        losses, drivers, states, flags = [], [], [], []
        for i in range(calls):
            if inject and on:
                gi = torch.Generator().manual_seed(100 + i)
                draws = {("z_fake", 0): torch.randn(2, 3, 64, 64, generator=gi), ("z_real", 0): torch.randn(2, 3, 64, 64, generator=gi),
                         ("u", 0): torch.rand(2, generator=gi), ("u", 1): torch.rand(2, generator=gi)}
                m.d_aug_injection = lambda kind, d, draws=draws: draws[(kind, d)].to(D0)
            m.set_input(data)
            with (ops.torch_ops_boundary() if boundary_last and i == calls - 1 else contextlib.nullcontext()), (seen or contextlib.nullcontext()):
                m.optimize_parameters()
            losses.append([float(getattr(m, "loss_" + n)) for n in names])
            drivers.append(m.step_driver)
            if on:
                states.append([c.apa_state.cpu().tolist() for c in calcs])
                flags.append([c.apa_flags.cpu().tolist() for c in calcs])
    torch.cuda.synchronize()
    return dict(losses=torch.tensor(losses, dtype=torch.float64), names=names, drivers=drivers, states=states, flags=flags, note=m.step_driver_note,
                dropped=[str(w.message) for w in rec if "jg_graph_" in str(w.message)], model=m)


def test_cut_d_aug_step_drivers_agree(monkeypatch):
    """six steps with both options on and the same injected draws under the default driver (captured graphs from the third step on: the
    augmentation launches run eagerly on the discriminator stream and write the graph's static operands, one real operand per discriminator)
    and under the sequential one: GAN losses at the forward tolerance, the same flags, p moved identically; the canary passed.  Then a run
    without injection (keys from torch's generator): finite losses, p inside [0, 1]."""
    import joligen_amd

    seq = _run(monkeypatch, "sequential", 6)
    r = _run(monkeypatch, "default", 6)
    assert seq["drivers"] == ["sequential"] * 6 and r["drivers"][0] != "sequential", (r["drivers"], r["note"])
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert r["drivers"][2:] == ["graph+graphG"] * 4 and not r["dropped"], (r["drivers"], r["note"], r["dropped"])
        st = next(iter(r["model"].driver.d_half.cache.values()))
        assert len(st.reals) == 2 and st.reals[0].data_ptr() != st.reals[1].data_ptr() and len(st.preds) == 2
    assert torch.isfinite(r["losses"]).all() and torch.isfinite(seq["losses"]).all()
    err = float(((r["losses"] - seq["losses"]).abs() / seq["losses"].abs()).max())
    print("default against sequential driver, GAN losses of six steps:", err, r["drivers"])
    assert err <= TOL_LOSS_FWD[torch.bfloat16], (r["losses"], seq["losses"])
    assert r["flags"] == seq["flags"] and any(f for step in r["flags"] for d in step for f in d) and not all(f for step in r["flags"] for d in step for f in d)
    for a, b in zip(r["states"], seq["states"]):
        assert [x[:2] for x in a] == [x[:2] for x in b], (r["states"], seq["states"])            # p and adjust of every discriminator, every step
    for d in range(2):                                                                           # every = 1: p moved in every step
        ps = [0.5] + [step[d][0] for step in r["states"]]
        assert all(a != b for a, b in zip(ps, ps[1:])) and all(abs(step[d][1]) == 1.0 for step in r["states"]), ps
    free = _run(monkeypatch, "default", 4, inject=False)
    assert torch.isfinite(free["losses"]).all() and all(0.0 <= x[0] <= 1.0 and abs(x[1]) == 1.0 for step in free["states"] for x in step)
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert free["drivers"][-1] == "graph+graphG" and not free["dropped"], (free["drivers"], free["note"])


class _SeenOps(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_cut_d_aug_step_through_torch_ops(monkeypatch):
    """a step under ops.torch_ops_boundary() with both options on goes through torch.ops.jg355.d_aug (fake batch, real operands) and
    torch.ops.jg355.apa_update (one per discriminator), with the losses of the ctypes path"""
    seen = _SeenOps()
    a = _run(monkeypatch, "sequential", 1)
    b = _run(monkeypatch, "sequential", 1, boundary_last=True, seen=seen)
    n_aug, n_upd = sum("jg355.d_aug" in n for n in seen.names), sum("jg355.apa_update" in n for n in seen.names)
    assert (n_aug, n_upd) == (2, 2), (n_aug, n_upd)
    assert float(((a["losses"] - b["losses"]).abs() / a["losses"].abs()).max()) <= TOL_LOSS_FWD[torch.bfloat16], (a["losses"], b["losses"])
    assert a["flags"] == b["flags"] and [x[:2] for x in a["states"][0]] == [x[:2] for x in b["states"][0]]


def test_cut_default_step_launches_no_d_aug(monkeypatch):
    """with both options off nothing new is launched: counters on ops.d_aug / ops.apa_update / ops.d_aug_key stay at 0 over two steps"""
    from joligen_amd import ops

    count = {"d_aug": 0, "apa_update": 0, "d_aug_key": 0}
    for k in count:
        def counted(*a, _k=k, _real=getattr(ops, k), **kw):
            count[_k] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ops, k, counted)
    r = _run(monkeypatch, "default", 2, on=False)
    assert torch.isfinite(r["losses"]).all() and count == {"d_aug": 0, "apa_update": 0, "d_aug_key": 0}, count
    assert r["model"].get_current_APA_prob() == {"APA_p": 0.0, "APA_adjust": 0.0} and not hasattr(r["model"], "fake_B_noisy")
    _run(monkeypatch, "sequential", 1, inject=False)      # (the counters do count when the options are on: noisy fake + real operands; one update per discriminator)
    assert count == {"d_aug": 2, "apa_update": 2, "d_aug_key": 1}, count
