"""GPU tests of data_online_context_pixels of the CUT model: the fused kernels (`jg_context_split`, `jg_context_frame`) against the restatement
of tests/context_ref.py, the identity of the in-kernel noise with `ops.d_aug`, the gradient, the argument checks, the torch.ops surface, and
`CUTModel` with the option on: against the step fixtures recorded from the unmodified reference (tests/golden/context/), under the step
drivers, through the torch.ops boundary, and with the option off (no launch).

The two entry points take contiguous tensors only (no leading dimensions, like jg_d_aug): there is no channel-slice case; instead every
output is written into a guarded buffer of tests/strided_util.py whose canaries must survive."""
import contextlib
import ctypes
import gc
import os
import random
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import context_ref as R
import jg_oracle as O
from pixel_loss_ref import ordered_bits
from strided_util import assert_canary_intact, assert_fully_written, make_slice
from test_context_host import FIXTURES, KEY, SHAPES
from test_oracle_golden import ReplayRandom, cut_ids

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "context")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
CPAD = 8
SIGMA = 0.1
# forward-only tolerance of the losses of a CUT step at identical weights (test_gpu_5_cutloss.py::TOL_LOSS_FWD)
TOL_LOSS_FWD = {torch.float16: 6e-3, torch.bfloat16: 4e-2}


@pytest.fixture(autouse=True)
def _collect_models_after_each_test():
    """A model and its step driver reference each other, and the pair owns captured hipGraphs, streams and their memory pools: only the cycle
    collector frees them.  Collected here, at the end of the test that built them, not whenever the collector next runs inside a later test."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _key(words=KEY):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy()).to(D0)


def kernel_inputs(shape, dtype, seed=7):
    """CPU tensors as the kernels read them: x fp32 NCHW at the framed size; inner / ctx 16-bit NHWC with NaN in every padding channel; z fp32
    NCHW at the framed size; dout 16-bit at the framed size"""
    B, S, c, C = shape
    H = S + 2 * c
    g = torch.Generator().manual_seed(seed + 10 * B + S)
    x = torch.rand(B, C, H, H, generator=g) * 2 - 1
    inner, ctx = torch.randn(B, S, S, CPAD, generator=g).to(dtype), torch.randn(B, H, H, CPAD, generator=g).to(dtype)
    inner[..., C:], ctx[..., C:] = float("nan"), float("nan")
    z = torch.randn(B, C, H, H, generator=g)
    dout = torch.randn(B, H, H, CPAD, generator=g).to(dtype)
    return x, inner, ctx, z, dout


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_context_kernels_vs_restatement(shape, dtype_name):
    from joligen_amd import ops

    dtype = DTYPES[dtype_name]
    B, S, c, C = shape
    H = S + 2 * c
    x, inner, ctx, z, dout = kernel_inputs(shape, dtype)
    # split: bit-exact, padding channels included; the same bits ops.to_nhwc writes
    gctx, gcrop = ops.context_split(x.to(D0), c, dtype)
    rctx, rcrop = R.split(x, c, dtype)
    assert gctx.dtype == dtype and tuple(gctx.shape) == (B, H, H, CPAD) and tuple(gcrop.shape) == (B, S, S, CPAD)
    assert torch.equal(_bits(gctx), _bits(rctx)) and torch.equal(_bits(gcrop), _bits(rcrop))
    assert torch.equal(_bits(gctx), _bits(ops.to_nhwc(x.to(D0), dtype))) and torch.equal(_bits(gcrop), _bits(gctx[:, c:-c, c:-c]))
    # plain frame: bit-exact, +0 in the padding channels whatever the inputs hold there; no second output without noise
    gi = inner.to(D0).requires_grad_(True)
    out, none = ops.context_frame(gi, ctx.to(D0), c, C)
    want = R.frame(inner, ctx, c, C)
    assert none is None and out.dtype == dtype and torch.equal(_bits(out), _bits(want)) and bool((_bits(out)[..., C:] == 0).all())
    # the gradient: the window of the incoming gradient, bit for bit; the frame contributes nothing
    out.backward(dout.to(D0))
    assert torch.equal(_bits(gi.grad), _bits(R.frame_grad(dout, c)))
    loud = dout.clone()
    ring = torch.ones(B, H, H, 1, dtype=torch.bool)
    ring[:, c:-c, c:-c] = False
    loud = torch.where(ring, torch.full_like(loud, 3e4), loud)
    gi2 = inner.to(D0).requires_grad_(True)
    ops.context_frame(gi2, ctx.to(D0), c, C)[0].backward(loud.to(D0))
    assert torch.equal(_bits(gi2.grad), _bits(gi.grad))
    # injected z: within one unit of the storage type of the float64 restatement, over the WHOLE framed image; the plain output is unchanged
    out_z, noisy = ops.context_frame(inner.to(D0), ctx.to(D0), c, C, SIGMA, z=z.to(D0))
    ref16 = R.noisy(want, C, SIGMA, z).to(dtype)
    ulps = (ordered_bits(noisy[..., :C]) - ordered_bits(ref16[..., :C])).abs()
    print(f"context_frame {shape} {dtype_name}: noisy max ulp {int(ulps.max())}, off by one {int((ulps == 1).sum())} of {ulps.numel()}")
    assert int(ulps.max()) <= 1 and bool((_bits(noisy)[..., C:] == 0).all()) and torch.equal(_bits(out_z), _bits(want))
    assert not noisy.requires_grad and not torch.equal(noisy[:, :c, :, :C], out_z[:, :c, :, :C])      # the frame is noised too
    # drawn z: bit-identical to ops.d_aug of the plain output at the same (sigma, key, call)
    for call in (0, 3):
        out_k, noisy_k = ops.context_frame(inner.to(D0), ctx.to(D0), c, C, SIGMA, key=_key(), call=call)
        (aug,), _ = ops.d_aug(out_k, C, SIGMA, key=_key(), call=call)
        assert torch.equal(_bits(noisy_k), _bits(aug)) and torch.equal(_bits(out_k), _bits(want)), call
    assert not torch.equal(_bits(noisy_k), _bits(ops.context_frame(inner.to(D0), ctx.to(D0), c, C, SIGMA, key=_key(), call=0)[1]))
    # the draw against the restatement of the generator on the framed grid (fp32 Box-Muller against float64: a few units of the storage type)
    zk = R.drawn_z(KEY, B, C, H, H, call=3)
    refk = R.noisy(want, C, SIGMA, zk)
    err = float(((noisy_k[..., :C].double().cpu() - refk[..., :C]).abs() / refk[..., :C].abs().clamp(min=1.0)).max())
    assert err <= 2.0 ** (-7 if dtype == torch.bfloat16 else -10), err


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_context_kernels_stay_inside_their_outputs(shape, dtype_name):
    """every output in a guarded buffer (canary pixels in front and behind, NaN canaries around the inputs): all of it written, nothing else"""
    from joligen_amd import _lib, ops

    dtype = DTYPES[dtype_name]
    B, S, c, C = shape
    H = S + 2 * c
    x, inner, ctx, z, _ = kernel_inputs(shape, dtype)
    mk = lambda shp, role, values=None: make_slice(shp, dtype, 1, left=0, right=0, guard=3, role=role, values=values, device=D0)
    b_inner, v_inner = mk((B, S, S, CPAD), "in", inner)
    b_ctx, v_ctx = mk((B, H, H, CPAD), "in", ctx)
    b_out, v_out = mk((B, H, H, CPAD), "out")
    b_noisy, v_noisy = mk((B, H, H, CPAD), "out")
    assert v_out.is_contiguous() and v_inner.is_contiguous()
    out, noisy = ops.context_frame(v_inner, v_ctx, c, C, SIGMA, key=_key(), call=1, outs=(v_out, v_noisy))
    torch.cuda.synchronize()
    assert out.data_ptr() == v_out.data_ptr() and noisy.data_ptr() == v_noisy.data_ptr()
    for b in (b_inner, b_ctx, b_out, b_noisy):
        assert_canary_intact(b)
    assert_fully_written(b_out)
    assert_fully_written(b_noisy)
    assert torch.equal(_bits(v_out), _bits(R.frame(inner, ctx, c, C)))
    b_c, v_c = mk((B, H, H, CPAD), "out")
    b_k, v_k = mk((B, S, S, CPAD), "out")
    xd = x.to(D0)
    rc = _lib.lib().jg_context_split(_lib.JG_F16 if dtype == torch.float16 else _lib.JG_BF16, xd.data_ptr(), v_c.data_ptr(), v_k.data_ptr(), B, C, H, H, c,
                                     CPAD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.JG_OK
    for b in (b_c, b_k):
        assert_canary_intact(b)
        assert_fully_written(b)
    rctx, rcrop = R.split(x, c, dtype)
    assert torch.equal(_bits(v_c), _bits(rctx)) and torch.equal(_bits(v_k), _bits(rcrop))


def test_context_argument_checks():
    """the C entry points answer with an error code before any launch (the outputs keep their sentinel); the Python surface raises"""
    from joligen_amd import _lib, ops

    lib = _lib.lib()
    B, S, c = 2, 4, 2
    H = S + 2 * c
    x = torch.zeros(B, 3, H, H, device=D0)
    ctx, crop = torch.full((B, H, H, CPAD), 5.0, device=D0, dtype=torch.float16), torch.full((B, S, S, CPAD), 5.0, device=D0, dtype=torch.float16)
    inner, out, noisy = torch.ones_like(crop), torch.full_like(ctx, 7.0), torch.full_like(ctx, 7.0)
    z, key = torch.zeros(B, 3, H, H, device=D0), _key()

    def split(dtype=0, xp=x.data_ptr(), cp=ctx.data_ptr(), kp=crop.data_ptr(), C=3, Hh=H, Ww=H, cc=c, cpad=CPAD, Bn=B):
        return lib.jg_context_split(dtype, xp, cp, kp, Bn, C, Hh, Ww, cc, cpad, None)

    for kw in (dict(cc=0), dict(cc=-1), dict(cc=4), dict(Hh=4), dict(xp=None), dict(cp=None), dict(kp=None), dict(C=0), dict(C=9), dict(cpad=12), dict(Bn=0),
               dict(cp=ctx.data_ptr() + 2), dict(kp=crop.data_ptr() + 2), dict(kp=ctx.data_ptr())):
        assert split(**kw) == _lib.JG_ERR_BAD_ARG, kw
    assert split(dtype=2) == _lib.JG_ERR_UNSUPPORTED

    def frame(dtype=0, ip=inner.data_ptr(), cp=ctx.data_ptr(), op=out.data_ptr(), np_=noisy.data_ptr(), sigma=0.1, zp=z.data_ptr(), keyp=None, ns=0,
              Hh=H, Ww=H, cc=c, C=3, cpad=CPAD):
        return lib.jg_context_frame(dtype, ip, cp, op, np_, sigma, zp, keyp, ns, 0, B, Hh, Ww, cc, C, cpad, None)

    for kw in (dict(cc=0), dict(cc=4), dict(Ww=3), dict(ip=None), dict(cp=None), dict(op=None), dict(C=0), dict(C=9), dict(cpad=12),
               dict(zp=None), dict(np_=None),                                      # sigma != 0: neither z nor key; no destination for the noise
               dict(sigma=float("nan")), dict(ns=1 << 16), dict(op=out.data_ptr() + 2), dict(np_=noisy.data_ptr() + 2), dict(ip=inner.data_ptr() + 2),
               dict(op=ctx.data_ptr()), dict(op=inner.data_ptr()), dict(np_=out.data_ptr()), dict(np_=ctx.data_ptr())):
        assert frame(**kw) == _lib.JG_ERR_BAD_ARG, kw
    assert frame(dtype=3) == _lib.JG_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((noisy == 7.0).all()) and bool((ctx == 5.0).all()) and bool((crop == 5.0).all())      # nothing was launched
    assert frame() == _lib.JG_OK and frame(zp=None, keyp=key.data_ptr()) == _lib.JG_OK and frame(sigma=0.0, zp=None, np_=None) == _lib.JG_OK
    assert split() == _lib.JG_OK
    torch.cuda.synchronize()
    # the Python surface
    for args, exc in (((x, 0, torch.float16), ValueError), ((x, 4, torch.float16), ValueError), ((x.double(), 1, torch.float16), TypeError),
                      ((x[0], 1, torch.float16), TypeError)):
        with pytest.raises(exc, match="context_split"):
            ops.context_split(*args)
    for args, kw, exc in (((inner, ctx, 1, 3), {}, ValueError), ((inner, ctx, 0, 3), {}, ValueError), ((inner[:1], ctx, c, 3), {}, ValueError),
                          ((inner.bfloat16(), ctx, c, 3), {}, TypeError), ((inner, ctx, c, 9), {}, ValueError),
                          ((inner, ctx, c, 3, 0.1), dict(z=z.double()), TypeError), ((inner, ctx, c, 3, 0.1), dict(z=z[:, :, 2:-2, 2:-2].contiguous()), TypeError),
                          ((inner, ctx, c, 3, 0.1), dict(key=key.float()), TypeError), ((inner, ctx, c, 3), dict(outs=(out[:1], None)), TypeError),
                          ((inner, ctx, c, 3), dict(outs=(None, noisy)), ValueError)):
        with pytest.raises(exc, match="context_frame"):
            ops.context_frame(*args, **kw)
    with pytest.raises(RuntimeError, match="jg_context_frame"):                    # noise without z and without a key
        ops.context_frame(inner, ctx, c, 3, 0.1)


def test_context_torch_ops_opcheck_and_boundary():
    """schema, fake kernels and the autograd registration of torch.ops.jg355.context_split / context_frame; `ops.context_*` under the boundary
    are bit-equal to the ctypes path, the gradient included"""
    from joligen_amd import ops

    J = torch.ops.jg355
    shape = (3, 16, 5, 4)
    B, S, c, C = shape
    x, inner, ctx, z, dout = (t.to(D0) for t in kernel_inputs(shape, torch.bfloat16))
    key = _key()
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(J.context_split.default, (x, c, False, 0), test_utils=utils)
    torch.library.opcheck(J.context_split.default, (x, c, True, 16), test_utils=utils)
    torch.library.opcheck(J.context_frame.default, (inner, ctx, c, C, 0.0, None, None, 0, 0, False), test_utils=utils)
    torch.library.opcheck(J.context_frame.default, (inner, ctx, c, C, SIGMA, z, None, 0, 0, True), test_utils=utils)
    torch.library.opcheck(J.context_frame.default, (inner, ctx, c, C, SIGMA, None, key, 0, 2, True), test_utils=utils)
    torch.library.opcheck(J.context_frame.default, (inner.clone().requires_grad_(True), ctx, c, C, 0.0, None, None, 0, 0, False),
                          test_utils=utils + ("test_autograd_registration",))
    torch.library.opcheck(J.context_frame_bwd.default, (dout, c), test_utils=utils)
    a_ctx, a_crop = ops.context_split(x, c, torch.bfloat16)
    with ops.torch_ops_boundary():
        b_ctx, b_crop = ops.context_split(x, c, torch.bfloat16)
    assert torch.equal(_bits(a_ctx), _bits(b_ctx)) and torch.equal(_bits(a_crop), _bits(b_crop))
    for kw in (dict(), dict(sigma=SIGMA, z=z), dict(sigma=SIGMA, key=key, call=1)):
        ia, ib, ic = (inner.clone().requires_grad_(True) for _ in range(3))
        oa, na = ops.context_frame(ia, ctx, c, C, **kw)
        with ops.torch_ops_boundary():
            ob, nb = ops.context_frame(ib, ctx, c, C, **kw)
            outs = (torch.empty_like(ctx), torch.empty_like(ctx) if kw else None)
            oc, nc = ops.context_frame(ic, ctx, c, C, outs=outs, **kw)
        assert torch.equal(_bits(oa), _bits(ob)) and torch.equal(_bits(oa), _bits(oc)) and torch.equal(_bits(oa), _bits(outs[0]))
        assert (na is None and nb is None and nc is None) or (torch.equal(_bits(na), _bits(nb)) and torch.equal(_bits(na), _bits(nc)) and nc is outs[1]
                                                              and not nb.requires_grad)
        for o, i in ((oa, ia), (ob, ib), (oc, ic)):
            o.backward(dout)
        assert torch.equal(_bits(ia.grad), _bits(ib.grad)) and torch.equal(_bits(ia.grad), _bits(ic.grad))
        assert torch.equal(_bits(ia.grad), _bits(R.frame_grad(dout.cpu(), c)))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _build_from_fixture(g, dtype, **over):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    c, hp = g["cfg"], g["hp"]
    cfg = {"model_type": "cut", "G": {"netG": "resnet", "ngf": c["ngf"], "nblocks": c["n_blocks"]}, "D": {"netDs": ["basic"], "ndf": c["ndf"]},
           "alg": {"cut": {"nce_layers": c["nce_layers"], "num_patches": c["num_patches"], "nce_loss": c["nce_loss"]}},
           "dataaug": {"D_noise": hp["dataaug_D_noise"], "APA": hp["dataaug_APA"], "APA_p": hp["dataaug_APA_p"], "APA_target": hp["dataaug_APA_target"],
                       "APA_every": hp["dataaug_APA_every"], "APA_nimg": hp["dataaug_APA_nimg"]},
           "data": {"crop_size": c["S"], "load_size": c["S"], "online_context_pixels": hp["data_online_context_pixels"]},
           "train": {"batch_size": c["B"], "pool_size": c["pool"], "G_ema": True, "G_ema_beta": hp["ema_beta"], "G_lr": hp["lr_G"], "D_lr": hp["lr_D"]}}
    return create_model(opt_from_json(cfg, overrides=dict({"jg_act_dtype": "fp16" if dtype == torch.float16 else "bf16", "gpu_ids": "0"}, **over)), 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_cut_model_context_vs_reference_golden(name, dtype):
    """CUTModel from the configuration of the reference's step fixture, synthesised weights (seeds 0 / 1 / 3 as in the recipe), with the recorded
    patch ids, pool draws (get_random's included), torch.normal and torch.rand draws injected: every loss of step 0 (the D losses included) at
    the forward tolerance of the existing CUT step test; fake_B_with_context = the model's fake_B inside the window and real_A_with_context on
    the frame, both bit for bit (the frame also against the reference's recorded one, rounded once); over all four steps every pool draw consumed in order, the flags, the
    trajectory of p bit for bit, adjust, get_current_APA_prob(), and the noisy framed fake to one unit of the storage type."""
    c, aug = FIXTURES[name]
    g = torch.load(os.path.join(DIR, f"cutstep_{name}.pt"), weights_only=False)
    cfg, hp = g["cfg"], g["hp"]
    S, sigma = cfg["S"], hp["dataaug_D_noise"]
    model = _build_from_fixture(g, dtype, jg_early_D=False)
    assert model.loss_names == g["loss_names"] and model.context == c and model.visual_names[-1] == g["context_visual_names"]
    s0 = g["steps"][0]
    model.data_dependent_initialize({"A": s0["A"], "B": s0["B"]})
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.netD_B_basic.load_state_dict(O.synth_state_dict(model.netD_B_basic.state_dict(), seed=1))
    model.netF.load_state_dict(O.synth_state_dict(model.netF.state_dict(), seed=3))
    calc = model.D_B_basic_loss_calculator
    nl, tol = len(cfg["nce_layers"].split(",")), TOL_LOSS_FWD[dtype]
    for it, s in enumerate(g["steps"]):
        d = s["d_aug"]
        draws = {("z_fake", 0): d["noise"][0] / sigma, ("z_real", 0): d["noise"][1] / sigma, ("u", 0): d["u"][0]} if aug else {}
        model.d_aug_injection = (lambda kind, i, draws=draws: draws[(kind, i)].to(D0).contiguous()) if aug else None
        model.set_pool_rng(ReplayRandom(s["pool_draws"]))
        ids_ab, ids_idt = cut_ids(s, nl, cfg["num_patches"])
        model.patch_ids_injection = lambda call, shapes, a=ids_ab, b=ids_idt: [i.to(D0) for i in (a if call == 0 else b)]
        model.set_input({"A": s["A"], "B": s["B"]})
        assert tuple(model.real_A.shape) == (2, S, S, CPAD) and tuple(model.real_B_with_context.shape) == (2, S + 2 * c, S + 2 * c, CPAD)
        assert tuple(model.real_A_nchw.shape) == (2, 3, S, S) and torch.equal(model.real_A_nchw.cpu(), s["A"][:, :, c:-c, c:-c])
        model.optimize_parameters()
        torch.cuda.synchronize()
        assert model.step_driver == "sequential" and model.fake_B_pool.rng.i == len(s["pool_draws"])      # every recorded draw consumed, in order
        fwc = model.fake_B_with_context.detach()
        assert tuple(fwc.shape) == (2, S + 2 * c, S + 2 * c, CPAD)
        assert torch.equal(_bits(fwc[:, c:-c, c:-c]), _bits(model.fake_B))                                 # the window: fake_B, bit for bit
        assert torch.equal(_bits(fwc), _bits(R.frame(model.fake_B.detach().cpu(), model.real_A_with_context.cpu(), c, 3)))      # the frame: real_A_with_context
        if it == 0:
            losses = {k: float(v) for k, v in model.get_current_losses().items()}
            for n in g["loss_names"]:
                ref = s["losses"][n]
                print(name, n, losses[n], ref)
                assert abs(losses[n] - ref) <= tol * abs(ref) + 1e-4, (n, losses[n], ref)
            ref_fwc = d["fake_B_with_context"].permute(0, 2, 3, 1)
            assert torch.equal(_bits(fwc[:, :c, :, :3]), _bits(ref_fwc[:, :c].to(dtype)))                  # the reference's frame, rounded once
            assert torch.equal(_bits(fwc[:, :, -c:, :3]), _bits(ref_fwc[:, :, -c:].to(dtype)))
        if aug:
            want = (fwc[..., :3].double().cpu() + d["noise"][0].permute(0, 2, 3, 1).double()).to(dtype)
            ulps = (ordered_bits(model.fake_B_with_context_noisy[..., :3].contiguous()) - ordered_bits(want.contiguous())).abs()
            assert int(ulps.max()) <= 1, (it, int(ulps.max()))
            assert bool((model.fake_B_with_context_noisy[..., 3:] == 0).all())
            assert calc.apa_flags.cpu().tolist() == d["flags"][0].tolist(), (it, calc.apa_flags.tolist(), d["flags"][0].tolist())
            state = calc.apa_state.cpu()
            print(name, it, "p", float(state[0]), "adjust", float(state[1]), "s", float(state[2]), "reference s", float(d["s"][0]))
            assert state[0].numpy().tobytes() == d["p"][0].numpy().tobytes(), (it, float(state[0]), float(d["p"][0]))
            assert float(state[1]) == float(d["adjust"][0])
            assert model.get_current_APA_prob() == d["APA_prob"]
            assert tuple(model.APA_img.shape) == tuple(model.real_B_with_context.shape)
        else:
            assert not hasattr(model, "fake_B_with_context_noisy") and model.get_current_APA_prob() == {"APA_p": 0.0, "APA_adjust": 0.0}


C_CTX = 8
_CUT = {"model_type": "cut", "G": {"netG": "resnet", "ngf": 32, "nblocks": 2}, "D": {"netDs": ["projected_d", "basic"], "ndf": 32, "proj_interp": 128},
        "alg": {"cut": {"nce_layers": "0,4,8", "nce_loss": "patchnce", "num_patches": 128}},
        "data": {"crop_size": 64, "load_size": 64, "online_context_pixels": C_CTX},
        "dataaug": {"D_noise": 0.1, "APA": True, "APA_p": 0.5, "APA_every": 1, "APA_nimg": 1},
        "train": {"batch_size": 2, "G_ema": True, "iter_size": 1, "pool_size": 4, "G_lr": 0.0, "D_lr": 0.0}}


def _run(monkeypatch, driver, calls, c=C_CTX, inject=True, boundary_last=False, seen=None):
    """`calls` x optimize_parameters() on one batch at learning rate zero, crop 64 inside a frame of `c` pixels (0: the option off, plain 64 x 64
    data), noise and APA on, projected + PatchGAN discriminators; driver "sequential" or "default" (no switch set); `inject`: the same z / u
    draws for every run (seeded per step), else drawn in the kernels.  Returns per call the GAN losses of both groups (independent of the
    patch ids, which the drivers draw differently), the APA state of every discriminator, its flags, and the driver."""
    from joligen_amd import ops
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    for var in ("JG_EARLY_D", "JG_GRAPH_D", "JG_GRAPH_G"):
        if driver == "sequential":
            monkeypatch.setenv(var, "0")
        else:
            monkeypatch.delenv(var, raising=False)
    monkeypatch.delenv("JG_DBG_GRAPH_CANARY_FAIL", raising=False)
    H = 64 + 2 * c
    gen = torch.Generator().manual_seed(14)
    data = {"A": torch.rand(2, 3, H, H, generator=gen) * 2 - 1, "B": torch.rand(2, 3, H, H, generator=gen) * 2 - 1}
    cfg = dict(_CUT, data=dict(_CUT["data"], online_context_pixels=c))
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
            if inject:
                gi = torch.Generator().manual_seed(100 + i)
                draws = {("z_fake", 0): torch.randn(2, 3, H, H, generator=gi), ("z_real", 0): torch.randn(2, 3, H, H, generator=gi),
                         ("u", 0): torch.rand(2, generator=gi), ("u", 1): torch.rand(2, generator=gi)}
                m.d_aug_injection = lambda kind, d, draws=draws: draws[(kind, d)].to(D0)
            m.set_input(data)
            with (ops.torch_ops_boundary() if boundary_last and i == calls - 1 else contextlib.nullcontext()), (seen or contextlib.nullcontext()):
                m.optimize_parameters()
            losses.append([float(getattr(m, "loss_" + n)) for n in names])
            drivers.append(m.step_driver)
            states.append([cc.apa_state.cpu().tolist() for cc in calcs])
            flags.append([cc.apa_flags.cpu().tolist() for cc in calcs])
    torch.cuda.synchronize()
    return dict(losses=torch.tensor(losses, dtype=torch.float64), names=names, drivers=drivers, states=states, flags=flags, note=m.step_driver_note,
                dropped=[str(w.message) for w in rec if "jg_graph_" in str(w.message)], model=m, data=data)


def test_cut_context_step_drivers_agree(monkeypatch):
    """six steps with the frame, noise and APA on and the same injected draws under the default driver (captured graphs from the third step on:
    the frame launch is part of graph F, which reads static copies of the two with-context images; the discriminator graph's static
    operands are framed) and under the sequential one: GAN losses at the forward tolerance, the same flags, p moved identically; the canaries
    passed.  Then a run without injection (the step's Philox key drawn inside graph F): finite losses, p inside [0, 1]."""
    import joligen_amd

    framed = (2, 64 + 2 * C_CTX, 64 + 2 * C_CTX, CPAD)
    seq = _run(monkeypatch, "sequential", 6)
    r = _run(monkeypatch, "default", 6)
    assert seq["drivers"] == ["sequential"] * 6 and r["drivers"][0] != "sequential", (r["drivers"], r["note"])
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert r["drivers"][2:] == ["graph+graphG"] * 4 and not r["dropped"], (r["drivers"], r["note"], r["dropped"])
        m = r["model"]
        std = next(iter(m.driver.d_half.cache.values()))
        assert len(std.reals) == 2 and std.reals[0].data_ptr() != std.reals[1].data_ptr() and len(std.preds) == 2
        assert all(tuple(t.shape) == framed for t in std.reals + std.fakes)
        stg = next(iter(m.driver.g_half.cache.values()))
        assert tuple(stg.ctx_A.shape) == tuple(stg.ctx_B.shape) == framed and tuple(stg.real_A.shape) == (2, 64, 64, CPAD)
        assert tuple(stg.outs["fake_B_with_context"].shape) == tuple(stg.outs["fake_B_with_context_noisy"].shape) == framed
        assert m.real_A_with_context.data_ptr() == stg.ctx_A.data_ptr()
        assert len({m.driver.d_stream.cuda_stream, m.driver.gan_stream.cuda_stream, m.driver.cap_stream.cuda_stream}) == 3
    assert torch.isfinite(r["losses"]).all() and torch.isfinite(seq["losses"]).all()
    err = float(((r["losses"] - seq["losses"]).abs() / seq["losses"].abs()).max())
    print("default against sequential driver, GAN losses of six steps:", err, r["drivers"])
    assert err <= TOL_LOSS_FWD[torch.bfloat16], (r["losses"], seq["losses"])
    assert r["flags"] == seq["flags"] and any(f for step in r["flags"] for d in step for f in d) and not all(f for step in r["flags"] for d in step for f in d)
    for a, b in zip(r["states"], seq["states"]):
        assert [x[:2] for x in a] == [x[:2] for x in b], (r["states"], seq["states"])            # p and adjust of every discriminator, every step
    for mm in (seq["model"], r["model"]):                                                        # the pool and the APA substitutes are framed
        assert tuple(mm.APA_img.shape) == framed and all(tuple(im.shape[1:]) == framed[1:] for im in mm.fake_B_pool.images)
    free = _run(monkeypatch, "default", 4, inject=False)
    assert torch.isfinite(free["losses"]).all() and all(0.0 <= x[0] <= 1.0 and abs(x[1]) == 1.0 for step in free["states"] for x in step)
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert free["drivers"][-1] == "graph+graphG" and not free["dropped"], (free["drivers"], free["note"])
    fm = free["model"]                       # the replayed frame: still fake_B inside, real_A_with_context around it; the noise moved the copy
    fwc = fm.fake_B_with_context
    assert torch.equal(_bits(fwc), _bits(R.frame(fm.fake_B.cpu(), fm.real_A_with_context.cpu(), C_CTX, 3)))
    assert not torch.equal(_bits(fm.fake_B_with_context_noisy), _bits(fwc))


def test_step_driver_streams_are_distinct_hip_streams():
    """torch hands its 32 pool streams out round-robin: with 31 streams created in between, the next one is the first again.  The step driver's
    streams -- discriminator half, GAN fork, capture stream of the generator graphs -- must still be four different HIP streams: the launch
    layer keys its split-K workspace by raw stream, and the discriminator half runs beside the replayed backward of the generator."""
    from types import SimpleNamespace

    from joligen_amd.models.cut_step import CUTStepDriver

    drv = CUTStepDriver(SimpleNamespace(device=torch.device(D0)))
    keep, handles = [], []
    for name in ("d_stream", "cap_stream", "gan_stream", "wg_stream"):
        handles.append(drv.stream(name).cuda_stream)
        assert drv.stream(name).cuda_stream == handles[-1]                 # created once
        keep += [torch.cuda.Stream(device=D0) for _ in range(31)]          # the pool is back at the slot just handed out
        assert keep[-1].cuda_stream != handles[-1] and torch.cuda.Stream(device=D0).cuda_stream == handles[-1]
        keep += [torch.cuda.Stream(device=D0) for _ in range(31)]
    assert len(set(handles)) == 4, [hex(h) for h in handles]


class _SeenOps(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_cut_context_step_through_torch_ops(monkeypatch):
    """a step under ops.torch_ops_boundary() sees torch.ops.jg355.context_frame exactly once (one launch: the plain and the noisy framed fake)
    and its backward once, with the losses of the ctypes path"""
    seen = _SeenOps()
    a = _run(monkeypatch, "sequential", 1)
    b = _run(monkeypatch, "sequential", 1, boundary_last=True, seen=seen)
    n_frame = sum(n == "jg355.context_frame.default" for n in seen.names)
    n_bwd = sum(n == "jg355.context_frame_bwd.default" for n in seen.names)
    n_aug = sum(n == "jg355.d_aug.default" for n in seen.names)
    assert (n_frame, n_bwd, n_aug) == (1, 1, 1), (n_frame, n_bwd, n_aug)          # (d_aug: the real operands only; the fake's noise is the frame's)
    assert float(((a["losses"] - b["losses"]).abs() / a["losses"].abs()).max()) <= TOL_LOSS_FWD[torch.bfloat16], (a["losses"], b["losses"])
    assert a["flags"] == b["flags"] and [x[:2] for x in a["states"][0]] == [x[:2] for x in b["states"][0]]


def test_cut_without_context_launches_nothing_of_it(monkeypatch):
    """c = 0: counters on ops.context_split / ops.context_frame stay at 0 over two steps of the default driver and no with-context attribute
    appears; they do count with the option on"""
    from joligen_amd import ops

    count = {"context_split": 0, "context_frame": 0}
    for k in count:
        def counted(*a, _k=k, _real=getattr(ops, k), **kw):
            count[_k] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ops, k, counted)
    r = _run(monkeypatch, "default", 2, c=0)
    m = r["model"]
    assert torch.isfinite(r["losses"]).all() and count == {"context_split": 0, "context_frame": 0}, count
    assert m.context == 0 and not hasattr(m, "fake_B_with_context") and not hasattr(m, "real_A_with_context") and hasattr(m, "fake_B_noisy")
    assert tuple(m.real_A.shape) == (2, 64, 64, CPAD) and all("context" not in n for grp in m.visual_names for n in grp)
    _run(monkeypatch, "sequential", 1)
    assert count == {"context_split": 2 * 2, "context_frame": 1}, count          # data_dependent_initialize + the step's set_input; one frame


def test_cut_context_set_input_and_visuals(monkeypatch):
    """data of the wrong size raises a ValueError that names both sizes; the four context visuals are made on demand, in the reference's
    order, resized to the crop"""
    r = _run(monkeypatch, "sequential", 1)
    m, data = r["model"], r["data"]
    for bad in (64, 64 + 2 * C_CTX + 2):
        with pytest.raises(ValueError, match=rf"\[B, C, 80, 80\] \(data_crop_size 64 \+ 2 x 8 context pixels\), got \(2, 3, {bad}, {bad}\)"):
            m.set_input({"A": torch.zeros(2, 3, bad, bad), "B": data["B"]})
    with pytest.raises(ValueError, match=r"data\['B'\]"):
        m.set_input({"A": data["A"], "B": torch.zeros(2, 3, 64, 64)})
    assert not hasattr(m, "real_A_with_context_vis") and not hasattr(m, "mask_context_vis")      # not computed per step
    m.compute_visuals(2)
    vis = m.get_current_visuals(2)[-1]
    assert list(vis) == ["real_A_with_context_vis", "real_B_with_context_vis", "fake_B_with_context_vis", "mask_context_vis"]
    assert all(tuple(vis[k].shape) == (2, 3, 64, 64) for k in list(vis)[:3]) and tuple(vis["mask_context_vis"].shape) == (2, 64, 64)
    assert torch.equal(vis["real_A_with_context_vis"].cpu(), F.interpolate(data["A"], size=(64, 64)))
    assert torch.equal(vis["real_B_with_context_vis"].cpu(), F.interpolate(data["B"], size=(64, 64)))
    assert torch.equal(vis["mask_context_vis"].cpu(), F.interpolate(R.mask_context(2, 3, 80, 80, C_CTX, dtype=torch.float32), size=(64, 64))[:, 0])
    fwc = m.fake_B_with_context.detach()[..., :3].float().permute(0, 3, 1, 2).cpu()
    assert torch.equal(vis["fake_B_with_context_vis"].cpu(), F.interpolate(fwc, size=(64, 64)))
