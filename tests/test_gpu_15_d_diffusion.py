"""GPU tests of dataaug_D_diffusion: the fused kernels (`jg_d_diffusion`, `jg_d_diffusion_bwd`, `jg_d_diffusion_update`) against the float64
restatement of tests/d_diffusion_ref.py and the fixtures recorded from the unmodified reference (tests/golden/d_diffusion/), the in-kernel
draws, the argument checks, the torch.ops surface, `ProjectedDiscriminator` with the augmentation against the reference's run, and `CUTModel`
with the option on under the step drivers and off (no launch)."""
import contextlib
import ctypes
import os
import random
import warnings

import numpy as np
import pytest
import torch

import d_diffusion_ref as R
import jg_oracle as O
from pixel_loss_ref import ordered_bits
from test_d_diffusion_host import A_REL, B_REL, WIDTHS, check_tables
from test_oracle_golden import projd_state

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "d_diffusion")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
HWS = (8, 4, 2, 1)
# forward-only tolerance of the losses of a CUT step at identical weights (test_gpu_5_cutloss.py::TOL_LOSS_FWD)
TOL_LOSS_FWD = {torch.float16: 6e-3, torch.bfloat16: 4e-2}
KEY = (0x1234ABCD, 0x0F1E2D3C)


def _load(name):
    return torch.load(os.path.join(DIR, name), weights_only=False)


def _key(words=KEY):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy()).to(D0)


def make_state(T=None, n=None, t_epl=None, p=0.0):
    """a DDiffusionState on the device: fresh (p = 0), or the restated tables of T with `t_epl`"""
    from joligen_amd import ops

    st = ops.DDiffusionState.fresh(D0)
    if T is not None:
        a, b = R.tables(T)
        st.a.copy_(torch.from_numpy(a).float())
        st.b.copy_(torch.from_numpy(b).float())
        st.Tn.copy_(torch.tensor([T, n if n is not None else 0], dtype=torch.int32))
        st.p.fill_(p)
        if t_epl is not None:
            st.t_epl.copy_(torch.as_tensor(t_epl, dtype=torch.int32))
    return st


_SHARED = {}


def shared_state():
    """T = 188 (p = 0.37) with 24 drawn entries of t_epl: computed once, read by every test that needs a noisy state"""
    if "st" not in _SHARED:
        u = np.random.default_rng(3).random(64).astype(np.float32)
        _SHARED["t_epl"] = R.t_epl(u, 188, 24)
        _SHARED["st"] = make_state(188, 24, _SHARED["t_epl"], 0.37)
    return _SHARED["st"], _SHARED["t_epl"]


def kernel_inputs(B, shapes, dtype, t_epl, seed=7):
    """per level (C, H, W): x NHWC 16-bit, dy NHWC 16-bit, t int32 [B, C] from t_epl, z fp32 [B, C, H, W] (CPU tensors)"""
    g = torch.Generator().manual_seed(seed + B)
    xs, dys, ts, zs = [], [], [], []
    for C, H, W in shapes:
        xs.append(torch.randn(B, H, W, C, generator=g).to(dtype))
        dys.append(torch.randn(B, H, W, C, generator=g).to(dtype))
        ts.append(torch.as_tensor(t_epl)[torch.randint(0, 64, (B, C), generator=g)].to(torch.int32))
        zs.append(torch.randn(B, C, H, W, generator=g))
    return xs, dys, ts, zs


def run_case(B, shapes, dtype, what):
    from joligen_amd import ops

    st, t_epl = shared_state()
    xs, dys, ts, zs = kernel_inputs(B, shapes, dtype, t_epl)
    xd = [x.to(D0).requires_grad_(True) for x in xs]
    outs, tu = ops.d_diffusion(xd, st, 0.5, ts=[t.to(D0) for t in ts], zs=[z.to(D0) for z in zs])
    torch.autograd.backward(outs, [d.to(D0) for d in dys])
    torch.cuda.synchronize()
    a, b = st.a.cpu().numpy(), st.b.cpu().numpy()
    worst = [0, 0]
    for l, (x, dy, t, z) in enumerate(zip(xs, dys, ts, zs)):
        assert torch.equal(tu[l].cpu(), t) and tu[l].dtype == torch.int32
        nchw = lambda v: v.permute(0, 3, 1, 2).double().numpy()
        ref = torch.from_numpy(R.q_sample(nchw(x), a, b, t.numpy(), z.numpy(), 0.5)).permute(0, 2, 3, 1).to(dtype)
        rdx = torch.from_numpy(R.q_sample_bwd(nchw(dy), a, t.numpy())).permute(0, 2, 3, 1).to(dtype)
        out, dx = outs[l].detach().cpu(), xd[l].grad.cpu()
        assert out.dtype == dtype and out.shape == x.shape and torch.isfinite(out).all()
        uf = (ordered_bits(out.contiguous()) - ordered_bits(ref.contiguous())).abs()
        ub = (ordered_bits(dx.contiguous()) - ordered_bits(rdx.contiguous())).abs()
        worst = [max(worst[0], int(uf.max())), max(worst[1], int(ub.max()))]
        assert int((t > 0).sum()) > 0 and not torch.equal(out, x)               # noise is present
        zero = (t == 0)[:, None, None, :].expand_as(x)                           # t = 0 channels: the input bit for bit
        assert torch.equal(out[zero].view(torch.int16), x[zero].view(torch.int16))
    print(f"d_diffusion {what} B={B} {dtype}: max ulp forward {worst[0]}, backward {worst[1]}")
    assert worst[0] <= 1 and worst[1] <= 1, worst          # one rounding of an fp32 result: one unit in the last place of the storage type


LITE0 = [(c, s, s) for c, s in zip(WIDTHS, HWS)]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("levels", [4, 1, 2])
def test_d_diffusion_kernel_vs_float64_restatement(levels, B, dtype_name):
    """the four lite0 widths at 8x8, 4x4, 2x2, 1x1 (odd totals: a partial last block), and one / two levels"""
    run_case(B, LITE0[:levels] if levels != 2 else LITE0[1:3], DTYPES[dtype_name], f"{levels} level(s)")


def test_d_diffusion_grid_stride_second_trip():
    """one level whose 16-byte groups exceed the launch's grid cap: the grid-stride loop takes a second (partial) trip"""
    from joligen_amd import ops

    cap = ops.d_diffusion_grid_cap()
    C, H = 24, 420                                   # B * H * H * C / 8 = 1 058 400 groups against a cap of 4096 blocks x 256 threads
    B = 2
    groups = B * H * H * C // 8
    assert cap < groups < 2 * cap, (cap, groups)
    run_case(B, [(C, H, H)], torch.float16, "over the grid cap")


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_d_diffusion_fresh_state_is_the_identity(dtype_name):
    from joligen_amd import ops

    dtype = DTYPES[dtype_name]
    st = make_state()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(3, s, s, c, generator=g).to(dtype) for c, s in zip(WIDTHS, HWS)]
    xs[0][0, 0, 0, :4] = torch.tensor([0.0, -0.0, 6e-8, -6e-8]).to(dtype)           # signed zeros and subnormals pass as they are
    outs, tu = ops.d_diffusion([x.to(D0) for x in xs], st, 0.5, key=_key())
    for x, o, t in zip(xs, outs, tu):
        assert torch.equal(o.cpu().view(torch.int16), x.view(torch.int16)) and int(t.abs().sum()) == 0


def test_d_diffusion_drawn_mode():
    """drawn t: entries of t_epl, each of 64 distinct entries within 5 binomial standard deviations; drawn noise: (out - a x) / (0.5 b) has
    mean 0 and variance 1 within 5 standard errors; another key, other draws; the same key, the same bits"""
    from joligen_amd import ops

    dist = np.arange(64) * 7 + 2                     # 64 distinct values in 2..443
    st = make_state(500, 48, dist, 1.0)
    B, C = 40, 320                                   # B * C = 12800 draws
    x = torch.zeros(B, 2, 2, C, device=D0, dtype=torch.float16)
    (o1,), (t1,) = ops.d_diffusion([x], st, 0.5, key=_key())
    t = t1.cpu().numpy().ravel()
    assert set(t.tolist()) <= set(dist.tolist())
    counts = np.array([(t == v).sum() for v in dist])
    n, q = B * C, 1.0 / 64
    sd = np.sqrt(n * q * (1 - q))
    print("t counts: min", counts.min(), "max", counts.max(), "expected", n * q, "5 sd", 5 * sd)
    assert (np.abs(counts - n * q) <= 5 * sd).all(), counts
    # constant t_epl: the normals behind the output
    tc = 300
    st2 = make_state(500, 48, np.full(64, tc), 1.0)
    B, C, H = 2, 320, 16
    x = torch.zeros(B, H, H, C, device=D0, dtype=torch.float16)
    (o,), (tt,) = ops.d_diffusion([x], st2, 0.5, key=_key())
    assert bool((tt == tc).all())
    bt = float(st2.b[tc])
    z = (o.float() / (0.5 * bt)).double().cpu().numpy()
    N = z.size
    m, v = z.mean(), z.var()
    print(f"drawn normals: N {N} mean {m:.3e} (5 se {5 / np.sqrt(N):.3e}) variance - 1 {v - 1:.3e} (5 se {5 * np.sqrt(2 / N):.3e})")
    assert abs(m) <= 5 / np.sqrt(N) and abs(v - 1) <= 5 * np.sqrt(2 / N)
    (o_same,), _ = ops.d_diffusion([x], st2, 0.5, key=_key())
    (o_other,), _ = ops.d_diffusion([x], st2, 0.5, key=_key((1, 2)))
    (o_call,), _ = ops.d_diffusion([x], st2, 0.5, key=_key(), call=1)
    assert torch.equal(o, o_same) and not torch.equal(o, o_other) and not torch.equal(o, o_call)
    # levels do not share draws: the same map at two levels of one launch
    xs = [x[:, :2, :2].contiguous(), x[:, :2, :2].contiguous()]
    (a0, a1), (t0, t1b) = ops.d_diffusion(xs, make_state(500, 48, dist, 1.0), 0.5, key=_key())
    assert not torch.equal(a0, a1) and not torch.equal(t0, t1b)


def test_d_diffusion_update_kernel():
    """along the sequences recorded from the reference: p, T, n bit-equal; tables within the two bounds of the host test; t_epl equal to the
    restatement with injected u; with drawn u entries [0, n) in 2..T and [n, 64) zero"""
    from joligen_amd import ops

    g = _load("diffusion_fn.pt")
    rng = np.random.default_rng(5)
    ref_tabs = {t["T"]: t for t in g["tables"]}
    for useq in g["updates"]:
        st = make_state()
        for i, s in enumerate(useq["steps"]):
            u = rng.random(64).astype(np.float32)
            loss = s["loss"].to(D0)
            p0 = float(st.p)
            ops.d_diffusion_update(st, loss, useq["B"] * useq["every"], u=torch.from_numpy(u).to(D0))
            torch.cuda.synchronize()
            p, (T, n) = st.p.cpu(), st.Tn.cpu().tolist()
            assert p.numpy().tobytes() == s["p"].reshape(1).numpy().tobytes(), (i, float(p), float(s["p"]))
            assert (T, n) == (s["T"], s["n"]), (i, T, n, s["T"], s["n"])
            rp, rT, rn, ra, rb, rt = R.update(np.float32(p0), s["loss"].numpy(), useq["B"] * useq["every"], u)
            a, b = st.a.cpu().numpy(), st.b.cpu().numpy()
            check_tables(a, b, ra[:T + 1], rb[:T + 1], T)                   # against the restatement
            if T in ref_tabs:                                               # and against the reference's own tables where recorded
                check_tables(a, b, ref_tabs[T]["a"].numpy(), ref_tabs[T]["b"].numpy(), T)
            assert (a[T + 1:] == 0).all() and (b[T + 1:] == 0).all()
            assert st.t_epl.cpu().tolist() == rt.tolist(), (i, T, n)
    # the reference's tables for every recorded p, reached from p by an update with loss == 0.9 (adjust = 0)
    for t in g["tables"]:
        st = make_state()
        st.p.fill_(float(t["p"]))
        ops.d_diffusion_update(st, torch.tensor(0.9, device=D0), 8, key=_key())
        T, n = st.Tn.cpu().tolist()
        assert st.p.cpu().numpy().tobytes() == np.float32(float(t["p"])).tobytes() and (T, n) == (t["T"], t["n"])
        ea, eb = check_tables(st.a.cpu().numpy(), st.b.cpu().numpy(), t["a"].numpy(), t["b"].numpy(), T)
        print(f"update kernel p={float(t['p']):.6f} T={T} n={n}: a {ea:.3e} (bound {A_REL}) b {eb:.3e} (bound {B_REL})")
        te = st.t_epl.cpu().numpy()
        assert ((te[:n] >= 2) & (te[:n] <= T)).all() and (te[n:] == 0).all()
        st2 = make_state()
        st2.p.fill_(float(t["p"]))
        ops.d_diffusion_update(st2, torch.tensor(0.9, device=D0), 8, key=_key((5, 6)))
        assert n == 0 or not torch.equal(st.t_epl, st2.t_epl)              # another key, another t_epl
    # a loss that is not a number leaves p where it is
    st = make_state()
    st.p.fill_(0.25)
    ops.d_diffusion_update(st, torch.tensor(float("nan"), device=D0), 1000, key=_key())
    assert float(st.p) == 0.25 and st.Tn.cpu().tolist() == list(R.T_n(0.25))


def test_d_diffusion_argument_checks():
    """the C entry points answer with an error code before any launch (the outputs keep their sentinel); the Python surface raises"""
    from joligen_amd import _lib, ops

    lib = _lib.lib()
    B, H, W, C = 2, 4, 4, 24
    st = make_state()
    x = torch.ones(B, H, W, C, device=D0, dtype=torch.float16)
    out, t_out = torch.full_like(x, 5.0), torch.full((B, C), 9, device=D0, dtype=torch.int32)
    t_in, z, key = torch.zeros(B, C, device=D0, dtype=torch.int32), torch.zeros(B, C, H, W, device=D0), _key()
    arr = lambda *ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)

    def call(xs=arr(x.data_ptr()), outs=arr(out.data_ptr()), tos=arr(t_out.data_ptr()), tis=arr(t_in.data_ptr()), zs=arr(z.data_ptr()), Hs=ints(H),
             Ws=ints(W), Cs=ints(C), nl=1, dtype=0, Bn=B, a=st.a.data_ptr(), b=st.b.data_ptr(), te=st.t_epl.data_ptr(), ns=0.5, keyp=None):
        return lib.jg_d_diffusion(dtype, nl, xs, outs, tos, tis, zs, Hs, Ws, Cs, Bn, a, b, te, ns, keyp, 0, None)

    bad = [dict(Cs=ints(20)), dict(Cs=ints(0)), dict(Cs=ints(4)), dict(nl=0), dict(nl=5), dict(dtype=2), dict(xs=None), dict(outs=None), dict(tos=None),
           dict(xs=arr(None)), dict(outs=arr(None)), dict(tos=arr(None)), dict(xs=arr(x.data_ptr() + 2)), dict(outs=arr(out.data_ptr() + 2)),
           dict(outs=arr(x.data_ptr())), dict(tos=arr(t_in.data_ptr())), dict(Hs=ints(0)), dict(Ws=ints(0)), dict(Bn=0), dict(a=None), dict(b=None),
           dict(te=None), dict(ns=float("nan")), dict(tis=None), dict(zs=None), dict(zs=arr(None)), dict(tis=arr(None)), dict(Hs=None), dict(Cs=None)]
    for kw in bad:
        assert call(**kw) == _lib.JG_ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((t_out == 9).all())                  # nothing was launched
    assert call() == _lib.JG_OK and call(tis=None, zs=None, keyp=key.data_ptr()) == _lib.JG_OK
    torch.cuda.synchronize()
    assert bool((out == 1.0).all()) and bool((t_out == 0).all())
    dx = torch.full_like(x, 5.0)

    def bwd(dys=arr(x.data_ptr()), dxs=arr(dx.data_ptr()), ts=arr(t_in.data_ptr()), Cs=ints(C), nl=1, dtype=0, a=st.a.data_ptr()):
        return lib.jg_d_diffusion_bwd(dtype, nl, dys, dxs, ts, ints(H), ints(W), Cs, B, a, None)

    for kw in (dict(Cs=ints(12)), dict(nl=0), dict(nl=5), dict(dtype=3), dict(dys=None), dict(dxs=arr(None)), dict(ts=arr(None)), dict(a=None),
               dict(dxs=arr(x.data_ptr()))):
        assert bwd(**kw) == _lib.JG_ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert bool((dx == 5.0).all())
    assert bwd() == _lib.JG_OK
    loss, u = torch.tensor([1.0], device=D0), torch.full((64,), 0.5, device=D0)

    def upd(p=st.p.data_ptr(), Tn=st.Tn.data_ptr(), a=st.a.data_ptr(), b=st.b.data_ptr(), te=st.t_epl.data_ptr(), lp=loss.data_ptr(), num=8.0, den=1e5,
            up=u.data_ptr(), keyp=None):
        return lib.jg_d_diffusion_update(p, Tn, a, b, te, lp, num, den, up, keyp, 0, None)

    for kw in (dict(p=None), dict(Tn=None), dict(a=None), dict(b=None), dict(te=None), dict(lp=None), dict(num=-1.0), dict(den=0.0), dict(up=None),
               dict(num=float("nan"))):
        assert upd(**kw) == _lib.JG_ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert float(st.p) == 0.0 and st.Tn.cpu().tolist() == [5, 0]
    assert upd() == _lib.JG_OK
    torch.cuda.synchronize()
    assert st.p.cpu().numpy().tobytes() == np.float32(R.update_p(0.0, 1.0, 8.0)).tobytes()
    # the Python surface
    st = make_state()
    for args, kw, exc in ((([x[..., :20].contiguous()], st, 0.5), dict(key=key), RuntimeError), (([x] * 5, st, 0.5), dict(key=key), ValueError),
                          (([x], st, 0.5), dict(ts=[t_in.long()], zs=[z]), TypeError), (([x], st, 0.5), dict(ts=[t_in], zs=[z[:1]]), TypeError),
                          (([x], st, 0.5), dict(ts=[t_in, t_in], zs=[z]), ValueError), (([x], st, 0.5), dict(key=key.float()), TypeError),
                          (([x, x.bfloat16()], st, 0.5), dict(key=key), TypeError), (([x], st, 0.5), {}, RuntimeError)):
        with pytest.raises(exc, match="d_diffusion"):
            ops.d_diffusion(*args, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.d_diffusion([x.cpu()], st, 0.5, key=key)
    bad_state = ops.DDiffusionState(st.p, st.Tn, st.a[:100], st.b, st.t_epl)
    with pytest.raises(TypeError, match="state.a"):
        ops.d_diffusion([x], bad_state, 0.5, key=key)
    with pytest.raises(TypeError, match="d_diffusion_update"):
        ops.d_diffusion_update(st, torch.tensor(1.0, device=D0, dtype=torch.float64), 8)
    with pytest.raises(TypeError, match="d_diffusion_update"):
        ops.d_diffusion_update(st, torch.tensor(1.0, device=D0), 8, u=u[:8])


def test_d_diffusion_torch_ops_opcheck_and_boundary():
    """schema, fake kernels and autograd registration of torch.ops.jg355.d_diffusion / d_diffusion_bwd / d_diffusion_update; `ops.d_diffusion` and
    `ops.d_diffusion_update` under the boundary are bit-equal to the ctypes path, gradients included"""
    from joligen_amd import ops

    J = torch.ops.jg355
    st, t_epl = shared_state()
    xs, dys, ts, zs = kernel_inputs(2, LITE0[1:3], torch.bfloat16, t_epl)
    xs, dys, ts, zs = ([v.to(D0) for v in grp] for grp in (xs, dys, ts, zs))
    key = _key()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(J.d_diffusion.default, ([x.clone().requires_grad_(True) for x in xs], st.a, st.b, st.t_epl, 0.5, None, ts, zs, 0), test_utils=utils)
    torch.library.opcheck(J.d_diffusion.default, (xs, st.a, st.b, st.t_epl, 0.5, key, [], [], 1), test_utils=utils[:2])
    torch.library.opcheck(J.d_diffusion_bwd.default, (dys, ts, st.a), test_utils=("test_schema", "test_faketensor"))
    s1 = make_state()
    torch.library.opcheck(J.d_diffusion_update.default, (*s1.tensors(), torch.tensor([1.0], device=D0), 8.0, 1e5, None, key, 0),
                          test_utils=("test_schema", "test_faketensor"))
    for kw in (dict(ts=ts, zs=zs), dict(key=key)):
        res = []
        for boundary in (False, True):
            xd = [x.clone().requires_grad_(True) for x in xs]
            with (ops.torch_ops_boundary() if boundary else contextlib.nullcontext()):
                outs, tu = ops.d_diffusion(xd, st, 0.5, **kw)
                torch.autograd.backward(outs, dys)
            res.append((outs, tu, [x.grad for x in xd]))
        for grp_a, grp_b in zip(*res):
            assert all(torch.equal(a, b) for a, b in zip(grp_a, grp_b))
        assert all(g is not None and not torch.equal(g, d) for g, d in zip(res[1][2], dys))
    sa, sb = make_state(), make_state()
    u = torch.rand(64, device=D0)
    for s in (sa, sb):
        s.p.fill_(0.5)
    ops.d_diffusion_update(sa, torch.tensor(1.5, device=D0), 1000, u=u)
    with ops.torch_ops_boundary():
        ops.d_diffusion_update(sb, torch.tensor(1.5, device=D0), 1000, u=u)
    assert all(torch.equal(a, b) for a, b in zip(sa.tensors(), sb.tensors())) and float(sa.p) == float(R.update_p(0.5, 1.5, 1000))


# ---- the projected discriminator -------------------------------------------------------------------------------------------------------------
def load_state_from_fixture(dif, state):
    """the reference's state (tables of T + 1 entries) into the module's device buffers"""
    T = state["T"]
    dif.p.fill_(float(state["p"]))
    dif.Tn.copy_(torch.tensor([T, state["n"]], dtype=torch.int32))
    for buf, ref in ((dif.alphas_bar_sqrt, state["a"]), (dif.one_minus_alphas_bar_sqrt, state["b"])):
        buf.zero_()
        buf[:T + 1].copy_(ref)
    dif.t_epl.copy_(state["t_epl"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_projected_discriminator_with_diffusion_vs_reference_golden(dtype):
    """the sequence of tests/test_gpu_6_projd.py::test_projected_discriminator_vs_reference_golden on projd_diffusion.pt: the reference ran
    with diffusion_aug=True at p = 0.37; its state and the recorded draws of each of the three forwards are injected (a forward pre-hook swaps
    them).  Same bounds and the same measured-floor rule as that test applies to projd.pt (same backbone, weights and inputs: the floor of
    projd.pt in profiles/r03_rounding_yardstick_projd.json).  Then `update`: p, T and n equal the reference's."""
    from joligen_amd import ops
    from joligen_amd.modules.projected_d import ProjectedDiscriminator, hinge_loss
    from test_gpu_6_projd import _yard, relerr

    g = _load("projd_diffusion.pt")
    c = g["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = ProjectedDiscriminator("efficientnet", interp=c["interp"], img_size=c["S"], backbone="standin", diffusion_aug=True)
    assert list(net.state_dict().keys()) == g["keys"]
    net.load_state_dict(projd_state(g, 5))
    net.jg_finalize(torch.device(D0), dtype)
    net.train()
    dif = net.freeze_feature_network.diffusion
    load_state_from_fixture(dif, g["state"])
    calls = []

    def swap(mod, args):
        dr = g["draws"][len(calls)]
        mod.inject_t, mod.inject_z = [t.to(D0).contiguous() for t in dr["t"]], [z.to(D0).contiguous() for z in dr["z"]]
        calls.append(1)

    dif.register_forward_pre_hook(swap)
    for n, p in net.named_parameters():
        p.requires_grad_(not n.startswith("freeze"))
    yard = _yard("projd.pt", dtype)
    real = ops.to_nhwc(g["real"].to(D0), dtype, 8)
    fake = ops.to_nhwc(g["fake"].to(D0), dtype, 8)
    pred_real = net(real)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dif.t_used, g["draws"][0]["t"]))
    pred_fake = net(fake)
    assert tuple(pred_real.shape) == tuple(g["pred_real"].shape)
    tol = 6e-3 if dtype == torch.float16 else 4e-2
    print("pred_real", relerr(pred_real, g["pred_real"]), "bound", tol)
    assert relerr(pred_real, g["pred_real"]) < tol, relerr(pred_real, g["pred_real"])
    loss_real = hinge_loss(pred_real, True)
    loss_D = (loss_real + hinge_loss(pred_fake, False)) * 0.5
    print("loss_D", float(loss_D), float(g["loss_D"]), "loss_D_real", float(loss_real), float(g["loss_D_real"]))
    assert abs(float(loss_D) - float(g["loss_D"])) < tol * abs(float(g["loss_D"]))
    net.arena.g.zero_()
    loss_D.backward()
    torch.cuda.synchronize()
    bad = []
    P = dict(net.named_parameters())
    for k, ref in g["grad_checks"].items():
        v = P[k].grad.detach().float().cpu()
        mine = torch.stack([v.norm(), (v * O.projection_vector(k, v.shape)).sum()])
        t = max(4 * tol, 0.08, 2.0 * yard["grad_worst"]) * float(ref[0]) + 1e-7      # >= twice the measured rounding floor
        if abs(float(mine[0] - ref[0])) > t or abs(float(mine[1] - ref[1])) > 2 * t * max(1.0, v.numel() ** 0.5 / 4):
            bad.append((k, mine.tolist(), ref.tolist()))
    assert not bad, bad[:6]
    fk = ops.to_nhwc(g["fake"].to(D0), dtype, 8).requires_grad_(True)
    loss_G = hinge_loss(net(fk), True, relu=False)
    assert len(calls) == 3
    print("loss_G", float(loss_G), float(g["loss_G"]))
    assert abs(float(loss_G) - float(g["loss_G"])) < tol * abs(float(g["loss_G"])) + 2e-3
    ls = 1024.0 if dtype == torch.float16 else 1.0
    (loss_G * ls).backward()
    dfk = fk.grad.permute(0, 3, 1, 2)[:, :3].float() / ls
    print("dfake", relerr(dfk, g["dfake"]), "bound", 2.0 * yard["dfake_rel"])
    assert relerr(dfk, g["dfake"]) < 2.0 * yard["dfake_rel"], (relerr(dfk, g["dfake"]), yard["dfake_rel"])
    # the update on the device scalar: sign(loss_D_real - 0.9) as in the reference (the fixture keeps 0.05 of margin)
    dif.update(loss_real.detach(), c["B"] * c["every"])
    torch.cuda.synchronize()
    assert dif.p.cpu().numpy().tobytes() == g["after"]["p"].reshape(1).numpy().tobytes(), (float(dif.p), float(g["after"]["p"]))
    assert dif.Tn.cpu().tolist() == [g["after"]["T"], g["after"]["n"]]
    assert "p" not in net.state_dict() and not any("diffusion" in k for k in net.state_dict())


# ---- the model ------------------------------------------------------------------------------------------------------------------------
_CUT = {"model_type": "cut", "G": {"netG": "resnet", "ngf": 32, "nblocks": 2}, "D": {"netDs": ["projected_d", "basic"], "ndf": 32, "proj_interp": 128},
        "alg": {"cut": {"nce_layers": "0,4,8", "nce_loss": "patchnce", "num_patches": 128}}, "data": {"crop_size": 64, "load_size": 64},
        "dataaug": {"D_diffusion": True, "D_diffusion_every": 1},
        "train": {"batch_size": 2, "G_ema": True, "iter_size": 1, "pool_size": 4, "G_lr": 0.0, "D_lr": 0.0}}
P_START = 0.37


def _run(monkeypatch, driver, calls, on=True, inject=True, boundary_last=False, seen=None):
    """`calls` x optimize_parameters() on one batch at learning rate zero with the option on (`on`), projected + PatchGAN discriminators, the
    64-pixel crop the other CUT driver tests use; driver "sequential" or "default" (no switch set).  The state starts at p = 0.37 (noise is
    present); `inject`: the same t / z / u draws in every forward and update (static tensors: a captured graph keeps reading them), else drawn
    in the kernels.  Returns per call the GAN losses of both groups, loss_D_real of the projected discriminator, p / T / n, and the driver."""
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
        calc = m.D_B_projected_d_loss_calculator
        # loss_D_real > 0.9 for the whole run, by the initial state: the logits of this seed are positive on average (hinge loss 0.8); the last
        # convolution of every mini-discriminator has no bias, so negating its weight negates the logits (sigma is unchanged): loss ~ 1.2
        with torch.no_grad():
            for disc in m.netD_B_projected_d.discriminator.mini_discs.values():
                disc.main[-1].weight_orig.neg_()
        m.netD_B_projected_d.arena.dirty = True
        dif = None
        if on:
            dif = m.netD_B_projected_d.freeze_feature_network.diffusion
            gi = torch.Generator().manual_seed(100)
            dif.p.fill_(P_START)                      # the state of p = 0.37 from the update kernel itself (loss == 0.9: p stays)
            ops.d_diffusion_update(dif.state, torch.tensor(0.9, device=D0), 0, u=torch.rand(64, generator=gi).to(D0))
            if inject:
                te = dif.t_epl.cpu()
                dif.inject_t = [te[torch.randint(0, 64, (2, c), generator=gi)].to(D0).contiguous() for c in WIDTHS]
                dif.inject_z = [torch.randn(2, c, 128 // s, 128 // s, generator=gi).to(D0) for c, s in zip(WIDTHS, (4, 8, 16, 32))]
                dif.inject_u = torch.rand(64, generator=gi).to(D0)
        losses, drivers, states, lreal = [], [], [], []
        for i in range(calls):
            m.set_input(data)
            with (ops.torch_ops_boundary() if boundary_last and i == calls - 1 else contextlib.nullcontext()), (seen or contextlib.nullcontext()):
                m.optimize_parameters()
            losses.append([float(getattr(m, "loss_" + n)) for n in names])
            drivers.append(m.step_driver)
            lreal.append(float(calc.loss_D_real))
            if on:
                states.append((dif.p.cpu().numpy().tobytes(), dif.Tn.cpu().tolist()))
    torch.cuda.synchronize()
    return dict(losses=torch.tensor(losses, dtype=torch.float64), names=names, drivers=drivers, states=states, lreal=lreal, note=m.step_driver_note,
                dropped=[str(w.message) for w in rec if "jg_graph_" in str(w.message)], model=m)


def test_cut_d_diffusion_step_drivers_agree(monkeypatch):
    """six steps with the option on and the same injected draws under the default driver (captured graphs from the third step on: the noising
    runs INSIDE both graphs, the update eagerly after them, rewriting the state they read) and under the sequential one: GAN losses at the
    forward tolerance; loss_D_real > 0.9 throughout, so p after the six steps is six increments exactly under both drivers -- the update
    kernel read the loss of each replay.  Then a run without injection (keys from torch's generator inside the graphs): finite, the same p."""
    import joligen_amd

    seq = _run(monkeypatch, "sequential", 6)
    r = _run(monkeypatch, "default", 6)
    assert seq["drivers"] == ["sequential"] * 6 and r["drivers"][0] != "sequential", (r["drivers"], r["note"])
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert r["drivers"][2:] == ["graph+graphG"] * 4 and not r["dropped"], (r["drivers"], r["note"], r["dropped"])
    assert torch.isfinite(r["losses"]).all() and torch.isfinite(seq["losses"]).all()
    err = float(((r["losses"] - seq["losses"]).abs() / seq["losses"].abs()).max())
    print("default against sequential driver, GAN losses of six steps:", err, r["drivers"], "loss_D_real", seq["lreal"], r["lreal"])
    assert err <= TOL_LOSS_FWD[torch.bfloat16], (r["losses"], seq["losses"])
    assert min(seq["lreal"] + r["lreal"]) > 0.95, (seq["lreal"], r["lreal"])          # far enough above 0.9 for bf16 rounding not to matter
    p, want = np.float32(P_START), []
    for _ in range(6):
        p = R.update_p(p, 1.0, 2 * 1)
        want.append((np.float32(p).tobytes(), list(R.T_n(p))))
    assert seq["states"] == want and r["states"] == want, (seq["states"], r["states"], want)
    free = _run(monkeypatch, "default", 4, inject=False)
    assert torch.isfinite(free["losses"]).all() and free["states"] == want[:4]
    if joligen_amd.HIP_GRAPHS_SAFE:
        assert free["drivers"][-1] == "graph+graphG" and not free["dropped"], (free["drivers"], free["note"])
    # the noise is there: the projected discriminator's losses differ from a run with the option off
    off = _run(monkeypatch, "sequential", 1, on=False)
    assert abs(float(off["losses"][0, 2]) - float(seq["losses"][0, 2])) > 1e-3 * abs(float(off["losses"][0, 2]))


class _SeenOps(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_cut_d_diffusion_step_through_torch_ops(monkeypatch):
    """a step under ops.torch_ops_boundary() with the option on goes through torch.ops.jg355.d_diffusion (three forwards of the projected
    discriminator) and d_diffusion_update, with the losses and the state of the ctypes path"""
    a = _run(monkeypatch, "sequential", 1)
    seen = _SeenOps()
    b = _run(monkeypatch, "sequential", 1, boundary_last=True, seen=seen)
    n_fwd = sum("jg355.d_diffusion.default" in n for n in seen.names)
    n_upd = sum("jg355.d_diffusion_update" in n for n in seen.names)
    assert (n_fwd, n_upd) == (3, 1), (n_fwd, n_upd)
    assert float(((a["losses"] - b["losses"]).abs() / a["losses"].abs()).max()) <= TOL_LOSS_FWD[torch.bfloat16], (a["losses"], b["losses"])
    assert a["states"] == b["states"]


def test_cut_default_step_launches_no_d_diffusion(monkeypatch):
    """with the option off nothing new is launched: counters on ops.d_diffusion / ops.d_diffusion_update / ops.d_aug_key stay at 0 over two steps"""
    from joligen_amd import ops

    count = {"d_diffusion": 0, "d_diffusion_update": 0, "d_aug_key": 0}
    for k in count:
        def counted(*a, _k=k, _real=getattr(ops, k), **kw):
            count[_k] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ops, k, counted)
    r = _run(monkeypatch, "default", 2, on=False)
    assert torch.isfinite(r["losses"]).all() and count == {"d_diffusion": 0, "d_diffusion_update": 0, "d_aug_key": 0}, count
    assert not hasattr(r["model"].netD_B_projected_d.freeze_feature_network, "diffusion") and r["model"].d_diffusion is False
    _run(monkeypatch, "sequential", 1, inject=False)      # (the counters do count when the option is on: three forwards, the step's update + _run's own)
    assert count == {"d_diffusion": 3, "d_diffusion_update": 2, "d_aug_key": 4}, count
