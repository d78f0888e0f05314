"""GPU tests of G_dropout in the diffusion UNet: the two kernels of csrc/dropout.hip for a dropout behind a low-resolution GroupNorm + nearest 2x
upsample (jg_gn_apply_drop_up2, jg_drop_pool2_bwd) on canary-guarded, strided operands (tests/strided_util.py); the fused schedule with the
mask in its GroupNorm 2 passes (jg355::unet_fused_drop) against the module-by-module graph on the same drawn key; eval mode; the torch.ops
surface; one consistency-model (cm, ect) and one cm_gan loss + backward on both graphs; three palette and three cm steps against fixtures recorded
from the unmodified reference with its Dropout draws (tests/golden/unet_dropout/, tests/tools/make_fixture_unet_dropout.py), teacher-forced by
the CPU oracle with the same masks (tests/unet_dropout_oracle.py), on the fused schedule, the module graph and under torch_ops_boundary().

Bounds.  jg_gn_apply_drop_up2 computes the fp32 expression of jg_gn_apply_drop and rounds once: bit-equal to that kernel on the materialised
upsample.  jg_drop_pool2_bwd: four products with exactly 0 or 1 / keep summed in fp32 and rounded once, against the fp32 torch formula on the
same 16-bit inputs, at the project's single-kernel bound 3e-3 (fp16) / 2e-2 (bf16) (tests/test_gpu_4_segformer.py:16).  Schedules: the bounds of
tests/test_gpu_1_model.py::test_fused_schedule_matches_module_graph, whose configuration this is: the two graphs run the same mask (it is a
function of key, stream, call and position alone), so dropout adds no term of its own to their difference."""
import pytest
import torch

import strided_util as su

pytestmark = pytest.mark.gpu
D0 = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
KTOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}            # tests/test_gpu_4_segformer.py:16
GUARD = 3
BAD = -1                                                       # JG_ERR_BAD_ARG (include/jg355.h)
# (B, H, W, C, left, right) at the LOW resolution: one 16-byte group per pixel | five groups inside a wider row (pixel stride 56); odd,
# non-square, a ragged last block
S_C8, S_C40 = (2, 3, 5, 8, 0, 0), (2, 3, 5, 40, 8, 8)
# more 16-byte groups of low-resolution pixels than jg_dropout_grid_cap(): the grid-stride loop takes a second trip
S_BIG = (3, 48, 48, 1280)


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _key(words=(0x1234ABCD, 0x8F1E2D3C)):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32, device=D0)


def _ld(v):
    assert v.stride(-1) == 1
    return v.stride(-2)


def _p(t):
    return None if t is None else t.data_ptr()


def _silu():
    from joligen_amd import _lib

    return _lib.JG_ACT_SILU


def _raw_up2(x, ab, y, act, keep, u, key, stream, call):
    from joligen_amd import _lib, ops

    B, H, W, C = x.shape
    return _lib.lib().jg_gn_apply_drop_up2(ops._dt(x), _p(x), _ld(x), _p(ab), _p(y), _ld(y), B, H, W, C, act, keep, _p(u), _p(key), stream, call, ops._st())


def _raw_pool(dy, g, keep, u, key, stream, call):
    from joligen_amd import _lib, ops

    B, H, W, C = g.shape
    return _lib.lib().jg_drop_pool2_bwd(ops._dt(dy), _p(dy), _ld(dy), _p(g), _ld(g), B, H, W, C, keep, _p(u), _p(key), stream, call, ops._st())


def _ab(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack((torch.rand((B, C), generator=g) + 0.5, torch.randn((B, C), generator=g) * 0.3), dim=-1).contiguous().to(D0)


def _cell_sum(t):
    B, H2, W2, C = t.shape
    return t.reshape(B, H2 // 2, 2, W2 // 2, 2, C).sum(dim=(2, 4))


@pytest.mark.parametrize("injected", [True, False], ids=["u", "drawn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [S_C8, S_C40], ids=["3x5x8", "3x5x40_ld56"])
def test_apply_drop_up2_is_apply_drop_on_the_upsample(shape, dtype, injected):
    from joligen_amd import launch
    from joligen_amd.modules import unet_exec

    B, H, W, C, left, right = shape
    keep = 0.75
    g = torch.Generator().manual_seed(1)
    xb, x = su.make_slice((B, H, W, C), dtype, 0, left=left, right=right, guard=GUARD, role="in", values=torch.randn((B, H, W, C), generator=g) * 1.5,
                          device=D0)
    yb, y = su.make_slice((B, 2 * H, 2 * W, C), dtype, 0, left=left, right=right, guard=GUARD, role="out", device=D0)
    u = torch.rand((B, C, 2 * H, 2 * W), generator=g).to(D0) if injected else None
    key = None if injected else _key()
    ab = _ab(B, C, 2)
    assert _raw_up2(x, ab, y, _silu(), keep, u, key, 7, 2) == 0
    torch.cuda.synchronize()
    su.assert_canary_intact(xb)
    su.assert_canary_intact(yb)
    su.assert_fully_written(yb)
    ref = launch.gn_apply_drop(unet_exec.up2(x.contiguous(), 1.0), ab, _silu(), keep, u, key, 7, 2)
    assert torch.equal(y, ref), relerr(y, ref)
    frac = float((y != 0).float().mean())
    assert 0.5 < frac < 0.95, frac
    if injected:
        m = (u < keep).permute(0, 2, 3, 1)
        assert bool((y[~m] == 0).all()) and bool((y[m] != 0).float().mean() > 0.99)
    # without a table: a = 1, b = 0
    assert _raw_up2(x, None, y, 0, keep, u, key, 7, 2) == 0
    assert torch.equal(y, launch.gn_apply_drop(unet_exec.up2(x.contiguous(), 1.0), None, 0, keep, u, key, 7, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [S_C8, S_C40], ids=["3x5x8", "3x5x40_ld56"])
def test_drop_pool2_bwd_injected(shape, dtype):
    B, H, W, C, left, right = shape
    keep = 0.5
    g = torch.Generator().manual_seed(3)
    db, dy = su.make_slice((B, 2 * H, 2 * W, C), dtype, 0, left=left, right=right, guard=GUARD, role="in",
                           values=torch.randn((B, 2 * H, 2 * W, C), generator=g), device=D0)
    gb, gl = su.make_slice((B, H, W, C), dtype, 0, left=left, right=right, guard=GUARD, role="out", device=D0)
    u = torch.rand((B, C, 2 * H, 2 * W), generator=g).to(D0)
    assert _raw_pool(dy, gl, keep, u, None, 0, 0) == 0
    torch.cuda.synchronize()
    su.assert_canary_intact(db)
    su.assert_canary_intact(gb)
    su.assert_fully_written(gb)
    m = (u < keep).permute(0, 2, 3, 1)
    ref = _cell_sum(dy.float() * m.float() / keep)
    e = relerr(gl, ref)
    print(f"{shape} {dtype}: g {e:.2e} (bound {KTOL[dtype]:.0e})")
    assert e < KTOL[dtype], e
    dead = _cell_sum(m.float()) == 0
    assert bool(dead.any()) and bool((gl[dead] == 0).all()), "a cell whose four elements were dropped is not exactly 0"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [S_C8, S_C40], ids=["3x5x8", "3x5x40_ld56"])
def test_drop_pool2_bwd_regenerates_the_forward_mask(shape, dtype):
    """drawn masks on guarded, strided operands: dy = 1, keep = 0.5: g = 2 x (the number of elements of the cell that the forward kernel kept)"""
    B, H, W, C, left, right = shape
    key, stream, call = _key(), 11, 4
    ones = lambda h, w: torch.ones((B, h, w, C))
    xb, x = su.make_slice((B, H, W, C), dtype, 0, left=left, right=right, guard=GUARD, role="in", values=ones(H, W), device=D0)
    yb, y = su.make_slice((B, 2 * H, 2 * W, C), dtype, 0, left=left, right=right, guard=GUARD, role="out", device=D0)
    db, dy = su.make_slice((B, 2 * H, 2 * W, C), dtype, 0, left=left, right=right, guard=GUARD, role="in", values=ones(2 * H, 2 * W), device=D0)
    gb, g = su.make_slice((B, H, W, C), dtype, 0, left=left, right=right, guard=GUARD, role="out", device=D0)
    assert _raw_up2(x, None, y, 0, 0.5, None, key, stream, call) == 0 and _raw_pool(dy, g, 0.5, None, key, stream, call) == 0
    torch.cuda.synchronize()
    for buf in (xb, yb, db, gb):
        su.assert_canary_intact(buf)
    su.assert_fully_written(yb)
    su.assert_fully_written(gb)
    assert torch.equal(g.float(), _cell_sum((y != 0).float()) * 2.0)
    frac, n = float((y != 0).float().mean()), y.numel()
    assert abs(frac - 0.5) <= 5 * (0.25 / n) ** 0.5, frac
    y0 = y.clone()
    assert _raw_up2(x, None, y, 0, 0.5, None, key, stream, call) == 0 and torch.equal(y, y0)             # the same triple: the same mask
    for other in ((key, stream, call + 1), (key, stream + 1, call), (_key((0x1234ABCC, 0x8F1E2D3C)), stream, call)):
        assert _raw_up2(x, None, y, 0, 0.5, None, *other) == 0
        assert float(((y != 0) != (y0 != 0)).float().mean()) > 0.3


def test_beyond_the_grid_cap():
    from joligen_amd import _lib, launch
    from joligen_amd.modules import unet_exec

    B, H, W, C = S_BIG
    cap = int(_lib.lib().jg_dropout_grid_cap())
    assert cap < B * H * W * (C // 8) <= 2 * cap, cap
    keep, key = 0.75, _key()
    x = torch.randn((B, H, W, C), device=D0, generator=torch.Generator(device=D0).manual_seed(4)).to(torch.bfloat16)
    ab = _ab(B, C, 5)
    y = launch.gn_apply_drop_up2(x, ab, _silu(), keep, None, key, 3, 1)
    ref = launch.gn_apply_drop(unet_exec.up2(x, 1.0), ab, _silu(), keep, None, key, 3, 1)
    assert torch.equal(y, ref)
    n = y.numel()
    frac = float((y != 0).double().mean())            # SiLU(v) == 0 only at v == 0
    assert abs(frac - keep) <= 5 * (keep * (1 - keep) / n) ** 0.5, frac
    del ref
    dy = torch.randn(y.shape, device=D0, generator=torch.Generator(device=D0).manual_seed(6)).to(torch.float16)
    g = launch.drop_pool2_bwd(dy, keep, None, key, 3, 1)
    m = (y != 0)
    want = _cell_sum(dy.float() * m.float() / keep)
    e = relerr(g, want)
    assert e < KTOL[torch.float16], e


def test_bad_arguments_are_refused():
    B, H, W, C = 2, 3, 5, 8
    x = torch.ones((B, H, W, C), device=D0, dtype=torch.bfloat16)
    y = torch.ones((B, 2 * H, 2 * W, C), device=D0, dtype=torch.bfloat16)
    wide = torch.ones((B, 2 * H, 2 * W, 12), device=D0, dtype=torch.bfloat16)
    key = _key()
    assert _raw_up2(x, None, y, 0, 0.5, None, key, 0, 0) == 0 and _raw_pool(y, x, 0.5, None, key, 0, 0) == 0
    for keep in (0.0, 1.5, float("nan")):
        assert _raw_up2(x, None, y, 0, keep, None, key, 0, 0) == BAD and _raw_pool(y, x, keep, None, key, 0, 0) == BAD
    assert _raw_up2(x, None, y, 0, 0.5, None, None, 0, 0) == BAD and _raw_pool(y, x, 0.5, None, None, 0, 0) == BAD          # a draw without key
    assert _raw_up2(x, None, y, 0, 0.5, None, key, 1 << 16, 0) == BAD and _raw_pool(y, x, 0.5, None, key, 1 << 16, 0) == BAD
    assert _raw_up2(x, None, y, 99, 0.5, None, key, 0, 0) == BAD                                                             # activation
    assert _raw_up2(x[..., 1:], None, y, 0, 0.5, None, key, 0, 0) == BAD                                                     # alignment, C % 8
    assert _raw_up2(x, None, wide[..., 2:10], 0, 0.5, None, key, 0, 0) == BAD and _raw_pool(wide[..., 2:10], x, 0.5, None, key, 0, 0) == BAD
    from joligen_amd import _lib, ops

    L, dt, st = _lib.lib(), ops._dt(x), ops._st()
    assert L.jg_gn_apply_drop_up2(dt, _p(x), 4, None, _p(y), C, B, H, W, C, 0, 0.5, None, _p(key), 0, 0, st) == BAD           # stride < C
    assert L.jg_drop_pool2_bwd(dt, _p(y), C, _p(x), C, B, 0, W, C, 0.5, None, _p(key), 0, 0, st) == BAD                        # H < 1
    assert L.jg_drop_pool2_bwd(dt, _p(y), C, None, C, B, H, W, C, 0.5, None, _p(key), 0, 0, st) == BAD                         # no output
    torch.cuda.synchronize()


def test_torch_ops_opcheck():
    J = torch.ops.jg355
    B, H, W, C = 2, 3, 5, 8
    g = torch.Generator().manual_seed(9)
    x = torch.randn((B, H, W, C), generator=g).to(torch.bfloat16).to(D0)
    dy = torch.randn((B, 2 * H, 2 * W, C), generator=g).to(torch.bfloat16).to(D0)
    u = torch.rand((B, C, 2 * H, 2 * W), generator=g).to(D0)
    key, ab = _key(), _ab(B, C, 1)
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(J.gn_apply_drop_up2.default, (x, ab, _silu(), 0.75, u, None, 0, 0), test_utils=utils)
    torch.library.opcheck(J.gn_apply_drop_up2.default, (x, None, 0, 0.75, None, key, 3, 1), test_utils=utils)
    torch.library.opcheck(J.drop_pool2_bwd.default, (dy, 0.75, u, None, 0, 0), test_utils=utils)
    torch.library.opcheck(J.drop_pool2_bwd.default, (dy, 0.75, None, key, 3, 1), test_utils=utils)
    with pytest.raises(ValueError, match="dropout"):
        J.gn_apply_drop_up2(x, ab, 0, 0.75, u[..., :-1], None, 0, 0)
    with pytest.raises(ValueError, match="dropout"):
        J.drop_pool2_bwd(dy, 0.75, None, None, 0, 0)


# ---- the schedules ---------------------------------------------------------------------------------------------------------------------------
P_DROP = 0.25
CFG = dict(ngf=64, mults=[1, 2], res_blocks=[1, 1], attn_res=[2], S=64, B=2)       # test_fused_schedule_matches_module_graph


def _net(efficient, dtype, golden_dir, everywhere):
    from joligen_amd.modules.unet_generator_attn import ResBlock
    from test_gpu_1_model import build_net

    net, _ = build_net(dict(CFG, efficient=efficient), dtype, golden_dir, G_dropout=P_DROP)
    unet = net.denoise_fn.model
    blocks = [m for m in unet.modules() if isinstance(m, ResBlock)]
    assert unet.dropout == P_DROP and [rb.dropout for rb in unet.middle_block if isinstance(rb, ResBlock)] == [P_DROP, P_DROP]
    if everywhere:      # the reference's UNet hands its rate to the middle block only; every kind of block (down, up, 1x1 skip) with it here
        for rb in blocks:
            rb.dropout = P_DROP
    net.arena.ensure_fresh()
    return net, unet, blocks


@pytest.mark.parametrize("everywhere", [False, True], ids=["middle", "every_block"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("efficient", [True, False], ids=["eff", "noeff"])
def test_fused_schedule_matches_module_graph_with_dropout(golden_dir, efficient, dtype, everywhere):
    from joligen_amd import ops
    from test_gpu_1_model import TOL_OUT

    net, unet, blocks = _net(efficient, dtype, golden_dir, everywhere)
    g = torch.Generator().manual_seed(7)
    x0 = ops.to_nhwc(torch.randn(CFG["B"], 6, CFG["S"], CFG["S"], generator=g).to(D0), dtype, 8)
    emb0 = torch.randn(CFG["B"], unet.cond_embed_dim, generator=g).to(D0)
    R = ops.to_nhwc(torch.randn(CFG["B"], 3, CFG["S"], CFG["S"], generator=g).to(D0), dtype, 8)
    key = _key()
    res, live = {}, [rb for rb in blocks if rb.dropout]
    assert len(live) == (len(blocks) if everywhere else 2)
    unet.train(True)
    for fused in (False, True):
        unet.jg_fused = fused
        unet.dropout_state.begin_step(key)
        net.arena.g.zero_()
        x = x0.clone().requires_grad_(True)
        emb = emb0.clone().requires_grad_(True)
        out = unet(x, emb)
        name = type(out.grad_fn).__name__.lower()
        assert ("unet_fused_drop" in name) == fused, name
        out.backward(R)
        torch.cuda.synchronize()
        res[fused] = (out.detach().float(), x.grad.float(), emb.grad.clone(), net.arena.g.clone())
        assert all(unet.dropout_state.calls[rb.out_layers[2].stream] == 1 for rb in live)
    unet.jg_fused = True
    tol = 4 * TOL_OUT[dtype]
    errs = [relerr(res[True][i], res[False][i]) for i in range(4)]
    print(f"eff={efficient} {dtype} every={everywhere}: out {errs[0]:.2e} dx {errs[1]:.2e} demb {errs[2]:.2e} grad {errs[3]:.2e} (bound {tol:.0e}, 2x for gradients)")
    assert errs[0] < tol and errs[1] < 2 * tol and errs[2] < 2 * tol and errs[3] < 2 * tol, errs
    # it is a dropout: another call of the same key changes the output, the same call reproduces it
    with torch.no_grad():
        unet.dropout_state.begin_step(key)
        again, other = unet(x0, emb0).float(), unet(x0, emb0).float()
    e_same, e_other = relerr(again, res[True][0]), relerr(other, again)
    print(f"    the same call again {e_same:.2e}, the next call {e_other:.2e}")
    assert e_same < tol and e_other > 5 * max(e_same, 1e-4), (e_same, e_other)


@pytest.mark.parametrize("efficient", [True, False], ids=["eff", "noeff"])
def test_eval_mode_is_the_network_without_dropout(golden_dir, efficient):
    from joligen_amd import ops

    dtype = torch.float16
    net, unet, blocks = _net(efficient, dtype, golden_dir, True)
    g = torch.Generator().manual_seed(8)
    x0 = ops.to_nhwc(torch.randn(CFG["B"], 6, CFG["S"], CFG["S"], generator=g).to(D0), dtype, 8)
    emb0 = torch.randn(CFG["B"], unet.cond_embed_dim, generator=g).to(D0)
    outs = {}
    unet.train(False)
    with torch.no_grad():
        for fused in (True, False):
            unet.jg_fused = fused
            outs[fused, "drop"] = unet(x0, emb0).float()
        assert not unet.dropout_state.calls and unet.dropout_state.key is None           # nothing was invoked, nothing was drawn
        unet.dropout = 0.0
        for rb in blocks:
            rb.dropout = 0.0
        for fused in (True, False):
            unet.jg_fused = fused
            outs[fused, "none"] = unet(x0, emb0).float()
    unet.jg_fused = True
    # the same launches on the same values; the GroupNorm statistics are fp32 atomics (tests/test_gpu_1_model.py:644)
    assert relerr(outs[True, "drop"], outs[True, "none"]) < 2e-3 and relerr(outs[False, "drop"], outs[False, "none"]) < 2e-3


def test_unet_fused_drop_ops(golden_dir):
    """schema and fake kernels of the pair; the op is a function of (key, call); an empty key with no injected uniforms is refused"""
    net, unet, blocks = _net(True, torch.bfloat16, golden_dir, True)
    from joligen_amd import ops

    g = torch.Generator().manual_seed(5)
    x0 = ops.to_nhwc(torch.randn(CFG["B"], 6, CFG["S"], CFG["S"], generator=g).to(D0), torch.bfloat16, 8)
    emb0 = torch.randn(CFG["B"], unet.cond_embed_dim, generator=g).to(D0)
    R = ops.to_nhwc(torch.randn(CFG["B"], 3, CFG["S"], CFG["S"], generator=g).to(D0), torch.bfloat16, 8)
    unet.train(True)
    with torch.no_grad():
        unet(x0, emb0)                                   # builds the executor and its handle
    exe = unet._jg_executor
    emb_all = unet._emb_all(emb0.float().contiguous()).all.detach()
    key = _key()
    J = torch.ops.jg355
    args = (x0, emb_all, net.arena.w16, net.arena.w16T, key, 3, exe.handle, False)
    torch.library.opcheck(J.unet_fused_drop, args, test_utils=("test_schema", "test_faketensor"))
    a, _ = J.unet_fused_drop(*args)
    b, _ = J.unet_fused_drop(*args)
    c, _ = J.unet_fused_drop(*(args[:5] + (4,) + args[6:]))
    # two launches of the same (key, call): the same mask, the GroupNorm statistics are fp32 atomics (TOL_OUT of tests/test_gpu_1_model.py:15 for
    # bf16 outputs); the next call: another mask
    from test_gpu_1_model import TOL_OUT

    assert relerr(b, a) < TOL_OUT[torch.bfloat16] and relerr(c, a) > 0.2, (relerr(b, a), relerr(c, a))
    out, tape = J.unet_fused_drop(*(args[:7] + (True,)))
    net.arena.g.zero_()
    dx, demb = J.unet_fused_drop_bwd(R, tape, net.arena.g, exe.handle, True)
    torch.cuda.synchronize()
    assert dx.shape == x0.shape and bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(demb).all()) and float(net.arena.g.abs().sum()) > 0


@pytest.mark.parametrize("ft_mode", ["cm", "ect"])
def test_consistency_model_loss_and_backward_on_both_graphs(ft_mode):
    """cm_model with G_dropout: the student and the no-grad teacher are two invocations (calls 0 and 1 of every live placeholder, one key per
    optimize_parameters); the loss and the gradient arena of the fused schedule against the module graph on the same key"""
    import jg_oracle as O
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json
    from test_gpu_1_model import TOL_OUT

    c = dict(ngf=64, mults=[1, 2], res_blocks=[1, 1], attn_res=[2], efficient=True, S=64, B=2)
    opt = opt_from_json({}, dict(model_type="cm", G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"],
                                 G_unet_mha_attn_res=c["attn_res"], G_unet_mha_vit_efficient=c["efficient"], data_crop_size=c["S"],
                                 train_batch_size=c["B"], gpu_ids="0", jg_act_dtype="fp16", train_optim="adamw", train_G_ema=True,
                                 train_iter_size=1, checkpoints_dir="/tmp/jg_amd_ckpt/", name="cm_drop", alg_ddpm_ft_mode=ft_mode,
                                 G_dropout=P_DROP))
    model = create_model(opt, 0)
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.setup(opt)
    model.single_gpu()
    net = model.netG_A
    unet = net.cm_model
    assert unet.dropout == P_DROP and model.unet_dropout_state is unet.dropout_state
    paths = [m.path for m in unet.modules() if hasattr(m, "stream")]
    assert "cm_model.middle_block.0.out_layers.2" in paths and len(set(paths)) == len(paths)
    g = torch.Generator().manual_seed(9)
    Bimg = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    mask = torch.zeros(2, 1, 64, 64, dtype=torch.int64)
    mask[:, :, 10:40, 20:50] = 1
    A = Bimg * (1 - mask) + torch.randn(Bimg.shape, generator=g) * mask
    noise = torch.randn(Bimg.shape, generator=g)
    second = torch.randn(2, generator=g) if ft_mode == "ect" else torch.tensor([3, 7])
    model.rng_injection = lambda b: (noise, second)
    live = [rb.out_layers[2].stream for rb in unet._res_blocks if rb.dropout]
    assert len(live) == 2
    rates = [rb.dropout for rb in unet._res_blocks]

    def both_graphs(drop):
        unet.dropout = P_DROP if drop else 0.0
        for rb, p in zip(unet._res_blocks, rates):
            rb.dropout = p if drop else 0.0
        res = {}
        for fused in (False, True):
            unet.jg_fused = fused
            net.current_t = 0
            torch.manual_seed(1234)
            model.begin_dropout_step()
            key = unet.dropout_state.key.clone()
            model.set_input({"A": A, "B": Bimg, "B_label_mask": mask})
            net.arena.g.zero_()
            getattr(model, model.group_G.backward_functions[0])()
            model.loss_G_tot.backward()
            torch.cuda.synchronize()
            assert [unet.dropout_state.calls.get(s, 0) for s in live] == ([2, 2] if drop else [0, 0])
            res[fused] = (float(model.loss_G_tot.detach()), net.arena.g.clone(), key)
        unet.jg_fused = True
        assert torch.equal(res[True][2], res[False][2])
        return abs(res[True][0] - res[False][0]) / abs(res[False][0]), relerr(res[True][1], res[False][1]), res

    # the floor: the distance of the two graphs on this very step with the rate set to 0 (the launches of before).  The consistency loss is a
    # distance of two nearly equal outputs, so its gradient carries the 16-bit rounding of either graph far more visibly than the UNet-level
    # gradients that TOL_OUT was set for.  Both graphs draw the same mask and multiply by exactly 0 or 1 / keep: dropout adds no term, and the
    # bound is that of tests/test_gpu_13_cm_gan.py:466 on a measured floor: max(2 x floor, the UNet-level bound)
    # (the floor is itself one draw of a noisy distance -- fp32 atomics order, split-K weight gradients: the larger of two draws)
    fl_l, fl_g = (max(v) for v in zip(*(both_graphs(False)[:2] for _ in range(2))))
    e_l, e_g, res = both_graphs(True)
    tol = 4 * TOL_OUT[torch.float16]
    print(f"{ft_mode}: loss {res[True][0]:.6f} / {res[False][0]:.6f} ({e_l:.2e}, floor {fl_l:.2e}), gradient arena {e_g:.2e} (floor {fl_g:.2e}); "
          f"bounds {max(tol, 2 * fl_l):.1e} / {max(2 * tol, 2 * fl_g):.1e}")
    assert e_l < max(tol, 2 * fl_l) and e_g < max(2 * tol, 2 * fl_g), (e_l, e_g, fl_l, fl_g)
    assert e_l < 2.0 ** -10, e_l          # the loss at the run-to-run floor of tests/test_gpu_13_cm_gan.py:484-485


# ---- three palette steps against the fixture recorded from the unmodified reference with its Dropout draws -------------------------------------
@pytest.mark.parametrize("graph", ["fused", "module", "torch_ops"])
@pytest.mark.parametrize("dtype_name", ["fp16", "bf16"])
def test_palette_three_steps_with_the_recorded_masks(golden_dir, dtype_name, graph):
    """3 x optimize_parameters() of the tiny_eff recipe with G_dropout = 0.25, the reference's (t, u, noise) and the reference's masks injected,
    TEACHER-FORCED by the CPU oracle with the same masks (tests/unet_dropout_oracle.py; it reproduces the reference's losses and parameter
    checksums: tests/test_unet_dropout_host.py, its loss is re-asserted here).  Per step: the loss on identical weights within TOL_LOSS_FWD
    of tests/test_gpu_1_model.py:157, the update within COS_UPDATE (:158) -- the bounds of the same step without dropout -- and every
    recorded (module path, invocation) consumed exactly once."""
    import contextlib
    import os

    import parity_util as PU
    import unet_dropout_oracle as UO
    from joligen_amd import ops
    from test_gpu_1_model import COS_UPDATE, TOL_LOSS_FWD, load, make_model, palette_trainer

    g = load(os.path.join(golden_dir, "unet_dropout"), "palette_step_tiny_eff.pt")
    hp = g["hp"]
    model = make_model(g["cfg"], dtype_name, golden_dir, hp, G_dropout=hp["G_dropout"])
    dtype = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    net = model.netG_A
    unet = net.denoise_fn.model
    unet.jg_fused = graph == "fused"
    sd0 = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    tr = palette_trainer(sd0, g["cfg"], hp)
    keep = 1.0 - hp["G_dropout"]
    for it, s in enumerate(g["steps"]):
        table, asked = UO.table_of(s), []

        def rand(path, call, shape, device, table=table, asked=asked):
            asked.append((path, call))
            m = table[(path, call)]
            assert tuple(m.shape) == tuple(shape), (path, call, tuple(m.shape), tuple(shape))
            return UO.uniforms(m).to(device)

        unet.dropout_rand = rand
        PU.force_state(net, {k: tr.P[k] for k in tr.param_names}, tr.m, tr.v, tr.step, tr.ema)
        before, ref_before = PU.snapshot(net), {k: tr.P[k].clone() for k in tr.param_names}
        model.rng_injection = lambda b, s=s: (s["t"], s["u"], s["noise"])
        model.set_input({"A": s["A"], "B": s["B"], "B_label_mask": s["mask"], "A_img_paths": ["x"]})
        with (ops.torch_ops_boundary() if graph == "torch_ops" else contextlib.nullcontext()):
            model.optimize_parameters()
        loss = float(model.get_current_losses()["G_tot"])
        if graph == "fused":
            assert unet._jg_executor is not None
        with UO.recorded_masks(table, keep) as used:
            loss_ref = float(tr.optimize_parameters(s["B"], s["A"], s["mask"], s["noise"], s["t"], s["u"]))
        assert used == set(table) and sorted(asked) == sorted(table), (asked, sorted(table))
        assert abs(loss_ref - float(s["loss"])) < 2e-4 * abs(float(s["loss"])) + 1e-6        # oracle == reference fixture
        print(f"{graph} {dtype_name} it{it}: loss {loss:.6f} oracle {loss_ref:.6f} reference {float(s['loss']):.6f} ({abs(loss - float(s['loss'])) / abs(float(s['loss'])):.2e} of the reference's)")
        assert abs(loss - float(s["loss"])) < TOL_LOSS_FWD[dtype] * abs(float(s["loss"])), (it, loss, float(s["loss"]))      # of the reference's value
        PU.check_update(f"unet_dropout {graph} {dtype_name} it{it}", before, PU.snapshot(net), ref_before, {k: tr.P[k] for k in tr.param_names},
                        COS_UPDATE[dtype])
    unet.dropout_rand = None


@pytest.mark.parametrize("graph", ["fused", "module", "torch_ops"])
@pytest.mark.parametrize("dtype_name", ["fp16", "bf16"])
def test_cm_three_steps_with_the_recorded_masks(golden_dir, dtype_name, graph):
    """the same for cm_model in mode "cm" (tests/test_gpu_2_cm.py::test_cm_three_steps_vs_reference_golden, its COS_UPDATE; the loss within the step bound of tests/test_gpu_1_model.py:157, 5e-3 / 3e-2, of the reference's value):
    the student takes the reference's invocation 0 of every Dropout and the no-grad teacher invocation 1, whichever of the two the host
    issues first"""
    import contextlib
    import os

    import jg_oracle as O
    import parity_util as PU
    import unet_dropout_oracle as UO
    from joligen_amd import ops
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json
    from test_gpu_1_model import TOL_LOSS_FWD      # the project's step bound, 5e-3 fp16 / 3e-2 bf16, for the cm step as for the palette step
    from test_gpu_2_cm import COS_UPDATE
    from test_oracle_golden import cm_cfg_of

    g = torch.load(os.path.join(golden_dir, "unet_dropout", "cm_step_tiny_eff.pt"), weights_only=False)
    hp, c = g["hp"], g["cfg"]
    dtype = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    opt = opt_from_json({}, dict(model_type="cm", G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"],
                                 G_unet_mha_attn_res=c["attn_res"], G_unet_mha_vit_efficient=c["efficient"], data_crop_size=c["S"],
                                 train_batch_size=c["B"], gpu_ids="0", jg_act_dtype=dtype_name, train_iter_size=1, checkpoints_dir="/tmp/jg_amd_ckpt/",
                                 name="cm_drop", train_G_lr=hp["lr"], train_beta1=hp["beta1"], train_beta2=hp["beta2"], train_optim_eps=hp["eps"],
                                 train_optim_weight_decay=hp["weight_decay"], train_G_ema_beta=hp["ema_beta"], train_G_ema=hp["ema"],
                                 alg_diffusion_lambda_G=hp["lambda_G"], train_optim=hp["optim"], G_dropout=hp["G_dropout"]))
    model = create_model(opt, 0)
    model.netG_A.load_state_dict(O.synth_state_dict(model.netG_A.state_dict(), seed=0))
    model.setup(opt)
    model.single_gpu()
    net = model.netG_A
    net.current_t = 0
    unet = net.cm_model
    unet.jg_fused = graph == "fused"
    sd0 = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    tr = O.OracleCMTrainer(sd0, cm_cfg_of(c), g["total_t"], lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"],
                           weight_decay=hp["weight_decay"], ema_beta=hp["ema_beta"] if hp["ema"] else None, lambda_G=hp["lambda_G"], optim=hp["optim"])
    keep = 1.0 - hp["G_dropout"]
    for it, s in enumerate(g["steps"]):
        table, asked = UO.table_of(s), []

        def rand(path, call, shape, device, table=table, asked=asked):
            asked.append((path, call))
            return UO.uniforms(table[(path, call)]).to(device)

        unet.dropout_rand = rand
        PU.force_state(net, {k: tr.P[k] for k in tr.param_names}, tr.m, tr.v, tr.step, tr.ema)
        before, ref_before = PU.snapshot(net), {k: tr.P[k].clone() for k in tr.param_names}
        model.rng_injection = lambda b, s=s: (s["noise"], s["timesteps"])
        model.set_input({"A": s["A"], "B": s["B"], "B_label_mask": s["mask"], "A_img_paths": ["x"]})
        with (ops.torch_ops_boundary() if graph == "torch_ops" else contextlib.nullcontext()):
            model.optimize_parameters()
        loss = float(model.get_current_losses()["G_tot"])
        with UO.recorded_masks(table, keep) as used:
            loss_ref = float(tr.optimize_parameters(s["B"], s["mask"], s["noise"], s["timesteps"]))
        assert used == set(table) and sorted(asked) == sorted(table), (asked, sorted(table))
        assert abs(loss_ref - float(s["loss"])) < 2e-4 * abs(float(s["loss"])) + 1e-6        # oracle == reference fixture
        print(f"cm {graph} {dtype_name} it{it}: loss {loss:.6f} oracle {loss_ref:.6f} reference {float(s['loss']):.6f} ({abs(loss - float(s['loss'])) / abs(float(s['loss'])):.2e} of the reference's)")
        assert abs(loss - float(s["loss"])) < TOL_LOSS_FWD[dtype] * abs(float(s["loss"])), (it, loss, float(s["loss"]))      # of the reference's value
        PU.check_update(f"cm unet_dropout {graph} {dtype_name} it{it}", before, PU.snapshot(net), ref_before, {k: tr.P[k] for k in tr.param_names},
                        COS_UPDATE[dtype])
    unet.dropout_rand = None


def test_cm_gan_loss_and_backward_on_both_graphs():
    """cm_gan with G_dropout and a drawn key, fused schedule against module graph: the generator's loss (consistency + GAN term) at the
    run-to-run floor of tests/test_gpu_13_cm_gan.py:484-485 (two device runs of the same values: fp16 storage, atomics: < 2^-10 of the loss).
    The gradient arenas are printed beside their distance at a rate of 0 and held to the same gradient (cosine), not to a multiple of that
    distance: measured 9.5e-2, 9.6e-2, 1.09e-1 with dropout against 7.6e-2, 6.0e-2, 6.7e-2 without -- the GAN term's gradient through the
    discriminator is that noisy in fp16 on either graph, and 1.3 to 1.6 times a noisy floor is too close to any factor to assert on.  The
    gradients of both graphs with dropout are asserted where they are quiet: on the UNet (test_fused_schedule_matches_module_graph_with_dropout)
    and on the cm / ect losses (test_consistency_model_loss_and_backward_on_both_graphs)."""
    from test_gpu_13_cm_gan import make_model

    c = dict(ngf=64, mults=[1, 2], res_blocks=[1, 1], attn_res=[2], efficient=True, S=64, B=2)
    model = make_model(c, "fp16", G_dropout=P_DROP)
    net = model.netG_A
    unet = net.cm_model
    assert unet.dropout == P_DROP and model.unet_dropout_state is unet.dropout_state
    g = torch.Generator().manual_seed(9)
    Bimg = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    mask = torch.zeros(2, 1, 64, 64, dtype=torch.int64)
    mask[:, :, 10:40, 20:50] = 1
    A = Bimg * (1 - mask) + torch.randn(Bimg.shape, generator=g) * mask
    noise, timesteps = torch.randn(Bimg.shape, generator=g), torch.tensor([3, 7])
    model.rng_injection = lambda b: (noise, timesteps)
    live = [rb.out_layers[2].stream for rb in unet._res_blocks if rb.dropout]
    rates = [rb.dropout for rb in unet._res_blocks]

    def both_graphs(drop):
        unet.dropout = P_DROP if drop else 0.0
        for rb, p in zip(unet._res_blocks, rates):
            rb.dropout = p if drop else 0.0
        res = {}
        for fused in (False, True):
            unet.jg_fused = fused
            net.current_t = 0
            torch.manual_seed(4321)
            model.begin_dropout_step()
            model.set_input({"A": A, "B": Bimg, "B_label_mask": mask})
            model._group_flags(model.group_G)
            net.arena.g.zero_()
            model.compute_cm_gan_loss()
            model.loss_G_tot.backward()
            torch.cuda.synchronize()
            assert [unet.dropout_state.calls.get(s, 0) for s in live] == ([2, 2] if drop else [0, 0])
            res[fused] = (float(model.loss_G_tot.detach()), net.arena.g.clone())
        unet.jg_fused = True
        return abs(res[True][0] - res[False][0]) / abs(res[False][0]), relerr(res[True][1], res[False][1]), res

    # (the floor is itself one draw of a noisy distance -- fp32 atomics order, split-K weight gradients: the larger of two draws)
    fl_l, fl_g = (max(v) for v in zip(*(both_graphs(False)[:2] for _ in range(2))))
    e_l, e_g, res = both_graphs(True)
    a, b = res[True][1].double(), res[False][1].double()
    cos = float((a * b).sum() / (a.norm() * b.norm()))
    print(f"cm_gan: loss {res[True][0]:.6f} / {res[False][0]:.6f} ({e_l:.2e}, rate 0: {fl_l:.2e}; bound {2.0 ** -10:.2e}), gradient arena {e_g:.2e} "
          f"(rate 0: {fl_g:.2e}), cosine {cos:.4f}")
    assert e_l < 2.0 ** -10, (e_l, fl_l)
    assert cos > 0.9, (cos, e_g, fl_g)          # COS_UPDATE of the fp16 step tests (tests/test_gpu_2_cm.py:69): the same direction


@pytest.mark.parametrize("graph", ["fused", "modules"])
def test_palette_step_with_dropout_is_bit_reproducible_in_deterministic_mode(golden_dir, graph):
    """JG_DETERMINISTIC=1 with G_dropout: two optimize_parameters() from the same state and the same seed (the key of the masks is drawn on
    torch's generator), twice: loss, parameters, Adam moments and EMA are torch.equal -- jg_gn_bwd_reduce_drop keeps the ordered form of the
    reduction it replaces, and the masks are a function of (key, stream, call)"""
    import jg_oracle as O
    from joligen_amd import _lib
    from test_gpu_1_model import make_model

    c = dict(ngf=32, mults=[1, 2, 4], res_blocks=[1, 1, 1], attn_res=[4], efficient=True, S=64, B=3)
    g = torch.Generator().manual_seed(5)
    S, B = c["S"], c["B"]
    Bimg = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    mask = torch.zeros(B, 1, S, S, dtype=torch.int64)
    mask[:, :, 6:40, 10:50] = 1
    A = Bimg * (1 - mask) + torch.randn(B, 3, S, S, generator=g) * mask
    draws = [O.draw_step_randomness(torch.Generator().manual_seed(9 + i), Bimg, 2000) for i in range(2)]

    def run():
        prev = _lib.set_tuning("JG_DETERMINISTIC", 1)
        try:
            model = make_model(c, "bf16", golden_dir, train_G_ema=True, G_dropout=P_DROP)
            model.netG_A.denoise_fn.model.jg_fused = graph == "fused"
            torch.manual_seed(77)
            out, keys = [], []
            for i in range(2):
                model.rng_injection = lambda b, i=i: draws[i]
                model.set_input({"A": A, "B": Bimg, "B_label_mask": mask})
                model.optimize_parameters()
                torch.cuda.synchronize()
                ar = model.netG_A.arena
                keys.append(model.unet_dropout_state.key.clone())
                out.append(dict(loss=model.loss_G_tot.detach().clone(), p=ar.p.clone(), m=ar.m.clone(), v=ar.v.clone(), ema=ar.ema.clone()))
            assert not torch.equal(keys[0], keys[1])                 # a fresh key per step
            return out, keys
        finally:
            _lib.set_tuning("JG_DETERMINISTIC", prev)

    (a, ka), (b, kb) = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(ka, kb))
    for i, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert torch.equal(x[k], y[k]), (graph, "call", i, k, float((x[k].double() - y[k].double()).abs().max()))


# ---- single ResBlocks against the unmodified reference with its Dropout draw -------------------------------------------------------------------
def _fused_resblock(rb, x, film, R):
    """res_fwd / res_bwd of the fused schedule on ONE block: the executor's block routines with the pools, the tape and the input's statistics
    (what the producing convolution's epilogue leaves: sum and sum of squares per image and channel) set up by hand -> (out, dx, dfilm)"""
    from joligen_amd.modules import unet_exec as X

    exe = object.__new__(X.UNetExecutor)
    exe._side, exe._g1x1, exe.tape, exe.drop, exe.emb = None, [], [], (None, 0), film
    B, H, W, C = x.shape
    exe.pool = X._Pool(1 << 20, x.device)
    st = exe.pool.take(B, C)
    xf = x.float()
    st[:, 0, :, 0], st[:, 0, :, 1] = xf.sum(dim=(1, 2)), (xf * xf).sum(dim=(1, 2))
    fresh = lambda b, h, w, c: (torch.empty((b, h, w, c), device=x.device, dtype=x.dtype), exe.pool.take(b, c))
    out = exe.res_fwd(rb, X.Act(x, st, H * W, 0), fresh)
    exe.bpool, exe.demb = X._Pool(1 << 20, x.device), torch.zeros_like(film)
    dx = exe.res_bwd(exe.tape[0], R, [])
    exe.wgrad_join()
    torch.cuda.synchronize()
    return out.t, dx, exe.demb


@pytest.mark.parametrize("graph", ["fused", "module"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["plain", "down", "up_eff", "up_noeff"])
def test_resblock_with_the_recorded_mask_vs_reference(golden_dir, name, dtype, graph):
    """one ResBlock with dropout 0.25 and the reference's mask injected, on the block routines of the fused schedule and on the module graph:
    output, input gradient and embedding gradient against the unmodified reference's (tests/golden/unet_dropout/resblock_*.pt), at TOL_OUT /
    TOL_GRAD of tests/test_gpu_1_model.py::test_unet_vs_reference_golden.  up_eff is the block whose GroupNorm runs at the low resolution
    with the mask at the high one (jg_gn_apply_drop_up2 / jg_drop_pool2_bwd)."""
    import os

    import jg_oracle as O
    import torch.nn as nn
    import unet_dropout_oracle as UO
    from joligen_amd.arena import ParamArena
    from joligen_amd.modules.dropout import DropoutState, bind_dropout
    from joligen_amd.modules.unet_generator_attn import ResBlock
    from test_gpu_1_model import TOL_GRAD, TOL_OUT

    g = torch.load(os.path.join(golden_dir, "unet_dropout", f"resblock_{name}.pt"), weights_only=False)
    c = g["cfg"]
    rb = ResBlock(c["channels"], c["emb_channels"], c["p"], "groupnorm32", out_channel=c["out_channel"], use_scale_shift_norm=True, up=c["up"],
                  down=c["down"], efficient=c["efficient"])
    assert list(rb.state_dict()) == g["keys"]
    rb.load_state_dict(O.synth_state_dict({k: torch.empty(g["shapes"][k]) for k in g["keys"]}, seed=g["seed"]))
    holder = nn.Module()
    holder.rb = rb
    arena = ParamArena(holder, torch.device(D0), dtype)
    arena.ensure_fresh()
    rb.train()
    (path, call, shape, bits), asked = g["dropout"][0], []
    st = DropoutState()
    st.rand = lambda p, k, s, dev: asked.append((p, k, tuple(s))) or UO.uniforms(UO.unpack(bits, shape)).to(dev)
    bind_dropout(rb, st)
    x = g["x"].to(D0).permute(0, 2, 3, 1).contiguous().to(dtype)
    emb = g["emb"].to(D0)
    R = g["R"].to(D0).permute(0, 2, 3, 1).contiguous().to(dtype)
    lin = rb.emb_layers[1]
    if graph == "fused":
        rb.emb_slice = (0, 2 * c["out_channel"])
        embg = emb.clone().requires_grad_(True)
        film = torch.nn.functional.linear(torch.nn.functional.silu(embg), lin.weight.detach(), lin.bias.detach())
        out, dx, dfilm = _fused_resblock(rb, x, film.detach().contiguous(), R)
        film.backward(dfilm)
        demb = embg.grad
    else:
        xg, embg = x.clone().requires_grad_(True), emb.clone().requires_grad_(True)
        out = rb(xg, embg)
        out.backward(R)
        torch.cuda.synchronize()
        dx, demb = xg.grad, embg.grad
    assert asked == [(path, call, tuple(shape))], asked
    e_out = relerr(out.permute(0, 3, 1, 2), g["out"])
    e_dx = relerr(dx.permute(0, 3, 1, 2), g["dx"])
    e_demb = relerr(demb, g["demb"])
    print(f"resblock {name} {graph} {dtype}: out {e_out:.2e} (bound {TOL_OUT[dtype]:.0e}) dx {e_dx:.2e} demb {e_demb:.2e} (bound {TOL_GRAD[dtype]:.1e})")
    assert e_out < TOL_OUT[dtype] and e_dx < TOL_GRAD[dtype] and e_demb < TOL_GRAD[dtype], (e_out, e_dx, e_demb)
