"""Timing of G_dropout / D_dropout of the CUT model on the GPU:

1. the three fused passes of csrc/dropout.hip (normalise + ReLU + dropout, and the two backward passes, the mask drawn in the kernel and never
   stored) beside the same passes without dropout (jg_gn_apply, jg_gn_bwd_reduce_ld_acc, jg_gn_bwd_apply) and beside the composed form -- the
   plain pass plus a mask materialised by torch.rand and multiplied in a pass of its own -- on the block tensor of the ResNet generator, HIP
   events around C entry points that write preallocated outputs, with the bytes each pass must move and the rate over them;
2. one optimize_parameters() of cut_model (resnet 9 blocks + basic D) with dropout off and with G_dropout + D_dropout: both models are built
   once and timed ALTERNATELY in rounds in one process, so that the spread over the rounds stands beside the difference.

    python tools/dropout_bench.py [--batch 16] [--size 256] [--warmup 20] [--iters 100] [--step-warmup 8] [--rounds 5] [--round-steps 10]
        [--no-step] [--out profiles/dropout.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import joligen_amd  # noqa: E402,F401  (before the first HIP call: the package makes captured graphs safe to replay, joligen_amd/__init__.py)

HBM_PEAK = 8.0e12          # bytes/s, HBM3E specification of the MI355X
HBM_COPY = 6.29e12         # bytes/s, measured float4 copy
KEEP = 0.5


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def kernel_rows(a, shape):
    from joligen_amd import _lib, ops
    from joligen_amd._lib import check

    B, H, W, C = shape
    HW, N = H * W, B * H * W * C
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    x = torch.randn(shape, device=d, generator=g).to(torch.bfloat16)
    dy = torch.randn(shape, device=d, generator=g).to(torch.bfloat16)
    y, dx, dym = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    L, dt, st, act = _lib.lib(), ops._dt(x), ops._st(), _lib.JG_ACT_RELU
    f32 = dict(device=d, dtype=torch.float32)
    sums, ab, mr = torch.zeros((B, C, 2), **f32), torch.empty((B, C, 2), **f32), torch.empty((B, C, 2), **f32)
    check(L.jg_gn_stats_ld(dt, x.data_ptr(), C, sums.data_ptr(), C, B, HW, C, st), "jg_gn_stats_ld")
    check(L.jg_gn_coef(sums.data_ptr(), None, None, None, 0, ab.data_ptr(), mr.data_ptr(), B, HW, C, C, 1e-5, st), "jg_gn_coef")
    red, pqr = torch.zeros((B, C, 2), **f32), torch.empty((B, C, 3), **f32)
    check(L.jg_gn_bwd_reduce_ld_acc(dt, x.data_ptr(), C, dy.data_ptr(), C, ab.data_ptr(), red.data_ptr(), B, HW, C, act, st), "jg_gn_bwd_reduce_ld_acc")
    check(L.jg_gn_bwd_coef(red.data_ptr(), None, None, None, 0, mr.data_ptr(), pqr.data_ptr(), None, None, None, 0, B, HW, C, C, st), "jg_gn_bwd_coef")
    key = ops.d_aug_key(d)
    X, DY, Y, DX, AB, PQR, RED, KEY = (t.data_ptr() for t in (x, dy, y, dx, ab, pqr, red, key))
    drop = (KEEP, None, KEY, 1, 0, st)

    fused = {"forward apply": lambda: L.jg_gn_apply_drop(dt, X, C, AB, Y, C, B, H, W, C, act, *drop),
             "backward reduce": lambda: L.jg_gn_bwd_reduce_drop(dt, X, C, DY, C, AB, RED, B, H, W, C, act, *drop),
             "backward apply": lambda: L.jg_gn_bwd_apply_drop(dt, X, C, DY, C, AB, PQR, DX, C, B, H, W, C, act, *drop)}
    plain = {"forward apply": lambda: L.jg_gn_apply(dt, X, AB, Y, B, HW, C, act, st),
             "backward reduce": lambda: L.jg_gn_bwd_reduce_ld_acc(dt, X, C, DY, C, AB, RED, B, HW, C, act, st),
             "backward apply": lambda: L.jg_gn_bwd_apply(dt, X, DY, AB, PQR, DX, B, HW, C, act, st)}
    mask = [None]

    def composed_fwd():           # the mask is drawn, kept for the backward and multiplied in a pass of its own
        L.jg_gn_apply(dt, X, AB, Y, B, HW, C, act, st)
        mask[0] = (torch.rand(shape, device=d) < KEEP).to(torch.bfloat16).mul_(1.0 / KEEP)
        y.mul_(mask[0])

    def composed_reduce():        # the masked gradient is formed once and read by both backward passes
        torch.mul(dy, mask[0], out=dym)
        L.jg_gn_bwd_reduce_ld_acc(dt, X, C, dym.data_ptr(), C, AB, RED, B, HW, C, act, st)

    def composed_apply():
        L.jg_gn_bwd_apply(dt, X, dym.data_ptr(), AB, PQR, DX, B, HW, C, act, st)

    composed = {"forward apply": composed_fwd, "backward reduce": composed_reduce, "backward apply": composed_apply}
    nbytes = {"forward apply": 2 * N * 2, "backward reduce": 2 * N * 2, "backward apply": 3 * N * 2}
    for fn in list(fused.values()) + list(plain.values()):
        assert fn() == 0
    rows = []
    for name in ("forward apply", "backward reduce", "backward apply"):
        t_f, m_f = timed(fused[name], a.warmup, a.iters)
        t_p, m_p = timed(plain[name], a.warmup, a.iters)
        t_c, m_c = timed(composed[name], a.warmup, a.iters)
        rate = lambda t: nbytes[name] / (t * 1e-3) / 1e12
        rows.append(f"| {list(shape)} | {name} | {nbytes[name] / 1e6:.1f} MB | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) = {rate(t_f):.2f} TB/s | "
                    f"{t_p * 1e3:.1f} us ({m_p * 1e3:.1f}) = {rate(t_p):.2f} TB/s | {t_f / t_p:.2f} | {t_c * 1e3:.1f} us ({m_c * 1e3:.1f}) | {t_c / t_f:.2f} |")
    return rows


def step_model(dropout, batch, size, switches=True):
    """the model of `bench.py --model cut` (resnet 9 blocks, basic D), with or without G_dropout + D_dropout; switches False: dropout off AND
    `jg_nce_reuse_feats` / `jg_batched_nce` off, the passes a step with G_dropout issues but without the dropout in them"""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(model_type="cut", G_netG="resnet_9blocks", G_ngf=64, G_nblocks=9, D_netDs=["basic"], D_ndf=64, data_crop_size=size, data_load_size=size,
              train_batch_size=batch, train_iter_size=1, train_optim="adam", train_G_ema=True, train_G_ema_beta=0.999, gpu_ids="0", jg_act_dtype="bf16",
              name="dropout_bench", checkpoints_dir="/tmp/jg_bench_ckpt/", G_dropout=bool(dropout), D_dropout=bool(dropout))
    if not switches:
        ov.update(jg_nce_reuse_feats=False, jg_batched_nce=False)
    opt = opt_from_json({}, ov)
    torch.manual_seed(0)
    model = create_model(opt, 0)
    g = torch.Generator().manual_seed(1)
    data = {k: (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda() for k in ("A", "B")}
    model.data_dependent_initialize(data)
    model.setup(opt)
    model.single_gpu()

    def step():
        model.set_input(data)
        model.optimize_parameters()

    return model, step


def step_rows(a):
    import time
    import warnings

    variants = ("off", "off, jg_nce_reuse_feats = jg_batched_nce = False", "G_dropout + D_dropout")
    built = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for v in variants:
            built[v] = step_model(v.startswith("G_dropout"), a.batch, a.size, switches="False" not in v)
            for _ in range(a.step_warmup):
                built[v][1]()
            torch.cuda.synchronize()
        ms = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v in variants:                      # alternated: every round times every configuration once
                step = built[v][1]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.round_steps):
                    step()
                torch.cuda.synchronize()
                ms[v].append((time.perf_counter() - t0) * 1e3 / a.round_steps)
    med = {v: statistics.median(ms[v]) for v in variants}
    notes = {v: ("reuse_feats %s, batched_nce %s" % (bool(built[v][0]._reuse_feats()), bool(built[v][0]._batched_nce()))) for v in variants}
    return [f"| {v} | {med[v]:.2f} | {min(ms[v]):.2f} - {max(ms[v]):.2f} | {med[v] - med['off']:+.2f} | {built[v][0].step_driver} | {notes[v]} |" for v in variants]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50 and a.step_warmup >= 4 and a.rounds >= 3      # (the step graphs are captured on the third step)
    assert torch.cuda.is_available(), "dropout_bench.py measures on the GPU; there is no CPU path"

    B, S = a.batch, a.size
    shapes = [(B, S // 4, S // 4, 256), (B, S // 8, S // 8, 512)]
    lines = ["# G_dropout / D_dropout: the fused normalise + ReLU + dropout passes and the CUT step", "",
             "Command: `python tools/dropout_bench.py " + " ".join(sys.argv[1:]) + "`", "",
             f"{torch.cuda.get_device_name(0)}, bf16.  HIP events around each C entry point on preallocated outputs, {a.warmup} warm-up + {a.iters} timed calls, "
             "median (minimum in brackets).  `fused`: csrc/dropout.hip, keep = 0.5, the mask drawn in the kernel (two Philox4x32-10 calls per 16-byte "
             "group) and never stored.  `plain`: the pass without dropout (jg_gn_apply / jg_gn_bwd_reduce_ld_acc / jg_gn_bwd_apply).  `composed`: the plain "
             "pass plus torch: forward = apply, torch.rand, compare, cast, scale, multiply in place; backward reduce = dy * mask into a buffer, then the "
             "plain reduce; backward apply = the plain apply on that buffer.  Bytes: what the pass must move (16-bit x [, dy] read, y / dx written); the "
             f"rate is over those bytes.  The tensors are {shapes[0][0] * shapes[0][1] * shapes[0][2] * shapes[0][3] * 2 / 1e6:.1f} MB and "
             f"{shapes[1][0] * shapes[1][1] * shapes[1][2] * shapes[1][3] * 2 / 1e6:.1f} MB: a pass's operands fit the 256 MiB Infinity Cache and the loop "
             f"re-runs it on the same operands, so this is not an HBM-only rate (HBM: {HBM_PEAK / 1e12:.1f} TB/s specification, {HBM_COPY / 1e12:.2f} TB/s measured copy).",
             "", "| tensor | pass | bytes | fused | plain | fused / plain | composed | composed / fused |", "|---|---|---|---|---|---|---|---|"]
    for shape in shapes:
        lines += kernel_rows(a, shape)
    if not a.no_step:
        lines += ["", f"One `optimize_parameters()` of cut_model, resnet_9blocks + basic D (set_input on a device-resident batch included), batch {B}, {S} x {S}, "
                  f"bf16; {a.step_warmup} warm-up steps per model, then {a.rounds} rounds that time {a.round_steps} steps of each configuration in turn (host "
                  "clock around steps that end in a device synchronise).  With G_dropout the key-side features are not reused from the forward and the "
                  "contrastive terms are not batched (every encoder pass draws its own mask, as in the reference), so the difference to `off` is dropout plus those "
                  "two switches; the middle row has the switches off and no dropout, which separates the two.", "",
                  "| options | ms per step (median of rounds) | spread over rounds | difference to off | step driver | resolved switches |", "|---|---|---|---|---|---|"]
        lines += step_rows(a)
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
