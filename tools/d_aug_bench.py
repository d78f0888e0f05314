"""Timing of the discriminator-input augmentations of the CUT model (dataaug_D_noise, dataaug_APA) on the GPU:

1. the fused launches (ops.d_aug: jg_d_aug of csrc/d_aug.hip, noise and flags drawn in the kernel, the outputs written into preallocated "static
   operand" tensors) beside the same operands composed from torch ops (randn, multiply-add, rand, where, copy into the static operand), HIP events,
   with the bytes each fused launch moves and the rate over them against the HBM peak; and ops.apa_update beside its torch composition;
2. one optimize_parameters() of cut_model -- resnet 9 blocks + basic D, and the benchmarked SegFormer + [projected_d (ViT), basic] selection of
   `bench.py` -- with the options off, with noise, with APA and with both: the four models are built once and timed ALTERNATELY in rounds in one
   process, so that the spread of one configuration over the rounds stands beside the differences between configurations.

    python tools/d_aug_bench.py [--batch 16] [--size 256] [--warmup 20] [--iters 100] [--step-warmup 8] [--rounds 5] [--round-steps 10]
        [--no-step] [--out profiles/d_aug.md]
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
SIGMA = 0.1


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


def kernel_rows(a, dtype_name):
    from joligen_amd import ops

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    B, S, C = a.batch, a.size, 3
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    img = lambda: torch.randn(B, S, S, 8, device=d, generator=g).to(dtype)
    src, alts, statics = img(), [img(), img()], [img(), img()]
    ps = [torch.tensor([0.5], device=d), torch.tensor([0.5], device=d)]
    key = ops.d_aug_key(d)
    px16 = B * S * S * 16

    def fused_noise():
        ops.d_aug(src, C, SIGMA, key=key, call=1, outs=statics[:1])

    def fused_both():
        return ops.d_aug(src, C, SIGMA, key=key, call=1, alts=alts, ps=ps, outs=statics)

    def fused_apa():
        ops.d_aug(src, C, 0.0, key=key, call=1, alts=alts, ps=ps, outs=statics)

    def torch_noisy():
        return (src.float() + SIGMA * torch.randn(src.shape, device=d)).to(dtype)

    def torch_noise():
        statics[0].copy_(torch_noisy())

    def torch_select(base):
        for k in range(2):
            flag = (torch.rand(B, device=d) < ps[k]).view(B, 1, 1, 1)
            statics[k].copy_(torch.where(flag, alts[k], base))

    _, flags = fused_both()
    torch.cuda.synchronize()
    fl = flags.bool().cpu()
    # per sample: src is read when a target is unflagged, alt_d when target d is flagged; every target is written
    rd_both = (int((~fl).any(0).sum()) + int(fl.sum())) * (px16 // B)
    rows = []
    for label, fused, composed, nlaunch, rd, wr in (
            ("noise (1 operand)", fused_noise, torch_noise, 1, px16, px16),
            ("APA (2 discriminators)", fused_apa, lambda: torch_select(src), 2, rd_both, 2 * px16),
            ("noise + APA (2 discriminators)", fused_both, lambda: torch_select(torch_noisy()), 2, rd_both, 2 * px16)):
        t_f, m_f = timed(fused, a.warmup, a.iters)
        t_t, m_t = timed(composed, a.warmup, a.iters)
        rate = (rd + wr) / (t_f * 1e-3)
        rows.append(f"| {dtype_name} | {label} | {nlaunch} | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) | {(rd + wr) / 1e6:.1f} MB | {rate / 1e12:.2f} TB/s = "
                    f"{100 * rate / HBM_PEAK:.0f} % of 8.0 (spec), {100 * rate / HBM_COPY:.0f} % of 6.29 (copy) | {t_t * 1e3:.1f} us ({m_t * 1e3:.1f}) | {t_t / t_f:.1f} |")
    # the update of p: PatchGAN logit map of this batch (channel 0 of [B, S/8 - 2, S/8 - 2, 8])
    h = max(S // 8 - 2, 1)
    pred = torch.randn(B, h, h, 8, device=d, generator=g).to(dtype)
    state = torch.tensor([0.5, 0.0, 0.0], device=d)

    def fused_update():
        ops.apa_update(pred, state, 0.6, B * 4, 50 * 1000, channel0=True)

    host = {"p": 0.5}

    def torch_update():          # the reference's form: p is a host value, read back every time (a synchronisation)
        s = pred[..., 0].float().sign().mean()
        adjust = torch.sign(s - 0.6)
        host["p"] = min(max(host["p"] + float(adjust) * (B * 4) / (50 * 1000), 0.0), 1.0)

    t_f, m_f = timed(fused_update, a.warmup, a.iters)
    t_t, m_t = timed(torch_update, a.warmup, a.iters)
    upd = f"| {dtype_name} | `ops.apa_update` on [{B}, {h}, {h}, 8] | 1 | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) | | | {t_t * 1e3:.1f} us ({m_t * 1e3:.1f}), with its host read | {t_t / t_f:.1f} |"
    return rows + [upd]


def step_model(kind, variant, batch, size):
    """`kind` "resnet": the model of `bench.py --model cut` (resnet 9 blocks, basic D); "segformer": its benchmarked CUT leg (SegFormer-attn G,
    [projected_d (ViT), basic] D); `variant`: which of the two options are on"""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    seg = kind == "segformer"
    ov = dict(model_type="cut", G_netG="segformer_attn_conv" if seg else "resnet", G_ngf=64, G_nblocks=9, D_netDs=["projected_d", "basic"] if seg else ["basic"],
              D_ndf=64, D_proj_interp=size, D_proj_network_type="vitsmall" if seg else "efficientnet", data_crop_size=size, data_load_size=size,
              train_batch_size=batch, train_iter_size=1, train_optim="adam", train_G_ema=True, train_G_ema_beta=0.999, gpu_ids="0", jg_act_dtype="bf16",
              name="d_aug_bench", checkpoints_dir="/tmp/jg_bench_ckpt/")
    if variant in ("noise", "both"):
        ov["dataaug_D_noise"] = SIGMA
    if variant in ("APA", "both"):
        ov.update(dataaug_APA=True, dataaug_APA_p=0.5)
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


def step_rows(a, kind):
    import time
    import warnings

    variants = ("off", "noise", "APA", "both")
    built = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for v in variants:
            built[v] = step_model(kind, v, a.batch, a.size)
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
    rows = [f"| {kind} | {v} | {med[v]:.2f} | {min(ms[v]):.2f} - {max(ms[v]):.2f} | {med[v] - med['off']:+.2f} | {built[v][0].step_driver} |" for v in variants]
    for v in variants:
        m = built[v][0]
        assert all(0.0 <= float(getattr(m, dn + "_loss_calculator").adaptive_pseudo_augmentation_p) <= 1.0 for dn in m.discriminators_names)
    built.clear()
    torch.cuda.empty_cache()
    return rows


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
    assert torch.cuda.is_available(), "d_aug_bench.py measures on the GPU; there is no CPU path"

    B, S = a.batch, a.size
    lines = [f"# dataaug_D_noise / dataaug_APA: the fused discriminator-input kernel and the CUT step, [{B}, {S}, {S}, 8] images, 3 valid channels",
             "",
             f"{torch.cuda.get_device_name(0)}.  HIP events around each call (the Python wrapper included), {a.warmup} warm-up + {a.iters} timed calls, median "
             "(minimum in brackets).  The fused launches draw noise and flags in the kernel (Philox4x32-10, Box-Muller) and write preallocated operands; "
             "the composition is randn, multiply-add, rand, where and the copy into the same operands.  Bytes: what the fused launch reads (src once per "
             f"sample that has an unflagged target, alt where flagged) and writes; one image tensor is {B * S * S * 16 / 1e6:.1f} MB, so every operand of a call "
             "fits the 256 MiB Infinity Cache: the rate is over those bytes, it is not an HBM-only rate.",
             "",
             "| dtype | operands formed | fused kernel launches | fused | bytes moved | rate over them | torch composition | torch / fused |",
             "|---|---|---|---|---|---|---|---|"]
    for dtype_name in ("bf16", "fp16"):
        lines += kernel_rows(a, dtype_name)
    if not a.no_step:
        lines += ["", f"One `optimize_parameters()` (set_input on a device-resident batch included), batch {B}, {S} x {S}, bf16; {a.step_warmup} warm-up steps per "
                  f"model, then {a.rounds} rounds that time {a.round_steps} steps of every configuration in turn (host clock around steps that end in a "
                  "device synchronise).  `spread`: the fastest and slowest round of that configuration; `difference`: median against the options-off median.",
                  "", "| model | options | ms per step (median of rounds) | spread over rounds | difference to off | step driver |", "|---|---|---|---|---|---|"]
        for kind in ("resnet", "segformer"):
            lines += step_rows(a, kind)
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
