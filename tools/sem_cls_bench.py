"""Timing of the semantic-consistency class branch of the CUT model (train_semantic_cls) on the GPU:

1. the fused class-loss launch (ops.cls_loss: jg_cls_loss of csrc/sem_cls.hip -- loss, gradient, argmax and the device-side gate in one launch)
   beside the same results composed from torch ops (cross_entropy, its gradient by autograd, argmax, the gate read on the device and multiplied
   in), HIP events, warm-up first, medians;
2. one optimize_parameters() of cut_model at the shape of examples/example_gan_mnist2USPS.json (mobile_resnet_attn, 6 blocks, basic D, 128 x 128,
   batch 4, dataaug_D_noise) with the option on and off, the two models built once and timed ALTERNATELY in rounds in one process;
3. `--step-only off --json`: the option-off step alone, one JSON line -- run from this checkout and, with `--root <other checkout>`, from the
   parent commit's, alternately, to compare the option-off step with the parent's.

    python tools/sem_cls_bench.py [--warmup 20] [--iters 200] [--step-warmup 8] [--rounds 5] [--round-steps 10] [--no-step] [--out profiles/sem_cls.md]
    python tools/sem_cls_bench.py --step-only off --json [--root /path/to/parent/checkout]
"""
import argparse
import json
import os
import statistics
import sys
import time

_ap = argparse.ArgumentParser()
_ap.add_argument("--warmup", type=int, default=20)
_ap.add_argument("--iters", type=int, default=200)
_ap.add_argument("--step-warmup", type=int, default=8)
_ap.add_argument("--rounds", type=int, default=5)
_ap.add_argument("--round-steps", type=int, default=10)
_ap.add_argument("--no-step", action="store_true")
_ap.add_argument("--step-only", default="", choices=["", "off", "on"])
_ap.add_argument("--json", action="store_true")
_ap.add_argument("--root", default="", help="import joligen_amd from this checkout instead of the one this file lives in")
_ap.add_argument("--out", default="")
ARGS = _ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root) if ARGS.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import joligen_amd  # noqa: E402,F401  (before the first HIP call: the package makes captured graphs safe to replay, joligen_amd/__init__.py)

SHAPES = [(4, 10), (16, 10), (256, 1000)]


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


def kernel_rows(a):
    from joligen_amd import ops

    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    rows = []
    for B, n in SHAPES:
        logits = torch.randn(B, n, device=d, generator=g) * 3
        target = torch.randint(0, n, (B,), device=d, generator=g)
        prev = torch.tensor(0.5, device=d)

        def fused():
            return ops._cls_loss_launch(logits, target, ops.CLS_CE, 1.0, prev, 1.0, None, False)

        def composed():
            x = logits.detach().requires_grad_(True)
            gate = (~(prev > 1.0)).float()
            loss = torch.nn.functional.cross_entropy(x, target) * gate
            (dl,) = torch.autograd.grad(loss, x)
            return loss, dl, x.argmax(dim=1)

        lf, df, af = fused()
        lt, dt, at = composed()
        torch.cuda.synchronize()
        assert abs(float(lf) - float(lt)) <= 1e-5 * abs(float(lt)) and torch.equal(af, at) and float((df - dt).abs().max()) <= 1e-6
        t_f, m_f = timed(fused, a.warmup, a.iters)
        t_t, m_t = timed(composed, a.warmup, a.iters)
        rows.append(f"| ({B}, {n}) fp32 | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) | {t_t * 1e3:.1f} us ({m_t * 1e3:.1f}) | {t_t / t_f:.1f} |")
    return rows


def step_model(on):
    """the mnist2USPS example's shape; `on`: train_semantic_cls"""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    B, S = 4, 128
    ov = dict(model_type="cut", G_netG="mobile_resnet_attn", G_ngf=64, G_nblocks=6, D_netDs=["basic"], D_ndf=64, data_crop_size=S, data_load_size=S,
              train_batch_size=B, train_iter_size=1, train_optim="adam", train_G_lr=2e-5, train_D_lr=1e-5, dataaug_D_noise=0.001, gpu_ids="0",
              jg_act_dtype="bf16", name="sem_cls_bench", checkpoints_dir="/tmp/jg_bench_ckpt/")
    if on:
        ov.update(train_semantic_cls=True, cls_nf=64, cls_semantic_nclasses=10)
    opt = opt_from_json({}, ov)
    torch.manual_seed(0)
    model = create_model(opt, 0)
    g = torch.Generator().manual_seed(1)
    data = {k: (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda() for k in ("A", "B")}
    data["A_label_cls"] = torch.randint(0, 10, (B,), generator=g)
    model.data_dependent_initialize(data)
    model.setup(opt)
    model.single_gpu()

    def step():
        model.set_input(data)
        model.optimize_parameters()

    return model, step


def time_rounds(steps, a):
    """steps: {label: step function}; every round times every label once, in turn"""
    for step in steps.values():
        for _ in range(a.step_warmup):
            step()
        torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.round_steps):
                step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.round_steps)
    return ms


def main():
    a = ARGS
    assert a.warmup >= 10 and a.iters >= 50 and a.step_warmup >= 4 and a.rounds >= 3      # (the step graphs are captured on the third step)
    assert torch.cuda.is_available(), "sem_cls_bench.py measures on the GPU; there is no CPU path"
    import warnings

    if a.step_only:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model, step = step_model(a.step_only == "on")
            ms = time_rounds({"x": step}, a)["x"]
        print(json.dumps({"option": a.step_only, "root": os.path.abspath(a.root) if a.root else "", "ms_per_step_median": round(statistics.median(ms), 3),
                          "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "rounds": a.rounds, "round_steps": a.round_steps,
                          "step_driver": model.step_driver}))
        return 0
    lines = ["# train_semantic_cls: the fused class-loss kernel and the CUT step of the mnist2USPS example's shape", "",
             f"{torch.cuda.get_device_name(0)}.  HIP events around each call (the Python wrapper included), {a.warmup} warm-up + {a.iters} timed calls, median "
             "(minimum in brackets).  Fused: one `jg_cls_loss` launch gives the loss, its gradient, the argmax and applies the gate read from device "
             "memory.  Composition: `cross_entropy` times the gate (a device-side comparison, no host read), its gradient through autograd, `argmax`.", "",
             "| logits | fused | torch composition | torch / fused |", "|---|---|---|---|"]
    lines += kernel_rows(a)
    if not a.no_step:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            built = {"off": step_model(False), "on": step_model(True)}
            ms = time_rounds({k: v[1] for k, v in built.items()}, a)
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines += ["", "One `optimize_parameters()` (set_input on a device-resident batch included): mobile_resnet_attn, 6 blocks, ngf 64, basic D, 128 x 128, "
                  f"batch 4, dataaug_D_noise 0.001, bf16; {a.step_warmup} warm-up steps per model, then {a.rounds} rounds that time {a.round_steps} steps of each "
                  "configuration in turn (host clock around steps that end in a device synchronise).  With the option on the step runs the three groups "
                  "in sequence (no early-D, no captured graphs) and the classifier (cls_nf 64) makes three train-mode passes.", "",
                  "| train_semantic_cls | ms per step (median of rounds) | spread over rounds | difference to off | step driver |", "|---|---|---|---|---|"]
        lines += [f"| {k} | {med[k]:.2f} | {min(ms[k]):.2f} - {max(ms[k]):.2f} | {med[k] - med['off']:+.2f} | {built[k][0].step_driver} |" for k in ("off", "on")]
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
