"""Timing of the two fused launches of data_online_context_pixels (csrc/context.hip) on the GPU beside the same results composed from ops the
project already had:

  split : ops.context_split (one read of the fp32 NCHW image -> framed image + crop)      against   ops.to_nhwc + ops.crop2d
  frame : ops.context_frame (select + noisy copy, noise drawn in the kernel, preallocated   against   zero pad (F.pad) + mask multiply-add (torch) +
          outputs)                                                                                  ops.d_aug into the preallocated noisy output

The two forms of a row are timed ALTERNATELY in rounds in one process (HIP events around `--calls` back-to-back calls, so that the event pair
is not what is measured); the table gives the median over the rounds and the range, the bytes each fused launch has to move and the rate over
them.  Before any timing the outputs of the two forms are compared: a speed-up of a different result is not one.

    python tools/context_bench.py [--batch 16] [--size 256] [--context 32] [--dtype bf16] [--warmup 20] [--calls 50] [--rounds 9]
        [--out profiles/context.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

import joligen_amd  # noqa: E402,F401

HBM_PEAK = 8.0e12          # bytes/s, HBM3E specification of the MI355X
HBM_COPY = 6.29e12         # bytes/s, measured float4 copy (profiles/d_aug.md)
SIGMA = 0.1


def timed(fn, calls):
    """ms per call: HIP events around `calls` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(forms, warmup, calls, rounds):
    """{name: [ms per call of every round]}, the forms taking turns inside every round"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            out[k].append(timed(fn, calls))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--context", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("context_bench.py measures on the GPU: no device found (nothing is timed on the CPU)")
    from joligen_amd import ops

    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    B, S, c, C, cpad = a.batch, a.size, a.context, 3, 8
    H = S + 2 * c
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    x = torch.rand(B, C, H, H, device=d, generator=g) * 2 - 1
    ctx, _ = ops.context_split(x, c, dtype)
    inner = ops.to_nhwc(torch.rand(B, C, S, S, device=d, generator=g) * 2 - 1, dtype)
    key = ops.d_aug_key(d)
    out, noisy, noisy2 = (torch.empty_like(ctx) for _ in range(3))
    mask = torch.ones(1, H, H, 1, device=d, dtype=dtype)
    mask[:, c:-c, c:-c] = 0

    def split_fused():
        return ops.context_split(x, c, dtype)

    def split_composed():
        full = ops.to_nhwc(x, dtype)
        return full, ops.crop2d(full, c, c, S, S)

    def frame_fused():
        return ops.context_frame(inner, ctx, c, C, SIGMA, key=key, call=0, outs=(out, noisy))

    def frame_composed():
        framed = F.pad(inner, (0, 0, c, c, c, c)) + mask * ctx
        ops.d_aug(framed, C, SIGMA, key=key, call=0, outs=[noisy2])
        return framed, noisy2

    # the same results first
    sf, sc = split_fused(), split_composed()
    ff, fc = frame_fused(), frame_composed()
    torch.cuda.synchronize()
    same = {"split ctx": torch.equal(sf[0], sc[0]), "split crop": torch.equal(sf[1], sc[1]), "frame out": torch.equal(ff[0], fc[0]),
            "frame noisy": torch.equal(ff[1], fc[1])}
    if not all(same.values()):
        raise SystemExit(f"the fused and the composed form disagree: {same}")

    px = 16 * B                                   # bytes of one 8-channel 16-bit pixel, all samples
    rows = {
        # fused: x read once, framed image and crop written.  composed: + the framed image's window read again for the crop
        "split": (dict(fused=split_fused, composed=split_composed), 4 * B * C * H * H + px * (H * H + S * S), 1, 2),
        # fused: one 16-byte read per framed pixel (crop or surroundings), two writes
        "frame + noise": (dict(fused=frame_fused, composed=frame_composed), px * H * H + 2 * px * H * H, 1, 4),
    }
    lines = [f"shape: B = {B}, crop {S} x {S}, c = {c} (framed {H} x {H}), {a.dtype}, C = {C} in Cpad = {cpad}; {a.rounds} rounds of {a.calls} calls per form, "
             f"the forms alternating; device: {torch.cuda.get_device_name(0)}", "",
             "| launch | fused: us per call, median (min - max) | launches | bytes the fused form moves | rate over them | composed: us per call, median (min - max) | launches | composed / fused |",
             "|---|---|---|---|---|---|---|---|"]
    for label, (forms, nbytes, nl_f, nl_c) in rows.items():
        t = alternate(forms, a.warmup, a.calls, a.rounds)
        mf, mc = statistics.median(t["fused"]), statistics.median(t["composed"])
        rate = nbytes / (mf * 1e-3)
        lines.append(f"| {label} | {mf * 1e3:.1f} ({min(t['fused']) * 1e3:.1f} - {max(t['fused']) * 1e3:.1f}) | {nl_f} | {nbytes / 1e6:.1f} MB | "
                     f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of 8.0 (spec), {100 * rate / HBM_COPY:.0f} % of 6.29 (copy) | "
                     f"{mc * 1e3:.1f} ({min(t['composed']) * 1e3:.1f} - {max(t['composed']) * 1e3:.1f}) | {nl_c} | {mc / mf:.2f} |")
    lines += ["", "results compared before timing (bit-equal): " + ", ".join(same)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
