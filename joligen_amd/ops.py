"""Host-side operators over libjg355.so: thin launch wrappers, the autograd formulas that chain
the hand-written forward/backward kernels, and the `torch.ops.jg355.*` registrations.

Conventions
  * activations: 16-bit (torch.float16 / torch.bfloat16), logical AND physical NHWC
    `[B, H, W, C]` (or `[B, T, C]`), contiguous, C % 8 == 0;
  * parameters: fp32 views into a ParamArena (joligen_amd/arena.py); kernels ACCUMULATE parameter
    gradients straight into `param.grad` (an arena view) -- the autograd Functions return None
    for parameter inputs, which are passed only so that autograd tracks them;
  * every kernel is launched on torch's current stream; nothing here synchronises.

PyTorch is used for device memory (caching allocator), streams and the autograd tape only.
"""
from __future__ import annotations

import ctypes as C
import math
import os

from typing import Optional, Tuple

import torch

from ._autograd import JGFunction
from . import _lib
from ._lib import (JG_ACT_LRELU, JG_ACT_NONE, JG_ACT_RELU, JG_ACT_SILU, JG_ACT_TANH, JG_OUT_ATOMIC_F32, JG_OUT_STORE_T, ConvArgs,
                   WgradArgs, check)
from . import launch
from .launch import SINKHORN_ITERS, _DT, _dt, _p, _raw_stream, _st, sgemm  # noqa: F401  (plumbing, re-exported under its old names)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("joligen_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")


# ======================================================================================
# raw launchers
# ======================================================================================
# bench.py sets this to a list to time every launch of the dominant kernel with HIP events
# (start/stop recorded on the launch stream); entries: (kernel, ev_start, ev_stop, algorithmic flops)
KERNEL_TIMING = None
# fused (flash-style) attention kernel for head dim 32; JG_FLASH_ATTENTION=0 selects the GEMM + softmax pipeline
FLASH_ATTENTION = __import__("os").environ.get("JG_FLASH_ATTENTION", "1") != "0"

def _halo_ok(nbatch, H, W, Cin, Cout, R, S, pad, stride):
    """mirror of the dispatch conditions of conv_halo.hip / wgrad_halo.hip (labels for bench.py only)"""
    return (nbatch == 1 and R == 3 and S == 3 and pad == 1 and stride == 1 and Cin % 64 == 0 and Cout % 64 == 0
            and H % 16 == 0 and W % 16 == 0)


def _conv_kernel_name(nbatch, H, W, Cin, Cout, R, S, pad, stride, M=0):
    if _halo_ok(nbatch, H, W, Cin, Cout, R, S, pad, stride):
        return "conv3x3_halo_kernel"
    if (nbatch == 1 and R == 1 and S == 1 and pad == 0 and stride == 1 and Cin % 32 == 0 and Cin <= 256 and Cout % 64 == 0 and M >= 65536
            and M % 16 == 0 and os.environ.get("JG_CONV1X1", "1") != "0"):
        return "conv1x1_stream_kernel"
    if (nbatch == 1 and R == 3 and S == 3 and pad == 1 and stride == 1 and Cin == 8 and Cout % 64 == 0 and M >= 65536 and M % 16 == 0
            and os.environ.get("JG_CONV1X1", "1") != "0"):
        return "conv3x3_c8_stream_kernel"
    return "conv_nt_glds_kernel<256,64,64,4,1>" if Cout <= 64 else "conv_nt_glds_kernel<128,128,64,2,2>"


def _wgrad_kernel_name(nbatch, H, W, Cin, Cout, R, S, pad, stride, out_mode):
    if out_mode == JG_OUT_ATOMIC_F32 and _halo_ok(nbatch, H, W, Cin, Cout, R, S, pad, stride):
        return "wgrad3x3_halo_kernel"
    return "wgrad_tn_tr_kernel<1>" if Cout <= 64 else "wgrad_tn_tr_kernel<2>"


_CONV_WS = {}               # (device index, stream) -> fp32 scratch of the split-K form of the generic conv kernel (jg_conv_args.ws)
CONV_WS_BYTES = 32 << 20


def _conv_ws(dev):
    key = (dev.index, _raw_stream(dev.index))
    ws = _CONV_WS.get(key)
    if ws is None:
        ws = _CONV_WS[key] = torch.empty(CONV_WS_BYTES // 4, device=dev, dtype=torch.float32)
    return ws


def conv_nt(x, w, y, *, B, H, W, Cin, Cout, R, S, pad, stride, Ho, Wo, ldx, ldw, ldy, bias=None, res=None,
            ldres=0, alpha=1.0, res_scale=1.0, out_f32=False, nbatch=1, nh=1, sx=(0, 0), sw=(0, 0), sy=(0, 0),
            sr=(0, 0), x_off=0, w_off=0, y_off=0, dtype=None, stats=None, ldstats=0, stats_slots=1, gn_reduce=None, pad_mode=0, res_mode=0, x_mode=0, y_mode=0,
            apply=None, gn_bwd_apply=None):
    """jg_conv2d_nt with element offsets into the operand tensors.
    apply = (ab, y_norm, ldyn, act): jg_conv1x1_gn_apply -- the launch also writes act(a x + b) of its input; returns False (nothing
    launched) when the shape is not the streaming 1x1 kernel's.
    gn_bwd_apply = (gx, gdy, ab, pqr, add1, scale1, add2, scale2, act): jg_conv1x1_gn_bwd_apply -- the epilogue adds the GroupNorm-backward
    apply step of the output tensor; returns False likewise."""
    a = ConvArgs()
    es = 2
    a.x = x.data_ptr() + x_off * es
    a.w = w.data_ptr() + w_off * es
    a.y = y.data_ptr() + y_off * (4 if out_f32 else es)
    a.bias = _p(bias)
    a.res = _p(res)
    a.B, a.H, a.W, a.Cin, a.Cout, a.R, a.S, a.pad, a.stride, a.Ho, a.Wo = B, H, W, Cin, Cout, R, S, pad, stride, Ho, Wo
    a.ldx, a.ldw, a.ldy, a.ldres = ldx, ldw, ldy, ldres
    a.nbatch, a.nh = nbatch, nh
    a.sxb, a.sxh = sx
    a.swb, a.swh = sw
    a.syb, a.syh = sy
    a.srb, a.srh = sr
    a.alpha, a.res_scale, a.out_f32 = alpha, res_scale, int(out_f32)
    a.stats, a.ldstats, a.stats_slots = _p(stats), ldstats, stats_slots
    a.pad_mode = pad_mode
    a.res_mode = res_mode
    a.x_mode = x_mode
    a.y_mode = y_mode
    if B * Ho * Wo <= 16384 and R * S * Cin >= 1024:      # few output tiles, long reduction: let the library cut the K loop (needs scratch)
        ws = _conv_ws(x.device)
        a.ws, a.ws_bytes = ws.data_ptr(), CONV_WS_BYTES
    if gn_reduce is not None:   # (norm input x, pixel stride, ab coefficients, act): GroupNorm-backward reductions in the epilogue
        gx, gldx, gab, gact = gn_reduce
        a.stats_mode, a.gn_x, a.gn_ldx, a.gn_ab, a.gn_act = 1, gx.data_ptr(), gldx, gab.data_ptr(), gact
    if KERNEL_TIMING is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()  # current stream == the stream the kernel is launched on
    if gn_bwd_apply is not None:
        gx, gdy, gab, gpqr, a1, s1, a2, s2, gact = gn_bwd_apply
        rc = _lib.lib().jg_conv1x1_gn_bwd_apply(dtype if dtype is not None else _dt(x), C.byref(a), gx.data_ptr(), gx.stride(-2), gdy.data_ptr(),
                                                gdy.stride(-2), gab.data_ptr(), gpqr.data_ptr(), _p(a1), a1.stride(-2) if a1 is not None else 0, s1,
                                                _p(a2), a2.stride(-2) if a2 is not None else 0, s2, gact, _st())
        if rc == _lib.JG_ERR_UNSUPPORTED:
            return False
        check(rc, "jg_conv1x1_gn_bwd_apply")
    elif apply is not None:
        ab, yn, ldyn, act = apply
        rc = _lib.lib().jg_conv1x1_gn_apply(dtype if dtype is not None else _dt(x), C.byref(a), ab.data_ptr(), yn.data_ptr(), ldyn, act, _st())
        if rc == _lib.JG_ERR_UNSUPPORTED:
            return False
        check(rc, "jg_conv1x1_gn_apply")
    else:
        check(_lib.lib().jg_conv2d_nt(dtype if dtype is not None else _dt(x), C.byref(a), _st()), "jg_conv2d_nt")
    if KERNEL_TIMING is not None:
        ev1.record()
        ran = _lib.lib().jg_last_kernel().decode()      # the instance the dispatch picked ("" where the site records none)
        if x_mode == 2:    # sub-pixel form: 4 of the 9 tap-MACs per output pixel are executed -- count the MFMA work actually done
            KERNEL_TIMING.append((ran or "conv3x3_halo_kernel<subpixel>", ev0, ev1, 2.0 * B * Ho * Wo * Cout * 4 * Cin, (nbatch, B, Ho, Wo, Cin, Cout, 2),
                                  2.0 * nbatch * (B * (Ho // 2) * (Wo // 2) * Cin + B * Ho * Wo * Cout) + 2.0 * 16 * Cin * Cout))
        elif y_mode == 2:  # sub-pixel input gradient: 16 tap-MACs per low-resolution pixel (4 per pixel of dO); dO read once, the low-resolution result written once
            KERNEL_TIMING.append((ran or "conv3x3_halo_kernel<subpixel dgrad>", ev0, ev1, 2.0 * B * H * W * Cout * 4 * Cin, (nbatch, B, Ho, Wo, Cin, Cout, 2),
                                  2.0 * nbatch * (B * H * W * Cin + B * (Ho // 2) * (Wo // 2) * Cout) + 2.0 * 16 * Cin * Cout))
        else:
            KERNEL_TIMING.append((ran or _conv_kernel_name(nbatch, H, W, Cin, Cout, R, S, pad, stride, B * Ho * Wo if (stats is None or (R == 3 and Cin == 8 and gn_reduce is None)) else 0), ev0, ev1,
                                  2.0 * nbatch * B * Ho * Wo * Cout * R * S * Cin, (nbatch, B, Ho, Wo, Cin, Cout, R),
                                  # algorithmic HBM bytes: every input / output / residual element once (16-bit), the weights once; the fused
                                  # launches also move the normalised copy of the input (apply) or gx, gdy and the addends (gn_bwd_apply)
                                  2.0 * nbatch * (B * H * W * Cin + B * Ho * Wo * Cout * (2 if res is not None else 1)) + 2.0 * R * S * Cin * Cout
                                  + (2.0 * B * H * W * Cin if apply is not None else 0.0)
                                  + (2.0 * B * Ho * Wo * Cout * (2 + (gn_bwd_apply[4] is not None) + (gn_bwd_apply[6] is not None)) if gn_bwd_apply is not None else 0.0)))


def wgrad_tn(dy, x, dw, *, B, H, W, Cin, Cout, R, S, pad, stride, Ho, Wo, lddy, ldx, lddw, dbias=None, Cin_out=0,
             Cout_out=0, splitk=1, nbatch=1, nh=1, sdy=(0, 0), sx=(0, 0), sdw=(0, 0), alpha=1.0,
             out_mode=JG_OUT_ATOMIC_F32, dy_off=0, x_off=0, dw_off=0, dbias_scale=0.0, pad_mode=0, x_mode=0, defer=True):
    a = WgradArgs()
    a.dy = dy.data_ptr() + dy_off * 2
    a.x = x.data_ptr() + x_off * 2
    a.dw = dw.data_ptr() + dw_off * dw.element_size()
    a.dbias = _p(dbias)
    a.B, a.H, a.W, a.Cin, a.Cout, a.R, a.S, a.pad, a.stride, a.Ho, a.Wo = B, H, W, Cin, Cout, R, S, pad, stride, Ho, Wo
    a.Cin_out, a.Cout_out = Cin_out, Cout_out
    a.lddy, a.ldx, a.lddw = lddy, ldx, lddw
    a.nbatch, a.nh, a.splitk = nbatch, nh, splitk
    a.sdyb, a.sdyh = sdy
    a.sxb, a.sxh = sx
    a.sdwb, a.sdwh = sdw
    a.alpha, a.out_mode, a.dbias_scale = alpha, out_mode, dbias_scale
    a.pad_mode = pad_mode
    a.x_mode = x_mode
    # never under the torch.ops boundary: jg355::conv2d_wgrad hands a TEMPORARY dw / dbias back to autograd, which accumulates it into .grad at
    # once -- a launch deferred to the flush would write into a tensor nobody reads any more (silently zero gradients)
    if (defer and WGRAD_DEFER is not None and nbatch == 1 and out_mode == JG_OUT_ATOMIC_F32 and pad_mode == 0 and x_mode == 0 and KERNEL_TIMING is None
            and not TORCH_OPS_BOUNDARY and not _IN_OP):
        WGRAD_DEFER.append((_dt(dy), a, (dy, x, dw, dbias)))       # launched with its peers by flush_deferred_wgrads(); operands kept alive
        if _WGRAD_SIDE is not None and len(WGRAD_DEFER) >= _WGRAD_SIDE[1]:
            flush_deferred_wgrads()
        return
    if KERNEL_TIMING is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    check(_lib.lib().jg_conv2d_wgrad_tn(_dt(dy), C.byref(a), _st()), "jg_conv2d_wgrad_tn")
    if KERNEL_TIMING is not None:
        ev1.record()
        KERNEL_TIMING.append((_lib.lib().jg_last_kernel().decode() or _wgrad_kernel_name(nbatch, H, W, Cin, Cout, R, S, pad, stride, out_mode), ev0, ev1,
                              # x_mode 2 (sub-pixel form): 16 of the 36 tap-MACs per low-resolution pixel are executed -- the MFMA work actually done
                              2.0 * nbatch * B * Ho * Wo * Cout * (4 if x_mode == 2 else R * S) * Cin, (nbatch, B, Ho, Wo, Cin, Cout, R, splitk),
                              2.0 * nbatch * (B * H * W * Cin + B * Ho * Wo * Cout) + 4.0 * R * S * Cin * Cout))


# Deferred small weight gradients (round 5): inside `with deferred_wgrads():` every weight-gradient launch of a backward (plain zero padding) is
# collected instead of issued, and the context's exit issues them as GROUPED launches (jg_conv2d_wgrad_tn_group, 16 problems per grid).  The
# SegFormer generator's backward has ~190 of them per cut_model step, each a 10 - 40 us launch on 8 - 64 workgroups; they only feed the gradient
# arena (fp32 atomics), nothing downstream in the backward reads them.  Their operands (dy, x) stay alive until the flush.
WGRAD_DEFER = None
WGRAD_GROUP = os.environ.get("JG_WGRAD_GROUP", "1") != "0"


_WGRAD_SIDE = None          # (stream, flush threshold) of the active deferred_wgrads context, or None: flush on the current stream at the exit


def flush_deferred_wgrads():
    """issue the collected problems as grouped launches: on the current stream, or -- inside `deferred_wgrads(stream=...)` -- on that stream,
    ordered behind everything enqueued on the current stream so far (their operands are complete), leaving the current stream free to go on
    with the input-gradient chain"""
    global WGRAD_DEFER
    todo, WGRAD_DEFER = WGRAD_DEFER, ([] if WGRAD_DEFER is not None else None)
    if not todo:
        return 0
    by_dt = {}
    for dt, a, keep in todo:
        by_dt.setdefault(dt, []).append(a)
    if os.environ.get("JG_WGRAD_DUMP"):        # dev: the problems of one flush (tools/wgrad_group_model.py reads this)
        with open(os.environ["JG_WGRAD_DUMP"], "a") as f:
            f.write("flush %d\n" % len(todo))
            for dt, a, keep in todo:
                f.write("%d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (a.B, a.H, a.W, a.Cin, a.Cout, a.R, a.S, a.pad, a.stride, a.Ho, a.Wo, a.splitk, int(bool(a.dbias))))
    side = _WGRAD_SIDE[0] if _WGRAD_SIDE is not None else None
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
        for dt, a, keep in todo:
            for t in keep[:2]:
                t.record_stream(side)              # dy / x come from the current stream's allocator pool
        ctx = torch.cuda.stream(side)
    else:
        import contextlib

        ctx = contextlib.nullcontext()
    with ctx:
        for dt, args in by_dt.items():
            arr = (WgradArgs * len(args))(*args)
            check(_lib.lib().jg_conv2d_wgrad_tn_group(dt, arr, len(args), _st()), "jg_conv2d_wgrad_tn_group")
    return len(todo)


class deferred_wgrads:
    """collect the weight-gradient launches of the enclosed backward and issue them grouped (JG_WGRAD_GROUP=0: off).  Without `stream`: one flush at
    the exit, on the current stream.  With `stream`: a flush onto that stream every `every` collected problems and at the exit, where the current
    stream joins it -- the grouped launches are bandwidth-bound full-chip kernels, the backward chain next to them is a string of small launches."""

    def __init__(self, stream=None, every=48):
        self.stream, self.every = stream, every

    def __enter__(self):
        global WGRAD_DEFER, _WGRAD_SIDE
        self.prev = WGRAD_DEFER
        if WGRAD_GROUP and WGRAD_DEFER is None:
            WGRAD_DEFER = []
            _WGRAD_SIDE = (self.stream, self.every) if self.stream is not None else None
        return self

    def __exit__(self, *exc):
        global WGRAD_DEFER, _WGRAD_SIDE
        if self.prev is None and WGRAD_DEFER is not None:
            try:
                if exc[0] is None:
                    flush_deferred_wgrads()
                    if _WGRAD_SIDE is not None:
                        torch.cuda.current_stream().wait_stream(_WGRAD_SIDE[0])
            finally:
                WGRAD_DEFER = None
                _WGRAD_SIDE = None


def axpby(a, alpha=1.0, b=None, beta=0.0, alpha_dev=None, out=None):
    y = torch.empty_like(a) if out is None else out
    check(_lib.lib().jg_axpby(_dt(a), a.data_ptr(), alpha, _p(alpha_dev), _p(b), beta, y.data_ptr(), a.numel(), _st()),
          "jg_axpby")
    return y


# ======================================================================================
# convolution
# ======================================================================================
class ConvMeta:
    """Geometry + working weight copies of one conv layer (filled by ParamArena)."""

    __slots__ = ("Cin", "Cout", "Cin_real", "Cout_real", "R", "S", "pad", "stride", "w16", "w16T", "weight", "bias",
                 "bias_pad")

    def out_hw(self, H, W):
        return ((H + 2 * self.pad - self.R) // self.stride + 1, (W + 2 * self.pad - self.S) // self.stride + 1)


WGRAD_TARGET_BLOCKS = int(os.environ.get("JG_WGRAD_TARGET_BLOCKS", "1536"))
WGRAD_MAX_SPLITK = 512  # deeper splits only add atomic traffic on a tiny output
WGRAD_SPLIT_PIX = int(os.environ.get("JG_WGRAD_SPLIT_PIX", "256"))     # fewest pixels a K slice of the weight gradient is worth


def _wgrad_splitk(tiles, mpix, nbatch=1):
    want = max(1, (WGRAD_TARGET_BLOCKS + tiles - 1) // tiles)
    cap = max(1, mpix // WGRAD_SPLIT_PIX)
    return max(1, min(want, cap, WGRAD_MAX_SPLITK, 65535 // max(1, nbatch)))


def conv2d_forward(x, m: ConvMeta, res=None, res_scale=1.0, alpha=1.0, stats=None):
    _require_cuda(x)
    B, H, W, Cin = x.shape
    assert Cin == m.Cin, (Cin, m.Cin)
    Ho, Wo = m.out_hw(H, W)
    y = torch.empty((B, Ho, Wo, m.Cout), device=x.device, dtype=x.dtype)
    conv_nt(x, m.w16, y, B=B, H=H, W=W, Cin=Cin, Cout=m.Cout, R=m.R, S=m.S, pad=m.pad, stride=m.stride, Ho=Ho, Wo=Wo,
            ldx=Cin, ldw=m.R * m.S * Cin, ldy=m.Cout, bias=m.bias_pad if m.bias_pad is not None else m.bias, res=res,
            ldres=m.Cout, alpha=alpha, res_scale=res_scale, stats=stats)
    return y


def dilate2d(x, Ho, Wo, stride):
    """zero insertion: y[:, s*i, s*j] = x[:, i, j] in a [B, Ho, Wo, C] buffer."""
    B, H, W, Cc = x.shape
    y = torch.empty((B, Ho, Wo, Cc), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_dilate2d(_dt(x), x.contiguous().data_ptr(), y.data_ptr(), B, H, W, Cc, Ho, Wo, stride, _st()), "jg_dilate2d")
    return y


# stride-2 transposed convolutions (input gradient of a stride-2 convolution, nn.ConvTranspose2d) in the four-phase form of the halo-resident
# kernel (jg_transposed_fold + jg_conv2d_nt x_mode 2) instead of a zero-dilated copy + a stride-1 convolution over it; JG_PHASE_TCONV=0: off
PHASE_TCONV = os.environ.get("JG_PHASE_TCONV", "1") != "0"
PATCH_DGRAD = os.environ.get("JG_PATCH_DGRAD", "1") != "0"      # round 6: input gradient of kernel == stride convolutions as one GEMM (conv2d_dgrad)


def phase_tconv_ok(m: ConvMeta, Hout, Wout, C, N):
    """shape limits of the phase form: kernel 3 or 4, stride 2, padding 1, output exactly twice the input, the halo kernel's channel / tile multiples"""
    return (PHASE_TCONV and m.stride == 2 and m.R == m.S and m.R in (3, 4) and m.pad == 1 and C % 64 == 0 and N % 64 == 0 and Hout % 32 == 0
            and Wout % 32 == 0)


def phase_tconv(x, m: ConvMeta, y, bias=None, alpha=1.0):
    """y [B, 2h, 2w, N] = transposed convolution of x [B, h, w, C] with the strided convolution's weights (m.w16T [N][R][S][C])"""
    B, h, w, C = x.shape
    N = y.shape[-1]
    wf = torch.empty((4, N, 2, 2, C), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_transposed_fold(_dt(x), m.w16T.data_ptr(), wf.data_ptr(), N, C, m.R, m.S, m.pad, _st()), "jg_transposed_fold")
    conv_nt(x, wf, y, B=B, H=2 * h, W=2 * w, Cin=C, Cout=N, R=3, S=3, pad=1, stride=1, Ho=2 * h, Wo=2 * w, ldx=C, ldw=4 * C, ldy=N, bias=bias,
            alpha=alpha, x_mode=2)
    return y


def conv2d_dgrad(dy, m: ConvMeta, x_shape, alpha=1.0):
    """dx = conv(dy, flipped/transposed weights).  Stride s > 1: the same stride-1 convolution over the zero-dilated
    dy (length H + 2p - k + 1 per axis) with pad k-1-p."""
    B, H, W, Cin = x_shape
    _, Ho, Wo, Cout = dy.shape
    dx = torch.empty(x_shape, device=dy.device, dtype=dy.dtype)
    if m.stride != 1:
        if H == 2 * Ho and W == 2 * Wo and phase_tconv_ok(m, H, W, Cout, Cin):
            return phase_tconv(dy, m, dx, alpha=alpha)
        if (PATCH_DGRAD and Cin == 8 and m.Cin_real <= 4 and Cout % 8 == 0 and m.R * m.S * Cout * 16 <= 65536
                and Ho == (H + 2 * m.pad - m.R) // m.stride + 1 and Wo == (W + 2 * m.pad - m.S) // m.stride + 1):
            # onto an image (<= 4 real channels): gather form, s^2 x fewer multiply-adds than the dilated convolution and no MFMA padding of 3 -> 8
            check(_lib.lib().jg_conv_dgrad_gather(_dt(dy), dy.contiguous().data_ptr(), m.w16.data_ptr(), dx.data_ptr(), B, H, W, Ho, Wo, Cout, m.R, m.S,
                                                  m.stride, m.pad, alpha, _st()), "jg_conv_dgrad_gather")
            return dx
        if PATCH_DGRAD and m.stride == m.R == m.S and m.pad == 0 and H == Ho * m.R and W == Wo * m.S:
            # kernel == stride (the spatial-reduction convolutions of the MiT attention, segformer/backbone.py): the patches do not overlap, the
            # input gradient of a patch is dy . W -- ONE GEMM with R S Cin output columns per output pixel + a depth-to-space copy.  (The dilated
            # form below runs an R x S convolution over a tensor of which one tap in R S is non-zero: 64 x the MFMA work at sr_ratio 8.)
            N = m.R * m.S * Cin
            wt = m.w16.view(Cout, N).t().contiguous()                          # [(ky, kx, ci)][co]
            tmp = torch.empty((B, Ho, Wo, N), device=dy.device, dtype=dy.dtype)
            conv_nt(dy, wt, tmp, B=B, H=Ho, W=Wo, Cin=Cout, Cout=N, R=1, S=1, pad=0, stride=1, Ho=Ho, Wo=Wo, ldx=Cout, ldw=Cout, ldy=N, alpha=alpha)
            dx.view(B, Ho, m.R, Wo, m.S, Cin).copy_(tmp.view(B, Ho, Wo, m.R, m.S, Cin).permute(0, 1, 3, 2, 4, 5))
            return dx
        Hd, Wd = H + 2 * m.pad - m.R + 1, W + 2 * m.pad - m.S + 1
        dyd = dilate2d(dy, Hd, Wd, m.stride)
        conv_nt(dyd, m.w16T, dx, B=B, H=Hd, W=Wd, Cin=Cout, Cout=Cin, R=m.R, S=m.S, pad=m.R - 1 - m.pad, stride=1, Ho=H, Wo=W,
                ldx=Cout, ldw=m.R * m.S * Cout, ldy=Cin, alpha=alpha)
        return dx
    conv_nt(dy, m.w16T, dx, B=B, H=Ho, W=Wo, Cin=Cout, Cout=Cin, R=m.R, S=m.S, pad=m.R - 1 - m.pad, stride=1, Ho=H, Wo=W,
            ldx=Cout, ldw=m.R * m.S * Cout, ldy=Cin, alpha=alpha)
    return dx


def conv2d_wgrad(dy, x, m: ConvMeta, alpha=1.0, want_w=True, want_b=True):
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    wg = m.weight.grad
    if wg is None:
        raise RuntimeError("conv weight has no arena-backed .grad (module not finalised by ParamArena)")
    ktot = m.R * m.S * Cin
    tiles = ((Cout + 127) // 128) * ((ktot + 127) // 128)  # Cout <= 64 runs the 64-row tile: same count
    splitk = _wgrad_splitk(tiles, B * Ho * Wo)
    dbias = m.bias.grad if (want_b and m.bias is not None) else None
    wgrad_tn(dy, x, wg, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=m.R, S=m.S, pad=m.pad, stride=m.stride, Ho=Ho, Wo=Wo,
             lddy=Cout, ldx=Cin, lddw=m.R * m.S * m.Cin_real, dbias=dbias, Cin_out=m.Cin_real, Cout_out=m.Cout_real,
             splitk=splitk, alpha=alpha)


# ---- row-packed 7x7 head (round 6) -----------------------------------------------------------------------------------------------------------
HEAD7_PACKED = os.environ.get("JG_HEAD7_PACKED", "1") != "0"
_HEAD7_BUFS = {}      # per convolution (keyed by its 16-bit weight copy): the packed weight buffers of _Head7x7Fn


def head7_ok(x_pad, m: ConvMeta):
    """shapes the row-packed form serves: 7x7, stride 1, no padding of its own (the caller has reflect-padded), 64 k input channels, <= 4 real
    output channels, a map the halo-resident kernels tile (W a multiple of 16)"""
    if not HEAD7_PACKED or TORCH_OPS_BOUNDARY or KERNEL_TIMING is not None or not x_pad.is_cuda:
        return False
    B, Hp, Wp, Cin = x_pad.shape
    return (m.R == 7 and m.S == 7 and m.stride == 1 and m.pad == 0 and Cin == m.Cin and Cin % 64 == 0 and m.Cout_real <= 4 and (Wp - 6) % 16 == 0
            and Hp > 6 and B * (Hp - 6) * (Wp - 6) >= 65536 and x_pad.dtype in (torch.float16, torch.bfloat16))


class _Head7x7Fn(JGFunction):
    """act(conv7x7(x_pad) + b) for <= 4 output channels, row-packed (csrc/elementwise.hip tapsum7): a 1 x 7 convolution onto 7 x 4 packed
    channels on the halo-resident kernel, then the sum over the tap rows -- 7 x fewer multiply-adds than the 7x7 convolution whose 3 output
    channels are padded to an MFMA tile of 32; the backward is the same two steps transposed."""

    @staticmethod
    def forward(ctx, x_pad, weight, bias, meta, act):
        m = meta
        x_pad = x_pad.contiguous()
        B, Hp, Wp, Cin = x_pad.shape
        H, W = Hp - 6, Wp - 6
        dev, dt = x_pad.device, x_pad.dtype
        # packed weight copies, rebuilt from the arena's 16-bit copy on every forward (two small launches; the buffers persist with the module so
        # that a captured graph replays into the same addresses): wz [32 = (ky, c)][1][7][Cin] for the forward stage and the weight
        # gradient's layout, wzT [Cin][1][7 flipped][32] for the input-gradient stage
        key = (m.w16.data_ptr(), dt, Cin)
        bufs = _HEAD7_BUFS.get(key)
        if bufs is None:
            bufs = _HEAD7_BUFS[key] = (torch.zeros((8, 4, 7, Cin), device=dev, dtype=dt), torch.zeros((Cin, 7, 8, 4), device=dev, dtype=dt))
        wz, wzT = bufs
        wz[:7].copy_(m.w16[:4].permute(1, 0, 2, 3))
        wzT[:, :, :7].copy_(m.w16[:4].permute(3, 2, 1, 0).flip(1))              # [ci][6 - kx][ky][c]
        z = torch.empty((B, Hp, W, 32), device=dev, dtype=dt)
        conv_nt(x_pad, wz, z, B=B, H=Hp, W=Wp, Cin=Cin, Cout=32, R=1, S=7, pad=0, stride=1, Ho=Hp, Wo=W, ldx=Cin, ldw=7 * Cin, ldy=32)
        out = torch.empty((B, H, W, 8), device=dev, dtype=dt)
        b4 = m.bias_pad                                                        # fp32, padded to the 8-channel pixel (None: no bias)
        if b4 is None and m.bias is not None:
            b4 = torch.zeros(4, device=dev, dtype=torch.float32)
            b4[:m.Cout_real].copy_(m.bias.detach()[:m.Cout_real])
        check(_lib.lib().jg_tapsum7(_dt(x_pad), z.data_ptr(), _p(b4), out.data_ptr(), B, H, W, act, _st()), "jg_tapsum7")
        ctx.save_for_backward(x_pad, out, wzT)
        ctx.cfg = (m, act)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x_pad, out, wzT = ctx.saved_tensors
        m, act = ctx.cfg
        dout = dout.contiguous()
        B, Hp, Wp, Cin = x_pad.shape
        H, W = Hp - 6, Wp - 6
        dev, dt = x_pad.device, x_pad.dtype
        Hz = (Hp + 7) // 8 * 8
        dz = torch.empty((B, Hz, W, 32), device=dev, dtype=dt)
        dzm = torch.empty((B, Hp, W + 12, 32), device=dev, dtype=dt)
        check(_lib.lib().jg_tapspread7(_dt(dout), dout.data_ptr(), out.data_ptr(), dz.data_ptr(), dzm.data_ptr(), B, H, W, Hz, act, _st()), "jg_tapspread7")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x_pad)
            conv_nt(dzm, wzT, dx, B=B, H=Hp, W=W + 12, Cin=32, Cout=Cin, R=1, S=7, pad=0, stride=1, Ho=Hp, Wo=Wp, ldx=32, ldw=7 * 32, ldy=Cin)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            wg = m.weight.grad
            if wg is None:
                raise RuntimeError("conv weight has no arena-backed .grad (module not finalised by ParamArena)")
            acc = torch.zeros(32 * 7 * Cin + 32, device=dev, dtype=torch.float32)          # packed weight gradient + bias sums, one clear
            dwz, db = acc[:32 * 7 * Cin].view(8, 4, 7, Cin), acc[32 * 7 * Cin:]
            wgrad_tn(dz, x_pad, dwz, B=B, H=Hp, W=Wp, Cin=Cin, Cout=32, R=1, S=7, pad=0, stride=1, Ho=Hz, Wo=W, lddy=32, ldx=Cin, lddw=7 * Cin, dbias=db,
                     Cin_out=Cin, Cout_out=32, splitk=1, defer=False)
            cr = m.Cout_real
            wg.permute(0, 2, 3, 1)[:cr].add_(dwz[:7, :cr].permute(1, 0, 2, 3)[..., :m.Cin_real])      # physical [Cout][R][S][Cin]
            if m.bias is not None and ctx.needs_input_grad[2]:
                m.bias.grad[:cr].add_(db[:cr])
        return dx, None, None, None, None


def head_conv7(x_pad, m: ConvMeta, act=0):
    """ReflectionPad2d(3)'s output -> act(Conv2d(Cin, <= 4, 7)(x_pad)) [B, H, W, 8]; callers check head7_ok first"""
    return _Head7x7Fn.apply(x_pad, m.weight, m.bias, m, act)


class _Conv2dFn(JGFunction):
    @staticmethod
    def forward(ctx, x, weight, bias, res, meta, res_scale, alpha, stats=None):
        # stats (round 6, conv2d_stats): a zeroed fp32 [B, Cout, 2] buffer the launch's epilogue fills with the per-(image, channel) sum and sum
        # of squares of its output -- the statistics pass of the InstanceNorm / GroupNorm that follows (not a differentiable input)
        y = conv2d_forward(x, meta, res, res_scale, alpha, stats)
        ctx.save_for_backward(x)
        ctx.meta, ctx.res_scale, ctx.alpha, ctx.has_res = meta, res_scale, alpha, res is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        m = ctx.meta
        dy = dy.contiguous()
        dx = dres = None
        if ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(dy, m, x.shape, ctx.alpha)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            conv2d_wgrad(dy, x, m, ctx.alpha, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        if ctx.has_res and ctx.needs_input_grad[3]:
            dres = dy if ctx.res_scale == 1.0 else axpby(dy, ctx.res_scale)
        return dx, None, None, dres, None, None, None, None


# torch.ops boundary mode: inside `with torch_ops_boundary():` every op of the palette step -- convolutions, norms,
# attention, resampling, the embedding MLPs, q_sample and the loss -- is a call of `torch.ops.jg355.*` (torch.library custom ops with
# fake kernels and autograd formulas) on the fp32 master parameters; concatenations / scalings are plain ATen ops and autograd assembles
# the backward.  Same kernels through the same C ABI; what it gives up is what the arena-accumulating nodes and the fused UNet schedule
# exist for (no gradient copies, one autograd node).  tests/test_gpu_1_model.py::test_palette_step_through_torch_ops pins the two forms.
TORCH_OPS_BOUNDARY = False


class torch_ops_boundary:
    def __enter__(self):
        global TORCH_OPS_BOUNDARY
        self.prev, TORCH_OPS_BOUNDARY = TORCH_OPS_BOUNDARY, True

    def __exit__(self, *a):
        global TORCH_OPS_BOUNDARY
        TORCH_OPS_BOUNDARY = self.prev


def _conv2d_via_torch_ops(x, m: ConvMeta, res, res_scale, alpha):
    """the layer on torch.ops.jg355.conv2d_nt with its fp32 MASTER weight as a differentiable input ([Cout, R, S, Cin], zero-padded to
    the 8-channel granularity of the activations like the arena's working copy)"""
    import torch.nn.functional as F

    w = m.weight.reshape(m.Cout_real, m.Cin_real, m.R, m.S).permute(0, 2, 3, 1)
    b = m.bias
    if m.Cin != m.Cin_real or m.Cout != m.Cout_real:
        w = F.pad(w, (0, m.Cin - m.Cin_real, 0, 0, 0, 0, 0, m.Cout - m.Cout_real))
        if b is not None:
            b = F.pad(b, (0, m.Cout - m.Cout_real))
    return torch.ops.jg355.conv2d_nt(x, w, b, res, m.pad, m.stride, alpha, res_scale if res is not None else 0.0)


# round 6, A/B: InstanceNorm statistics of the mobile ResNet blocks in the epilogue of the point-wise convolution in front (jg_conv_args.stats, as the
# fused UNet schedule does for its 3x3 layers).  MEASURED SLOWER: mobile_resnet_attn + [projected_d, basic] 45.0 -> 49.3 ms -- on a 45 us GEMM-shaped
# launch the LDS-transposed reduction + 256 fp32 atomics per tile cost more than the 27 us statistics pass they replace.  Off.
CONV_STATS = os.environ.get("JG_CONV_STATS", "0") != "0"


def conv2d_stats(x, meta: ConvMeta):
    """(conv2d(x), sums): sums fp32 [B, Cout, 2] = per-(image, channel) sum / sum of squares of the output, accumulated by the convolution's
    epilogue (jg_conv_args.stats) -- hand it to group_norm(..., sums=sums) and the norm skips its statistics pass; None where the epilogue form
    does not exist (shape limits of jg_conv2d_nt's stats: whole 256-pixel tiles inside an image, 64-channel multiples; op boundary; timing runs)"""
    B, H, W, _ = x.shape
    Ho, Wo = meta.out_hw(H, W)
    if (not CONV_STATS or TORCH_OPS_BOUNDARY or KERNEL_TIMING is not None or (Ho * Wo) % 256 or meta.Cout % 64 or meta.R != meta.S or meta.R not in (1, 3)
            or meta.stride != 1 or _lib.lib().jg_get_tuning(b"JG_DETERMINISTIC") != 0):
        return conv2d(x, meta), None
    sums = torch.zeros((B, meta.Cout, 2), device=x.device, dtype=torch.float32)
    return _Conv2dFn.apply(x, meta.weight, meta.bias, None, meta, 1.0, 1.0, sums), sums


def conv2d(x, meta: ConvMeta, res=None, res_scale=1.0, alpha=1.0):
    """y = alpha*conv(x) + bias + res_scale*res   (nn.Conv2d / Conv1d(k=1) of the reference)."""
    if TORCH_OPS_BOUNDARY:
        return _conv2d_via_torch_ops(x, meta, res, res_scale, alpha)
    return _Conv2dFn.apply(x, meta.weight, meta.bias, res, meta, res_scale, alpha)


# input gradient of the reflect-padded 3x3 convolutions on the halo-resident kernel + a ring kernel (1, round 6) or as a full convolution over
# the padded domain on the im2col kernel + reflect_pad_bwd (0: rounds 1-5)
REFLECT_DGRAD_HALO = os.environ.get("JG_REFLECT_DGRAD_HALO", "1") != "0"


def reflect_conv_ok(x, m: ConvMeta):
    """shape limits of pad_mode = 1 (halo-resident kernels): ReflectionPad2d(1) + 3x3 / stride 1 / pad 0 convolution"""
    B, H, W, Cin = x.shape
    return (m.R == 3 and m.S == 3 and m.stride == 1 and m.pad == 0 and Cin % 64 == 0 and m.Cout % 64 == 0 and H % 16 == 0
            and W % 16 == 0 and H >= 16 and W >= 16 and B * H * W * max(Cin, m.Cout) < (1 << 31))


class _ReflectConv2dFn(JGFunction):
    """nn.ReflectionPad2d(1) -> nn.Conv2d(3x3, padding 0) as one launch: the halo-resident kernel mirrors the border pixels while
    it loads its halo, so the padded tensor is never written.  Backward: the weight gradient reads x with the same mirrored halo;
    the input gradient is the full convolution over the (H+2, W+2) padded domain folded back by the reflection's adjoint."""

    @staticmethod
    def forward(ctx, x, weight, bias, meta, with_identity=False):
        _require_cuda(x)
        x = x.contiguous()
        B, H, W, Cin = x.shape
        m = meta
        y = torch.empty((B, H, W, m.Cout), device=x.device, dtype=x.dtype)
        conv_nt(x, m.w16, y, B=B, H=H, W=W, Cin=Cin, Cout=m.Cout, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=Cin, ldw=9 * Cin,
                ldy=m.Cout, bias=m.bias_pad if m.bias_pad is not None else m.bias, pad_mode=1)
        ctx.save_for_backward(x)
        ctx.meta = m
        ctx.with_identity = with_identity
        if with_identity:          # (x, conv(x)): the gradient of the residual branch `x + f(x)` comes back through the first output
            return x.view_as(x), y
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        (x,) = ctx.saved_tensors
        m = ctx.meta
        did, dy = grads if ctx.with_identity else (None, grads[0])
        if dy is None:
            return did, None, None, None, None
        dy = dy.contiguous()
        B, H, W, Cin = x.shape
        dx = None
        if ctx.needs_input_grad[0]:
            if REFLECT_DGRAD_HALO and m.Cout % 64 == 0 and Cin % 64 == 0:
                # round 6: the interior of the padded-domain gradient IS the zero-padded input gradient on H x W (halo-resident kernel); the
                # one-pixel ring of the reflection's adjoint is added by jg_reflect_dgrad_border (csrc/reflect_border.hip).  The residual
                # branch's gradient (with_identity) rides in as the residual addend of that convolution: no accumulation launch of autograd's
                dx = torch.empty_like(x)
                res = did.contiguous() if did is not None else None
                did = None
                conv_nt(dy, m.w16T, dx, B=B, H=H, W=W, Cin=m.Cout, Cout=Cin, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, ldx=m.Cout, ldw=9 * m.Cout,
                        ldy=Cin, res=res, ldres=Cin)
                ws = torch.empty(_lib.lib().jg_reflect_dgrad_border_ws_floats(B, H, W, Cin), device=x.device, dtype=torch.float32)
                check(_lib.lib().jg_reflect_dgrad_border(_dt(dy), dy.data_ptr(), m.Cout, m.w16T.data_ptr(), dx.data_ptr(), Cin, ws.data_ptr(), B, H, W,
                                                         m.Cout, Cin, 1.0, _st()), "jg_reflect_dgrad_border")
            else:
                dx = launch.reflect_pad2d_bwd(conv2d_dgrad(dy, m, (B, H + 2, W + 2, Cin)), 1)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            wg = m.weight.grad
            if wg is None:
                raise RuntimeError("conv weight has no arena-backed .grad (module not finalised by ParamArena)")
            dbias = m.bias.grad if (ctx.needs_input_grad[2] and m.bias is not None) else None
            wgrad_tn(dy, x, wg, B=B, H=H, W=W, Cin=Cin, Cout=m.Cout, R=3, S=3, pad=1, stride=1, Ho=H, Wo=W, lddy=m.Cout, ldx=Cin,
                     lddw=9 * m.Cin_real, dbias=dbias, Cin_out=m.Cin_real, Cout_out=m.Cout_real,
                     splitk=_wgrad_splitk(((m.Cout + 127) // 128) * ((9 * Cin + 127) // 128), B * H * W), pad_mode=1)
        if did is not None and dx is not None:          # (the fold path: no residual epilogue there)
            dx = axpby(dx, 1.0, did.contiguous(), 1.0)
        elif did is not None:
            dx = did
        return dx, None, None, None, None


def reflect_conv2d_id(x, meta: ConvMeta):
    """(x, conv(reflection_pad(x, 1))): use the first output as the identity of `x + f(x)` -- its gradient is added inside the input-gradient
    convolution of this layer (round 6) instead of by autograd's accumulation kernel"""
    return _ReflectConv2dFn.apply(x, meta.weight, meta.bias, meta, True)


def reflect_conv2d(x, meta: ConvMeta):
    """conv(reflection_pad(x, 1)) for a 3x3 / pad-0 ConvMeta (see reflect_conv_ok)."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.reflect_conv2d(x, meta.weight.permute(0, 2, 3, 1), meta.bias)
    return _ReflectConv2dFn.apply(x, meta.weight, meta.bias, meta)


# ======================================================================================
# GroupNorm (+FiLM, +SiLU) / InstanceNorm1d
# ======================================================================================
# Zeroed fp32 scratch for the accumulating reductions of the norm nodes (round 6): jg_gn_stats / jg_gn_bwd_reduce clear their [B, C, 2] rows with a
# hipMemsetAsync of their own -- one 5 us launch per norm and direction, 245 per step of the mobile ResNet generator.  The rows now come out of a
# chunk that ONE torch.zeros clears (4 MB, ~60 norms); a chunk lives as long as any row handed out of it.
ZERO_POOL = os.environ.get("JG_ZERO_POOL", "1") != "0"
_ZERO_CHUNK = {}


def zero_pool_reset(device=None, allocate=False):
    """forget the current chunk(s); allocate: start a fresh one NOW on the current stream.  A hipGraph capture calls this as its first action
    (allocate=True: the chunk's clear becomes a node of THAT graph and is replayed with it) and again after the capture (the eager code must
    not take rows out of a captured chunk, whose clear it does not replay)."""
    for k in [k for k in _ZERO_CHUNK if device is None or k[0] == device]:
        del _ZERO_CHUNK[k]
    if allocate and ZERO_POOL and device is not None:
        _ZERO_CHUNK[(device, torch.cuda.current_stream(device).cuda_stream)] = [torch.zeros(1 << 20, device=device, dtype=torch.float32), 0,
                                                                               torch.cuda.is_current_stream_capturing()]


def zeros_f32(n, device):
    """n zeroed fp32 values (a view of a pooled chunk; never written by anyone else).  Chunks are per STREAM: a row is used on the stream
    that enqueued its chunk's clear (a forked branch of a capture gets a chunk of its own, cleared on that branch).  Inside a capture that did
    not prepare a chunk (zero_pool_reset) every request is a torch.zeros of its own: a row is only ever cleared by a launch of the graph
    that accumulates into it."""
    n = (int(n) + 63) // 64 * 64
    if not ZERO_POOL or n > (1 << 18) or device.type != "cuda":
        return torch.zeros(n, device=device, dtype=torch.float32)
    cap = torch.cuda.is_current_stream_capturing()
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    st = _ZERO_CHUNK.get(key)
    if st is not None and st[2] != cap:
        st = None
    if st is None and cap and not any(v[2] for v in _ZERO_CHUNK.values()):
        return torch.zeros(n, device=device, dtype=torch.float32)          # a capture that did not opt in
    if st is None or st[1] + n > st[0].numel():
        st = _ZERO_CHUNK[key] = [torch.zeros(1 << 20, device=device, dtype=torch.float32), 0, cap]
    out = st[0][st[1]:st[1] + n]
    st[1] += n
    return out


def _drop_args(x, keep, u, key, stream, call, shape=None):
    """the checked dropout arguments (keep, u, key, stream, call) of the fused passes of csrc/dropout.hip: u fp32 [B, C, H, W] injected uniforms
    or None = drawn in the kernel from the two-word device tensor `key` (d_aug_key); shape: that of the mask [B, H, W, C] where it is not x's"""
    keep, stream, call = float(keep), int(stream), int(call)
    if x.dim() != 4 or not 0.0 < keep <= 1.0 or not 0 <= stream < 65536 or not 0 <= call < 2 ** 32:
        raise ValueError(f"dropout: x [B, H, W, C], keep in (0, 1], stream < 65536 (got {tuple(x.shape)}, keep={keep}, stream={stream}, call={call})")
    B, H, W, C = x.shape if shape is None else shape
    if u is not None:
        if u.dtype != torch.float32 or tuple(u.shape) != (B, C, H, W):
            raise ValueError(f"dropout: u must be fp32 [B, C, H, W] = {(B, C, H, W)}, got {u.dtype} {tuple(u.shape)}")
        u, key = u.contiguous(), None
    elif key is None or key.numel() != 2 or key.element_size() != 4:
        raise ValueError("dropout: a draw needs the two-word Philox key (ops.d_aug_key)")
    _require_cuda(x, u, key)
    return keep, u, key, stream, call


def _group_norm_launch(x, gamma, beta, film, G, act, eps, sums=None, add=None, drop=None):
    """the GroupNorm forward chain: statistics (unless given), coefficients, apply (+ add) -> (y, ab [B, C, 2], mr [B, G, 2]);
    drop = (keep, u, key, stream, call): nn.Dropout behind the activation, inside the apply pass"""
    _require_cuda(x)
    L = _lib.lib()
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    dev, st, dt = x.device, _st(), _dt(x)
    ab = torch.empty((B, C, 2), device=dev, dtype=torch.float32)
    mr = torch.empty((B, G, 2), device=dev, dtype=torch.float32)
    ldfilm = film.stride(0) if film is not None else 0
    if sums is None:            # (given: the producing convolution's epilogue has accumulated them, ops.conv2d_stats)
        sums = zeros_f32(B * C * 2, dev)[:B * C * 2].view(B, C, 2)
        check(L.jg_gn_stats_ld(dt, x.data_ptr(), C, sums.data_ptr(), C, B, HW, C, st), "jg_gn_stats_ld")
    check(L.jg_gn_coef(sums.data_ptr(), _p(gamma), _p(beta), _p(film), ldfilm, ab.data_ptr(), mr.data_ptr(), B, HW, C,
                       G, eps, st), "jg_gn_coef")
    if drop is not None:
        return launch.gn_apply_drop(x, ab, act, *drop), ab, mr
    y = torch.empty_like(x)
    if add is not None:          # y = act(norm(x)) + add in the apply pass (round 6); d(add) = dy
        add = add.contiguous()
        check(L.jg_gn_apply_add(dt, x.data_ptr(), C, ab.data_ptr(), add.data_ptr(), C, y.data_ptr(), C, B, HW, C, act, st), "jg_gn_apply_add")
    else:
        check(L.jg_gn_apply(dt, x.data_ptr(), ab.data_ptr(), y.data_ptr(), B, HW, C, act, st), "jg_gn_apply")
    return y, ab, mr


class _GroupNormFn(JGFunction):
    @staticmethod
    def forward(ctx, x, gamma, beta, film, G, act, eps, sums=None, add=None):
        y, ab, mr = _group_norm_launch(x, gamma, beta, film, G, act, eps, sums, add)
        ctx.save_for_backward(x, ab, mr, gamma, beta, film)
        ctx.G, ctx.act = G, act
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, ab, mr, gamma, beta, film = ctx.saved_tensors
        L = _lib.lib()
        dy = dy.contiguous()
        B, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * C)
        dev, st, dt = x.device, _st(), _dt(x)
        red = zeros_f32(B * C * 2, dev)[:B * C * 2].view(B, C, 2)
        pqr = torch.empty((B, C, 3), device=dev, dtype=torch.float32)
        want_film = film is not None and ctx.needs_input_grad[3]
        dfilm = torch.empty((B, 2 * C), device=dev, dtype=torch.float32) if want_film else None
        dgamma = gamma.grad if (gamma is not None and ctx.needs_input_grad[1]) else None
        dbeta = beta.grad if (beta is not None and ctx.needs_input_grad[2]) else None
        if (gamma is not None and ctx.needs_input_grad[1] and dgamma is None):
            raise RuntimeError("norm weight has no arena-backed .grad")
        ldfilm = film.stride(0) if film is not None else 0
        check(L.jg_gn_bwd_reduce_ld_acc(dt, x.data_ptr(), C, dy.data_ptr(), C, ab.data_ptr(), red.data_ptr(), B, HW, C, ctx.act, st),
              "jg_gn_bwd_reduce_ld_acc")
        check(L.jg_gn_bwd_coef(red.data_ptr(), _p(gamma), _p(beta), _p(film), ldfilm, mr.data_ptr(), pqr.data_ptr(),
                               _p(dgamma), _p(dbeta), _p(dfilm), 2 * C, B, HW, C, ctx.G, st), "jg_gn_bwd_coef")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(L.jg_gn_bwd_apply(dt, x.data_ptr(), dy.data_ptr(), ab.data_ptr(), pqr.data_ptr(), dx.data_ptr(), B, HW,
                                    C, ctx.act, st), "jg_gn_bwd_apply")
        return dx, None, None, dfilm, None, None, None, None, (dy if ctx.needs_input_grad[8] else None)


def _gn_drop_bwd_launch(x, dy, ab, mr, gamma, beta, film, G, act, drop, red, dgamma, dbeta, dfilm, want_dx=True):
    """the GroupNorm backward chain behind a fused dropout: reduce (mask regenerated) -> coefficients -> apply (mask regenerated); `red` is
    zeroed [B, C, 2]; dgamma / dbeta are accumulated into, dfilm is written (None: not wanted) -> dx"""
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    pqr = torch.empty((B, C, 3), device=x.device, dtype=torch.float32)
    ldfilm = film.stride(0) if film is not None else 0
    launch.gn_bwd_reduce_drop(x, dy, ab, red, act, *drop)
    check(_lib.lib().jg_gn_bwd_coef(red.data_ptr(), _p(gamma), _p(beta), _p(film), ldfilm, mr.data_ptr(), pqr.data_ptr(), _p(dgamma), _p(dbeta),
                                    _p(dfilm), 2 * C, B, HW, C, G, _st()), "jg_gn_bwd_coef")
    return launch.gn_bwd_apply_drop(x, dy, ab, pqr, act, *drop) if want_dx else None


class _GroupNormDropFn(JGFunction):
    """_GroupNormFn with nn.Dropout behind the activation: y = m * act(norm(x)) / keep.  The mask is not saved: the backward passes
    regenerate it from (u | key, stream, call)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, film, G, act, eps, sums, keep, u, key, stream, call):
        x = x.contiguous()
        drop = _drop_args(x, keep, u, key, stream, call)
        y, ab, mr = _group_norm_launch(x, gamma, beta, film, G, act, eps, sums, None, drop)
        ctx.save_for_backward(x, ab, mr, gamma, beta, film, drop[1], drop[2])
        ctx.G, ctx.act, ctx.drop = G, act, (drop[0], drop[3], drop[4])
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, ab, mr, gamma, beta, film, u, key = ctx.saved_tensors
        keep, stream, call = ctx.drop
        B, C = x.shape[0], x.shape[-1]
        red = zeros_f32(B * C * 2, x.device)[:B * C * 2].view(B, C, 2)
        want_film = film is not None and ctx.needs_input_grad[3]
        dfilm = torch.empty((B, 2 * C), device=x.device, dtype=torch.float32) if want_film else None
        dgamma = gamma.grad if (gamma is not None and ctx.needs_input_grad[1]) else None
        dbeta = beta.grad if (beta is not None and ctx.needs_input_grad[2]) else None
        if (gamma is not None and ctx.needs_input_grad[1] and dgamma is None):
            raise RuntimeError("norm weight has no arena-backed .grad")
        dx = _gn_drop_bwd_launch(x, dy.contiguous(), ab, mr, gamma, beta, film, ctx.G, ctx.act, (keep, u, key, stream, call), red, dgamma, dbeta,
                                 dfilm, ctx.needs_input_grad[0])
        return (dx, None, None, dfilm) + (None,) * 9


class _ActDropFn(JGFunction):
    """m * act(x) / keep where no normalisation precedes the activation (the PatchGAN's first layer); the backward reads x, not y: a dropped
    element of y says nothing about the sign of x"""

    @staticmethod
    def forward(ctx, x, act, keep, u, key, stream, call):
        x = x.contiguous()
        drop = _drop_args(x, keep, u, key, stream, call)
        ctx.save_for_backward(x, drop[1], drop[2])
        ctx.act, ctx.drop = act, (drop[0], drop[3], drop[4])
        return launch.gn_apply_drop(x, None, act, *drop)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, u, key = ctx.saved_tensors
        keep, stream, call = ctx.drop
        return (launch.gn_bwd_apply_drop(x, dy.contiguous(), None, None, ctx.act, keep, u, key, stream, call),) + (None,) * 6


def activation_dropout(x, act, keep, u=None, key=None, stream=0, call=0):
    """nn.Dropout(1 - keep)(act(x)) in one pass on x [B, H, W, C] (act: JG_ACT_NONE / RELU / LRELU / SILU); the arguments as in group_norm"""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.act_drop(x, act, float(keep), u, key, int(stream), int(call))
    return _ActDropFn.apply(x, act, keep, u, key, stream, call)


_GN_STATUS = {}


def gn_status(device):
    """the sticky error word of jg_gn_bwd_fused (one per device): non-zero = an inter-workgroup wait of a fused GroupNorm backward
    expired (that launch's numbers are invalid).  `check_gn_status()` reads it (host synchronisation: tests, bench, smoke)."""
    key = torch.device(device).index or 0
    t = _GN_STATUS.get(key)
    if t is None:
        t = _GN_STATUS[key] = torch.zeros(4, device=device, dtype=torch.int32)
    return t


def check_gn_status():
    for k, t in _GN_STATUS.items():
        if int(t[0]) != 0:
            raise RuntimeError(f"jg_gn_bwd_fused: an inter-workgroup wait expired on cuda:{k} (results of that launch are invalid)")


def group_norm(x, G, gamma=None, beta=None, film=None, act=JG_ACT_NONE, eps=1e-5, sums=None, add=None, keep=None, u=None, key=None, stream=0,
               call=0):
    """act(GroupNorm_G(x) * gamma + beta [* (1 + scale) + shift]); statistics in fp32.  sums: the [B, C, 2] statistics of x where a
    convolution's epilogue has already taken them (conv2d_stats).
    keep (None: no dropout, the launches are those of before): nn.Dropout(1 - keep) behind the activation in the same pass, x [B, H, W, C];
    u: injected uniforms fp32 [B, C, H, W], else the mask is drawn in the kernel from `key` (d_aug_key), `stream` (< 65536, the Dropout
    module) and `call` (its invocation within the step).  Under TORCH_OPS_BOUNDARY the functional ops take their own statistics, with or
    without dropout: `sums` is not used there."""
    if keep is not None:
        if add is not None:
            raise ValueError("group_norm: dropout and a residual addend do not occur behind one normalisation")
        if TORCH_OPS_BOUNDARY:
            return torch.ops.jg355.group_norm_act_drop(x, gamma, beta, film, G, act, eps, float(keep), u, key, int(stream), int(call))
        return _GroupNormDropFn.apply(x, gamma, beta, film, G, act, eps, sums, keep, u, key, stream, call)
    if TORCH_OPS_BOUNDARY:
        y = torch.ops.jg355.group_norm_act(x, gamma, beta, film, G, act, eps)
        return y if add is None else y + add
    return _GroupNormFn.apply(x, gamma, beta, film, G, act, eps, sums, add)


# ======================================================================================
# CUT networks: transposed convolution, reflection padding, stand-alone activations
# ======================================================================================
def conv_transpose2d_forward(x, m: ConvMeta, output_padding=0):
    """nn.ConvTranspose2d(Cin_t, Cout_t, k, stride s, padding p, output_padding op).  `m` holds the weight as the
    stride-s CONV whose input-gradient this is (m.Cout = Cin_t, m.Cin = Cout_t): forward = stride-1 conv of the
    zero-dilated input with m.w16T (the flipped / transposed copy)."""
    B, H, W, Cin_t = x.shape
    assert Cin_t == m.Cout, (Cin_t, m.Cout)
    Ho = (H - 1) * m.stride - 2 * m.pad + m.R + output_padding
    Wo = (W - 1) * m.stride - 2 * m.pad + m.S + output_padding
    y = torch.empty((B, Ho, Wo, m.Cin), device=x.device, dtype=x.dtype)
    if Ho == 2 * H and Wo == 2 * W and phase_tconv_ok(m, Ho, Wo, Cin_t, m.Cin):
        return phase_tconv(x.contiguous(), m, y, bias=m.bias)
    Hd, Wd = Ho + 2 * m.pad - m.R + 1, Wo + 2 * m.pad - m.S + 1
    xd = dilate2d(x, Hd, Wd, m.stride)
    conv_nt(xd, m.w16T, y, B=B, H=Hd, W=Wd, Cin=Cin_t, Cout=m.Cin, R=m.R, S=m.S, pad=m.R - 1 - m.pad, stride=1, Ho=Ho, Wo=Wo,
            ldx=Cin_t, ldw=m.R * m.S * Cin_t, ldy=m.Cin, bias=m.bias)
    return y


class _ConvTranspose2dFn(JGFunction):
    @staticmethod
    def forward(ctx, x, weight, bias, meta, output_padding):
        _require_cuda(x)
        y = conv_transpose2d_forward(x, meta, output_padding)
        ctx.save_for_backward(x)
        ctx.meta = meta
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        m = ctx.meta
        dy = dy.contiguous()
        B, H, W, Cin_t = x.shape
        _, Ho, Wo, Cout_t = dy.shape
        dx = None
        if ctx.needs_input_grad[0]:      # the forward of the stride-s convolution
            dx = torch.empty_like(x)
            conv_nt(dy, m.w16, dx, B=B, H=Ho, W=Wo, Cin=Cout_t, Cout=Cin_t, R=m.R, S=m.S, pad=m.pad, stride=m.stride, Ho=H, Wo=W,
                    ldx=Cout_t, ldw=m.R * m.S * Cout_t, ldy=Cin_t)
        if ctx.needs_input_grad[1]:
            wg = m.weight.grad
            if wg is None:
                raise RuntimeError("conv-transpose weight has no arena-backed .grad")
            ktot = m.R * m.S * Cout_t
            tiles = ((Cin_t + 127) // 128) * ((ktot + 127) // 128)
            wgrad_tn(x, dy, wg, B=B, H=Ho, W=Wo, Cin=Cout_t, Cout=Cin_t, R=m.R, S=m.S, pad=m.pad, stride=m.stride, Ho=H, Wo=W,
                     lddy=Cin_t, ldx=Cout_t, lddw=ktot, splitk=_wgrad_splitk(tiles, B * H * W))
        if ctx.needs_input_grad[2] and m.bias is not None:
            check(_lib.lib().jg_channel_sum(_dt(dy), dy.data_ptr(), Cout_t, m.bias.grad.data_ptr(), B * Ho * Wo, Cout_t, 1.0, _st()),
                  "jg_channel_sum")
        return dx, None, None, None, None


def conv_transpose2d(x, meta: ConvMeta, output_padding=0):
    if TORCH_OPS_BOUNDARY:
        from .ops_library_cut import conv_transpose2d_via_ops

        return conv_transpose2d_via_ops(x, meta, output_padding)
    return _ConvTranspose2dFn.apply(x, meta.weight, meta.bias, meta, output_padding)


class _ReflectPadFn(JGFunction):
    @staticmethod
    def forward(ctx, x, pad):
        _require_cuda(x)
        ctx.pad = pad
        return launch.reflect_pad2d(x.contiguous(), pad)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return launch.reflect_pad2d_bwd(dy.contiguous(), ctx.pad), None


def reflect_pad2d(x, pad):
    """nn.ReflectionPad2d(pad) on NHWC."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.reflect_pad2d(x, pad)
    return _ReflectPadFn.apply(x, pad)


def _crop_window(x, top, left, Ho, Wo):
    """y = x[:, top:top+Ho, left:left+Wo] of a contiguous NHWC tensor (jg_crop2d, adjoint 0), no autograd"""
    B, H, W, Cc = x.shape
    y = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_crop2d(_dt(x), x.data_ptr(), y.data_ptr(), B, H, W, Cc, top, left, Ho, Wo, 0, _st()), "jg_crop2d")
    return y


class _CropFn(JGFunction):
    @staticmethod
    def forward(ctx, x, top, left, Ho, Wo):
        _require_cuda(x)
        x = x.contiguous()
        ctx.cfg = (x.shape[1], x.shape[2], top, left)
        return _crop_window(x, top, left, Ho, Wo)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        H, W, top, left = ctx.cfg
        dy = dy.contiguous()
        B, Ho, Wo, Cc = dy.shape
        dx = torch.empty(B, H, W, Cc, device=dy.device, dtype=dy.dtype)
        check(_lib.lib().jg_crop2d(_dt(dy), dy.data_ptr(), dx.data_ptr(), B, H, W, Cc, top, left, Ho, Wo, 1, _st()), "jg_crop2d")
        return dx, None, None, None, None


def crop2d(x, top, left, Ho, Wo):
    """x[:, top:top+Ho, left:left+Wo] on NHWC (adjoint: zero-filled placement)."""
    return _CropFn.apply(x, top, left, Ho, Wo)


class _ActFn(JGFunction):
    @staticmethod
    def forward(ctx, x, act):
        _require_cuda(x)
        y = launch.act_fwd(x.contiguous(), act)
        ctx.save_for_backward(y)
        ctx.act = act
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return launch.act_bwd(y, dy.contiguous(), ctx.act), None


def activation(x, act):
    """stand-alone nn.ReLU / nn.LeakyReLU(0.2) / nn.Tanh (JG_ACT_*) where no normalisation precedes the activation."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.act(x, act)
    return _ActFn.apply(x, act)


# ======================================================================================
# resampling / concat
# ======================================================================================
def _pool(x, scale):
    B, H, W, Cc = x.shape
    y = torch.empty((B, H // 2, W // 2, Cc), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_pool2x2(_dt(x), x.data_ptr(), y.data_ptr(), B, H, W, Cc, scale, _st()), "jg_pool2x2")
    return y


def _up(x, scale):
    B, H, W, Cc = x.shape
    y = torch.empty((B, H * 2, W * 2, Cc), device=x.device, dtype=x.dtype)
    check(_lib.lib().jg_upsample2x(_dt(x), x.data_ptr(), y.data_ptr(), B, H, W, Cc, scale, _st()), "jg_upsample2x")
    return y


class _AvgPool2Fn(JGFunction):
    @staticmethod
    def forward(ctx, x):
        return _pool(x, 0.25)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return _up(dy.contiguous(), 0.25)


class _Upsample2Fn(JGFunction):
    @staticmethod
    def forward(ctx, x):
        return _up(x, 1.0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return _pool(dy.contiguous(), 1.0)


def avg_pool2(x):
    return torch.ops.jg355.resample2(x, False, 0.25)


def upsample_nearest2(x):
    return torch.ops.jg355.resample2(x, True, 1.0)


def copy_channels(src, soff, dst, doff, n):
    P = src.numel() // src.shape[-1]
    check(_lib.lib().jg_copy_channels(_dt(src), src.data_ptr(), src.shape[-1], soff, dst.data_ptr(), dst.shape[-1], doff, P,
                                      n, _st()), "jg_copy_channels")


class _CatFn(JGFunction):
    @staticmethod
    def forward(ctx, a, b):
        Ca, Cb = a.shape[-1], b.shape[-1]
        y = torch.empty(a.shape[:-1] + (Ca + Cb,), device=a.device, dtype=a.dtype)
        copy_channels(a, 0, y, 0, Ca)
        copy_channels(b, 0, y, Ca, Cb)
        ctx.Ca, ctx.Cb = Ca, Cb
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        dy = dy.contiguous()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty(dy.shape[:-1] + (ctx.Ca,), device=dy.device, dtype=dy.dtype)
            copy_channels(dy, 0, da, 0, ctx.Ca)
        if ctx.needs_input_grad[1]:
            db = torch.empty(dy.shape[:-1] + (ctx.Cb,), device=dy.device, dtype=dy.dtype)
            copy_channels(dy, ctx.Ca, db, 0, ctx.Cb)
        return da, db


def cat_channels(a, b):
    """torch.cat([a, b], dim=1) of the reference (NCHW) == last-dim concat in NHWC."""
    if TORCH_OPS_BOUNDARY:
        return torch.cat([a, b], dim=-1)
    return _CatFn.apply(a, b)


# ======================================================================================
# attention core (QKVAttentionLegacy)
# ======================================================================================
def _gemm_geom(M, N, K):
    return dict(B=1, H=1, W=M, Cin=K, Cout=N, R=1, S=1, pad=0, stride=1, Ho=1, Wo=M)


def _transpose_heads(qkv, coff, nh, ch):
    B, T, C3 = qkv.shape
    out = torch.empty((B * nh, ch, T), device=qkv.device, dtype=qkv.dtype)
    check(_lib.lib().jg_transpose_heads(_dt(qkv), qkv.data_ptr(), C3, coff, 3 * ch, out.data_ptr(), B, T, nh, ch, _st()),
          "jg_transpose_heads")
    return out


def attn_core_fwd(qkv, nh):
    """qkv [B,T,3C] in the LEGACY head layout (channel = h*3ch + {q: 0..ch, k: ch..2ch, v: 2ch..3ch},
    unet_generator_attn.py:340) -> (a [B,T,C] with channel = h*ch + c, P [B*nh,T,T] softmax probabilities)."""
    _require_cuda(qkv)
    L = _lib.lib()
    B, T, C3 = qkv.shape
    Cc = C3 // 3
    ch = Cc // nh
    BH = B * nh
    dev, dt = qkv.device, _dt(qkv)
    if FLASH_ATTENTION and ch == 32 and T % 128 == 0:
        # fused kernel (attention.hip): the T x T logits stay on chip; aux = per-query logsumexp
        a = torch.empty((B, T, Cc), device=dev, dtype=qkv.dtype)
        lse = torch.empty((BH, T), device=dev, dtype=torch.float32)
        check(L.jg_attention_fwd(dt, qkv.data_ptr(), a.data_ptr(), lse.data_ptr(), B, T, nh, ch, _st()), "jg_attention_fwd")
        return a, lse
    scale2 = 1.0 / math.sqrt(ch)  # (ch^-1/4)^2
    S = torch.empty((BH, T, T), device=dev, dtype=torch.float32)
    conv_nt(qkv, qkv, S, **_gemm_geom(T, T, ch), ldx=C3, ldw=C3, ldy=T, alpha=scale2, out_f32=True, nbatch=BH, nh=nh,
            sx=(T * C3, 3 * ch), sw=(T * C3, 3 * ch), sy=(nh * T * T, T * T), w_off=ch)
    P = torch.empty((BH, T, T), device=dev, dtype=qkv.dtype)
    check(L.jg_softmax_fwd(dt, S.data_ptr(), P.data_ptr(), BH * T, T, _st()), "jg_softmax_fwd")
    del S
    Vt = _transpose_heads(qkv, 2 * ch, nh, ch)
    a = torch.empty((B, T, Cc), device=dev, dtype=qkv.dtype)
    conv_nt(P, Vt, a, **_gemm_geom(T, ch, T), ldx=T, ldw=T, ldy=Cc, nbatch=BH, nh=nh, sx=(nh * T * T, T * T),
            sw=(nh * ch * T, ch * T), sy=(T * Cc, ch))
    return a, P


def attn_core_bwd(qkv, P, da, nh, a=None):
    """Gradient of attn_core_fwd with respect to qkv.  `P` is the second result of attn_core_fwd (the
    probabilities [B*nh,T,T], or the logsumexp [B*nh,T] of the fused kernel, which also needs the output `a`)."""
    L = _lib.lib()
    da = da.contiguous()
    B, T, C3 = qkv.shape
    Cc = C3 // 3
    ch = Cc // nh
    BH = B * nh
    dev, dt = qkv.device, _dt(qkv)
    if P.dim() == 2:
        if a is None:
            raise RuntimeError("the fused attention backward needs the forward output")
        dqkv = torch.empty_like(qkv)
        dq_rows = torch.empty((BH, T), device=dev, dtype=torch.float32)
        check(L.jg_attention_bwd(dt, qkv.data_ptr(), a.data_ptr(), P.data_ptr(), da.data_ptr(), dqkv.data_ptr(),
                                 dq_rows.data_ptr(), B, T, nh, ch, _st()), "jg_attention_bwd")
        return dqkv
    scale2 = 1.0 / math.sqrt(ch)
    # dP = dA V^T
    dP = torch.empty((BH, T, T), device=dev, dtype=torch.float32)
    conv_nt(da, qkv, dP, **_gemm_geom(T, T, ch), ldx=Cc, ldw=C3, ldy=T, out_f32=True, nbatch=BH, nh=nh,
            sx=(T * Cc, ch), sw=(T * C3, 3 * ch), sy=(nh * T * T, T * T), w_off=2 * ch)
    dS = torch.empty((BH, T, T), device=dev, dtype=qkv.dtype)
    check(L.jg_softmax_bwd(dt, P.data_ptr(), dP.data_ptr(), dS.data_ptr(), BH * T, T, scale2, _st()), "jg_softmax_bwd")
    del dP
    dqkv = torch.empty_like(qkv)
    # dQ = dS K      (NT with K^T as the "weight" operand)
    Kt = _transpose_heads(qkv, ch, nh, ch)
    conv_nt(dS, Kt, dqkv, **_gemm_geom(T, ch, T), ldx=T, ldw=T, ldy=C3, nbatch=BH, nh=nh, sx=(nh * T * T, T * T),
            sw=(nh * ch * T, ch * T), sy=(T * C3, 3 * ch))
    # dK = dS^T Q ; dV = P^T dA     (TN: reduction index t is the row index of both operands)
    geom = dict(B=1, H=1, W=T, Cin=ch, Cout=T, R=1, S=1, pad=0, stride=1, Ho=1, Wo=T)
    wgrad_tn(dS, qkv, dqkv, **geom, lddy=T, ldx=C3, lddw=C3, nbatch=BH, nh=nh, sdy=(nh * T * T, T * T),
             sx=(T * C3, 3 * ch), sdw=(T * C3, 3 * ch), out_mode=JG_OUT_STORE_T, dw_off=ch)
    wgrad_tn(P, da, dqkv, **geom, lddy=T, ldx=Cc, lddw=C3, nbatch=BH, nh=nh, sdy=(nh * T * T, T * T),
             sx=(T * Cc, ch), sdw=(T * C3, 3 * ch), out_mode=JG_OUT_STORE_T, dw_off=2 * ch)
    return dqkv


class _AttnCoreFn(JGFunction):
    @staticmethod
    def forward(ctx, qkv, nh):
        a, P = attn_core_fwd(qkv, nh)
        ctx.save_for_backward(qkv, P, a)
        ctx.nh = nh
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, da):
        qkv, P, a = ctx.saved_tensors
        return attn_core_bwd(qkv, P, da, ctx.nh, a), None


def attention_core(qkv, n_heads):
    return torch.ops.jg355.attention_core(qkv, n_heads)[0]


# ======================================================================================
# small fp32 linear (embedding path)
# ======================================================================================
class _LinearFn(JGFunction):
    """inputs: x, W, b, act, dW, db, *track -- dW/db are the arena gradient views the kernel accumulates
    into; `track` are the nn.Parameters behind W/b, passed only so that autograd records the node."""

    @staticmethod
    def forward(ctx, x, W, b, act, dW, db, *track):
        _require_cuda(x, W)
        x = x.contiguous()
        y = launch.linear_fwd(x, W, b, act)
        ctx.save_for_backward(x, W)
        ctx.act, ctx.dW, ctx.db = act, dW, db
        ctx.want_param = any(t is not None and t.requires_grad for t in track)
        ctx.ntrack = len(track)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dW = db = None
        if ctx.want_param:
            dW, db = ctx.dW, ctx.db
            if dW is None:
                raise RuntimeError("linear weight has no arena-backed .grad")
        if ctx.needs_input_grad[0] or dW is not None:
            dx = launch.linear_bwd(x, W, dy, ctx.act, dW, db, ctx.needs_input_grad[0])
        return (dx, None, None, None, None, None) + (None,) * ctx.ntrack


def linear(x, weight, bias=None, act=JG_ACT_NONE):
    """y = act(x) @ weight.T + bias in fp32 (nn.Linear preceded by an optional SiLU)."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.linear_act(x, weight, bias, act)
    track = (weight,) if bias is None else (weight, bias)
    return _LinearFn.apply(x, weight, bias, act, weight.grad, None if bias is None else bias.grad, *track)


def linear_stacked(x, W, b, dW, db, act, track):
    """Several nn.Linear layers that share their input, run as one: W/b/dW/db are stacked arena views."""
    return _LinearFn.apply(x, W, b, act, dW, db, *track)


def gamma_embedding(gammas, dim, max_period=10000.0):
    """models/modules/diffusion_utils.py:8-42 for gammas [B,1] (or [B])."""
    if TORCH_OPS_BOUNDARY and not _IN_OP:
        return torch.ops.jg355.gamma_embedding(gammas, dim, float(max_period))
    g = gammas.reshape(-1).contiguous().float()
    emb = torch.empty((g.shape[0], dim), device=g.device, dtype=torch.float32)
    check(_lib.lib().jg_gamma_embedding(g.data_ptr(), emb.data_ptr(), g.shape[0], dim, float(max_period), _st()),
          "jg_gamma_embedding")
    return emb


# ======================================================================================
# CUT patch features and contrastive / adversarial losses (fp32)
# ======================================================================================
class _GatherPatchesFn(JGFunction):
    @staticmethod
    def forward(ctx, feat, ids, C, per):
        _require_cuda(feat, ids)
        B, H, W, ld = feat.shape
        G, P = (ids.shape[0], ids.shape[1]) if ids.dim() == 2 else (1, ids.numel())
        per = per if G > 1 else B
        out = torch.empty((B * P, C), device=feat.device, dtype=torch.float32)
        check(_lib.lib().jg_gather_rows_grouped(_dt(feat), feat.data_ptr(), ld, ids.data_ptr(), out.data_ptr(), B, H * W, C, P, G, per, _st()),
              "jg_gather_rows_grouped")
        ctx.save_for_backward(ids)
        ctx.shape, ctx.dtype, ctx.C, ctx.geo = feat.shape, feat.dtype, C, (G, P, per)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        B, H, W, ld = ctx.shape
        G, P, per = ctx.geo
        dfeat = torch.zeros(ctx.shape, device=dout.device, dtype=ctx.dtype)
        dout = dout.contiguous()
        check(_lib.lib().jg_scatter_rows_grouped(_DT[ctx.dtype], dfeat.data_ptr(), ld, ids.data_ptr(), dout.data_ptr(), B, H * W, ctx.C, P, G, per,
                                                 _st()), "jg_scatter_rows_grouped")
        return dfeat, None, None, None


def gather_patches(feat, ids, C, per=0):
    """feat [B,H,W,ld] 16-bit NHWC -> [B*P, C] fp32 rows at the flattened positions `ids` (shared by the batch):
    `feat.permute(0,2,3,1).flatten(1,2)[:, patch_id, :].flatten(0,1)` of cut_networks.py:45-57.  `ids` [G, P] with `per` > 0: G id sets,
    image b uses set (b // per) % G (one launch for the concatenated batches of several PatchSampleF calls)."""
    if ids.dim() == 2 and ids.shape[0] > 1:
        if per < 1 or TORCH_OPS_BOUNDARY:
            raise ValueError("grouped gather_patches needs per >= 1 and the ctypes path")
        return _GatherPatchesFn.apply(feat, ids.contiguous().long(), C, int(per))
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.gather_patches(feat, ids.contiguous().long(), C)
    return _GatherPatchesFn.apply(feat, ids.reshape(-1).contiguous().long(), C, 0)


class _L2NormFn(JGFunction):
    @staticmethod
    def forward(ctx, x, eps):
        y, nrm = launch.l2norm_fwd(x.contiguous(), eps)
        ctx.save_for_backward(y, nrm)
        ctx.eps = eps
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, nrm = ctx.saved_tensors
        return launch.l2norm_bwd(y, nrm, dy.contiguous(), ctx.eps), None


def l2_normalize(x, eps=1e-7):
    """torch.nn.functional.normalize(x, eps=eps) for fp32 [R, D] (cut_networks.py:66)."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.l2_normalize(x, eps)[0]
    return _L2NormFn.apply(x, eps)


class _PatchNCEFn(JGFunction):
    """Per-patch PatchNCE / MoNCE loss.  q, k: [nimg*P, D] fp32, L2-normalised.  k is detached in the positive logit and in the
    optimal-transport weights but NOT in the negative logits (base_NCE.py:52-66, monce.py:21-22), reproduced here."""

    @staticmethod
    def forward(ctx, q, k, nimg, T, pm1, monce):
        _require_cuda(q, k)
        q, k = q.contiguous(), k.contiguous()
        loss, S, K, uh, vh = launch.nce_fwd(q, k, nimg, T, pm1, monce)
        ctx.save_for_backward(q, k, S, K, uh, vh)
        ctx.cfg = (nimg, T, pm1, monce)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        dq, dk = launch.nce_bwd(*ctx.saved_tensors, dloss.contiguous().float(), *ctx.cfg, want_dk=ctx.needs_input_grad[1])
        return dq, dk, None, None, None, None


def patch_nce_loss(q, k, nimg, T, num_patches, monce=False):
    """BaseNCELoss.forward / MoNCELoss (base_NCE.py:17-50, monce.py:16-33): per-patch loss [nimg*P]."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.patch_nce(q, k, nimg, float(T), float(num_patches - 1), bool(monce))[0]
    return _PatchNCEFn.apply(q, k, nimg, float(T), float(num_patches - 1), bool(monce))


class _PatchHDCEFn(JGFunction):
    """Per-patch SRC_hDCE loss (NCE/SRC.py:46-75 weights, NCE/hDCE.py:16-38).  q, k: [nimg*P, D] fp32.  The weights come from the key
    Gram matrix inside the kernel (detached, never stored); the value is the cross-entropy of [l_pos | weighted l_neg] / T, the gradient
    that of logsumexp(weighted l_neg / T) - l_pos / T; k is detached in the positive logit but NOT in the negative logits."""

    @staticmethod
    def forward(ctx, q, k, nimg, T, gamma, wperiod, wcount):
        _require_cuda(q, k)
        q, k = q.contiguous(), k.contiguous()
        loss, S, G, stats = launch.hdce_fwd(q, k, nimg, T, gamma, wperiod, wcount)
        ctx.save_for_backward(q, k, S, G, stats)
        ctx.cfg = (nimg, T, gamma, wperiod, wcount)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        dq, dk = launch.hdce_bwd(*ctx.saved_tensors, dloss.contiguous().float(), *ctx.cfg, want_dk=ctx.needs_input_grad[1])
        return dq, dk, None, None, None, None, None


def patch_hdce_loss(q, k, nimg, T, gamma, wperiod=1, wcount=1):
    """SRC_Loss weights + PatchHDCELoss (NCE/SRC.py, NCE/hDCE.py): per-patch loss [nimg*P].  Problem b uses the weights iff
    (b % wperiod) < wcount; the others are the reference's `weight=None` mode (w == 1)."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.patch_hdce(q, k, int(nimg), float(T), float(gamma), int(wperiod), int(wcount))[0]
    return _PatchHDCEFn.apply(q, k, int(nimg), float(T), float(gamma), int(wperiod), int(wcount))


def hdce_weights(k, nimg, gamma):
    """the hDCE weights [nimg, P, P] of SRC_Loss(only_weight=True) with a zero diagonal (tests / inspection: training never stores them)"""
    _require_cuda(k)
    return launch.hdce_weights(k.detach().contiguous(), nimg, gamma)


GAN_MODES = {"lsgan": 0, "vanilla": 1, "wgangp": 2}


class _LSGANLossFn(JGFunction):
    @staticmethod
    def forward(ctx, pred, target, scale, mode=0):
        _require_cuda(pred)
        loss, ctx.dpred = launch.gan_loss(pred.contiguous(), mode, target, scale, ctx.needs_input_grad[0])
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dpred, ctx.dpred = ctx.dpred, None
        return axpby(dpred, 1.0, None, 0.0, alpha_dev=g.reshape(1).float(), out=dpred), None, None, None


def lsgan_loss(pred, target, scale=1.0):
    """GANLoss('lsgan') (loss.py:69-71): scale * mean((pred[..., 0] - target)^2) on an NHWC logit map whose channel 0 is valid."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.gan_loss(pred, 0, float(target), float(scale))[0]
    return _LSGANLossFn.apply(pred, float(target), float(scale), 0)


def gan_loss(pred, mode, target, scale=1.0):
    """GANLoss(mode) for mode in lsgan / vanilla / wgangp (loss.py:59-76) on an NHWC logit map whose channel 0 is valid; `target` is the label
    (real_label / fake_label)."""
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.gan_loss(pred, GAN_MODES[mode], float(target), float(scale))[0]
    return _LSGANLossFn.apply(pred, float(target), float(scale), GAN_MODES[mode])


# ======================================================================================
# DDPM glue + layout converters
# ======================================================================================
_IN_OP = False      # set while a torch.ops.jg355 implementation calls back into the plain helpers of this module


def ddpm_prepare(y0, ycond, noise, mask, gammas, act_dtype, cpad=8):
    if TORCH_OPS_BOUNDARY and not _IN_OP:
        return torch.ops.jg355.ddpm_prepare(y0, ycond, noise, mask, gammas, act_dtype == torch.float16, cpad)
    _require_cuda(y0, ycond, noise)
    B, Cc, H, W = y0.shape
    xin = torch.empty((B, H, W, cpad), device=y0.device, dtype=act_dtype)
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    check(_lib.lib().jg_ddpm_prepare(_DT[act_dtype], y0.contiguous().data_ptr(), ycond.contiguous().data_ptr(),
                                     noise.contiguous().data_ptr(), _p(m), gammas.contiguous().data_ptr(), xin.data_ptr(), B,
                                     Cc, H, W, cpad, _st()), "jg_ddpm_prepare")
    return xin


def lowres_roundtrip(x, scale_or_size, out=None):
    """Resize((H, W))(Resize((Hlo, Wlo))(x)) with torchvision's anti-aliased bilinear Resize, in one launch (jg_lowres_roundtrip_f32): the
    conditioning image of the palette model's super_resolution task (palette_model.py:120-130, 546-548).  x: fp32 NCHW; `scale_or_size`: a
    number = the down-scaling factor (Hlo = int(H / scale), as the reference sizes it) or a pair (Hlo, Wlo); `out`: optional contiguous fp32
    tensor of x's shape to write into (ctypes path only).  Not differentiated: x is data."""
    from . import resize_aa

    B, Cc, H, W = x.shape
    if isinstance(scale_or_size, (tuple, list)):
        Hlo, Wlo = (int(v) for v in scale_or_size)
    else:
        Hlo, Wlo = resize_aa.low_size(H, scale_or_size), resize_aa.low_size(W, scale_or_size)
    if not (1 <= Hlo <= H and 1 <= Wlo <= W):
        raise ValueError(f"lowres_roundtrip: low-resolution size {Hlo}x{Wlo} outside 1..{H} x 1..{W}")
    if TORCH_OPS_BOUNDARY and not _IN_OP and out is None:
        return torch.ops.jg355.lowres_roundtrip(x, Hlo, Wlo)
    _require_cuda(x, out)
    if x.dtype != torch.float32:
        raise TypeError(f"lowres_roundtrip takes the fp32 ground-truth image, got {x.dtype}")
    resize_aa.band_rows(H, W, Hlo, Wlo)          # NotImplementedError for a shape the kernel does not take
    x = x.contiguous()
    if out is None:
        y = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("lowres_roundtrip: `out` must be a contiguous fp32 tensor of x's shape on x's device")
    else:
        y = out
    if x.numel() == 0:
        return y
    kd = max(resize_aa.aa_taps(H, Hlo), resize_aa.aa_taps(W, Wlo))
    args = []
    for n_in, n_out, k in ((H, Hlo, kd), (W, Wlo, kd), (Hlo, H, 3), (Wlo, W, 3)):
        args += [t.data_ptr() for t in resize_aa.device_tables(n_in, n_out, x.device, k)]
    check(_lib.lib().jg_lowres_roundtrip_f32(x.data_ptr(), y.data_ptr(), *args, B * Cc, H, W, Hlo, Wlo, kd, _st()), "jg_lowres_roundtrip_f32")
    return y


class _MSELossFn(JGFunction):
    @staticmethod
    def forward(ctx, nh, noise, mask, w, lam, grad_scale, Cc):
        loss, dnh = launch.ddpm_mse_loss(nh, noise, mask, w, lam, grad_scale, Cc)
        ctx.save_for_backward(dnh)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        (dnh,) = ctx.saved_tensors
        gout = gout.contiguous().float()
        return axpby(dnh, 1.0, alpha_dev=gout), None, None, None, None, None, None


def ddpm_mse_loss(noise_hat_nhwc, noise, mask, w=None, lam=1.0, grad_scale=1.0):
    """lambda * MSE(w m noise, w m noise_hat) with its gradient produced in the same pass."""
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    wv = None if w is None else w.reshape(-1).contiguous().float()
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.ddpm_mse_loss(noise_hat_nhwc, noise.contiguous(), m, wv, float(lam), float(grad_scale), noise.shape[1])[0]
    return _MSELossFn.apply(noise_hat_nhwc, noise.contiguous(), m, wv, float(lam), float(grad_scale), noise.shape[1])


class _MultiScaleLossFn(JGFunction):
    @staticmethod
    def forward(ctx, nh, noise, mask, w, lam, grad_scale, Cc, nlevels, l1, multiscale):
        B, H, W, cpad = nh.shape
        losses = torch.zeros(nlevels, device=nh.device, dtype=torch.float32)
        dnh = torch.empty_like(nh)
        nws = sum(B * Cc * (H >> l) * (W >> l) for l in range(1, nlevels))
        ws = torch.empty(max(nws, 1), device=nh.device, dtype=torch.float32)
        check(_lib.lib().jg_ddpm_multiscale_loss(_dt(nh), noise.data_ptr(), nh.data_ptr(), _p(mask), _p(w), losses.data_ptr(),
                                                 dnh.data_ptr(), ws.data_ptr(), B, Cc, H, W, cpad, nlevels, int(l1), int(multiscale), lam,
                                                 grad_scale, _st()), "jg_ddpm_multiscale_loss")
        ctx.save_for_backward(dnh)
        ctx.mark_non_differentiable(losses)
        return losses.sum(), losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, _g_levels):
        (dnh,) = ctx.saved_tensors
        return (axpby(dnh, 1.0, alpha_dev=gout.contiguous().float().reshape(1)),) + (None,) * 9


def ddpm_loss(noise_hat_nhwc, noise, mask, w=None, lam=1.0, grad_scale=1.0, lossname="MSE", min_res=32):
    """alg_palette_loss in {MSE, L1, multiscale_MSE, multiscale_L1} (palette_model.py:231-256,597-618): returns
    (lambda * total, {resolution: lambda * term}) -- the per-resolution terms only for the multiscale variants."""
    if lossname == "MSE":
        return ddpm_mse_loss(noise_hat_nhwc, noise, mask, w, lam, grad_scale), {}
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    wv = None if w is None else w.reshape(-1).contiguous().float()
    S = noise_hat_nhwc.shape[1]
    multiscale = lossname.startswith("multiscale")
    if min_res != 32:
        raise NotImplementedError("MultiScaleDiffusionLoss.min_res is 32 in the reference")
    nlevels = 1
    if multiscale:
        import math

        nlevels = max(1, math.floor(math.log2(S)) - 5 + 1)        # resolutions 32 .. S (loss.py:406-409, palette_model.py:232-241)
    tot, levels = _MultiScaleLossFn.apply(noise_hat_nhwc, noise.contiguous(), m, wv, float(lam), float(grad_scale), noise.shape[1],
                                          nlevels, lossname.endswith("L1"), multiscale)
    return tot, ({str(S >> l): levels[l] for l in range(nlevels)} if multiscale else {})


# ======================================================================================
# consistency-model glue (cm_generator.py / cm_model.py of the reference)
# ======================================================================================
class _NoiseLevelEmbFn(JGFunction):
    @staticmethod
    def forward(ctx, sigmas, W, dW):
        s = sigmas.reshape(-1).contiguous().float()
        emb = torch.empty((s.shape[0], 2 * W.shape[0]), device=s.device, dtype=torch.float32)
        check(_lib.lib().jg_noise_level_embedding(s.data_ptr(), W.data_ptr(), emb.data_ptr(), s.shape[0], W.shape[0], _st()),
              "jg_noise_level_embedding")
        ctx.save_for_backward(s, W)
        ctx.dW = dW
        return emb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, demb):
        s, W = ctx.saved_tensors
        if ctx.dW is not None:
            demb = demb.contiguous().float()
            check(_lib.lib().jg_noise_level_embedding_bwd(s.data_ptr(), W.data_ptr(), demb.data_ptr(), ctx.dW.data_ptr(),
                                                          s.shape[0], W.shape[0], _st()), "jg_noise_level_embedding_bwd")
        return None, None, None


def noise_level_embedding(sigmas, W):
    """[sin | cos](sigma * W * 2 pi) (NoiseLevelEmbedding.forward, cm_generator.py:276-280); the gradient with respect
    to W is accumulated into W.grad (arena view) by the backward kernel."""
    _require_cuda(sigmas, W)
    return _NoiseLevelEmbFn.apply(sigmas, W, W.grad if W.requires_grad else None)


def cm_noisy(x, noise, sigma, mask, cond, act_dtype, cpad=8):
    """(noisy fp32 NCHW, UNet input 16-bit NHWC [cond | noisy | 0]) -- cm_generator.py:452-460,377-381."""
    _require_cuda(x, noise, sigma)
    B, Cc, H, W = x.shape
    Ccond = 0 if cond is None else cond.shape[1]
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    out = torch.empty_like(x, dtype=torch.float32)
    xin = torch.empty((B, H, W, cpad), device=x.device, dtype=act_dtype)
    check(_lib.lib().jg_cm_noisy(_DT[act_dtype], x.contiguous().float().data_ptr(), noise.contiguous().float().data_ptr(),
                                 sigma.contiguous().float().data_ptr(), _p(m), None if cond is None else cond.contiguous().float().data_ptr(),
                                 out.data_ptr(), xin.data_ptr(), B, Cc, Ccond, H, W, cpad, _st()), "jg_cm_noisy")
    return out, xin


def cm_combine(noisy, F_nhwc, cskip, cout):
    """c_skip * noisy + c_out * F as fp32 NCHW (cm_forward, cm_generator.py:383-385); no autograd (outputs / visuals)."""
    B, Cc, H, W = noisy.shape
    out = torch.empty_like(noisy)
    check(_lib.lib().jg_cm_combine(_dt(F_nhwc), noisy.data_ptr(), F_nhwc.data_ptr(), cskip.contiguous().data_ptr(),
                                   cout.contiguous().data_ptr(), out.data_ptr(), B, Cc, H, W, F_nhwc.shape[-1], _st()), "jg_cm_combine")
    return out


class _CMLossFn(JGFunction):
    @staticmethod
    def forward(ctx, Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w, chub, lam, grad_scale):
        B, Cc, H, W = noisy_n.shape
        loss = torch.zeros((), device=Fn.device, dtype=torch.float32)
        dFn = torch.empty_like(Fn)
        check(_lib.lib().jg_cm_loss(_dt(Fn), Fn.data_ptr(), Fc.data_ptr(), noisy_n.data_ptr(), noisy_c.data_ptr(), cs_n.data_ptr(),
                                    co_n.data_ptr(), cs_c.data_ptr(), co_c.data_ptr(), _p(mask), w.data_ptr(), loss.data_ptr(),
                                    dFn.data_ptr(), B, Cc, H, W, Fn.shape[-1], chub, lam, grad_scale, _st()), "jg_cm_loss")
        ctx.save_for_backward(dFn)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        (dFn,) = ctx.saved_tensors
        return (axpby(dFn, 1.0, alpha_dev=gout.contiguous().float()),) + (None,) * 12


def cm_loss(F_next, F_cur, noisy_next, noisy_cur, cs_n, co_n, cs_c, co_c, mask, loss_weights, lam=1.0, grad_scale=1.0):
    """compute_cm_loss (cm_model.py:353-375, no perceptual terms) on the two UNet outputs (NHWC 16-bit); gradient with
    respect to F_next produced in the same pass."""
    B, Cc, H, W = noisy_next.shape
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    chub = 0.00054 * math.sqrt(Cc * H * W)
    f = lambda t: t.reshape(-1).contiguous().float()
    return _CMLossFn.apply(F_next, F_cur.detach(), noisy_next, noisy_cur, f(cs_n), f(co_n), f(cs_c), f(co_c), m, f(loss_weights),
                           chub, float(lam), float(grad_scale))


def _cm_gan_head_launch(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w, lam, grad_scale):
    """(loss, dFn_cm, pred) of jg_cm_gan_head; every argument already contiguous / fp32 / int64 as the kernel reads it"""
    B, Cc, H, W = noisy_n.shape
    for name, t, dtype in (("F_cur", Fc, Fn.dtype), ("noisy_next", noisy_n, torch.float32), ("noisy_cur", noisy_c, torch.float32)):
        if t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"cm_gan_head: {name} must be contiguous {dtype}, got {t.dtype}")
    if tuple(Fn.shape[:3]) != (B, H, W) or Fc.shape != Fn.shape or noisy_c.shape != noisy_n.shape or not Fn.is_contiguous():
        raise ValueError(f"cm_gan_head: F {tuple(Fn.shape)} / {tuple(Fc.shape)} against noisy {tuple(noisy_n.shape)} / {tuple(noisy_c.shape)}")
    for v in (cs_n, co_n, cs_c, co_c, w):
        if v.numel() != B:
            raise ValueError(f"cm_gan_head: per-sample vectors must hold {B} values, got {v.numel()}")
    if mask is not None and mask.numel() != B * H * W:
        raise ValueError(f"cm_gan_head: mask {tuple(mask.shape)} is not [B,1,H,W]")
    loss = torch.zeros((), device=Fn.device, dtype=torch.float32)
    dFn = torch.empty_like(Fn)
    pred = torch.empty_like(Fn)
    chub = 0.00054 * math.sqrt(Cc * H * W)
    check(_lib.lib().jg_cm_gan_head(_dt(Fn), Fn.data_ptr(), Fc.data_ptr(), noisy_n.data_ptr(), noisy_c.data_ptr(), cs_n.data_ptr(),
                                    co_n.data_ptr(), cs_c.data_ptr(), co_c.data_ptr(), _p(mask), w.data_ptr(), loss.data_ptr(),
                                    dFn.data_ptr(), pred.data_ptr(), B, Cc, H, W, Fn.shape[-1], chub, lam, grad_scale, _st()), "jg_cm_gan_head")
    return loss, dFn, pred


def _cm_gan_head_bwd_launch(dFn, dpred, gloss, co_n, Cc):
    """dF_next = gloss * dFn_cm + co_n[b] * dpred in one launch (jg_cm_gan_head_bwd); dpred None = no gradient reached pred, gloss None =
    none reached the loss (a zero device scalar then)"""
    B, H, W, cpad = dFn.shape
    if dpred is not None:
        dpred = dpred.contiguous()
        if dpred.dtype != dFn.dtype or dpred.shape != dFn.shape:
            raise TypeError(f"cm_gan_head: the gradient of pred must be {dFn.dtype} {tuple(dFn.shape)}, got {dpred.dtype} {tuple(dpred.shape)}")
    g = torch.zeros((), device=dFn.device, dtype=torch.float32) if gloss is None else gloss.contiguous().float()
    dF = torch.empty_like(dFn)
    check(_lib.lib().jg_cm_gan_head_bwd(_dt(dFn), dFn.data_ptr(), _p(dpred), g.data_ptr(), co_n.data_ptr(), dF.data_ptr(), B, Cc, H, W, cpad,
                                        _st()), "jg_cm_gan_head_bwd")
    return dF


class _CMGanHeadFn(JGFunction):
    @staticmethod
    def forward(ctx, Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w, lam, grad_scale):
        loss, dFn, pred = _cm_gan_head_launch(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w, lam, grad_scale)
        ctx.save_for_backward(dFn, co_n)
        ctx.Cc = noisy_n.shape[1]
        ctx.set_materialize_grads(False)
        return loss, pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss, gpred):
        dFn, co_n = ctx.saved_tensors
        if gloss is None and gpred is None:
            return (None,) * 12
        return (_cm_gan_head_bwd_launch(dFn, gpred, gloss, co_n, ctx.Cc),) + (None,) * 11


def cm_gan_head(F_next, F_cur, noisy_next, noisy_cur, cs_n, co_n, cs_c, co_c, mask, loss_weights, lam=1.0, grad_scale=1.0):
    """The seam of cm_gan (cm_gan_model.py: compute_cm_gan_loss): compute_cm_loss on the two UNet outputs exactly as `cm_loss` computes it
    (`lam` scales this term only, its gradient carries `grad_scale`) AND the student's prediction pred = c_skip x_noisy + c_out F_next as
    NHWC 16-bit, the discriminators' input, in ONE launch (jg_cm_gan_head).  Returns (loss, pred); both carry gradient, and the backward is
    one launch too (jg_cm_gan_head_bwd): dF_next = g_loss * dFn_cm + c_out * dpred."""
    _require_cuda(F_next, F_cur, noisy_next, noisy_cur, loss_weights)
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    f = lambda t: t.reshape(-1).contiguous().float()
    args = (F_next, F_cur.detach(), noisy_next, noisy_cur, f(cs_n), f(co_n), f(cs_c), f(co_c), m, f(loss_weights), float(lam), float(grad_scale))
    if TORCH_OPS_BOUNDARY:
        return tuple(torch.ops.jg355.cm_gan_head(*args)[:2])
    return _CMGanHeadFn.apply(*args)


ECT_C = 1e-6                 # CMModel.c (cm_model.py:120)
_ECT_MAX_BLOCKS = _lib.JG_ECT_MAX_BLOCKS         # per-sample partial sums of jg_ect_loss (csrc/elementwise.hip)


def _ect_loss_launch(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, dt, lam, grad_scale):
    """(loss, dFn) of jg_ect_loss; every argument already contiguous / fp32 / int64 as the kernel reads it"""
    B, Cc, H, W = noisy_n.shape
    for name, t, dtype in (("F_cur", Fc, Fn.dtype), ("noisy_next", noisy_n, torch.float32), ("noisy_cur", noisy_c, torch.float32)):
        if t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"ect_loss: {name} must be contiguous {dtype}, got {t.dtype}")
    if tuple(Fn.shape[:3]) != (B, H, W) or Fc.shape != Fn.shape or noisy_c.shape != noisy_n.shape or not Fn.is_contiguous():
        raise ValueError(f"ect_loss: F {tuple(Fn.shape)} / {tuple(Fc.shape)} against noisy {tuple(noisy_n.shape)} / {tuple(noisy_c.shape)}")
    for v in (cs_n, co_n, cs_c, co_c, dt):
        if v.numel() != B:
            raise ValueError(f"ect_loss: per-sample vectors must hold {B} values, got {v.numel()}")
    if mask is not None and mask.numel() != B * H * W:
        raise ValueError(f"ect_loss: mask {tuple(mask.shape)} is not [B,1,H,W]")
    loss = torch.empty((), device=Fn.device, dtype=torch.float32)
    dFn = torch.empty_like(Fn)
    nws = B * min((H * W + 255) // 256, _ECT_MAX_BLOCKS)
    ws = torch.empty(nws, device=Fn.device, dtype=torch.float32)
    check(_lib.lib().jg_ect_loss(_dt(Fn), Fn.data_ptr(), Fc.data_ptr(), noisy_n.data_ptr(), noisy_c.data_ptr(), cs_n.data_ptr(),
                                 co_n.data_ptr(), cs_c.data_ptr(), co_c.data_ptr(), _p(mask), dt.data_ptr(), ws.data_ptr(), nws,
                                 loss.data_ptr(), dFn.data_ptr(), B, Cc, H, W, Fn.shape[-1], ECT_C, lam, grad_scale, _st()), "jg_ect_loss")
    return loss, dFn


class _ECTLossFn(JGFunction):
    @staticmethod
    def forward(ctx, Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, dt, lam, grad_scale):
        loss, dFn = _ect_loss_launch(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, dt, lam, grad_scale)
        ctx.save_for_backward(dFn)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        (dFn,) = ctx.saved_tensors
        return (axpby(dFn, 1.0, alpha_dev=gout.contiguous().float()),) + (None,) * 11


def ect_loss(F_next, F_cur, noisy_next, noisy_cur, cs_n, co_n, cs_c, co_c, mask, dt, lam=1.0, grad_scale=1.0):
    """compute_ect_loss (cm_model.py:412-442, no perceptual terms) on the two UNet outputs (NHWC 16-bit): lam * mean_b of
    (sqrt(sum_chw (m pred - m target)^2 + c^2) - c) / dt_b with dt = t - r; the gradient with respect to F_next comes out of the same
    call (jg_ect_loss: two launches, no atomics) and is saved for the backward."""
    _require_cuda(F_next, F_cur, noisy_next, noisy_cur, dt)
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype != torch.int64:
            m = m.long()
    f = lambda t: t.reshape(-1).contiguous().float()
    args = (F_next, F_cur.detach(), noisy_next, noisy_cur, f(cs_n), f(co_n), f(cs_c), f(co_c), m, f(dt), float(lam), float(grad_scale))
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.ect_loss(*args)[0]
    return _ECTLossFn.apply(*args)


PIXEL_OFF, PIXEL_L1, PIXEL_MSE = 0, 1, 2       # segment modes of jg_pixel_loss
_PIXEL_MAX_BLOCKS = _lib.JG_PIXEL_MAX_BLOCKS   # per-segment partial sums of jg_pixel_loss (csrc/elementwise.hip)


def _pixel_loss_check(x, y, C, modes, lambdas):
    """the argument checks of jg_pixel_loss / jg_pixel_loss_bwd, before any launch; returns (S, M, H, W, modes and lambdas padded to two)"""
    S = len(modes)
    if S not in (1, 2) or len(lambdas) != S or any(int(m) not in (PIXEL_OFF, PIXEL_L1, PIXEL_MSE) for m in modes):
        raise ValueError(f"pixel_loss: modes {list(modes)} / lambdas {list(lambdas)}: one or two segments, each mode 0 (off), 1 (L1) or 2 (MSE)")
    if x.dim() != 4 or y.dim() != 4:
        raise ValueError(f"pixel_loss: x {tuple(x.shape)} / y {tuple(y.shape)} are not NHWC images")
    if x.dtype not in _DT or y.dtype != x.dtype or not x.is_contiguous() or not y.is_contiguous():
        raise TypeError(f"pixel_loss: x and y must be contiguous and of one 16-bit dtype, got {x.dtype} / {y.dtype}")
    M, H, W, cpad = y.shape
    if x.shape[0] != S * M or tuple(x.shape[1:]) != (H, W, cpad) or not 1 <= int(C) <= cpad:
        raise ValueError(f"pixel_loss: x {tuple(x.shape)} is not {S} segment(s) of y {tuple(y.shape)} with {C} valid channels")
    return S, M, H, W, [int(m) for m in modes] + [PIXEL_OFF] * (2 - S), [float(v) for v in lambdas] + [0.0] * (2 - S)


def _pixel_loss_launch(x, y, C, modes, lambdas):
    """the S losses of jg_pixel_loss (fp32 [S])"""
    _require_cuda(x, y)
    S, M, H, W, md, lam = _pixel_loss_check(x, y, C, modes, lambdas)
    loss = torch.empty(S, device=x.device, dtype=torch.float32)
    nws = S * min((M * H * W + 255) // 256, _PIXEL_MAX_BLOCKS)
    ws = torch.empty(nws, device=x.device, dtype=torch.float32)
    check(_lib.lib().jg_pixel_loss(_dt(x), x.data_ptr(), y.data_ptr(), ws.data_ptr(), nws, loss.data_ptr(), S, M, int(C), H, W, x.shape[-1],
                                   md[0], md[1], lam[0], lam[1], _st()), "jg_pixel_loss")
    return loss


def _pixel_loss_bwd_launch(x, y, g, C, modes, lambdas):
    """d (sum_s g[s] loss[s]) / dx of jg_pixel_loss_bwd; g: the S upstream gradients, read on the device"""
    _require_cuda(x, y, g)
    S, M, H, W, md, lam = _pixel_loss_check(x, y, C, modes, lambdas)
    if g.numel() != S:
        raise ValueError(f"pixel_loss: the upstream gradient must hold {S} values, got {g.numel()}")
    g = g.reshape(-1).contiguous().float()
    dx = torch.empty_like(x)
    check(_lib.lib().jg_pixel_loss_bwd(_dt(x), x.data_ptr(), y.data_ptr(), g.data_ptr(), dx.data_ptr(), S, M, int(C), H, W, x.shape[-1],
                                       md[0], md[1], lam[0], lam[1], _st()), "jg_pixel_loss_bwd")
    return dx


class _PixelLossFn(JGFunction):
    @staticmethod
    def forward(ctx, x, y, C, modes, lambdas):
        loss = _pixel_loss_launch(x, y, C, modes, lambdas)
        ctx.save_for_backward(x, y)
        ctx.cfg = (C, modes, lambdas)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        return _pixel_loss_bwd_launch(x, y, gout, *ctx.cfg), None, None, None, None


def pixel_loss(x, y, C, modes, lambdas):
    """nn.L1Loss / nn.MSELoss between two 16-bit NHWC images over the C valid channels (cut_model.py:771-786): x [S*M, H, W, 8] in
    S = len(modes) segments of M images, each compared with the same y [M, H, W, 8]; modes[s] in (PIXEL_OFF, PIXEL_L1, PIXEL_MSE).
    Returns the S weighted losses lambdas[s] * mean (fp32 [S]; exactly 0 for an off segment).  The backward is ONE launch for all
    segments: d = x - y is recomputed and the S upstream gradients are read on the device (jg_pixel_loss_bwd); y receives no gradient."""
    modes, lambdas = tuple(int(m) for m in modes), tuple(float(v) for v in lambdas)
    if TORCH_OPS_BOUNDARY:
        return torch.ops.jg355.pixel_loss(x, y.detach(), int(C), list(modes), list(lambdas))
    return _PixelLossFn.apply(x, y.detach(), int(C), modes, lambdas)


# ---- class loss of the semantic-consistency branch (train_semantic_cls; csrc/sem_cls.hip) -------------------------------------------------
CLS_CE, CLS_MSE, CLS_L1 = 0, 1, 2              # modes of jg_cls_loss
_CLS_DT = {torch.float16: _lib.JG_F16, torch.bfloat16: _lib.JG_BF16, torch.float32: _lib.JG_CLS_F32}


def _cls_loss_check(logits, target, mode, prev, state):
    """the argument checks of jg_cls_loss, before any launch (ValueError); returns (B, n, row stride)"""
    if int(mode) not in (CLS_CE, CLS_MSE, CLS_L1):
        raise ValueError(f"cls_loss: mode {mode!r} is not 0 (cross entropy), 1 (MSE) or 2 (L1)")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"cls_loss: logits {tuple(logits.shape)} are not [B, n]")
    B, n = logits.shape
    if logits.dtype not in _CLS_DT:
        raise ValueError(f"cls_loss: logits must be float32, float16 or bfloat16, got {logits.dtype}")
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < n):
        raise ValueError(f"cls_loss: the rows of the logits must be contiguous (strides {tuple(logits.stride())})")
    if mode != CLS_CE and n != 1:
        raise ValueError(f"cls_loss: the regression modes take one value per sample, got n = {n}")
    want = torch.int64 if mode == CLS_CE else torch.float32
    if target.dtype != want or target.numel() != B or not target.is_contiguous():
        raise ValueError(f"cls_loss: target must be contiguous {want} with {B} entries, got {target.dtype} {tuple(target.shape)}")
    for name, t in (("prev", prev), ("state", state)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
            raise ValueError(f"cls_loss: {name} must be one float32 value in device memory")
    return B, n, (logits.stride(0) if B > 1 else max(n, logits.stride(0)))


def _cls_loss_launch(logits, target, mode, lam, prev, threshold, state, state_acc):
    """(loss fp32 scalar, dlogits [B, n] for a unit upstream gradient, argmax int64 [B]) of jg_cls_loss: one launch"""
    B, n, ld = _cls_loss_check(logits, target, mode, prev, state)
    _require_cuda(logits, target, prev, state)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty((B, n), device=logits.device, dtype=logits.dtype)
    argmax = torch.empty(B, device=logits.device, dtype=torch.int64)
    check(_lib.lib().jg_cls_loss(_CLS_DT[logits.dtype], int(mode), logits.data_ptr(), ld, target.data_ptr(), B, n, float(lam), _p(prev), float(threshold),
                                 loss.data_ptr(), dlogits.data_ptr(), n, argmax.data_ptr(), _p(state), int(bool(state_acc)), _st()), "jg_cls_loss")
    return loss, dlogits, argmax


def _cls_loss_scale(dlogits, gout):
    """the saved unit gradient times the incoming scalar, read on the device"""
    g = gout.contiguous().float()
    if dlogits.dtype == torch.float32 or dlogits.numel() % 8:      # jg_axpby walks 16-bit data in groups of 8
        return (dlogits.float() * g).to(dlogits.dtype)
    return axpby(dlogits, 1.0, alpha_dev=g)


class _ClsLossFn(JGFunction):
    @staticmethod
    def forward(ctx, logits, target, mode, lam, prev, threshold, state, state_acc):
        loss, dlogits, argmax = _cls_loss_launch(logits, target, mode, lam, prev, threshold, state, state_acc)
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(argmax)
        return loss, argmax

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, _gargmax):
        (dlogits,) = ctx.saved_tensors
        return (_cls_loss_scale(dlogits, gout),) + (None,) * 7


def cls_loss(logits, target, mode=CLS_CE, lam=1.0, prev=None, threshold=1.0, state=None, state_acc=False):
    """The class loss of train_semantic_cls on logits [B, n] (fp32 or 16-bit; a row stride above n is allowed, the padding is not read):
    lam * gate * CrossEntropyLoss (mode CLS_CE, int64 labels) / MSELoss / L1Loss (CLS_MSE / CLS_L1, fp32 targets, n == 1), with
    gate = !(prev > threshold) read on the device (`prev`: fp32 device scalar; None: no gate), plus the per-row argmax (int64, lowest index on
    ties).  `state` (fp32 device scalar) receives the loss, or has it added with state_acc.  Returns (loss, argmax); loss, gradient and
    argmax come from one launch (jg_cls_loss), the backward scales the saved gradient by the incoming scalar."""
    args = (logits, target.detach(), int(mode), float(lam), prev, float(threshold), state, bool(state_acc))
    if TORCH_OPS_BOUNDARY:
        out = torch.ops.jg355.cls_loss(*args[:6])
        if state is not None:      # the functional op cannot write the gate state: one small device-side copy instead
            state.add_(out[0].detach()) if state_acc else state.copy_(out[0].detach())
        return out[0], out[2]
    return _ClsLossFn.apply(*args)


# ---- discriminator-input augmentations: dataaug_D_noise and adaptive pseudo augmentation (csrc/d_aug.hip) ----------------------------------
D_AUG_MAX = _lib.JG_D_AUG_MAX  # targets of one jg_d_aug launch
D_AUG_NOISE_STREAM = 0         # Philox stream id of the noise; the flags of target d draw on stream 1 + d unless the caller says otherwise


def d_aug_key(device):
    """the 64-bit Philox key of jg_d_aug as a two-word device tensor, drawn on torch's generator for `device` (torch.manual_seed decides it;
    the draw is legal inside a graph capture)"""
    return torch.randint(-2 ** 31, 2 ** 31, (2,), device=device, dtype=torch.int32)


def _d_aug_launch(src, C, sigma, z, key, noise_stream, call, alts, ps, us, streams, outs, flags):
    """jg_d_aug on checked arguments: `outs` (and `flags`, with `alts`) are written in place; nothing is returned"""
    import ctypes

    _require_cuda(src, z, key, *outs, *(alts or ()), *(ps or ()), *(us or ()), *((flags,) if flags is not None else ()))
    nd = len(outs)
    B, H, W, cpad = src.shape
    if not 1 <= nd <= D_AUG_MAX or (alts is not None and len(alts) != nd) or (alts is None and (ps is not None or us is not None)):
        raise ValueError(f"d_aug: 1..{D_AUG_MAX} targets, one alt per target, p / u only with alt (got {nd} outputs)")
    if alts is not None and (ps is None or len(ps) != nd or (us is not None and len(us) != nd) or flags is None or len(streams) != nd):
        raise ValueError("d_aug: alt needs one p, one stream id (and, when injected, one u) per target, and a flags tensor")
    for t in list(outs) + list(alts or ()):
        if t.dtype != src.dtype or tuple(t.shape) != tuple(src.shape) or not t.is_contiguous():
            raise TypeError(f"d_aug: every image must be contiguous {tuple(src.shape)} {src.dtype}, got {tuple(t.shape)} {t.dtype}")
    if not src.is_contiguous() or not 1 <= int(C) <= cpad:
        raise ValueError(f"d_aug: src must be a contiguous NHWC tensor with 1 <= C <= {cpad} (C = {C})")
    if z is not None and (z.dtype != torch.float32 or tuple(z.shape) != (B, int(C), H, W) or not z.is_contiguous()):
        raise TypeError(f"d_aug: z must be contiguous fp32 {(B, int(C), H, W)}, got {tuple(z.shape)} {z.dtype}")
    if key is not None and (key.dtype != torch.int32 or key.numel() != 2):
        raise TypeError("d_aug: key must hold two int32 words")
    for t, what, n in [(t, "p", 1) for t in (ps or ())] + [(t, "u", B) for t in (us or ())]:
        if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
            raise TypeError(f"d_aug: {what} must be contiguous fp32 with {n} element(s)")
    if flags is not None and (flags.dtype != torch.int32 or tuple(flags.shape) != (nd, B) or not flags.is_contiguous()):
        raise TypeError(f"d_aug: flags must be contiguous int32 {(nd, B)}")
    arr = lambda ts: None if ts is None else (ctypes.c_void_p * nd)(*[t.data_ptr() for t in ts])
    fl = None if flags is None else (ctypes.c_void_p * nd)(*[flags[d].data_ptr() for d in range(nd)])
    sid = None if alts is None else (ctypes.c_uint32 * nd)(*[int(v) for v in streams])
    check(_lib.lib().jg_d_aug(_dt(src), src.data_ptr(), nd, arr(alts), arr(ps), arr(outs), fl, arr(us), sid, float(sigma), _p(z), _p(key),
                              int(noise_stream), int(call), B, H, W, int(C), cpad, _st()), "jg_d_aug")


def d_aug(src, C, sigma=0.0, z=None, key=None, call=0, alts=None, ps=None, us=None, streams=None, outs=None, noise_stream=D_AUG_NOISE_STREAM):
    """The discriminator inputs of a step from ONE launch (dataaug_D_noise: util/util.py:296-300; APA: models/modules/loss.py:199-212), on 16-bit
    NHWC images [B, H, W, Cpad] with C valid channels: for every target d (one without `alts`, else one per entry)
        out_d[b] = flag_d[b] ? alts[d][b] : src[b] + sigma * z[b],      flag_d[b] = u_d[b] < ps[d]  (ps[d]: fp32 scalar on the device)
    z: fp32 [B, C, H, W] (injected) or None: drawn in the kernel from `key` (d_aug_key) at call index `call`, shared by all targets;
    us: one fp32 [B] per target (injected) or None: drawn in the kernel on the Philox streams `streams` (default 1 + d).
    outs: tensors to write (the static operands of a captured graph), default fresh ones.  Returns (outs, flags int32 [nd, B] or None).
    Not differentiable: the reference detaches these inputs."""
    nd = len(alts) if alts is not None else 1
    src = src.detach()
    if alts is not None:
        alts = [a.detach() for a in alts]
        streams = list(streams) if streams is not None else [1 + d for d in range(nd)]
    if TORCH_OPS_BOUNDARY:
        o, f = torch.ops.jg355.d_aug(src, list(alts or ()), list(ps or ()), list(us or ()), list(streams or ()), int(C), float(sigma), z, key,
                                     int(noise_stream), int(call))
        if outs is not None:
            for dst, t in zip(outs, o):
                dst.copy_(t)
        return (list(outs) if outs is not None else list(o.unbind(0))), (f if alts is not None else None)
    if outs is None:
        outs = [torch.empty_like(src) for _ in range(nd)]
    flags = torch.empty((nd, src.shape[0]), device=src.device, dtype=torch.int32) if alts is not None else None
    _d_aug_launch(src, C, sigma, z, key, noise_stream, call, alts, ps, us, streams, list(outs), flags)
    return list(outs), flags


def _apa_update_launch(pred, state, n, stride, target, num, den):
    _require_cuda(pred, state)
    if state.dtype != torch.float32 or state.numel() != 3 or not state.is_contiguous():
        raise TypeError("apa_update: state must be contiguous fp32 [3] = (p, adjust, s)")
    if not pred.is_contiguous() or n < 1 or stride < 1 or (n - 1) * stride >= pred.numel():
        raise ValueError(f"apa_update: {n} elements at stride {stride} do not fit the contiguous prediction {tuple(pred.shape)}")
    sp = state.data_ptr()
    check(_lib.lib().jg_apa_update(_dt(pred), pred.data_ptr(), int(n), int(stride), sp, sp + 4, sp + 8, float(target), float(num), float(den),
                                   _st()), "jg_apa_update")


def apa_update(pred, state, target, num, den, channel0=False):
    """update_adaptive_pseudo_augmentation_p (models/modules/loss.py:214-231) in one launch, IN PLACE on `state` = fp32 [3] (p, adjust, s) on the
    device: s = mean(sign(pred)), adjust = sign(s - target), p = clamp(p + adjust * num / den, 0, 1) with num = batch size * dataaug_APA_every,
    den = dataaug_APA_nimg * 1000.  pred: the 16-bit prediction on the (substituted) real batch; channel0: an NHWC logit map whose channel 0 is
    valid (PatchGAN), else every element (projected logits).  No host read."""
    pred = pred.detach()
    stride = pred.shape[-1] if channel0 else 1
    n = pred.numel() // stride
    if TORCH_OPS_BOUNDARY:
        torch.ops.jg355.apa_update(pred, state, n, stride, float(target), float(num), float(den))
    else:
        _apa_update_launch(pred, state, n, stride, float(target), float(num), float(den))
    return state


# ---- dataaug_D_diffusion: Diffusion-GAN noise on the projected discriminator's backbone features (csrc/d_diffusion.hip) ---------------------
D_DIFFUSION_MAX, D_DIFFUSION_TABLE, D_DIFFUSION_EPL = _lib.JG_D_DIFFUSION_MAX, _lib.JG_D_DIFFUSION_TABLE, _lib.JG_D_DIFFUSION_EPL


class DDiffusionState:
    """the device state of the augmentation: p fp32 [1] (strength), Tn int32 [2] (T, n), the tables a = sqrt(cumprod alpha) and
    b = sqrt(1 - cumprod alpha) fp32 [501], t_epl int32 [64].  `fresh` is the reference's start p = 0: T = 5, t_epl = 0, a[0] = 1, b[0] = 0"""

    __slots__ = ("p", "Tn", "a", "b", "t_epl")

    def __init__(self, p, Tn, a, b, t_epl):
        self.p, self.Tn, self.a, self.b, self.t_epl = p, Tn, a, b, t_epl

    @classmethod
    def fresh(cls, device):
        st = cls(torch.zeros(1, device=device), torch.tensor([_lib.JG_D_DIFFUSION_T_MIN, 0], device=device, dtype=torch.int32),
                 torch.zeros(D_DIFFUSION_TABLE, device=device), torch.zeros(D_DIFFUSION_TABLE, device=device),
                 torch.zeros(D_DIFFUSION_EPL, device=device, dtype=torch.int32))
        st.a[0] = 1.0
        return st

    def tensors(self):
        return self.p, self.Tn, self.a, self.b, self.t_epl

    def check(self):
        for t, dt, n, what in ((self.p, torch.float32, 1, "p"), (self.Tn, torch.int32, 2, "Tn"), (self.a, torch.float32, D_DIFFUSION_TABLE, "a"),
                               (self.b, torch.float32, D_DIFFUSION_TABLE, "b"), (self.t_epl, torch.int32, D_DIFFUSION_EPL, "t_epl")):
            if t.dtype != dt or t.numel() != n or not t.is_contiguous():
                raise TypeError(f"d_diffusion: state.{what} must be contiguous {dt} with {n} element(s), got {tuple(t.shape)} {t.dtype}")
        _require_cuda(*self.tensors())


def d_diffusion_grid_cap():
    """the most 16-byte groups (8 elements each) one jg_d_diffusion launch has in flight; larger problems loop"""
    return int(_lib.lib().jg_d_diffusion_grid_cap())


def _dd_arrays(maps):
    import ctypes

    n = len(maps)
    I = ctypes.c_int * n
    return I(*[m.shape[1] for m in maps]), I(*[m.shape[2] for m in maps]), I(*[m.shape[3] for m in maps])


def _dd_ptrs(ts, n):
    import ctypes

    return None if ts is None else (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])


def _dd_check_maps(xs, what):
    n = len(xs)
    if not 1 <= n <= D_DIFFUSION_MAX:
        raise ValueError(f"{what}: 1..{D_DIFFUSION_MAX} feature maps, got {n}")
    _require_cuda(*xs)
    for x in xs:
        if x.dim() != 4 or x.dtype != xs[0].dtype or x.shape[0] != xs[0].shape[0] or not x.is_contiguous() or x.numel() == 0:
            raise TypeError(f"{what}: every map must be a contiguous NHWC tensor of one 16-bit dtype and one batch size, got {tuple(x.shape)} {x.dtype}")
    return n, xs[0].shape[0]


# ---- data_online_context_pixels: the loader's image split into crop + surroundings, the frame around the translated crop (csrc/context.hip) --
def _context_split_check(x, c):
    _require_cuda(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise TypeError(f"context_split: an fp32 NCHW image is expected, got {tuple(x.shape)} {x.dtype}")
    if c < 1 or x.shape[2] - 2 * c < 1 or x.shape[3] - 2 * c < 1:
        raise ValueError(f"context_split: c = {c} leaves no crop inside an image of {tuple(x.shape[2:])} (c >= 1 and size > 2 c are required)")


def context_split(x_nchw, c, act_dtype, cpad=None):
    """set_input with data_online_context_pixels = c (models/base_model.py:389-431) from ONE read of the fp32 NCHW image [B, C, S + 2c, S + 2c]:
    -> (ctx [B, S + 2c, S + 2c, Cpad], crop [B, S, S, Cpad] = ctx[:, c:-c, c:-c]), 16-bit NHWC, what ops.to_nhwc would write.  No autograd."""
    c = int(c)
    _context_split_check(x_nchw, c)
    x = x_nchw.contiguous()
    if TORCH_OPS_BOUNDARY:
        return tuple(torch.ops.jg355.context_split(x, c, act_dtype == torch.float16, int(cpad or 0)))
    return launch.context_split(x, c, act_dtype, cpad)


def _context_frame_check(inner, ctx, c, C, z, key, outs):
    _require_cuda(inner, ctx, z, key, *(outs or ()))
    if inner.dim() != 4 or ctx.dim() != 4 or inner.dtype != ctx.dtype or not ctx.is_contiguous():
        raise TypeError(f"context_frame: inner and ctx must be 16-bit NHWC tensors of one dtype, ctx contiguous (got {tuple(inner.shape)} {inner.dtype}, "
                        f"{tuple(ctx.shape)} {ctx.dtype})")
    B, H, W, cpad = ctx.shape
    if c < 1 or tuple(inner.shape) != (B, H - 2 * c, W - 2 * c, cpad) or H - 2 * c < 1 or W - 2 * c < 1:
        raise ValueError(f"context_frame: inner {tuple(inner.shape)} is not the window of ctx {tuple(ctx.shape)} at c = {c} (c >= 1)")
    if not 1 <= C <= cpad:
        raise ValueError(f"context_frame: 1 <= C <= {cpad} is required (C = {C})")
    if z is not None and (z.dtype != torch.float32 or tuple(z.shape) != (B, C, H, W) or not z.is_contiguous()):
        raise TypeError(f"context_frame: z must be contiguous fp32 {(B, C, H, W)}, got {tuple(z.shape)} {z.dtype}")
    if key is not None and (key.dtype != torch.int32 or key.numel() != 2):
        raise TypeError("context_frame: key must hold two int32 words")
    if outs is not None:
        if len(outs) != 2 or outs[0] is None:
            raise ValueError("context_frame: outs = (out, out_noisy or None)")
        for t in outs:
            if t is not None and (t.dtype != ctx.dtype or tuple(t.shape) != tuple(ctx.shape) or not t.is_contiguous()):
                raise TypeError(f"context_frame: every output must be contiguous {tuple(ctx.shape)} {ctx.dtype}, got {tuple(t.shape)} {t.dtype}")


class _ContextFrameFn(JGFunction):
    """(out, out_noisy) from one launch; the gradient of `out` with respect to `inner` is its window (jg_crop2d), the frame and the noisy copy
    carry none"""

    @staticmethod
    def forward(ctx_, inner, ctx, c, C, sigma, z, key, noise_stream, call, outs, want_noisy):
        out, noisy = launch.context_frame(inner.contiguous(), ctx, c, C, sigma, z, key, noise_stream, call, *(outs or (None, None)), want_noisy)
        ctx_.cfg = (c, inner.shape[1], inner.shape[2])
        if noisy is None:
            return out, None
        ctx_.mark_non_differentiable(noisy)
        return out, noisy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx_, dout, _dnoisy):
        c, Hi, Wi = ctx_.cfg
        return (_crop_window(dout.contiguous(), c, c, Hi, Wi),) + (None,) * 10


def context_frame(inner, ctx, c, C, sigma=0.0, z=None, key=None, call=0, outs=None, noise_stream=D_AUG_NOISE_STREAM):
    """compute_fake_with_context (models/base_model.py:609-636) with the dataaug_D_noise of the framed image folded in (cut_model.py:668-682), on
    16-bit NHWC tensors: out [B, S + 2c, S + 2c, Cpad] = inner [B, S, S, Cpad] inside the window, ctx on the frame; with sigma != 0 also
    out_noisy = out + sigma * z over the whole framed image -- z fp32 [B, C, S + 2c, S + 2c] (injected) or None: drawn in the kernel from `key`
    (d_aug_key) at call index `call`, bit-identical to ops.d_aug(out, C, sigma, key=key, call=call).  outs: (out, out_noisy or None), tensors to
    write (the static operands of a captured graph), default fresh ones.  Returns (out, out_noisy or None).  Differentiable in `inner` through
    `out` (the window of the incoming gradient); ctx and out_noisy are detached, as the reference's D inputs are."""
    c, C, sigma = int(c), int(C), float(sigma)
    ctx = ctx.detach()
    _context_frame_check(inner, ctx, c, C, z, key, outs)
    want_noisy = sigma != 0.0 or (outs is not None and outs[1] is not None)
    if TORCH_OPS_BOUNDARY:
        out, noisy = torch.ops.jg355.context_frame(inner, ctx, c, C, sigma, z, key, int(noise_stream), int(call), want_noisy)
        noisy = noisy.detach() if want_noisy else None
        if outs is not None:      # the op is functional: the caller's destinations get copies (the gradient still flows through `out`)
            outs[0].copy_(out.detach())
            if outs[1] is not None:
                outs[1].copy_(noisy)
                noisy = outs[1]
        return out, noisy
    return _ContextFrameFn.apply(inner, ctx, c, C, sigma, z, key, int(noise_stream), int(call), None if outs is None else tuple(outs), want_noisy)


def _d_diffusion_launch(xs, a, b, t_epl, noise_std, key, call, ts, zs, outs, t_outs):
    """jg_d_diffusion on checked tensors: `outs` and `t_outs` are written in place"""
    n, B = _dd_check_maps(xs, "d_diffusion")
    for grp, what in ((ts, "ts"), (zs, "zs")):
        if grp is not None and len(grp) != n:
            raise ValueError(f"d_diffusion: {what} needs one entry per map (None: drawn)")
    for l, x in enumerate(xs):
        C = x.shape[3]
        t = None if ts is None else ts[l]
        z = None if zs is None else zs[l]
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (B, C) or not t.is_contiguous()):
            raise TypeError(f"d_diffusion: t of level {l} must be contiguous int32 {(B, C)}, got {tuple(t.shape)} {t.dtype}")
        if z is not None and (z.dtype != torch.float32 or tuple(z.shape) != (B, C, x.shape[1], x.shape[2]) or not z.is_contiguous()):
            raise TypeError(f"d_diffusion: z of level {l} must be contiguous fp32 {(B, C, x.shape[1], x.shape[2])}, got {tuple(z.shape)} {z.dtype}")
        _require_cuda(t, z)
    if key is not None and (key.dtype != torch.int32 or key.numel() != 2):
        raise TypeError("d_diffusion: key must hold two int32 words")
    _require_cuda(key)
    H, W, C = _dd_arrays(xs)
    check(_lib.lib().jg_d_diffusion(_dt(xs[0]), n, _dd_ptrs(xs, n), _dd_ptrs(outs, n), _dd_ptrs(t_outs, n), _dd_ptrs(ts, n), _dd_ptrs(zs, n), H, W, C, B,
                                    a.data_ptr(), b.data_ptr(), t_epl.data_ptr(), float(noise_std), _p(key), int(call), _st()), "jg_d_diffusion")


def _d_diffusion_bwd_launch(dys, t_saved, a):
    n, B = _dd_check_maps(dys, "d_diffusion_bwd")
    dxs = [torch.empty_like(d) for d in dys]
    H, W, C = _dd_arrays(dys)
    check(_lib.lib().jg_d_diffusion_bwd(_dt(dys[0]), n, _dd_ptrs(dys, n), _dd_ptrs(dxs, n), _dd_ptrs(t_saved, n), H, W, C, B, a.data_ptr(), _st()),
          "jg_d_diffusion_bwd")
    return dxs


class _DDiffusionFn(JGFunction):
    """the noised copies of up to four feature maps from one launch; saves only the t it used.  The backward reads the table `a` as it is
    THEN: an update between a forward and its backward would change it, and the step drivers update after both (as the reference does)"""

    @staticmethod
    def forward(ctx, state, noise_std, key, call, ts, zs, *xs):
        xs = [x.contiguous() for x in xs]
        outs = [torch.empty_like(x) for x in xs]
        t_outs = [torch.empty((x.shape[0], x.shape[3]), device=x.device, dtype=torch.int32) for x in xs]
        _d_diffusion_launch(xs, state.a, state.b, state.t_epl, noise_std, key, call, ts, zs, outs, t_outs)
        ctx.a = state.a
        ctx.save_for_backward(*t_outs)
        ctx.mark_non_differentiable(*t_outs)
        return (*outs, *t_outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        n = len(ctx.saved_tensors)
        dxs = _d_diffusion_bwd_launch([d.contiguous() for d in g[:n]], list(ctx.saved_tensors), ctx.a)
        return (None,) * 6 + tuple(dxs)


def d_diffusion(xs, state, noise_std, key=None, ts=None, zs=None, call=0):
    """Diffusion.forward of the reference (projected_d/diffusion.py:139-159) on up to four 16-bit NHWC feature maps [B, H_l, W_l, C_l]
    (C_l % 8 == 0) in ONE launch: out_l = a[t_l] * x_l + (noise_std * b[t_l]) * z_l with one t per (sample, channel), taken from `state`
    (DDiffusionState) on the device.  ts: per level an int32 [B, C_l] (injected) or None: t = t_epl[6 random bits], drawn in the kernel from
    `key` (d_aug_key); zs: per level an fp32 [B, C_l, H_l, W_l] (injected) or None: drawn in the kernel.  Returns (outs, ts_used).
    Differentiable in xs (dx_l = a[t_l] * dy_l, one launch for all levels)."""
    xs = list(xs)
    state.check()
    n = len(xs)
    if TORCH_OPS_BOUNDARY:
        if (ts is not None and any(t is None for t in ts)) or (zs is not None and any(z is None for z in zs)):
            raise ValueError("d_diffusion through torch.ops: ts / zs are given for every level or not at all")
        res = torch.ops.jg355.d_diffusion(xs, state.a, state.b, state.t_epl, float(noise_std), key, list(ts or ()), list(zs or ()), int(call))
        return list(res[:n]), list(res[n:])
    res = _DDiffusionFn.apply(state, float(noise_std), key, int(call), None if ts is None else list(ts), None if zs is None else list(zs), *xs)
    return list(res[:n]), list(res[n:])


def _d_diffusion_update_launch(p, Tn, a, b, t_epl, loss, num, den, u, key, call):
    _require_cuda(loss, u, key)
    if loss.dtype != torch.float32 or loss.numel() != 1:
        raise TypeError(f"d_diffusion_update: loss_real must be an fp32 scalar on the device, got {tuple(loss.shape)} {loss.dtype}")
    if u is not None and (u.dtype != torch.float32 or u.numel() != D_DIFFUSION_EPL or not u.is_contiguous()):
        raise TypeError(f"d_diffusion_update: u must be contiguous fp32 [{D_DIFFUSION_EPL}]")
    if key is not None and (key.dtype != torch.int32 or key.numel() != 2):
        raise TypeError("d_diffusion_update: key must hold two int32 words")
    check(_lib.lib().jg_d_diffusion_update(p.data_ptr(), Tn.data_ptr(), a.data_ptr(), b.data_ptr(), t_epl.data_ptr(), loss.data_ptr(), float(num),
                                           float(den), _p(u), _p(key), int(call), _st()), "jg_d_diffusion_update")


def d_diffusion_update(state, loss_real, batch_times_every, u=None, key=None, call=0):
    """DiscriminatorGANLoss.update's diffusion branch + Diffusion.update_T (loss.py:315-331, diffusion.py:125-137) in one launch, IN PLACE on
    `state`: p <- clip(p + sign(loss_real - 0.9) * batch_times_every / (100 * 1000), 0, 1) in fp32, then T, n, the tables and t_epl from p.
    loss_real: fp32 scalar on the device (no host read); u: fp32 [64] uniforms of t_epl's inverse-CDF draw (injected) or None: drawn in the
    kernel from `key` (default: a fresh d_aug_key)."""
    state.check()
    loss = loss_real.detach().reshape(1)
    if u is None and key is None:
        key = d_aug_key(loss.device)
    if TORCH_OPS_BOUNDARY:
        torch.ops.jg355.d_diffusion_update(*state.tensors(), loss, float(batch_times_every), 100.0 * 1000.0, u, key, int(call))
    else:
        _d_diffusion_update_launch(*state.tensors(), loss, float(batch_times_every), 100.0 * 1000.0, u, key, int(call))
    return state


class _ToNCHWFn(JGFunction):
    @staticmethod
    def forward(ctx, x, Cc):
        B, H, W, cpad = x.shape
        y = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
        check(_lib.lib().jg_nhwc_to_nchw_f32(_dt(x), x.data_ptr(), y.data_ptr(), B, Cc, H, W, cpad, _st()), "nhwc_to_nchw")
        ctx.cpad, ctx.dtype = cpad, x.dtype
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return to_nhwc(dy.contiguous().float(), ctx.dtype, ctx.cpad), None


def to_nchw_f32(x, Cc):
    return _ToNCHWFn.apply(x, Cc)


def to_nhwc(x, act_dtype, cpad=None):
    """NCHW fp32 -> NHWC 16-bit with the channel count padded to `cpad` (multiple of 8). No autograd."""
    B, Cc, H, W = x.shape
    cpad = cpad or (Cc + 7) // 8 * 8
    y = torch.empty((B, H, W, cpad), device=x.device, dtype=act_dtype)
    check(_lib.lib().jg_nchw_f32_to_nhwc(_DT[act_dtype], x.contiguous().data_ptr(), y.data_ptr(), B, Cc, H, W, cpad, _st()),
          "nchw_to_nhwc")
    return y


# ======================================================================================
# torch.ops.jg355.* -- the op surface north_star names: every op is a torch.library custom op with a fake (meta) kernel and an
# autograd formula built from the C-ABI kernels, so the ops trace (torch.compile / FakeTensor), compose with autograd and pass
# torch.library.opcheck.  The ops are FUNCTIONAL (gradients are returned).  The module graph uses them where a functional op costs
# nothing (attention core, pooling, upsampling); convolutions and normalisations of the training path keep their arena-accumulating
# autograd nodes (`_Conv2dFn`, `_GroupNormFn`, modules/unet_exec.py), whose weight / affine gradients are atomically added IN PLACE
# into the flat gradient arena -- returning them as tensors would add a full-arena copy to every step.
# ======================================================================================
def _conv_out_hw(H, W, R, S, pad, stride):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


@torch.library.custom_op("jg355::conv2d_nt", mutates_args=())
def _op_conv2d_nt(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], res: Optional[torch.Tensor], pad: int, stride: int,
                  alpha: float, res_scale: float) -> torch.Tensor:
    """x [B,H,W,Cin] 16-bit NHWC, w [Cout,R,S,Cin] 16-bit (or the fp32 master weight: rounded to x's type inside, gradient returned in
    fp32), bias fp32 [Cout], res like y: y = alpha conv(x, w) + bias + res_scale res"""
    B, H, W, Cin = x.shape
    Cout, R, S, _ = w.shape
    Ho, Wo = _conv_out_hw(H, W, R, S, pad, stride)
    y = torch.empty((B, Ho, Wo, Cout), device=x.device, dtype=x.dtype)
    x, w = x.contiguous(), w.to(x.dtype).contiguous()       # an fp32 master weight is rounded here, as the arena's working copy is
    conv_nt(x, w, y, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo, ldx=Cin,
            ldw=R * S * Cin, ldy=Cout, bias=bias, res=None if res is None else res.contiguous(), ldres=Cout, alpha=alpha, res_scale=res_scale)
    return y


@_op_conv2d_nt.register_fake
def _(x, w, bias, res, pad, stride, alpha, res_scale):
    B, H, W, _ = x.shape
    Cout, R, S, _ = w.shape
    Ho, Wo = _conv_out_hw(H, W, R, S, pad, stride)
    return x.new_empty((B, Ho, Wo, Cout))


@torch.library.custom_op("jg355::conv2d_wgrad", mutates_args=())
def _op_conv2d_wgrad(dy: torch.Tensor, x: torch.Tensor, R: int, S: int, pad: int, stride: int, alpha: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dW fp32 [Cout,R,S,Cin], dbias fp32 [Cout]) of y = alpha conv(x, W) + bias for the output gradient dy"""
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    dw = torch.zeros((Cout, R, S, Cin), device=x.device, dtype=torch.float32)
    db = torch.zeros((Cout,), device=x.device, dtype=torch.float32)
    ktot = R * S * Cin
    splitk = _wgrad_splitk(((Cout + 127) // 128) * ((ktot + 127) // 128), B * Ho * Wo)
    wgrad_tn(dy.contiguous(), x.contiguous(), dw, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, pad=pad, stride=stride, Ho=Ho, Wo=Wo,
             lddy=Cout, ldx=Cin, lddw=ktot, dbias=db, splitk=splitk, alpha=alpha)
    return dw, db


@_op_conv2d_wgrad.register_fake
def _(dy, x, R, S, pad, stride, alpha):
    return x.new_empty((dy.shape[-1], R, S, x.shape[-1]), dtype=torch.float32), x.new_empty((dy.shape[-1],), dtype=torch.float32)


def _conv2d_nt_setup(ctx, inputs, output):
    x, w, bias, res, pad, stride, alpha, res_scale = inputs
    ctx.save_for_backward(x, w)
    ctx.geo = (pad, stride, alpha, res_scale, bias is not None, res is not None)


def _conv2d_nt_backward(ctx, dy):
    x, w = ctx.saved_tensors
    pad, stride, alpha, res_scale, has_bias, has_res = ctx.geo
    Cout, R, S, Cin = w.shape
    dy = dy.contiguous()
    dx = dw = db = dres = None
    if ctx.needs_input_grad[0]:          # input gradient = the same kernel on the flipped / transposed weights
        wT = w.to(dy.dtype).permute(3, 1, 2, 0).flip(1, 2).contiguous()
        dyd = dy
        if stride != 1:                  # stride s: over the zero-dilated dy (length H + 2p - k + 1 per axis), as ops.conv2d_dgrad
            H, W_ = x.shape[1], x.shape[2]
            dyd = torch.ops.jg355.dilate2d(dy, H + 2 * pad - R + 1, W_ + 2 * pad - S + 1, stride)
        dx = torch.ops.jg355.conv2d_nt(dyd, wT, None, None, R - 1 - pad, 1, alpha, 0.0)
    if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
        dwf, dbf = torch.ops.jg355.conv2d_wgrad(dy, x, R, S, pad, stride, alpha)
        dw = dwf.to(w.dtype) if ctx.needs_input_grad[1] else None
        db = dbf if (has_bias and ctx.needs_input_grad[2]) else None
    if has_res and ctx.needs_input_grad[3]:
        dres = dy if res_scale == 1.0 else (dy.float() * res_scale).to(dy.dtype)
    return dx, dw, db, dres, None, None, None, None


_op_conv2d_nt.register_autograd(_conv2d_nt_backward, setup_context=_conv2d_nt_setup)


@torch.library.custom_op("jg355::group_norm_act", mutates_args=())
def _op_group_norm_act(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], film: Optional[torch.Tensor],
                       groups: int, act: int, eps: float) -> torch.Tensor:
    """act(GroupNorm_groups(x) gamma + beta [(1 + scale) + shift]); x NHWC 16-bit (any number of middle dims), film fp32 [B, 2C]"""
    return _group_norm_launch(x.contiguous(), gamma, beta, None if film is None else film.contiguous(), groups, act, eps)[0]


@_op_group_norm_act.register_fake
def _(x, gamma, beta, film, groups, act, eps):
    return torch.empty_like(x)


@torch.library.custom_op("jg355::group_norm_act_bwd", mutates_args=())
def _op_group_norm_act_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                           film: Optional[torch.Tensor], groups: int, act: int, eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dgamma [C], dbeta [C], dfilm [B, 2C]) -- the statistics are recomputed from x (two small kernels)"""
    L = _lib.lib()
    x, dy = x.contiguous(), dy.contiguous()
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    dev, st, dt = x.device, _st(), _dt(x)
    f32 = dict(device=dev, dtype=torch.float32)
    sums, ab, mr = torch.empty((B, C, 2), **f32), torch.empty((B, C, 2), **f32), torch.empty((B, groups, 2), **f32)
    film = None if film is None else film.contiguous()
    ldfilm = film.stride(0) if film is not None else 0
    check(L.jg_gn_stats(dt, x.data_ptr(), sums.data_ptr(), B, HW, C, st), "jg_gn_stats")
    check(L.jg_gn_coef(sums.data_ptr(), _p(gamma), _p(beta), _p(film), ldfilm, ab.data_ptr(), mr.data_ptr(), B, HW, C, groups, eps, st), "jg_gn_coef")
    red, pqr = torch.empty((B, C, 2), **f32), torch.empty((B, C, 3), **f32)
    dgamma, dbeta, dfilm = torch.zeros((C,), **f32), torch.zeros((C,), **f32), torch.zeros((B, 2 * C), **f32)
    check(L.jg_gn_bwd_reduce(dt, x.data_ptr(), dy.data_ptr(), ab.data_ptr(), red.data_ptr(), B, HW, C, act, st), "jg_gn_bwd_reduce")
    check(L.jg_gn_bwd_coef(red.data_ptr(), _p(gamma), _p(beta), _p(film), ldfilm, mr.data_ptr(), pqr.data_ptr(),
                           dgamma.data_ptr() if gamma is not None else None, dbeta.data_ptr() if beta is not None else None,
                           dfilm.data_ptr() if film is not None else None, 2 * C, B, HW, C, groups, st), "jg_gn_bwd_coef")
    dx = torch.empty_like(x)
    check(L.jg_gn_bwd_apply(dt, x.data_ptr(), dy.data_ptr(), ab.data_ptr(), pqr.data_ptr(), dx.data_ptr(), B, HW, C, act, st), "jg_gn_bwd_apply")
    return dx, dgamma, dbeta, dfilm


@_op_group_norm_act_bwd.register_fake
def _(x, dy, gamma, beta, film, groups, act, eps):
    B, C = x.shape[0], x.shape[-1]
    f = lambda *sh: x.new_empty(sh, dtype=torch.float32)
    return torch.empty_like(x), f(C), f(C), f(B, 2 * C)


def _gn_setup(ctx, inputs, output):
    x, gamma, beta, film, groups, act, eps = inputs
    ctx.save_for_backward(x, gamma, beta, film)
    ctx.cfg = (groups, act, eps)


def _gn_backward(ctx, dy):
    x, gamma, beta, film = ctx.saved_tensors
    groups, act, eps = ctx.cfg
    dx, dgamma, dbeta, dfilm = torch.ops.jg355.group_norm_act_bwd(x, dy, gamma, beta, film, groups, act, eps)
    return (dx if ctx.needs_input_grad[0] else None, dgamma if (gamma is not None and ctx.needs_input_grad[1]) else None,
            dbeta if (beta is not None and ctx.needs_input_grad[2]) else None,
            dfilm if (film is not None and ctx.needs_input_grad[3]) else None, None, None, None)


_op_group_norm_act.register_autograd(_gn_backward, setup_context=_gn_setup)


@torch.library.custom_op("jg355::group_norm_act_drop", mutates_args=())
def _op_group_norm_act_drop(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], film: Optional[torch.Tensor],
                            groups: int, act: int, eps: float, keep: float, u: Optional[torch.Tensor], key: Optional[torch.Tensor], stream: int,
                            call: int) -> torch.Tensor:
    """group_norm_act with nn.Dropout(1 - keep) behind the activation in the apply pass: x [B, H, W, C]; u fp32 [B, C, H, W] or None = drawn
    in the kernel from the two-word `key`, `stream` and `call`"""
    x = x.contiguous()
    return _group_norm_launch(x, gamma, beta, None if film is None else film.contiguous(), groups, act, eps, None, None,
                              _drop_args(x, keep, u, key, stream, call))[0]


@_op_group_norm_act_drop.register_fake
def _(x, gamma, beta, film, groups, act, eps, keep, u, key, stream, call):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("jg355::group_norm_act_drop_bwd", mutates_args=())
def _op_group_norm_act_drop_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                                film: Optional[torch.Tensor], groups: int, act: int, eps: float, keep: float, u: Optional[torch.Tensor],
                                key: Optional[torch.Tensor], stream: int, call: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dgamma [C], dbeta [C], dfilm [B, 2C]) -- the statistics are recomputed from x, the mask is regenerated"""
    L = _lib.lib()
    x, dy = x.contiguous(), dy.contiguous()
    drop = _drop_args(x, keep, u, key, stream, call)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    f32 = dict(device=x.device, dtype=torch.float32)
    sums, ab, mr = torch.empty((B, C, 2), **f32), torch.empty((B, C, 2), **f32), torch.empty((B, groups, 2), **f32)
    film = None if film is None else film.contiguous()
    ldfilm = film.stride(0) if film is not None else 0
    check(L.jg_gn_stats(_dt(x), x.data_ptr(), sums.data_ptr(), B, HW, C, _st()), "jg_gn_stats")
    check(L.jg_gn_coef(sums.data_ptr(), _p(gamma), _p(beta), _p(film), ldfilm, ab.data_ptr(), mr.data_ptr(), B, HW, C, groups, eps, _st()), "jg_gn_coef")
    dgamma, dbeta, dfilm = torch.zeros((C,), **f32), torch.zeros((C,), **f32), torch.zeros((B, 2 * C), **f32)
    dx = _gn_drop_bwd_launch(x, dy, ab, mr, gamma, beta, film, groups, act, drop, torch.zeros((B, C, 2), **f32), dgamma if gamma is not None else None,
                             dbeta if beta is not None else None, dfilm if film is not None else None)
    return dx, dgamma, dbeta, dfilm


@_op_group_norm_act_drop_bwd.register_fake
def _(x, dy, gamma, beta, film, groups, act, eps, keep, u, key, stream, call):
    B, C = x.shape[0], x.shape[-1]
    f = lambda *sh: x.new_empty(sh, dtype=torch.float32)
    return torch.empty_like(x, memory_format=torch.contiguous_format), f(C), f(C), f(B, 2 * C)


def _gnd_setup(ctx, inputs, output):
    x, gamma, beta, film, groups, act, eps, keep, u, key, stream, call = inputs
    ctx.save_for_backward(x, gamma, beta, film, u, key)
    ctx.cfg = (groups, act, eps, keep, stream, call)


def _gnd_backward(ctx, dy):
    x, gamma, beta, film, u, key = ctx.saved_tensors
    groups, act, eps, keep, stream, call = ctx.cfg
    dx, dgamma, dbeta, dfilm = torch.ops.jg355.group_norm_act_drop_bwd(x, dy, gamma, beta, film, groups, act, eps, keep, u, key, stream, call)
    return (dx if ctx.needs_input_grad[0] else None, dgamma if (gamma is not None and ctx.needs_input_grad[1]) else None,
            dbeta if (beta is not None and ctx.needs_input_grad[2]) else None,
            dfilm if (film is not None and ctx.needs_input_grad[3]) else None) + (None,) * 8


_op_group_norm_act_drop.register_autograd(_gnd_backward, setup_context=_gnd_setup)


@torch.library.custom_op("jg355::act_drop", mutates_args=())
def _op_act_drop(x: torch.Tensor, act: int, keep: float, u: Optional[torch.Tensor], key: Optional[torch.Tensor], stream: int,
                 call: int) -> torch.Tensor:
    """nn.Dropout(1 - keep)(act(x)) in one pass, no normalisation in front: x [B, H, W, C]"""
    x = x.contiguous()
    return launch.gn_apply_drop(x, None, act, *_drop_args(x, keep, u, key, stream, call))


@_op_act_drop.register_fake
def _(x, act, keep, u, key, stream, call):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("jg355::act_drop_bwd", mutates_args=())
def _op_act_drop_bwd(x: torch.Tensor, dy: torch.Tensor, act: int, keep: float, u: Optional[torch.Tensor], key: Optional[torch.Tensor], stream: int,
                     call: int) -> torch.Tensor:
    """dx = (dy m / keep) act'(x), the mask regenerated"""
    x = x.contiguous()
    return launch.gn_bwd_apply_drop(x, dy.contiguous(), None, None, act, *_drop_args(x, keep, u, key, stream, call))


@_op_act_drop_bwd.register_fake
def _(x, dy, act, keep, u, key, stream, call):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


def _ad_setup(ctx, inputs, output):
    x, act, keep, u, key, stream, call = inputs
    ctx.save_for_backward(x, u, key)
    ctx.cfg = (act, keep, stream, call)


def _ad_backward(ctx, dy):
    x, u, key = ctx.saved_tensors
    act, keep, stream, call = ctx.cfg
    return (torch.ops.jg355.act_drop_bwd(x, dy, act, keep, u, key, stream, call),) + (None,) * 6


_op_act_drop.register_autograd(_ad_backward, setup_context=_ad_setup)


# the two passes of a dropout behind a low-resolution GroupNorm + nearest 2x upsample (the up-blocks of the efficient diffusion UNet on the fused
# schedule, modules/unet_exec.py): plain functional kernels, the schedule's hand-written backward chains them
@torch.library.custom_op("jg355::gn_apply_drop_up2", mutates_args=())
def _op_gn_apply_drop_up2(x: torch.Tensor, ab: Optional[torch.Tensor], act: int, keep: float, u: Optional[torch.Tensor], key: Optional[torch.Tensor],
                          stream: int, call: int) -> torch.Tensor:
    """y [B, 2H, 2W, C] = m * act(a up2(x) + b) / keep from x [B, H, W, C]; ab fp32 [B, C, 2] (None: a = 1, b = 0); u fp32 [B, C, 2H, 2W] or None
    = drawn from `key` on the counter of the high-resolution map"""
    x = x.contiguous()
    B, H, W, C = x.shape
    if ab is not None:
        if ab.dtype != torch.float32 or tuple(ab.shape) != (B, C, 2):
            raise ValueError(f"gn_apply_drop_up2: ab must be fp32 [B, C, 2] = {(B, C, 2)}, got {ab.dtype} {tuple(ab.shape)}")
        ab = ab.contiguous()
        _require_cuda(ab)
    return launch.gn_apply_drop_up2(x, ab, act, *_drop_args(x, keep, u, key, stream, call, shape=(B, 2 * H, 2 * W, C)))


@_op_gn_apply_drop_up2.register_fake
def _(x, ab, act, keep, u, key, stream, call):
    B, H, W, C = x.shape
    return x.new_empty((B, 2 * H, 2 * W, C))


@torch.library.custom_op("jg355::drop_pool2_bwd", mutates_args=())
def _op_drop_pool2_bwd(dy: torch.Tensor, keep: float, u: Optional[torch.Tensor], key: Optional[torch.Tensor], stream: int, call: int) -> torch.Tensor:
    """g [B, H, W, C] = 2 x 2 sums of dy * m / keep from dy [B, 2H, 2W, C], the mask of gn_apply_drop_up2 regenerated"""
    dy = dy.contiguous()
    if dy.dim() != 4 or dy.shape[1] % 2 or dy.shape[2] % 2:
        raise ValueError(f"drop_pool2_bwd: dy [B, 2H, 2W, C], got {tuple(dy.shape)}")
    return launch.drop_pool2_bwd(dy, *_drop_args(dy, keep, u, key, stream, call))


@_op_drop_pool2_bwd.register_fake
def _(dy, keep, u, key, stream, call):
    B, H2, W2, C = dy.shape
    return dy.new_empty((B, H2 // 2, W2 // 2, C))


@torch.library.custom_op("jg355::attention_core", mutates_args=())
def _op_attention_core(qkv: torch.Tensor, heads: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """QKVAttentionLegacy core: qkv [B,T,3C] (legacy head layout) -> (a [B,T,C], aux) with aux = per-query logsumexp of the fused
    kernel (head dim 32, T % 128 == 0) or the softmax probabilities of the unfused path (what the backward needs)"""
    a, P = attn_core_fwd(qkv.contiguous(), heads)
    return a, P


@_op_attention_core.register_fake
def _(qkv, heads):
    B, T, C3 = qkv.shape
    Cc = C3 // 3
    a = qkv.new_empty((B, T, Cc))
    if FLASH_ATTENTION and Cc // heads == 32 and T % 128 == 0:
        return a, qkv.new_empty((B * heads, T), dtype=torch.float32)
    return a, qkv.new_empty((B * heads, T, T))


@torch.library.custom_op("jg355::attention_core_bwd", mutates_args=())
def _op_attention_core_bwd(qkv: torch.Tensor, aux: torch.Tensor, a: torch.Tensor, da: torch.Tensor, heads: int) -> torch.Tensor:
    return attn_core_bwd(qkv.contiguous(), aux, da, heads, a)


@_op_attention_core_bwd.register_fake
def _(qkv, aux, a, da, heads):
    return torch.empty_like(qkv)


def _attn_setup(ctx, inputs, output):
    qkv, heads = inputs
    a, aux = output
    ctx.save_for_backward(qkv, aux, a)
    ctx.heads = heads


def _attn_backward(ctx, da, daux):
    qkv, aux, a = ctx.saved_tensors
    return torch.ops.jg355.attention_core_bwd(qkv, aux, a, da.contiguous(), ctx.heads), None


_op_attention_core.register_autograd(_attn_backward, setup_context=_attn_setup)


@torch.library.custom_op("jg355::resample2", mutates_args=())
def _op_resample2(x: torch.Tensor, up: bool, scale: float) -> torch.Tensor:
    """up: nearest x2 upsample times `scale`; else 2x2 SUM pool times `scale` (avg_pool = 0.25).  Each is the other's adjoint."""
    return _up(x.contiguous(), scale) if up else _pool(x.contiguous(), scale)


@_op_resample2.register_fake
def _(x, up, scale):
    B, H, W, Cc = x.shape
    return x.new_empty((B, H * 2, W * 2, Cc)) if up else x.new_empty((B, H // 2, W // 2, Cc))


def _resample_setup(ctx, inputs, output):
    ctx.cfg = (inputs[1], inputs[2])


def _resample_backward(ctx, dy):
    up, scale = ctx.cfg
    return torch.ops.jg355.resample2(dy.contiguous(), not up, scale), None, None


_op_resample2.register_autograd(_resample_backward, setup_context=_resample_setup)


@torch.library.custom_op("jg355::linear_act", mutates_args=())
def _op_linear_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int) -> torch.Tensor:
    """y = act(x) @ weight.T + bias, fp32 (`emb_layers` / `cond_embed` of the UNet: nn.Linear behind an optional SiLU)"""
    return launch.linear_fwd(x.contiguous(), weight.contiguous(), bias, act)


@_op_linear_act.register_fake
def _(x, weight, bias, act):
    return x.new_empty((x.shape[0], weight.shape[0]), dtype=torch.float32)


@torch.library.custom_op("jg355::linear_act_bwd", mutates_args=())
def _op_linear_act_bwd(x: torch.Tensor, weight: torch.Tensor, dy: torch.Tensor, act: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    x, weight, dy = x.contiguous(), weight.contiguous(), dy.contiguous()
    dW, db = torch.zeros_like(weight), torch.zeros((weight.shape[0],), device=x.device, dtype=torch.float32)
    return launch.linear_bwd(x, weight, dy, act, dW, db), dW, db


@_op_linear_act_bwd.register_fake
def _(x, weight, dy, act):
    return torch.empty_like(x), torch.empty_like(weight), x.new_empty((weight.shape[0],), dtype=torch.float32)


def _linear_setup(ctx, inputs, output):
    x, weight, bias, act = inputs
    ctx.save_for_backward(x, weight)
    ctx.act, ctx.has_bias = act, bias is not None


def _linear_backward(ctx, dy):
    x, weight = ctx.saved_tensors
    dx, dW, db = torch.ops.jg355.linear_act_bwd(x, weight, dy.contiguous(), ctx.act)
    return (dx if ctx.needs_input_grad[0] else None, dW if ctx.needs_input_grad[1] else None,
            db if (ctx.has_bias and ctx.needs_input_grad[2]) else None, None)


_op_linear_act.register_autograd(_linear_backward, setup_context=_linear_setup)


@torch.library.custom_op("jg355::gamma_embedding", mutates_args=())
def _op_gamma_embedding(gammas: torch.Tensor, dim: int, max_period: float) -> torch.Tensor:
    """sinusoidal noise-level embedding (models/modules/diffusion_utils.py:8-42); not differentiated (the levels are data)"""
    global _IN_OP
    prev, _IN_OP = _IN_OP, True
    try:
        return gamma_embedding(gammas, dim, max_period)
    finally:
        _IN_OP = prev


@_op_gamma_embedding.register_fake
def _(gammas, dim, max_period):
    return gammas.new_empty((gammas.numel(), dim), dtype=torch.float32)


@torch.library.custom_op("jg355::ddpm_prepare", mutates_args=())
def _op_ddpm_prepare(y0: torch.Tensor, ycond: torch.Tensor, noise: torch.Tensor, mask: Optional[torch.Tensor], gammas: torch.Tensor,
                     fp16: bool, cpad: int) -> torch.Tensor:
    """q_sample + mask blend + cat([y_cond, y_noisy]) of DiffusionGenerator.forward (diffusion_generator.py:480-491) -> NHWC 16-bit"""
    global _IN_OP
    prev, _IN_OP = _IN_OP, True
    try:
        return ddpm_prepare(y0, ycond, noise, mask, gammas, torch.float16 if fp16 else torch.bfloat16, cpad)
    finally:
        _IN_OP = prev


@_op_ddpm_prepare.register_fake
def _(y0, ycond, noise, mask, gammas, fp16, cpad):
    B, _, H, W = y0.shape
    return y0.new_empty((B, H, W, cpad), dtype=torch.float16 if fp16 else torch.bfloat16)


@torch.library.custom_op("jg355::lowres_roundtrip", mutates_args=())
def _op_lowres_roundtrip(x: torch.Tensor, hlo: int, wlo: int) -> torch.Tensor:
    """anti-aliased bilinear resize to (hlo, wlo) and back (palette_model.py:546-548); not differentiated (the ground truth is data)"""
    global _IN_OP
    prev, _IN_OP = _IN_OP, True
    try:
        return lowres_roundtrip(x, (hlo, wlo))
    finally:
        _IN_OP = prev


@_op_lowres_roundtrip.register_fake
def _(x, hlo, wlo):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("jg355::ect_loss", mutates_args=())
def _op_ect_loss(Fn: torch.Tensor, Fc: torch.Tensor, noisy_n: torch.Tensor, noisy_c: torch.Tensor, cs_n: torch.Tensor, co_n: torch.Tensor,
                 cs_c: torch.Tensor, co_c: torch.Tensor, mask: Optional[torch.Tensor], dt: torch.Tensor, lam: float,
                 grad_scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(easy-consistency-tuning loss, its gradient w.r.t. Fn times grad_scale) of compute_ect_loss (cm_model.py:412-442): jg_ect_loss"""
    f = lambda t: t.reshape(-1).contiguous().float()
    m = None if mask is None else mask.contiguous().long()
    return _ect_loss_launch(Fn.contiguous(), Fc.contiguous(), noisy_n.contiguous(), noisy_c.contiguous(), f(cs_n), f(co_n), f(cs_c), f(co_c),
                            m, f(dt), lam, grad_scale)


@_op_ect_loss.register_fake
def _(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, dt, lam, grad_scale):
    return Fn.new_empty((), dtype=torch.float32), torch.empty_like(Fn, memory_format=torch.contiguous_format)


def _ect_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.set_materialize_grads(False)


def _ect_backward(ctx, gloss, gdFn):
    (dFn,) = ctx.saved_tensors
    g = None if gloss is None else axpby(dFn, 1.0, alpha_dev=gloss.contiguous().float())
    return (g,) + (None,) * 11


_op_ect_loss.register_autograd(_ect_backward, setup_context=_ect_setup)


@torch.library.custom_op("jg355::cm_gan_head", mutates_args=())
def _op_cm_gan_head(Fn: torch.Tensor, Fc: torch.Tensor, noisy_n: torch.Tensor, noisy_c: torch.Tensor, cs_n: torch.Tensor, co_n: torch.Tensor,
                    cs_c: torch.Tensor, co_c: torch.Tensor, mask: Optional[torch.Tensor], w: torch.Tensor, lam: float,
                    grad_scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(consistency loss, the student's prediction NHWC 16-bit, the loss's gradient w.r.t. Fn times grad_scale): jg_cm_gan_head"""
    f = lambda t: t.reshape(-1).contiguous().float()
    m = None if mask is None else mask.contiguous().long()
    loss, dFn, pred = _cm_gan_head_launch(Fn.contiguous(), Fc.contiguous(), noisy_n.contiguous(), noisy_c.contiguous(), f(cs_n), f(co_n),
                                          f(cs_c), f(co_c), m, f(w), lam, grad_scale)
    return loss, pred, dFn


@_op_cm_gan_head.register_fake
def _(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w, lam, grad_scale):
    e = lambda: torch.empty_like(Fn, memory_format=torch.contiguous_format)
    return Fn.new_empty((), dtype=torch.float32), e(), e()


def _cm_gan_head_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2], inputs[5])
    ctx.Cc = inputs[2].shape[1]
    ctx.set_materialize_grads(False)


def _cm_gan_head_backward(ctx, gloss, gpred, gdFn):
    dFn, co_n = ctx.saved_tensors
    g = None
    if gloss is not None or gpred is not None:
        g = _cm_gan_head_bwd_launch(dFn, gpred, gloss, co_n.reshape(-1).contiguous().float(), ctx.Cc)
    return (g,) + (None,) * 11


_op_cm_gan_head.register_autograd(_cm_gan_head_backward, setup_context=_cm_gan_head_setup)


@torch.library.custom_op("jg355::ddpm_mse_loss", mutates_args=())
def _op_ddpm_mse_loss(nh: torch.Tensor, noise: torch.Tensor, mask: Optional[torch.Tensor], w: Optional[torch.Tensor], lam: float,
                      grad_scale: float, channels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lambda MSE(w m noise, w m noise_hat), its gradient w.r.t. noise_hat times grad_scale) in one pass (palette_model.py:597-620)"""
    return launch.ddpm_mse_loss(nh.contiguous(), noise.contiguous(), mask, w, lam, grad_scale, channels)


@_op_ddpm_mse_loss.register_fake
def _(nh, noise, mask, w, lam, grad_scale, channels):
    return nh.new_empty((), dtype=torch.float32), torch.empty_like(nh)


def _mse_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.set_materialize_grads(False)


def _mse_backward(ctx, gloss, gdnh):
    (dnh,) = ctx.saved_tensors
    g = None if gloss is None else (dnh.float() * gloss.float()).to(dnh.dtype)
    return g, None, None, None, None, None, None


_op_ddpm_mse_loss.register_autograd(_mse_backward, setup_context=_mse_setup)



from . import ops_library_cut  # noqa: E402,F401  (registers the CUT-family torch.ops.jg355.* entries)
