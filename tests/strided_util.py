"""Channel-slice operands with canaries, for tests of the stride contract of include/jg355.h ("every tensor carries its own pixel stride
(elements, multiple of 8, >= C)"): the UNet executor never concatenates, every kernel is launched on channel slices of wider NHWC buffers.

A slice is a view [B, H, W, C] of ONE allocation laid out as  guard pixels | B*H*W pixels of `left + C + right` channels | guard pixels.
Everything outside the view is a canary:
  role "in" : NaN of the dtype -- an out-of-slice read that reaches the result poisons it (0 * NaN = NaN);
  role "out": one fixed bit pattern, compared bit for bit afterwards; the view itself is pre-filled with a second pattern so that an
              element the kernel never wrote is told apart from one it wrote;
  role "acc": canary as "out", view holding the given start values (zeros by default) -- operands a kernel accumulates into.
Nothing is ever accessed outside the allocation: a kernel that strays by less than `guard` pixels hits the canary, not foreign memory.

Plain torch, no GPU needed: tests/test_strided_util_host.py drives it with CPU stand-ins for a kernel.
"""
from collections import namedtuple

import torch

# finite in fp16 (59200. / 4444.) and in bf16 / fp32, far outside anything the tests compute
CANARY16, PREFILL16 = 0x7B3A, 0x6C57
CANARY32, PREFILL32 = 0x7B3A5C96, 0x6C57A3E1
_INT = {2: torch.int16, 4: torch.int32}

ViewSpec = namedtuple("ViewSpec", "shape left right guard role ld npix")
# unit: channel granularity of the placement (2 for statistics rows of (sum, sum of squares) float pairs)
Operand = namedtuple("Operand", "shape dtype role seed values scale unit", defaults=(0, None, 1.0, 1))
Pair = namedtuple("Pair", "contig strided contig_bufs strided_bufs kernels returns")

EXEC_LIKE = "exec"      # left a multiple of 64, as in the UNet concat buffers
ABI_MIN = "abi"         # left 8, right 24 (+16 per further operand): 16-byte aligned and nothing more
PLACEMENTS = (EXEC_LIKE, ABI_MIN)


def _signed(pattern, bits):
    return pattern - (1 << bits) if pattern >= (1 << (bits - 1)) else pattern


def _patterns(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    assert es in _INT, f"16- and 32-bit operands only, got {dtype}"
    return (_signed(CANARY16, 16), _signed(PREFILL16, 16)) if es == 2 else (_signed(CANARY32, 32), _signed(PREFILL32, 32))


def placement(kind, index, scale=1):
    """(left, right) of operand number `index` of a launch: no two operands of a launch share a pixel stride at equal C.
    scale: 2 for rows of (sum, sum of squares) pairs, whose channel unit is two floats."""
    if kind == EXEC_LIKE:
        left, right = 64 * (1 + index % 4), 8 * (1 + index) + 64 * (index // 4)
    elif kind == ABI_MIN:
        left, right = 8, 24 + 16 * index
    else:
        raise ValueError(kind)
    return left * scale, right * scale


def make_slice(shape_bhwc, dtype, seed, *, left, right, guard, role, values=None, scale=1.0, device="cpu"):
    """(buffer, view): `view` = buffer[guard pixels : -guard pixels] as [B, H, W, left + C + right][..., left : left + C]; see the module text.
    values: contents of the view (role "in" / "acc"), default randn(seed) * scale for "in" and zeros for "acc".  buffer.spec is the ViewSpec."""
    B, H, W, Cc = shape_bhwc
    assert guard >= 1 and left >= 0 and right >= 0 and role in ("in", "out", "acc")
    ld, npix = left + Cc + right, B * H * W
    canary, prefill = _patterns(dtype)
    idt = _INT[torch.empty((), dtype=dtype).element_size()]
    if role == "in":
        buf = torch.full(((npix + 2 * guard) * ld,), float("nan"), dtype=dtype)
    else:
        buf = torch.full(((npix + 2 * guard) * ld,), canary, dtype=idt).view(dtype)
    inner = buf[guard * ld:(guard + npix) * ld].view(B, H, W, ld)[..., left:left + Cc]
    if role == "out":
        inner.view(idt).fill_(prefill)
    elif values is not None:
        inner.copy_(values.reshape(shape_bhwc).to(dtype))
    elif role == "in":
        inner.copy_((torch.randn(shape_bhwc, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype))
    else:
        inner.zero_()
    buf = buf.to(device)
    view = buf[guard * ld:(guard + npix) * ld].view(B, H, W, ld)[..., left:left + Cc]
    buf.spec = ViewSpec(tuple(shape_bhwc), left, right, guard, role, ld, npix)
    return buf, view


def flat_of(view):
    """(the whole allocation behind `view` as a 1-D tensor sharing its memory, element offset of the view, pixel stride)"""
    n = view.untyped_storage().nbytes() // view.element_size()
    return torch.as_strided(view, (n,), (1,), 0), view.storage_offset(), view.stride(-2)


def _rows(buffer, spec):
    idt = _INT[buffer.element_size()]
    return buffer.detach().cpu().view(idt).view(spec.npix + 2 * spec.guard, spec.ld)


def _positions(mask, spec, limit=5):
    """first few True positions of a [rows, ld] mask as (pixel, channel) relative to the view's first pixel / first channel"""
    idx = mask.nonzero()[:limit].tolist()
    return [(p - spec.guard, c - spec.left) for p, c in idx]


def assert_canary_intact(buffer, view_spec=None):
    """every element outside the view still holds the canary, bit for bit (NaN canaries of role "in" included: inputs are never written)"""
    spec = view_spec or buffer.spec
    rows = _rows(buffer, spec)
    outside = torch.ones(rows.shape, dtype=torch.bool)
    outside[spec.guard:spec.guard + spec.npix, spec.left:spec.left + spec.shape[3]] = False
    if spec.role == "in":
        want = torch.full((1,), float("nan"), dtype=buffer.dtype).view(rows.dtype)
    else:
        want = torch.tensor([_patterns(buffer.dtype)[0]], dtype=rows.dtype)
    bad = outside & (rows != want)
    assert not bool(bad.any()), (f"{int(bad.sum())} elements outside the slice were overwritten; first (pixel, channel) relative to the view: "
                                 f"{_positions(bad, spec)} (view {spec.shape}, left {spec.left}, right {spec.right}, ld {spec.ld})")


def assert_fully_written(buffer, view_spec=None):
    """no element of a role-"out" view still holds the pre-fill pattern"""
    spec = view_spec or buffer.spec
    assert spec.role == "out"
    rows = _rows(buffer, spec)
    inside = torch.zeros(rows.shape, dtype=torch.bool)
    inside[spec.guard:spec.guard + spec.npix, spec.left:spec.left + spec.shape[3]] = True
    bad = inside & (rows == _patterns(buffer.dtype)[1])
    assert not bool(bad.any()), (f"{int(bad.sum())} elements of the output view were never written; first (pixel, channel): "
                                 f"{_positions(bad, spec)} (view {spec.shape}, ld {spec.ld})")


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def row_errors(got, ref):
    """per-row error ||got_r - ref_r||_2 / (||ref||_F / sqrt(nrows)), a row being the last-dimension vector: relative to the RMS row norm of the
    reference, so that a row whose true value is tiny does not blow up.  Independent roundings give every row the norm-wise relative error."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rms = float(ref.norm()) / (ref.shape[0] ** 0.5) + 1e-30
    return (got - ref).norm(dim=1) / rms


def assert_rows_close(got, ref, bound, what, worst=5):
    """every row of `got` within `bound` of `ref` (row_errors); reports the worst few (row index, error) pairs"""
    e = row_errors(got, ref)
    assert not bool(torch.isnan(e).any()), f"{what}: NaN in rows {torch.isnan(e).nonzero()[:worst, 0].tolist()}"
    top = torch.topk(e, min(worst, e.numel()))
    pairs = [(int(i), float(f"{float(v):.3e}")) for v, i in zip(top.values, top.indices)]
    assert float(top.values[0]) < bound, f"{what}: {int((e >= bound).sum())} of {e.numel()} rows outside the per-row bound {bound:.1e}; worst (row, error): {pairs}"
    return pairs[0]


def _default_last_kernel():
    from joligen_amd import _lib

    return _lib.lib().jg_last_kernel().decode()


def _default_set_tuning(name, value):
    from joligen_amd import _lib

    return _lib.set_tuning(name, value)


def _default_sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def run_pair(launch, operands, *, kind=EXEC_LIKE, tuning=None, device="cpu", guard=3, fixed=(), share=None, last_kernel=_default_last_kernel,
             set_tuning=_default_set_tuning, sync=_default_sync):
    """Run `launch(views)` twice under the same tuning switches: on contiguous operands (left = right = 0, guards kept), then on slices that hold
    the same values, every operand on its own stride (`placement(kind, i)`; names in `fixed` stay contiguous; `share` = {name: other} places
    `name` as `other` is placed, for entry points that take ONE stride for two operands, such as q and dq of jg_attn_smallkv_bwd2).
    operands: {name: Operand}; launch receives {name: view} and reads pixel strides from view.stride(-2).
    Returns Pair(contig views, strided views, contig buffers, strided buffers, (kernel after run 1, kernel after run 2), launch's returns)."""
    prev = {k: set_tuning(k, v) for k, v in (tuning or {}).items()}
    share = share or {}
    index = {name: i for i, name in enumerate(operands)}
    try:
        runs = []
        for strided in (False, True):
            bufs, views = {}, {}
            for i, (name, op) in enumerate(operands.items()):
                left, right = placement(kind, index[share.get(name, name)], op.unit) if strided and name not in fixed else (0, 0)
                bufs[name], views[name] = make_slice(op.shape, op.dtype, op.seed, left=left, right=right, guard=guard, role=op.role,
                                                     values=op.values, scale=op.scale, device=device)
            pads = [b.spec.ld - b.spec.shape[3] for n, b in bufs.items() if strided and n not in fixed and n not in share]
            assert len(set(pads)) == len(pads), pads
            ret = launch(views)
            sync()
            runs.append((views, bufs, last_kernel(), ret))
    finally:
        for k, v in prev.items():
            set_tuning(k, v)
    (v0, b0, k0, r0), (v1, b1, k1, r1) = runs
    return Pair(v0, v1, b0, b1, (k0, k1), (r0, r1))


def verify(pair, *, exact=(), approx=None, kernel=None):
    """assertions (a), (b) and (d) of the strided-operand tests on a Pair:
    (a) both launches went to the same kernel instance (and to `kernel`, if given);
    (b) outputs named in `exact` are bit-identical between the two launches, those in `approx` ({name: bound}) agree norm-wise;
    (d) every buffer's canary is intact, every role-"out" view is fully written, no output holds a NaN."""
    approx = approx or {}
    k0, k1 = pair.kernels
    assert k0 == k1, f"dispatch changed with the stride: contiguous -> {k0!r}, strided -> {k1!r}"
    if kernel is not None:
        assert k1 == kernel, f"expected kernel instance {kernel!r}, got {k1!r}"
    for bufs in (pair.contig_bufs, pair.strided_bufs):
        for name, buf in bufs.items():
            try:
                assert_canary_intact(buf)
                if buf.spec.role == "out":
                    assert_fully_written(buf)
            except AssertionError as e:
                raise AssertionError(f"operand {name!r} ({'strided' if bufs is pair.strided_bufs else 'contiguous'} launch): {e}") from None
    for name in list(exact) + list(approx):
        a, b = pair.strided[name], pair.contig[name]
        assert not bool(torch.isnan(a.float()).any()), f"NaN in output {name!r} of the strided launch"
        assert not bool(torch.isnan(b.float()).any()), f"NaN in output {name!r} of the contiguous launch"
        if name in approx:
            e = relerr(a, b)
            assert e < approx[name], f"output {name!r}: strided vs contiguous launch differ by {e:.3e} (bound {approx[name]:.1e})"
        else:
            idt = _INT[a.element_size()]
            same = a.contiguous().view(idt) == b.contiguous().view(idt)
            if not bool(same.all()):
                bad = (~same).reshape(-1, same.shape[-1]).cpu()
                raise AssertionError(f"output {name!r}: strided launch differs from the contiguous one in {int(bad.sum())} elements; first "
                                     f"(pixel, channel): {bad.nonzero()[:5].tolist()}")


Single = namedtuple("Single", "views bufs kernel ret")


def run_once(launch, operands, *, tuning=None, device="cpu", guard=3, last_kernel=_default_last_kernel, set_tuning=_default_set_tuning,
             sync=_default_sync):
    """One launch on contiguous guarded operands (left = right = 0) under the given tuning switches: run_pair's first half, for tests that
    compare with a reference instead of a second launch.  Returns Single(views, buffers, kernel after the launch, launch's return)."""
    prev = {k: set_tuning(k, v) for k, v in (tuning or {}).items()}
    try:
        bufs, views = {}, {}
        for name, op in operands.items():
            bufs[name], views[name] = make_slice(op.shape, op.dtype, op.seed, left=0, right=0, guard=guard, role=op.role, values=op.values,
                                                 scale=op.scale, device=device)
        ret = launch(views)
        sync()
        kernel = last_kernel()
    finally:
        for k, v in prev.items():
            set_tuning(k, v)
    return Single(views, bufs, kernel, ret)


def verify_once(single, *, kernel=None):
    """(a) the launch went to `kernel` (if given); (d) every canary is intact, every role-"out" view fully written, no output holds a NaN"""
    if kernel is not None:
        assert single.kernel == kernel, f"expected kernel instance {kernel!r}, got {single.kernel!r}"
    for name, buf in single.bufs.items():
        try:
            assert_canary_intact(buf)
            if buf.spec.role == "out":
                assert_fully_written(buf)
        except AssertionError as e:
            raise AssertionError(f"operand {name!r}: {e}") from None
        if buf.spec.role != "in":
            assert not bool(torch.isnan(single.views[name].float()).any()), f"NaN in output {name!r}"


def assert_bit_equal(got, ref, what):
    """`got` [..., C] equals the float64 `ref` (same shape) rounded to got's dtype, bit for bit, in every element; reports the count and the first
    few (pixel, channel) positions with got / want"""
    got = got.detach().cpu().contiguous()
    want = (ref.detach().cpu() + 0.0).to(got.dtype).contiguous()      # + 0.0: a zero of the reference is +0, as a sum that starts from +0 gives it
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    idt = _INT[got.element_size()]
    bad = got.view(idt) != want.view(idt)
    if bool(bad.any()):
        bad2 = bad.reshape(-1, bad.shape[-1])
        g2, w2 = got.reshape(bad2.shape), want.reshape(bad2.shape)
        first = [((p, c), float(g2[p, c]), float(w2[p, c])) for p, c in bad2.nonzero()[:5].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first ((pixel, channel), got, "
                             f"want): {first}")
