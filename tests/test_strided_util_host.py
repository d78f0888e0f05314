"""tests/strided_util.py against torch-on-CPU stand-ins for a kernel (no GPU): the harness accepts a correct stand-in and flags each class
of addressing bug the strided-operand GPU tests (test_gpu_17_strided_operands.py) exist to catch.

The stand-in computes y[p][c] = 0.5 * x[p][c] + 0.7 * res[p][c] the way a kernel does: flat element indices `base + p * ld + c` into the
allocation behind each operand, so a wrong stride or an index past the slice lands where it would on the device."""
import pytest
import torch

import strided_util as su

B, H, W, C = 2, 4, 8, 16
P = B * H * W
TILE = 16       # pixels per "tile" of the stand-in


def _idx(off, ld, npix, nch, p0=0, c0=0):
    return off + (p0 + torch.arange(npix))[:, None] * ld + (c0 + torch.arange(nch))[None, :]


def standin(v, bug=None):
    (fx, ox, ldx), (fr, orr, ldr), (fy, oy, ldy) = su.flat_of(v["x"]), su.flat_of(v["res"]), su.flat_of(v["y"])
    x = fx[_idx(ox, ldx, P, C)].float()
    r = fr[_idx(orr, ldy if bug == "res_uses_ldy" else ldr, P, C)].float()
    out = 0.5 * x + 0.7 * r
    if bug == "read_neighbour_times_zero":      # a K tail that multiplies the right-hand neighbour channels by zero
        out = out + 0.0 * fx[_idx(ox, ldx, P, 8, c0=C)].float().sum(1, keepdim=True)
    p0 = TILE if bug == "tile_unwritten" else 0
    fy[_idx(oy, ldy, P - p0, C, p0=p0)] = out[p0:].to(fy.dtype)
    if bug == "write_past_slice":               # one 8-channel group past the slice, in the first pixel
        fy[_idx(oy, ldy, 1, 8, c0=C)] = out[:1, :8].to(fy.dtype)
    if bug == "write_guard_pixel":              # the pixel after the last row
        fy[_idx(oy, ldy, 1, C, p0=P)] = out[:1].to(fy.dtype)


def _pair(dtype, kind, bug):
    ops = {"x": su.Operand((B, H, W, C), dtype, "in", 1), "y": su.Operand((B, H, W, C), dtype, "out"), "res": su.Operand((B, H, W, C), dtype, "in", 2)}
    return su.run_pair(lambda v: standin(v, bug), ops, kind=kind, last_kernel=lambda: "standin", set_tuning=lambda k, v: 0, sync=lambda: None)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
def test_correct_standin_is_accepted(kind, dtype):
    pair = _pair(dtype, kind, None)
    su.verify(pair, exact=["y"], kernel="standin")
    x, r = pair.strided["x"].double(), pair.strided["res"].double()
    assert su.relerr(pair.strided["y"], 0.5 * x + 0.7 * r) < 8e-3
    strides = {pair.strided[n].stride(-2) for n in ("x", "res", "y")}
    assert len(strides) == 3 and all(s % 8 == 0 and s > C for s in strides)        # every operand on its own stride
    for n in ("x", "res", "y"):
        assert pair.contig[n].stride(-2) == C and (pair.strided[n].storage_offset() * 2) % 16 == 0


BUGS = {
    "write_past_slice": "outside the slice were overwritten",
    "write_guard_pixel": "outside the slice were overwritten",
    "read_neighbour_times_zero": "NaN in output",
    "res_uses_ldy": "NaN in output|differs from the contiguous",
    "tile_unwritten": "never written",
}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kind", su.PLACEMENTS)
@pytest.mark.parametrize("bug", sorted(BUGS))
def test_sabotaged_standin_is_flagged(bug, kind, dtype):
    pair = _pair(dtype, kind, bug)
    with pytest.raises(AssertionError, match=BUGS[bug]):
        su.verify(pair, exact=["y"], kernel="standin")


def test_failure_reports_positions():
    pair = _pair(torch.float16, su.ABI_MIN, "write_past_slice")
    with pytest.raises(AssertionError) as e:
        su.assert_canary_intact(pair.strided_bufs["y"])
    assert "(0, 16)" in str(e.value)            # pixel 0, first channel past the 16-channel slice
    pair = _pair(torch.float16, su.ABI_MIN, "write_guard_pixel")
    with pytest.raises(AssertionError) as e:
        su.assert_canary_intact(pair.strided_bufs["y"])
    assert f"({P}, 0)" in str(e.value)
    pair = _pair(torch.float16, su.ABI_MIN, "tile_unwritten")
    with pytest.raises(AssertionError) as e:
        su.assert_fully_written(pair.strided_bufs["y"])
    assert "(0, 0)" in str(e.value)


def test_kernel_change_and_approx_bound_are_flagged():
    names = iter(["a", "b"])
    ops = {"x": su.Operand((B, H, W, C), torch.float16, "in", 1), "y": su.Operand((B, H, W, C), torch.float16, "out"),
           "res": su.Operand((B, H, W, C), torch.float16, "in", 2)}
    pair = su.run_pair(standin, ops, last_kernel=lambda: next(names), set_tuning=lambda k, v: 0, sync=lambda: None)
    with pytest.raises(AssertionError, match="dispatch changed with the stride"):
        su.verify(pair, exact=["y"])
    pair = _pair(torch.float16, su.EXEC_LIKE, None)
    pair.strided["y"][0, 0, 0, 0] += 1.0
    with pytest.raises(AssertionError, match="differ by"):
        su.verify(pair, approx={"y": 1e-5})


def test_statistics_rows_and_accumulators():
    """fp32 rows of (sum, sum of squares) pairs: 32-bit canary, placement in units of two floats, start values kept"""
    buf, view = su.make_slice((2, 4, 1, 2 * 8), torch.float32, 0, left=2 * 8, right=2 * 24, guard=2, role="acc")
    assert float(view.abs().max()) == 0.0 and view.stride(-2) == 2 * 40
    view += 1.0
    su.assert_canary_intact(buf)
    su.flat_of(view)[0][0] = 0.0
    with pytest.raises(AssertionError, match=r"\(-2, -16\)"):
        su.assert_canary_intact(buf)


def test_rows_close_flags_one_bad_row_that_the_norm_hides():
    """one wrong token row of a [2, 257, 384] bf16 output (20 % off) stays under the norm-wise bf16 bound of test_gpu_8_projd_vit.py (TOL = 1.2e-2:
    diluted by sqrt(514 rows)) and is caught by the per-row bound at 4 x that TOL"""
    tol = 1.2e-2
    ref = torch.randn(2, 257, 384, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    got = ref.to(torch.bfloat16)
    assert su.relerr(got, ref) < tol and su.assert_rows_close(got, ref, 4 * tol, "clean")[1] < tol
    got[1, 256] = (1.2 * ref[1, 256]).to(torch.bfloat16)         # the last (clamped tail) row of the last image
    assert su.relerr(got, ref) < tol, su.relerr(got, ref)
    e = su.row_errors(got, ref)
    assert e.shape == (514,) and int(e.argmax()) == 513 and 0.15 < float(e[513]) < 0.25
    with pytest.raises(AssertionError, match=r"1 of 514 rows outside the per-row bound.*\(513, "):
        su.assert_rows_close(got, ref, 4 * tol, "o")
    # relative to the RMS row norm: a row whose true value is tiny does not blow up
    ref[0, 3] *= 1e-6
    small = ref.to(torch.bfloat16)
    assert float(su.row_errors(small, ref)[3]) < 1e-6
    small[0, 5, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"NaN in rows \[5\]"):
        su.assert_rows_close(small, ref, 4 * tol, "o")


def test_shared_placement():
    """share = {name: other}: both operands on ONE stride in the strided launch, every other operand still on its own"""
    ops = {"x": su.Operand((B, H, W, C), torch.float16, "in", 1), "y": su.Operand((B, H, W, C), torch.float16, "out"),
           "res": su.Operand((B, H, W, C), torch.float16, "in", 2)}
    pair = su.run_pair(standin, ops, kind=su.ABI_MIN, share={"res": "x"}, last_kernel=lambda: "standin", set_tuning=lambda k, v: 0, sync=lambda: None)
    su.verify(pair, exact=["y"], kernel="standin")
    assert pair.strided["res"].stride(-2) == pair.strided["x"].stride(-2) != pair.strided["y"].stride(-2)
    assert pair.contig["res"].stride(-2) == C
