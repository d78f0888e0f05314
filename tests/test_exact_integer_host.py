"""CPU side of tests/test_gpu_23_exact_integer.py (no GPU):
  * for every row of tests/kernel_cases.py the integer inputs and the float64 reference are built and preconditions (i) and (ii) of the
    exact comparison asserted -- the GPU tests then never fail on their own inputs;
  * the exact comparison is sharp where the norm-wise bound of the existing tests is blind: a CPU stand-in kernel (F.conv2d in float32 on the
    same operands) with one local defect at a time fails strided_util.assert_bit_equal and passes relerr < TOL[bf16] on the same data;
  * every id of the tables is unique and every instance string test_gpu_17 / 19 / 20 name has a row.
"""
import pytest
import torch
import torch.nn.functional as F

import kernel_cases as kc
import strided_util as su

TOL_BF16 = 8e-3         # the norm-wise bound of test_gpu_0_ops.py / test_gpu_17 / 19 / 20 for bf16
MEASURED = {}           # table -> worst figures, printed by test_report_measured_preconditions


@pytest.mark.parametrize("case", kc.CONV_ROWS_ALL, ids=[c.id for c in kc.CONV_ROWS_ALL])
def test_conv_row_preconditions(case):
    """(i) for fp16 and bf16 and (ii) for the fused statistics, on the reference of the row (both dtypes share the integer problem)"""
    prob = kc.int_conv_problem(case)
    worst_y, worst_stats = kc.check_conv_preconditions(case, prob)
    assert worst_y > 0
    assert float((prob.ref * 2).frac().abs().max()) == 0.0          # a multiple of alpha = 0.5
    m = MEASURED.setdefault("conv", [0.0, "", 0.0, ""])
    if worst_y > m[0]:
        m[0], m[1] = worst_y, case.id
    if worst_stats > m[2]:
        m[2], m[3] = worst_stats, case.id
    print(f"{case.id}: density {prob.p:.3f}, worst |y| {worst_y}, worst statistics sum {worst_stats:.4e} ({worst_stats / kc.TWO24:.2f} of 2^24)")


@pytest.mark.parametrize("case", kc.WG_ROWS_ALL, ids=[c.id for c in kc.WG_ROWS_ALL])
def test_wgrad_row_preconditions(case):
    prob = kc.int_wgrad_problem(case.geo, kc.wgrad_opts(case))
    dw_units, db_units = kc.check_wgrad_preconditions(case.id, prob)
    real = prob.o["real_cout"]
    assert float(prob.dy[..., real:].abs().max() if real < case.geo[4] else 0.0) == 0.0        # padding channels stay zero
    assert float(prob.dy.abs().max()) == 2.0 and float(prob.x.abs().max()) == 1.0
    m = MEASURED.setdefault("wgrad", [0.0, "", 0.0, ""])
    if dw_units > m[0]:
        m[0], m[1] = dw_units, case.id
    if db_units > m[2]:
        m[2], m[3] = db_units, case.id
    print(f"{case.id}: density {prob.p:.3f}, dw <= {dw_units:.4e} units, dbias <= {db_units:.4e} units")


def test_wgrad_group_preconditions():
    for i, geo in enumerate(kc.WG_GROUP_GEOS):
        kc.check_wgrad_preconditions(f"group member {i}", kc.int_wgrad_problem(geo, {}, seed=10 * i))


def test_report_measured_preconditions():
    """the worst figures per table (run after the row tests; -s shows them)"""
    for table, (a, ida, b, idb) in MEASURED.items():
        print(f"{table}: worst {'|y|' if table == 'conv' else 'dw units'} {a} ({ida}); worst {'statistics' if table == 'conv' else 'dbias'} units {b:.4e} ({idb}),"
              f" {b / kc.TWO24:.2f} of 2^24")


def test_ids_unique_and_instances_covered():
    ids = [c.id for c in kc.CONV_ROWS_ALL]
    assert len(set(ids)) == len(ids)
    ids = [c.id for c in kc.WG_ROWS_ALL]
    assert len(set(ids)) == len(ids)
    assert [c.id for c in kc.CONV_ROWS_ALL[:len(kc.CONV_ROWS)]] == [c.id for c in kc.CONV_ROWS]      # test_gpu_17 keeps its old rows
    names = kc.all_instance_names()
    # test_gpu_17: the instance of every row it iterates over, and the two fused streaming launches (test_gpu_23 runs them by name)
    for c in kc.CONV_ROWS + kc.WG_ROWS:
        assert c.inst in names
    # test_gpu_19: NAMES per configuration; test_gpu_20: KERNEL
    for per_cfg in kc.SUBPIXEL_DGRAD_NAMES.values():
        assert set(per_cfg.values()) <= names
    assert kc.SUBPIXEL_WGRAD_KERNEL in names
    import ast
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    for fname, var in (("test_gpu_19_subpixel_dgrad.py", "NAMES"), ("test_gpu_20_subpixel_wgrad.py", "KERNEL")):
        tree = ast.parse(open(os.path.join(here, fname)).read())
        val = [n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == var][0]
        strings = {s.value for s in ast.walk(val) if isinstance(s, ast.Constant) and isinstance(s.value, str)}
        assert strings and strings <= names, (fname, strings - names)
    tree = ast.parse(open(os.path.join(here, "test_gpu_17_strided_operands.py")).read())
    families = {n.split("<")[0].split("+")[0] for n in names}
    named = {s.value for s in ast.walk(tree) if isinstance(s, ast.Constant) and isinstance(s.value, str) and s.value.split("<")[0].split("+")[0] in families
             and ": " not in s.value}        # (docstrings that begin with an instance name)
    named.discard("conv_nt_glds_kernel")          # a prefix test_refused_combinations matches with startswith, not an instance
    assert len(named) >= 4 and named <= names, named - names


# ======================================================================================================================================
# the comparison is sharp: local defects in a CPU stand-in
# ======================================================================================================================================
# forward stand-in: ReflectionPad2d(1) + conv3x3, alpha 0.5, bias, res_scale 2 at (4, 256, 256, 64 -> 8): 262144 pixels, the size of the largest
# rows.  A defect confined to 16 pixels carries 16 / 262144 of the squared norm of what it changes -- a relative error of a few 1e-3.
FWD_GEO = (4, 256, 256, 64, 8)


@pytest.fixture(scope="module")
def fwd():
    B, H, W, Cin, Cout = FWD_GEO
    p = kc.density(9 * Cin)
    x = kc.ternary((B, Cin, H, W), p, 201)
    w = kc.ternary((Cout, Cin, 3, 3), p, 202)
    bias = kc.integers((Cout,), -3, 3, 203)
    res = kc.integers((B, Cout, H, W), -4, 4, 204)
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")

    def finish(acc):
        return (kc.ALPHA * acc + bias.view(1, -1, 1, 1) + kc.RES_SCALE * res).to(torch.bfloat16)

    acc = F.conv2d(xp, w)                                   # the stand-in kernel: float32, exact on these operands
    ref = (kc.ALPHA * F.conv2d(xp.double(), w.double()) + bias.double().view(1, -1, 1, 1) + kc.RES_SCALE * res.double())
    assert kc.representable(ref, torch.bfloat16) and kc.representable(ref, torch.float16)
    return dict(x=x, xp=xp, w=w, acc=acc, ref=ref, finish=finish)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _blind_but_caught(got, ref, what):
    e = su.relerr(got, ref)
    print(f"{what}: norm-wise relative error {e:.3e} (bound {TOL_BF16:.1e})")
    assert 0 < e < TOL_BF16, f"{what}: the norm-wise check was expected to pass, {e:.3e}"
    with pytest.raises(AssertionError, match="differ from the exact reference"):
        su.assert_bit_equal(_nhwc(got), _nhwc(ref), what)


def test_correct_standin_is_exact(fwd):
    su.assert_bit_equal(_nhwc(fwd["finish"](fwd["acc"])), _nhwc(fwd["ref"]), "stand-in")


def test_tap_dropped_on_the_last_row_of_a_tile(fwd):
    """tap (r, s) = (0, 1) is zeroed on the last output row only, in one 16-pixel tile row"""
    H = FWD_GEO[1]
    w0 = fwd["w"].clone()
    w0[:, :, 0, 1] = 0
    acc = fwd["acc"].clone()
    acc[1:2, :, H - 1:H, 32:48] = F.conv2d(fwd["xp"][1:2, :, H - 1:H + 2, 32:50], w0)
    _blind_but_caught(fwd["finish"](acc), fwd["ref"], "one tap dropped on the last output row")


def test_halo_column_mirrored_from_the_wrong_side(fwd):
    """the right halo column of one 16-row tile (input column W, tap w + 1 of output column W - 1) holds column W - 1 instead of the mirrored
    column W - 2"""
    B, H, W, Cin, Cout = FWD_GEO
    xp = fwd["xp"][2:3, :, 64:64 + 18, W - 2:].clone()           # padded rows of output rows 64 .. 79, padded columns W - 2 .. W + 1
    xp[..., -1] = xp[..., -2]
    acc = fwd["acc"].clone()
    acc[2:3, :, 64:80, W - 2:] = F.conv2d(xp, fwd["w"])
    assert not torch.equal(acc, fwd["acc"])
    _blind_but_caught(fwd["finish"](acc), fwd["ref"], "one halo column mirrored from the wrong column")


def test_k_chunk_skipped_for_one_tile(fwd):
    """one K-step of 32 channels (tap (1, 1), channels 32 .. 63 of K = R S Cin) is skipped for one 16 x 16 output tile"""
    acc = fwd["acc"].clone()
    part = F.conv2d(fwd["x"][0:1, 32:64, 16:32, 48:64], fwd["w"][:, 32:64, 1:2, 1:2])
    acc[0:1, :, 16:32, 48:64] -= part
    _blind_but_caught(fwd["finish"](acc), fwd["ref"], "one 32-channel K-step skipped for one tile")


def test_dw_element_accumulated_twice():
    """one element of dw receives its gradient twice (two split-K slices overlapping by one K-step, seen from one element)"""
    case = [c for c in kc.WG_ROWS if c.id == "halo-cfg1"][0]
    prob = kc.int_wgrad_problem(case.geo, kc.wgrad_opts(case))
    ref, _ = kc.int_wgrad_reference(prob, case.geo)
    x32, dy32 = prob.x.permute(0, 3, 1, 2), prob.dy.permute(0, 3, 1, 2)
    wr = torch.zeros(case.geo[4], case.geo[3], 3, 3, requires_grad=True)
    F.conv2d(x32, wr, None, 1, 1).backward(dy32)                 # the stand-in kernel: float32
    g = kc.ALPHA * wr.grad.permute(0, 2, 3, 1).reshape(ref.shape)
    got = prob.dw0 + g
    assert torch.equal(got.double(), ref)
    su.assert_bit_equal(got, ref, "stand-in dw")
    rms = float(g.double().pow(2).mean().sqrt())
    i, j = [(i, j) for i, j in (g.abs() >= rms).nonzero()[:1].tolist()][0]
    bad = got.clone()
    bad[i, j] += g[i, j]
    e = su.relerr(bad, ref)
    print(f"dw element ({i}, {j}) accumulated twice: norm-wise relative error {e:.3e} (bound {TOL_BF16:.1e})")
    assert 0 < e < TOL_BF16
    with pytest.raises(AssertionError, match="1 of"):
        su.assert_bit_equal(bad, ref, "dw")
