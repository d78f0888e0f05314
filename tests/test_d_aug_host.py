"""Host-side tests of dataaug_D_noise / adaptive pseudo augmentation (APA) of the CUT model: the numpy restatement of the generator and the two
kernels (tests/d_aug_ref.py) against the Random123 known answers, its statistics, the fixtures recorded from the unmodified reference
(tests/tools/make_fixture_d_aug.py -> tests/golden/d_aug/), the option checks and the draw order on the pool's host RNG."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import d_aug_ref as R
import ref_shim
from test_oracle_golden import ReplayRandom

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "d_aug")
STEP_FIXTURES = ["noise", "apa", "noise_apa"]
FILES = [f"cutstep_{n}.pt" for n in STEP_FIXTURES] + ["apa_fn.pt"]
N_SHAPE = (4, 3, 256, 256)          # N = 4 * 3 * 256 * 256 draws for the statistics
KEY = (0x1234ABCD, 0x0F1E2D3C)


def _load(name):
    return torch.load(os.path.join(DIR, name), weights_only=False)


def test_philox4x32_10_known_answers():
    """the three known-answer vectors of Random123 (kat_vectors: philox4x32 10)"""
    pi = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                               ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                               (pi, (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = tuple(int(v) for v in R.philox4x32_10(counter, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    many = R.philox4x32_10((np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF])), (0, 0))
    assert int(many[0][0]) == 0x6627E8D5 and many[0].dtype == np.uint32            # vectorised over counters


def test_uniform_mapping_is_open_and_exact_in_fp32():
    x = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    u = R.uniform_open(x)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24 and bool((np.float32(u).astype(np.float64) == u).all())
    assert np.isfinite(np.log(np.float32(u))).all()


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def normal_statistics(z, z_other_stream):
    """(statistic, value, bound) of an [B, C, H, W] sample: all bounds are five standard errors of an iid N(0, 1) sample of its size"""
    n = z.size
    m, v = float(z.mean()), float(z.var())
    kurt = float(((z - m) ** 4).mean() / v ** 2 - 3.0)
    return [("mean", abs(m), 5 / np.sqrt(n)), ("variance", abs(v - 1), 5 * np.sqrt(2 / n)), ("excess kurtosis", abs(kurt), 5 * np.sqrt(24 / n)),
            ("neighbouring pixels (w)", abs(_corr(z[..., :-1], z[..., 1:])), 5 / np.sqrt(z[..., 1:].size)),
            ("neighbouring pixels (h)", abs(_corr(z[:, :, :-1], z[:, :, 1:])), 5 / np.sqrt(z[:, :, 1:].size)),
            ("channels 0 / 1", abs(_corr(z[:, 0], z[:, 1])), 5 / np.sqrt(z[:, 0].size)),
            ("channels 1 / 2", abs(_corr(z[:, 1], z[:, 2])), 5 / np.sqrt(z[:, 1].size)),
            ("channels 0 / 2", abs(_corr(z[:, 0], z[:, 2])), 5 / np.sqrt(z[:, 0].size)),
            ("samples", abs(_corr(z[:-1], z[1:])), 5 / np.sqrt(z[1:].size)),
            ("stream ids", abs(_corr(z, z_other_stream)), 5 / np.sqrt(n))]


def test_restatement_normals_statistics():
    B, C, H, W = N_SHAPE
    z = R.normals(KEY, B, C, H, W, stream=0, call=0)
    z2 = R.normals(KEY, B, C, H, W, stream=1, call=0)
    assert z.shape == N_SHAPE and np.isfinite(z).all()
    for what, val, bound in normal_statistics(z, z2):
        print(f"{what}: {val:.3e} (bound {bound:.3e})")
        assert val <= bound, (what, val, bound)
    assert not np.array_equal(z, R.normals(KEY, B, C, H, W, stream=0, call=1))            # another call site: other draws
    assert np.array_equal(z[:1, :, :4, :4], R.normals(KEY, 1, C, 256, 256)[:, :, :4, :4])  # counter-based: a sub-block needs no state


@pytest.mark.parametrize("p", [0.05, 0.5, 0.484, 0.9])
def test_restatement_flag_rate(p):
    n = 1 << 16
    u = R.flag_uniforms(KEY, n, stream=1, call=1)
    rate = float((np.float32(u) < np.float32(p)).mean())
    assert abs(rate - p) <= 5 * np.sqrt(p * (1 - p) / n), (rate, p)
    assert not np.array_equal(u, R.flag_uniforms(KEY, n, stream=2, call=1))


def test_restatement_d_aug_is_the_reference_blend():
    """apa_fn.pt: the reference's adaptive_pseudo_augmentation (fake * flag + real * (1 - flag)) on recorded uniforms is the select"""
    for s in _load("apa_fn.pt")["selects"]:
        nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
        out, flags = R.d_aug(nhwc(s["real"]), 3, alt=nhwc(s["fake"]), u=s["u"].numpy(), p=s["p"])
        assert np.array_equal(out, nhwc(s["out"]).astype(np.float64)), s["p"]
        assert flags.tolist() == (s["u"] < s["p"]).int().tolist()
    assert [s["p"] for s in _load("apa_fn.pt")["selects"]] == [0.5, 0.0, 1.0, 0.3]


def test_restatement_apa_update_equals_the_reference_bit_for_bit():
    ups = _load("apa_fn.pt")["updates"]
    seen = set()
    for c in ups:
        p, adjust, s = R.apa_update(c["pred"].numpy(), c["p0"], c["target"], c["B"] * c["every"], c["nimg"] * 1000)
        for mine, ref in ((p, c["p"]), (adjust, c["adjust"]), (s, c["s"])):
            assert np.float32(mine).tobytes() == ref.numpy().astype(np.float32).tobytes(), (c["layout"], c["p0"], float(mine), float(ref))
        seen.add((c["layout"], float(c["adjust"]), float(c["p"]) in (0.0, 1.0)))
    assert {l for l, _, _ in seen} == {"map", "flat"} and any(a == 0.0 for _, a, _ in seen)
    assert any(float(c["p"]) == 0.0 and c["p0"] > 0 for c in ups) and any(float(c["p"]) == 1.0 and c["p0"] < 1 for c in ups)      # both clamps


def _opt(over=None, **cut):
    from joligen_amd.options import opt_from_json

    return opt_from_json({"model_type": "cut", "alg": {"cut": cut}}, dict({"gpu_ids": "0"}, **(over or {})))


def test_d_aug_option_checks():
    from joligen_amd.models.cm_gan_model import check_cm_gan_options
    from joligen_amd.models.cut_model import CUT_DEFAULTS, check_d_aug_options, cut_loss_names
    from joligen_amd.modules.loss import DiscriminatorGANLoss

    for k, v in dict(dataaug_D_noise=0.0, dataaug_APA=False, dataaug_APA_target=0.6, dataaug_APA_p=0.0, dataaug_APA_every=4, dataaug_APA_nimg=50).items():
        assert CUT_DEFAULTS[k] == v, k                                       # options/train_options.py
    o = _opt()
    assert o.dataaug_APA_target == 0.6 and o.dataaug_APA_every == 4 and o.dataaug_APA_nimg == 50 and o.dataaug_APA_p == 0.0
    assert check_d_aug_options(o) == (0.0, False) and o.dataaug_APA is False and o.dataaug_D_noise == 0.0
    assert check_d_aug_options(_opt({"dataaug_D_noise": 0.1, "dataaug_APA": True, "D_netDs": ["basic"]})) == (0.1, True)
    assert check_d_aug_options(SimpleNamespace(D_netDs=["basic"])) == (0.0, False)
    with pytest.raises(ValueError, match="dataaug_D_noise"):
        check_d_aug_options(_opt({"dataaug_D_noise": -0.1}))
    with pytest.raises(ValueError, match="train_pool_size"):
        check_d_aug_options(_opt({"dataaug_APA": True, "train_pool_size": 0, "D_netDs": ["basic"]}))
    for bad in ({"dataaug_APA_p": 1.5}, {"dataaug_APA_every": 0}, {"dataaug_APA_nimg": 0}):
        with pytest.raises(ValueError, match="dataaug_APA"):
            check_d_aug_options(_opt(dict({"dataaug_APA": True, "D_netDs": ["basic"]}, **bad)))
    # the loss names do not change with either option
    assert cut_loss_names(_opt({"dataaug_D_noise": 0.1, "dataaug_APA": True}), ["D_B_basic"]) == ["G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic"]
    # cm_gan keeps refusing both; D-diffusion stays refused by the loss calculator
    with pytest.raises(NotImplementedError, match="dataaug_APA"):
        check_cm_gan_options(SimpleNamespace(dataaug_APA=True))
    with pytest.raises(NotImplementedError, match="dataaug_D_noise"):
        check_cm_gan_options(SimpleNamespace(dataaug_D_noise=0.1))
    with pytest.raises(NotImplementedError, match="diffusion"):
        DiscriminatorGANLoss(None, torch.device("cpu"), dataaug_D_diffusion=True)
    off = DiscriminatorGANLoss(None, torch.device("cpu"))
    assert off.adaptive_pseudo_augmentation_p == 0.0 and off.adjust == 0 and off.apa_state is None
    off.update(4)                                                            # APA off: nothing to launch
    on = DiscriminatorGANLoss(None, torch.device("cpu"), dataaug_APA=True, dataaug_APA_p=0.5)
    assert float(on.adaptive_pseudo_augmentation_p) == 0.5 and float(on.adjust) == 0.0 and on.apa_state.dtype == torch.float32


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_step_fixture_layout(name):
    assert os.path.getsize(os.path.join(DIR, f"cutstep_{name}.pt")) < 1 << 20
    g = _load(f"cutstep_{name}.pt")
    c, hp = g["cfg"], g["hp"]
    noise, apa = "noise" in name, "apa" in name
    assert (c["B"], c["pool"], c["iters"], c["nce_loss"]) == (2, 2, 4, "patchnce") and len(g["steps"]) == 4
    assert hp["dataaug_D_noise"] == (0.1 if noise else 0.0) and hp["dataaug_APA"] is apa
    assert g["loss_names"] == ["G_tot", "G_NCE", "G_NCE_Y", "G_GAN_D_B_basic", "D_tot", "D_GAN_D_B_basic"]
    if apa:
        assert (hp["dataaug_APA_p"], hp["dataaug_APA_every"], hp["dataaug_APA_nimg"], hp["dataaug_APA_target"]) == (0.5, 2, 1, 0.6)
    p = np.float32(0.5)
    for s in g["steps"]:
        d = s["d_aug"]
        assert len(d["noise"]) == (2 if noise else 0) and all(tuple(n.shape) == (2, 3, 32, 32) for n in d["noise"])
        assert len(d["u"]) == (1 if apa else 0)
        if not apa:
            continue
        assert d["flags"][0].tolist() == (d["u"][0] < float(p)).int().tolist() and abs(d["p_before"][0] - float(p)) < 1e-7
        assert abs(float(d["s"][0]) - hp["dataaug_APA_target"]) >= 0.05                      # the generation-time condition
        # the restatement on the recorded s: the trajectory of p, bit for bit
        p, adjust, _ = R.apa_update(np.full(1, float(d["s"][0]) - hp["dataaug_APA_target"]), p, 0.0, c["B"] * hp["dataaug_APA_every"], hp["dataaug_APA_nimg"] * 1000)
        assert np.float32(p).tobytes() == d["p"][0].numpy().tobytes() and float(adjust) == float(d["adjust"][0])
        assert d["APA_prob"] == {"APA_p": float(d["p"][0]), "APA_adjust": float(d["adjust"][0])}
    if apa:
        assert any(f for s in g["steps"] for f in s["d_aug"]["flags"][0].tolist()) and not all(f for s in g["steps"] for f in s["d_aug"]["flags"][0].tolist())


class _Rec:
    """a recording stand-in for the `random` module of the pools that replays a fixture's draws"""

    def __init__(self, log):
        self.replay, self.kinds = ReplayRandom(log), []

    def uniform(self, a, b):
        self.kinds.append("uniform")
        return self.replay.uniform(a, b)

    def randint(self, a, b):
        self.kinds.append("randint")
        return self.replay.randint(a, b)


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_pool_draw_order_equals_the_reference(name):
    """forward's two metric pools, then per discriminator `query` followed (APA) by `get_random`: the port's pools on the recorded draws
    consume the fixture's `pool_draws` exactly -- kinds in order and nothing left over -- in every step"""
    from joligen_amd.util.image_pool import ImagePool

    g = _load(f"cutstep_{name}.pt")
    B, apa = g["cfg"]["B"], g["hp"]["dataaug_APA"]
    pools = [ImagePool(g["cfg"]["pool"]) for _ in range(3)]          # real_A, real_B, fake_B
    for s in g["steps"]:
        rng = _Rec(s["pool_draws"])
        for p in pools:
            p.rng = rng
        imgs = torch.zeros(B, 1, 1, 8)
        pools[0].store(imgs)
        pools[1].store(imgs)
        pools[2].query(imgs)
        if apa:
            assert pools[2].get_random(B).shape[0] == B
        assert rng.replay.i == len(s["pool_draws"]) and rng.kinds == [k for k, _ in s["pool_draws"]]
        if apa:
            assert rng.kinds[-B:] == ["randint"] * B


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "models")),
                    reason="the reference tree is only present in the build container")
def test_d_aug_fixtures_regenerate(tmp_path):
    """the fixtures are outputs of the unmodified reference: the recipe writes them again, bit for bit"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(HERE, "tools", "make_fixture_d_aug.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    assert sorted(os.listdir(tmp_path)) == sorted(FILES) == sorted(os.listdir(DIR))
    for f in FILES:
        assert open(os.path.join(tmp_path, f), "rb").read() == open(os.path.join(DIR, f), "rb").read(), f
