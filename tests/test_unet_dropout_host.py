"""Host tests of G_dropout in the diffusion UNet (no device): the out_layers[2] placeholders keep the reference's state_dict keys, every one has
a Philox stream of its own and the path the reference gives the module, and the invocation counter of a placeholder advances once per
training-mode forward and returns to 0 with DropoutState.begin_step."""
import pytest
import torch

from joligen_amd.modules.dropout import DropoutState, FusedDropout, bind_dropout
from joligen_amd.modules.unet_generator_attn import ResBlock, UNet

KW = dict(image_size=32, in_channel=6, inner_channel=32, out_channel=3, res_blocks=[1, 1], attn_res=[16], tanh=False, n_timestep_train=2000,
          n_timestep_test=1000, norm="groupnorm32", group_norm_size=32, cond_embed_dim=64, channel_mults=(1, 2), efficient=True)


def test_state_dict_keys_do_not_depend_on_dropout():
    a, b = UNet(dropout=0.25, **KW), UNet(dropout=0, **KW)
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]
    for rb in a._res_blocks:
        assert isinstance(rb.out_layers[2], FusedDropout) and not list(rb.out_layers[2].parameters())


def test_streams_are_unique_and_paths_are_the_module_names():
    net = UNet(dropout=0.25, **KW)
    drops = {name: m for name, m in net.named_modules() if isinstance(m, FusedDropout)}
    assert len(drops) == len(net._res_blocks) == 10
    assert sorted(m.stream for m in drops.values()) == list(range(len(drops)))
    assert all(m.path == name and m.state is net.dropout_state for name, m in drops.items())
    # the rate reaches the middle block only, as in the reference's UNet (its input and output blocks are built with a dropout of 0)
    assert sorted(name for name, m in drops.items() if m.p) == ["middle_block.0.out_layers.2", "middle_block.2.out_layers.2"]
    # the owner of the network binds again under its own prefix: same streams, the reference's full module names
    assert bind_dropout(net, net.dropout_state, "denoise_fn.model.") == len(drops)
    assert drops["input_blocks.1.0.out_layers.2"].path == "denoise_fn.model.input_blocks.1.0.out_layers.2"
    assert sorted(m.stream for m in drops.values()) == list(range(len(drops)))


def test_call_counting_and_begin_step():
    net = UNet(dropout=0.25, **KW)
    st = net.dropout_state
    asked = []
    st.rand = lambda path, call, shape, device: asked.append((path, call, shape)) or torch.zeros(shape)
    rb = net.middle_block[0]
    assert isinstance(rb, ResBlock) and rb.drop_live()
    shape = (2, 8, 8, rb.out_channel)
    a0, a1 = rb.drop_args(shape, "cpu"), rb.drop_args(shape, "cpu")
    assert (a0["call"], a1["call"]) == (0, 1) and a0["stream"] == a1["stream"] == rb.out_layers[2].stream and a0["keep"] == 0.75
    assert asked == [("middle_block.0.out_layers.2", 0, (2, rb.out_channel, 8, 8)), ("middle_block.0.out_layers.2", 1, (2, rb.out_channel, 8, 8))]
    assert tuple(a0["u"].shape) == (2, rb.out_channel, 8, 8) and a0["key"] is None
    # the fused schedule names the call of its node; the counter moves past it
    assert rb.drop_args(shape, "cpu", call=5)["call"] == 5 and rb.drop_args(shape, "cpu")["call"] == 6
    other = net.middle_block[2]
    assert other.drop_args(shape, "cpu")["call"] == 0                      # a counter per placeholder
    st.begin_step()
    assert rb.drop_args(shape, "cpu")["call"] == 0 and other.drop_args(shape, "cpu")["call"] == 0
    # the key is replaced, never written in place
    k1, k2 = torch.tensor([1, 2], dtype=torch.int32), torch.tensor([3, 4], dtype=torch.int32)
    st.rand = None
    st.begin_step(k1)
    got = rb.drop_args(shape, "cpu")
    assert got["key"] is k1 and got["u"] is None and got["call"] == 0
    st.begin_step(k2)
    assert rb.drop_args(shape, "cpu")["key"] is k2 and torch.equal(k1, torch.tensor([1, 2], dtype=torch.int32))
    # eval(): the identity, nothing is invoked
    net.eval()
    assert not rb.drop_live()
    # the rate is read where it stands: a block whose rate was set from outside
    net.train()
    blk = net.input_blocks[1][0]
    assert not blk.drop_live()
    blk.dropout = 0.5
    assert blk.drop_live() and blk.drop_args((2, 8, 8, blk.out_channel), "cpu")["keep"] == 0.5


def test_a_block_outside_a_network_gets_a_state_of_its_own():
    rb = ResBlock(32, 64, 0.25, "groupnorm32", use_scale_shift_norm=True)
    assert rb.out_layers[2].state is None
    st = DropoutState()
    st.rand = lambda path, call, shape, device: torch.zeros(shape)
    bind_dropout(rb, st)
    assert rb.drop_args((1, 4, 4, 32), "cpu")["call"] == 0 and rb.out_layers[2].path == "out_layers.2"


# ---- the oracle with the reference's masks against the fixture recorded from the unmodified reference ------------------------------------------
import os  # noqa: E402

import jg_oracle as O  # noqa: E402
import unet_dropout_oracle as UO  # noqa: E402

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_dropout")


def _step_fixture(golden_dir):
    g = torch.load(os.path.join(DIR, "palette_step_tiny_eff.pt"), weights_only=False)
    sched = torch.load(os.path.join(golden_dir, "schedule.pt"), weights_only=False)
    ref_sd = {k: (sched[k.split(".")[-1]] if O._is_buffer(k) else torch.empty(g["shapes"][k])) for k in g["keys"]}
    return O.synth_state_dict(ref_sd, seed=0), g


def test_fixture_is_small_and_names_the_placeholders():
    assert os.path.getsize(os.path.join(DIR, "palette_step_tiny_eff.pt")) < 400_000
    g = torch.load(os.path.join(DIR, "palette_step_tiny_eff.pt"), weights_only=False)
    c = g["cfg"]
    net = UNet(image_size=c["S"], in_channel=6, inner_channel=c["ngf"], out_channel=3, res_blocks=c["res_blocks"], attn_res=c["attn_res"], tanh=False,
               n_timestep_train=2000, n_timestep_test=1000, norm="groupnorm32", group_norm_size=32, cond_embed_dim=32, channel_mults=c["mults"],
               efficient=c["efficient"], dropout=g["hp"]["G_dropout"])
    bind_dropout(net, net.dropout_state, "denoise_fn.model.")
    mine = sorted(m.path for m in net.modules() if isinstance(m, FusedDropout) and m.p)
    assert mine == sorted(g["live"])                                   # the modules the reference gives the rate to, by the reference's names
    for s in g["steps"]:
        assert sorted((p, k) for p, k, _, _ in s["dropout"]) == [(p, 0) for p in mine]      # one invocation per placeholder and step
        for _, _, shape, bits in s["dropout"]:
            frac = float(UO.unpack(bits, shape).float().mean())
            n = shape[0] * shape[1] * shape[2] * shape[3]
            assert abs(frac - 0.75) < 5 * (0.75 * 0.25 / n) ** 0.5, frac


def test_oracle_with_the_recorded_masks_reproduces_the_palette_step_fixture(golden_dir):
    """the bounds of tests/test_oracle_golden.py::test_palette_three_steps, the same quantities without dropout"""
    from test_oracle_golden import cfg_of

    sd, g = _step_fixture(golden_dir)
    hp, keep = g["hp"], 1.0 - g["hp"]["G_dropout"]
    mk = lambda: O.OraclePaletteTrainer(sd, cfg_of(g["cfg"]), lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"],
                                        weight_decay=hp["weight_decay"], ema_beta=hp["ema_beta"], lambda_G=hp["lambda_G"], optim=hp["optim"])
    tr = mk()
    s0 = g["steps"][0]
    plain = mk().optimize_parameters(s0["B"], s0["A"], s0["mask"], s0["noise"], s0["t"], s0["u"])
    assert abs(float(plain) - float(s0["loss"])) > 1e-3 * abs(float(s0["loss"]))          # the masks matter
    for s in g["steps"]:
        table = UO.table_of(s)
        with UO.recorded_masks(table, keep) as used:
            loss = tr.optimize_parameters(s["B"], s["A"], s["mask"], s["noise"], s["t"], s["u"])
        assert used == set(table)                                                          # every recorded invocation, exactly once
        torch.testing.assert_close(loss, s["loss"], rtol=2e-4, atol=1e-6)
        if "param_checks" in s:
            for kind, P in (("param_checks", tr.P), ("ema_checks", tr.ema)):
                for k, ref in s[kind].items():
                    v = P[k]
                    mine = torch.stack([v.norm(), (v * O.projection_vector(k, v.shape)).sum()])
                    torch.testing.assert_close(mine, ref, rtol=1e-4, atol=1e-4 * float(ref[0]) + 1e-6, msg=k)
    for k, ref in g["param_sample"].items():
        torch.testing.assert_close(tr.P[k].flatten()[:8], ref, rtol=1e-3, atol=2e-5, msg=k)


def test_oracle_with_the_recorded_masks_reproduces_the_cm_step_fixture():
    """the bounds of tests/test_oracle_golden.py::test_cm_three_steps; student and teacher are invocations 0 and 1 of every placeholder"""
    from test_oracle_golden import cm_cfg_of

    g = torch.load(os.path.join(DIR, "cm_step_tiny_eff.pt"), weights_only=False)
    assert os.path.getsize(os.path.join(DIR, "cm_step_tiny_eff.pt")) < 400_000
    sd = O.synth_state_dict({k: torch.empty(g["shapes"][k]) for k in g["keys"]}, seed=0)
    hp, keep = g["hp"], 1.0 - g["hp"]["G_dropout"]
    tr = O.OracleCMTrainer(sd, cm_cfg_of(g["cfg"]), g["total_t"], lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"],
                           weight_decay=hp["weight_decay"], ema_beta=hp["ema_beta"] if hp["ema"] else None, lambda_G=hp["lambda_G"], optim=hp["optim"])
    for s in g["steps"]:
        table = UO.table_of(s)
        assert sorted(table) == sorted((p, k) for p in g["live"] for k in (0, 1))
        with UO.recorded_masks(table, keep) as used:
            loss = tr.optimize_parameters(s["B"], s["mask"], s["noise"], s["timesteps"])
        assert used == set(table)
        torch.testing.assert_close(loss, s["loss"], rtol=2e-4, atol=1e-6)
        if "param_checks" in s:
            for kind, P in (("param_checks", tr.P), ("ema_checks", tr.ema)):
                if P is None:
                    continue
                for k, ref in s[kind].items():
                    v = P[k]
                    mine = torch.stack([v.norm(), (v * O.projection_vector(k, v.shape)).sum()])
                    torch.testing.assert_close(mine, ref, rtol=1e-4, atol=1e-4 * float(ref[0]) + 1e-6, msg=k)


RESBLOCKS = ["plain", "down", "up_eff", "up_noeff"]


@pytest.mark.parametrize("name", RESBLOCKS)
def test_oracle_with_the_recorded_mask_reproduces_the_resblock_fixture(name):
    """one ResBlock of the unmodified reference with dropout 0.25 (plain with the 1x1 skip, down, efficient up, plain up): output, input and
    embedding gradients and every parameter-gradient checksum, at the bounds of tests/test_oracle_golden.py::test_unet_forward_backward"""
    g = torch.load(os.path.join(DIR, f"resblock_{name}.pt"), weights_only=False)
    assert os.path.getsize(os.path.join(DIR, f"resblock_{name}.pt")) < 200_000
    c = g["cfg"]
    sd = O.synth_state_dict({k: torch.empty(g["shapes"][k]) for k in g["keys"]}, seed=g["seed"])
    P = {"rb." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    cfg = O.UNetCfg(efficient=c["efficient"], cond_embed_dim=c["emb_channels"])
    d = dict(up=c["up"], down=c["down"], cin=c["channels"], cout=c["out_channel"])
    table = {("rb." + p, k): UO.unpack(bits, shape) for p, k, shape, bits in g["dropout"]}
    x, emb = g["x"].clone().requires_grad_(True), g["emb"].clone().requires_grad_(True)
    with UO.recorded_masks(table, 1.0 - c["p"]) as used:
        out = O.resblock(P, "rb", x, emb, cfg, d)
        plain = None
    assert used == set(table) == {("rb.out_layers.2", 0)}
    with torch.no_grad():
        plain = O.resblock(P, "rb", x, emb, cfg, d)
    assert float((plain - g["out"]).norm() / g["out"].norm()) > 0.05          # the mask matters
    torch.testing.assert_close(out, g["out"], rtol=1e-4, atol=1e-5)
    (out * g["R"]).sum().backward()
    torch.testing.assert_close(x.grad, g["dx"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(emb.grad, g["demb"], rtol=1e-4, atol=1e-3)
    for k, ref in g["grad_checks"].items():
        v = P["rb." + k].grad
        mine = torch.stack([v.norm(), (v * O.projection_vector(k, v.shape)).sum()])
        torch.testing.assert_close(mine, ref, rtol=2e-4, atol=2e-4 * float(ref[0]) + 1e-6, msg=k)
