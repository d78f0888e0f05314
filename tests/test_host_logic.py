"""CPU: host-side logic that needs no GPU -- the C ABI library loads and exports every symbol
include/jg355.h declares, module trees reproduce the reference's state_dict keys/shapes, the flat
parameter arena's views/layout, options flattening, checkpoint hooks."""
import os
import re
import subprocess

import pytest
import torch

import jg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/jg355.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jg355.h")).read(), flags=re.S)


def _declared(hdr):
    """what the header declares, found WITHOUT the parser of joligen_amd._lib: function names, {struct: field names}, constant names"""
    funcs = sorted(set(re.findall(r"\b(jg_[a-z0-9_]+)\s*\(", hdr)) - {"jg_stream_t"})
    structs = {name: re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body)
               for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", hdr, flags=re.S)}
    return funcs, structs, sorted(set(re.findall(r"\bJG_[A-Z0-9_]+\b", hdr)))


@pytest.fixture(scope="module")
def compiler_view(tmp_path_factory):
    """What g++ makes of include/jg355.h: per function the result code + one code per parameter (from decltype(&jg_x): nothing is
    linked), sizeof and every field offset of every struct, the value of every JG_* constant."""
    funcs, structs, consts = _declared(_header())
    lines = ['#include <cstdio>\n#include <cstddef>\n#include "jg355.h"\n'
             'template <class T> struct code { static_assert(sizeof(T) == 0, "type outside the ABI"); };\n'
             "template <class T> struct code<T*> { static constexpr char v = 'p'; };\n"]
    lines += [f"template <> struct code<{t}> {{ static constexpr char v = '{c}'; }};\n"
              for t, c in (("const char*", "s"), ("int32_t", "i"), ("int64_t", "l"), ("uint32_t", "u"), ("uint64_t", "U"), ("float", "f"))]
    lines += ['template <class R, class... A> void sig(const char* name, R (*)(A...)) {\n  printf("F %s %c ", name, code<R>::v);\n'
              '  (putchar(code<A>::v), ...);\n  putchar(\'\\n\');\n}\nint main() {\n']
    lines += [f'  sig("{n}", (decltype(&{n}))nullptr);\n' for n in funcs]
    for st, fields in structs.items():
        lines.append(f'  printf("S {st} %zu\\n", sizeof({st}));\n')
        lines += [f'  printf("O {st}.{f} %zu\\n", offsetof({st}, {f}));\n' for f in fields]
    lines += [f'  printf("C {c} %lld\\n", (long long){c});\n' for c in consts]
    d = tmp_path_factory.mktemp("abi")
    (d / "abi.cpp").write_text("".join(lines) + "  return 0;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(d / "abi.cpp"), "-o", str(d / "abi")], check=True)
    view = {"F": {}, "S": {}, "O": {}, "C": {}}
    for kind, name, *rest in (ln.split() for ln in subprocess.run([str(d / "abi")], check=True, capture_output=True, text=True).stdout.splitlines()):
        view[kind][name] = (rest[0], rest[1] if len(rest) > 1 else "") if kind == "F" else int(rest[0])
    return view


def test_c_abi_exports_every_declared_symbol(compiler_view):
    """every declared entry point is bound with the argument and result types the compiler sees, and the library exports it"""
    import ctypes as C

    from joligen_amd import _lib

    path = _lib.build()
    declared = set(_declared(_header())[0])
    assert declared == set(_lib.SIGNATURES) == set(_lib.RESTYPES) == set(compiler_view["F"]), declared ^ set(_lib.SIGNATURES)
    codes = {C.c_int32: "i", C.c_int64: "l", C.c_uint32: "u", C.c_uint64: "U", C.c_float: "f", C.c_char_p: "s", C.c_void_p: "p"}

    def code(t):
        return "p" if issubclass(t, C._Pointer) else codes[t]

    mine = {n: (code(_lib.RESTYPES[n]), "".join(code(t) for t in _lib.SIGNATURES[n])) for n in _lib.SIGNATURES}
    assert mine == compiler_view["F"], {n: (mine[n], compiler_view["F"][n]) for n in mine if mine[n] != compiler_view["F"][n]}
    assert _lib.SIGNATURES["jg_conv2d_nt"][1] is C.POINTER(_lib.ConvArgs) and _lib.SIGNATURES["jg_conv2d_wgrad_tn"][1] is C.POINTER(_lib.WgradArgs)
    nm = subprocess.run(["nm", "-D", path], check=True, capture_output=True, text=True).stdout
    for name in declared:
        assert f" T {name}" in nm, name
    L = _lib.lib()  # dlopen + argtypes; no compute call (no GPU here)
    assert all(getattr(L, n).argtypes == _lib.SIGNATURES[n] and getattr(L, n).restype is _lib.RESTYPES[n] for n in declared)
    assert L.jg_version() >= 100
    assert b"bad argument" in L.jg_strerror(-1)


def test_struct_layout_matches_header(compiler_view):
    """ctypes mirrors of jg_conv_args / jg_wgrad_args (and every other struct of the header): field order as in the header, and the size
    and the offset of EVERY field equal to what a C++ compiler makes of include/jg355.h (g++)."""
    import ctypes as C

    from joligen_amd import _lib

    structs = _declared(_header())[1]
    assert set(structs) == set(_lib.STRUCTS) == set(compiler_view["S"]) and {"jg_conv_args", "jg_wgrad_args"} <= set(structs)
    assert _lib.ConvArgs is _lib.STRUCTS["jg_conv_args"] and _lib.WgradArgs is _lib.STRUCTS["jg_wgrad_args"]
    assert (len(structs["jg_conv_args"]), len(structs["jg_wgrad_args"])) == (47, 34)
    for st, names in structs.items():
        cls = _lib.STRUCTS[st]
        assert names == [f[0] for f in cls._fields_], (st, names)
        assert C.sizeof(cls) == compiler_view["S"][st], st
        mine = {f"{st}.{n}": getattr(cls, n).offset for n in names}
        theirs = {k: v for k, v in compiler_view["O"].items() if k.startswith(st + ".")}
        assert mine == theirs, (st, mine, theirs)


def test_constants_come_from_the_header(compiler_view):
    """every JG_* enum / #define value as the compiler sees it, and the Python names that size a workspace or refuse a shape by them"""
    from joligen_amd import _lib, ops, resize_aa

    assert _lib.CONSTANTS == compiler_view["C"]
    assert all(getattr(_lib, n) == v for n, v in compiler_view["C"].items())
    c = compiler_view["C"]
    assert ops._ECT_MAX_BLOCKS == c["JG_ECT_MAX_BLOCKS"] == 64 and ops._PIXEL_MAX_BLOCKS == c["JG_PIXEL_MAX_BLOCKS"] == 256
    assert resize_aa.MAX_TAPS == c["JG_LOWRES_MAX_TAPS"] == 65
    assert ops._CLS_DT[torch.float32] == c["JG_CLS_F32"] == 2 and ops._CLS_DT[torch.float16] == c["JG_F16"] and ops._CLS_DT[torch.bfloat16] == c["JG_BF16"]
    assert ops.D_AUG_MAX == c["JG_D_AUG_MAX"] == 4
    assert (ops.D_DIFFUSION_MAX, ops.D_DIFFUSION_TABLE, ops.D_DIFFUSION_EPL) == (c["JG_D_DIFFUSION_MAX"], c["JG_D_DIFFUSION_TABLE"], c["JG_D_DIFFUSION_EPL"]) == (4, 501, 64)


def test_header_parser_refuses_unknown_types():
    """the type map is closed: a declaration outside it is an error that names the declaration, never a void* guess"""
    from joligen_amd import _lib

    consts, structs, sigs, res = _lib.parse_header("enum { JG_A = 3 };\ntypedef struct { const float* p; int32_t a, b; } jg_t;\n"
                                                   "int64_t jg_x(int n, const jg_t* t, const char* s, float* const* q);")
    assert consts == {"JG_A": 3} and [f[0] for f in structs["jg_t"]._fields_] == ["p", "a", "b"]
    assert sigs == {"jg_x": [_lib.c_i32, _lib.C.POINTER(structs["jg_t"]), _lib.C.c_char_p, _lib.c_p]} and res == {"jg_x": _lib.c_i64}
    with pytest.raises(TypeError, match="jg_x"):
        _lib.parse_header("int jg_x(int n, double v);")
    with pytest.raises(TypeError, match="jg_t"):
        _lib.parse_header("typedef struct { int32_t n; double v; } jg_t;")
    for text in ("int jg_x(unsigned n);", "int jg_x(jg_t by_value);", "typedef struct { int32_t n[4]; } jg_t;", "enum { JG_A, JG_B };",
                 "static int jg_count;", "int jg_x(int (*callback)(int));"):
        with pytest.raises(TypeError):
            _lib.parse_header(text)


# (name, default) of every dispatch switch, as the table of csrc/capi.hip stood before it was generated from JG_TUNE_LIST
_TUNE_DEFAULTS = [("HALO_CFG", 0), ("WGRAD_HALO_CFG", 0), ("CONV_VARIANT", 6), ("WGRAD_VARIANT", 4), ("SINKHORN_GENERIC", 0), ("CONV1X1", 1),
                  ("GN_REVERSE", 1), ("HALO_DBG", 0), ("PERSIST64", 1), ("HALO_PIPE", 1), ("WGRAD_PIPE", 1), ("CONV_SPLITK", 1),
                  ("CONV_SMALL_TILE", 1), ("GN_FUSED", 1), ("GN_FUSED_CAP", 256), ("GN_FUSED_DBG", 0), ("GN_FUSED_SLEEP", 4),
                  ("WGRAD_LDS_PAD", 0), ("LN_BWD_CAP", 256), ("DW_BWD_CAP", 512), ("DW_BWD_PPT", 8), ("CONV_KXK", 1), ("CONV_RING", 1),
                  ("WGRAD_DEEP", 1), ("WGRAD_SW", 0), ("DETERMINISTIC", 0), ("WGRAD_GROUP_BLOCKS", 1024), ("SGEMM_SPLIT", 0),
                  ("WGRAD_BIG", 1), ("DW_RUN", 1)]

_TUNE_CHILD = """
import json, sys
from joligen_amd import _lib
L = _lib.lib()
names = json.loads(sys.argv[1])
out = {"defaults": [L.jg_get_tuning(n.encode()) for n in names], "get_unknown": L.jg_get_tuning(b"JG_NO_SUCH_SWITCH"),
       "set_unknown": L.jg_set_tuning(b"JG_NO_SUCH_SWITCH", 1), "prev": [], "back": []}
for n in names:
    v = L.jg_get_tuning(n.encode()) + 7
    out["prev"].append(_lib.set_tuning(n, v))
    out["back"].append(L.jg_get_tuning(n.encode()) - v)
out["after"] = [L.jg_get_tuning(n.encode()) for n in names]
out["torch"] = "torch" in sys.modules
print(json.dumps(out))
"""


def test_dispatch_switch_table_defaults_and_round_trip():
    """names, defaults and the set / get round trip of the 30 dispatch switches, in a fresh process without any JG_* variable in its
    environment (no GPU is initialised: the child never imports torch and launches nothing)"""
    import json
    import sys

    from joligen_amd import _lib

    _lib.build()
    assert len(_TUNE_DEFAULTS) == 30
    names = ["JG_" + n for n, _ in _TUNE_DEFAULTS]
    env = {k: v for k, v in os.environ.items() if not k.startswith("JG_")}
    r = subprocess.run([sys.executable, "-c", _TUNE_CHILD, json.dumps(names)], cwd=ROOT, env=env, check=True, capture_output=True, text=True)
    out = json.loads(r.stdout.splitlines()[-1])
    assert dict(zip(names, out["defaults"])) == {"JG_" + n: d for n, d in _TUNE_DEFAULTS}
    assert out["get_unknown"] == -1 and out["set_unknown"] == _lib.JG_ERR_BAD_ARG
    assert out["prev"] == out["defaults"] and out["back"] == [0] * 30       # every name sets its own slot ...
    assert out["after"] == [d + 7 for _, d in _TUNE_DEFAULTS]                # ... and no other name's
    assert out["torch"] is False


@pytest.mark.parametrize("name", ["tiny_eff", "tiny_noeff", "tiny_attn"])
def test_module_tree_has_reference_state_dict(golden_dir, name):
    from joligen_amd.models.palette_model import define_G
    from joligen_amd.options import opt_from_json

    g = torch.load(os.path.join(golden_dir, f"palette_step_{name}.pt"), weights_only=False)
    c = g["cfg"]
    opt = opt_from_json({}, dict(G_ngf=c["ngf"], G_unet_mha_channel_mults=c["mults"], G_unet_mha_res_blocks=c["res_blocks"],
                                 G_unet_mha_attn_res=c["attn_res"], G_unet_mha_vit_efficient=c["efficient"],
                                 data_crop_size=c["S"]))
    net = define_G(**vars(opt))
    sd = net.state_dict()
    assert list(sd.keys()) == g["keys"]
    for k, v in sd.items():
        assert tuple(v.shape) == g["shapes"][k], k
    sched = torch.load(os.path.join(golden_dir, "schedule.pt"), weights_only=False)
    for k, v in sd.items():
        if O._is_buffer(k):
            assert torch.equal(v, sched[k.split(".")[-1]]), k
    # zero-initialised layers of the reference (zero_module) are zero here too
    for k, v in sd.items():
        if k.endswith("out_layers.3.weight") or k.endswith("proj_out.weight") or k.endswith("out.2.weight"):
            assert float(v.abs().max()) == 0.0, k


def test_full_size_network_matches_survey_counts():
    from joligen_amd.models.palette_model import define_G
    from joligen_amd.options import opt_from_json

    net = define_G(**vars(opt_from_json({}, dict(data_crop_size=256))))
    assert sum(p.numel() for p in net.parameters()) == 59346627 + 2112
    assert len(net.state_dict()) == 338 and len(list(net.parameters())) == 324


def test_options_flatten_reference_json_layout():
    from joligen_amd.options import opt_from_json

    cfg = {"G": {"netG": "unet_mha", "ngf": 32, "unet_mha_vit_efficient": True},
           "alg": {"diffusion": {"lambda_G": 2.0, "task": "inpainting"}, "palette": {"loss": "MSE"}},
           "train": {"batch_size": 4, "iter_size": 16, "G_ema": True, "optim": "adamw"},
           "data": {"crop_size": 128, "online_creation": {"crop_size_A": 128}}, "gpu_ids": "0,1", "model_type": "palette"}
    opt = opt_from_json(cfg, {"train_iter_size": 1})
    assert opt.G_ngf == 32 and opt.G_unet_mha_vit_efficient is True and opt.alg_diffusion_lambda_G == 2.0
    assert opt.train_batch_size == 4 and opt.train_iter_size == 1 and opt.train_G_ema is True
    assert opt.data_online_creation_crop_size_A == 128 and opt.gpu_ids == [0, 1] and opt.isTrain
    assert opt_from_json({}, {"gpu_ids": "-1"}).gpu_ids == []


def test_train_continue_from_option_contract(tmp_path):
    """The host half of /root/reference/tests/test_train_continue_from.py: `train_continue` and `train_continue_from` exclude each other
    (options/train_options.py:694-697), the load suffix is `iter_<n>` when `train_load_iter > 0` (train.py:92-95), and
    `finetune_source.json` records the source checkpoints with the reference's keys (train.py:98-120).  The device half (setup() loads
    `<source>/<suffix>_net_<name>.pth`, save_dir stays the target run's) is tests/test_gpu_1_model.py::test_train_continue_from_loads_source_run."""
    import json

    import pytest

    from joligen_amd.options import get_train_load_suffix, opt_from_json, save_finetune_source_metadata

    with pytest.raises(ValueError, match="mutually exclusive"):
        opt_from_json({}, {"train_continue": True, "train_continue_from": "/tmp/source_run"})
    opt = opt_from_json({}, {"train_continue_from": "source_run", "train_load_iter": 123, "checkpoints_dir": str(tmp_path), "name": "target_run"})
    assert get_train_load_suffix(opt) == "iter_123"
    assert get_train_load_suffix(opt_from_json({}, {})) == "latest"
    path = save_finetune_source_metadata(opt, "python train.py ...", ["G_A"])
    meta = json.loads(open(path).read())
    assert path == str(tmp_path / "target_run" / "finetune_source.json")
    assert meta["train_continue_from"] == "source_run" and meta["load_suffix"] == "iter_123"
    assert meta["checkpoint_files"] == ["source_run/iter_123_net_G_A.pth"] and meta["command_line"] == "python train.py ..."
    assert save_finetune_source_metadata(opt_from_json({}, {}), "x", ["G_A"]) is None


def test_param_arena_layout_on_cpu():
    """The arena itself is plain tensor-view bookkeeping and can be exercised on the CPU device
    (only refresh()/adamw_step() launch kernels)."""
    from joligen_amd.arena import ParamArena
    from joligen_amd.models.palette_model import define_G
    from joligen_amd.options import opt_from_json

    opt = opt_from_json({}, dict(G_ngf=32, G_unet_mha_channel_mults=[1, 2], G_unet_mha_res_blocks=[1, 1], data_crop_size=16))
    net = define_G(**vars(opt))
    ref = {k: v.clone() for k, v in net.state_dict().items()}
    arena = ParamArena(net, "cpu", torch.bfloat16)
    # values preserved, logical shapes unchanged, conv weights physically KRSC
    for k, p in net.named_parameters():
        assert torch.equal(p.detach(), ref[k]), k
        assert p.grad is not None and p.grad.shape == p.shape
        off, n = arena.slices[k]
        assert p.data_ptr() == arena.p.data_ptr() + 4 * off
        assert p.grad.data_ptr() == arena.g.data_ptr() + 4 * off
        if p.dim() == 4:
            O_, I, R, S = p.shape
            assert p.stride() == (R * S * I, 1, S * I, I), (k, p.stride())
            flat = arena.p[off:off + n].view(O_, R, S, I)
            assert torch.equal(flat, ref[k].permute(0, 2, 3, 1))
    # the stacked embedding projection is one contiguous [sum(2C), emb] block in module order
    unet = net.denoise_fn.model
    Wall = arena.group_view("emb_layers.1.weight").view(unet.emb_total, unet.cond_embed_dim)
    off = 0
    for m in unet.modules():
        if hasattr(m, "emb_slice") and m.emb_slice is not None:
            assert m.emb_slice[0] == off
            assert torch.equal(Wall[off:off + m.emb_slice[1]], m.emb_layers[1].weight.detach())
            off += m.emb_slice[1]
    assert off == unet.emb_total
    # state_dict() hands out plain contiguous tensors in the reference layout
    sd = net.state_dict()
    for k, v in sd.items():
        assert v.is_contiguous() and torch.equal(v, ref[k]), k
        assert v.untyped_storage().nbytes() <= max(v.numel(), 1) * v.element_size() + 64
    # load_state_dict writes through the views and marks the 16-bit copies stale
    arena.dirty = False
    net.load_state_dict(O.synth_state_dict(sd, seed=3))
    assert arena.dirty
    k0 = "denoise_fn.model.input_blocks.1.0.in_layers.2.weight"
    off, n = arena.slices[k0]
    assert torch.equal(arena.p[off:off + n].view(32, 3, 3, 32), O.synth_state_dict(sd, seed=3)[k0].permute(0, 2, 3, 1))
    # working-copy descriptors: padded shapes and offsets are consistent
    desc = arena.desc.tolist()
    tot = 0
    for src, dst, dstT, cout, rs, cin, coutp, cinp in desc:
        assert dst == tot and coutp % 8 == 0 and cinp % 8 == 0 and coutp >= cout and cinp >= cin
        tot += coutp * rs * cinp
    assert tot <= arena.w16.numel()
    stem = net.denoise_fn.model.input_blocks[0][0].meta
    assert (stem.Cin, stem.Cin_real, stem.Cout) == (8, 6, 32)
    head = net.denoise_fn.model.out[2].meta
    assert (head.Cout, head.Cout_real) == (8, 3) and head.bias_pad is not None


def test_ops_refuse_cpu_tensors():
    """No CPU / eager fallback: the product path fails loudly without a GPU."""
    from joligen_amd import ops
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    with pytest.raises(RuntimeError, match="GPU only|no CPU"):
        ops.group_norm(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16), 1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            create_model(opt_from_json({}, {"gpu_ids": "0"}), 0)


def test_product_does_not_import_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    paths = [os.path.join(dirpath, f) for top in ("joligen_amd", "tools") for dirpath, _, files in os.walk(os.path.join(ROOT, top))
             for f in files if f.endswith(".py")]
    assert len(paths) > 20
    for path in paths:
        src = open(path).read()
        assert "jg_oracle" not in src and "ref_shim" not in src and "/root/reference" not in src.replace(
            "/root/reference/models", "").replace("/root/reference/", "REF/"), path


# the launches that the module graph and the torch.ops surface share: stated once, in joligen_amd/launch.py
_LAUNCH_LAYER = """jg_layernorm_fwd jg_layernorm_bwd jg_attn_smallkv_fwd jg_attn_smallkv_bwd2 jg_gelu_fwd jg_gelu_bwd jg_act_fwd jg_act_bwd
jg_reflect_pad2d jg_reflect_pad2d_bwd jg_l2norm_fwd jg_l2norm_bwd jg_nce_sinkhorn_fwd jg_nce_sinkhorn_bwd jg_nce_ce jg_row_axpy jg_nce_hdce
jg_gan_loss jg_hinge_loss jg_spectral_power_iter jg_spectral_wgrad_fix jg_bilinear2_fwd jg_bilinear2_bwd jg_linear_fwd jg_linear_bwd
jg_ddpm_mse_loss""".split()
# every other entry point with more than one call site, and why it is not a launch written once per surface
_MULTI_SITE_OK = {
    "jg_gn_stats": "BatchNorm2d of the SegFormer head and the recomputing GroupNorm backward of the functional op: different ops",
    "jg_gn_stats_ld": "GroupNorm forward and the UNet executor's strided form: different ops",
    "jg_gn_coef": "GroupNorm forward and the recomputing backward of the functional op",
    "jg_gn_apply": "GroupNorm and BatchNorm2d share the apply primitive",
    "jg_gn_bwd_reduce": "BatchNorm2d backward and the functional GroupNorm backward: different ops",
    "jg_gn_bwd_coef": "module-graph and functional GroupNorm backward are different launch chains (statistics saved / recomputed)",
    "jg_gn_bwd_apply": "GroupNorm (both chains) and BatchNorm2d share the apply primitive",
    "jg_bn_coef": "SyncBatchNorm and local branch of one forward",
    "jg_bn_bwd_coef": "SyncBatchNorm (local parameter sums, global dx sums) and local branch of one backward",
    "jg_crop2d": "forward and adjoint mode, in ops.crop2d and in the projected discriminator's padding node",
    "jg_scale": "DropPath, Dropout2d and the scaled branch gradient: one primitive, different ops",
    "jg_bilinear_bwd": "resize_concat and the fallback of resize_sum: different ops",
    "jg_layernorm_bwd_add": "LayerNorm with identity and add + LayerNorm: different nodes",
    "jg_ddpm_p_sample": "first and later steps of one sampling loop",
    "jg_transpose2d": "forward and backward of one node",
    "jg_refresh_weights": "trainable and frozen descriptor table in one function",
    "jg_last_kernel": "bench labels of the convolution and of the weight gradient",
    "jg_get_tuning": "the tuning accessor of _lib and the JG_DETERMINISTIC query of conv2d_stats",
}


def test_shared_launches_are_stated_once():
    """Both Python surfaces go through joligen_amd/launch.py: each shared C entry point has ONE textual call site, there; whatever else is
    called from more than one place is a primitive used by different ops and is listed above with its reason."""
    rx = re.compile(r"(lib\(\)|\bL)\.(jg_\w+)\(")
    sites = {}
    top = os.path.join(ROOT, "joligen_amd")
    for dirpath, _, files in os.walk(top):
        for f in files:
            if f.endswith(".py"):
                rel = os.path.relpath(os.path.join(dirpath, f), top)
                for n, line in enumerate(open(os.path.join(dirpath, f)), 1):
                    for m in rx.finditer(line):
                        sites.setdefault(m.group(2), []).append(f"{rel}:{n}")
    assert len(_LAUNCH_LAYER) == 26 and len(set(_LAUNCH_LAYER)) == 26
    for name in _LAUNCH_LAYER:
        where = sites.get(name, [])
        assert len(where) == 1 and where[0].startswith("launch.py:"), (name, where)
    multi = {k for k, v in sites.items() if len(v) > 1}
    assert not multi & set(_LAUNCH_LAYER)
    assert not set(_MULTI_SITE_OK) & set(_LAUNCH_LAYER)
    assert multi - set(_MULTI_SITE_OK) == set(), {k: sites[k] for k in multi - set(_MULTI_SITE_OK)}
    assert set(_MULTI_SITE_OK) - multi == set(), "stale allow-list entries"
    assert all(len(reason) > 10 for reason in _MULTI_SITE_OK.values())
    src = open(os.path.join(top, "launch.py")).read()
    imports = re.findall(r"^\s*(?:from\s+(\S+)\s+import\s+(.+)|import\s+(.+))$", src, re.M)
    assert imports
    for frm, names, plain in imports:
        text = f"{frm} {names} {plain}"
        assert not re.search(r"\b(ops_segformer|ops_library_cut|modules|ops)\b", text), text


def test_hot_kernels_do_not_spill(tmp_path):
    """The halo-resident convolution / weight-gradient kernels sit at the VGPR limit of their occupancy target: any scratch spill
    costs 2-3x (a reflect-padding edit once pushed the 8-row weight-gradient configuration into 95 spilled registers).  Compile
    the two translation units with -save-temps and require zero spills and zero private segment for every kernel in them."""
    import re
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "joligen_amd", "csrc")
    for src in ("conv_halo.hip", "wgrad_halo.hip", "conv_p64.hip"):
        out = tmp_path / src.replace(".hip", "")
        out.mkdir()
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-c", os.path.join(csrc, src), "-o",
                            str(out / "o.o"), "-save-temps=obj"], capture_output=True, text=True, cwd=str(out))
        assert r.returncode == 0, r.stderr[-2000:]
        asm = [f for f in os.listdir(out) if f.endswith("gfx950.s")]
        assert asm, os.listdir(out)
        text = open(out / asm[0]).read()
        names = re.findall(r"\.name:\s+(\S+)", text)
        spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
        priv = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
        assert names and len(spills) >= len([n for n in names if "halo_kernel" in n or "p64_kernel" in n])
        if src == "conv_p64.hip":
            # the persistent kernel sits at the 256-register limit of two waves per SIMD: a handful of loop-invariant scalars are
            # allowed to live in scratch (reloaded twice per tile); anything more means a whole array went there
            assert max(spills) <= 8, list(zip(names, spills, priv))
            continue
        assert max(spills) == 0 and max(priv) == 0, list(zip(names, spills, priv))
        # occupancy budgets (512 VGPRs per SIMD lane): LDS (66 KB per workgroup) holds the 64-wide tiles at two workgroups per CU =
        # two waves per SIMD, the 128x512 8-wave tile at one workgroup: both stay clear of the 256-register line with room to spare
        vg = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
        for nm, v in zip(names, vg):
            if "conv3x3_halo_kernel" in nm and "Li64ELi256E" in nm:
                assert v <= 168, (nm, v)
            if "conv3x3_halo_kernel" in nm and "Li128ELi512E" in nm:
                assert v <= 168, (nm, v)


def test_image_pool_matches_reference_semantics():
    """util/image_pool.py:19-56 behaviour of joligen_amd.util.image_pool.ImagePool (host logic, CPU tensors): fill phase, 50 % swap
    with a random stored image, draw order uniform -> randint, detached returns; against the oracle restatement with the same RNG."""
    import random

    import torch

    import jg_oracle as O
    from joligen_amd.util.image_pool import ImagePool

    for size in (0, 1, 3):
        ref, mine = O.OracleImagePool(size, random.Random(7)), ImagePool(size, random.Random(7))
        for it in range(15):
            x = (torch.full((2, 4, 4, 8), float(it)) + torch.arange(2).view(2, 1, 1, 1) * 0.5).requires_grad_(size > 0)
            a, b = ref.query(x), mine.query(x)
            assert torch.equal(a, b)
            assert size == 0 or not b.requires_grad
        assert len(mine) == min(size, 30) if size else True


def test_cut_options_and_forced_segformer_settings():
    """CUT defaults of cut_model.py (:39-137) and the settings the reference enforces for a SegFormer generator (:205-210); the model
    class itself refuses to build without a GPU (no CPU fallback in the product path)."""
    import pytest
    import torch

    from joligen_amd.models.cut_model import CUT_DEFAULTS
    from joligen_amd.options import opt_from_json

    assert CUT_DEFAULTS["alg_cut_nce_T"] == 0.07 and CUT_DEFAULTS["alg_cut_num_patches"] == 256
    assert CUT_DEFAULTS["alg_cut_nce_layers"] == "0,4,8,12,16" and CUT_DEFAULTS["alg_cut_nce_loss"] == "monce"
    opt = opt_from_json({"model_type": "cut", "G": {"netG": "segformer_attn_conv"}, "alg": {"cut": {"nce_T": 0.07}}}, {"gpu_ids": "0"})
    assert opt.alg_cut_nce_T == 0.07 and opt.G_netG == "segformer_attn_conv"
    if not torch.cuda.is_available():
        from joligen_amd.models import create_model

        with pytest.raises(RuntimeError, match="MI355X"):
            create_model(opt, 0)


def test_early_exchange_parameter_coverage_of_the_fused_backward():
    """Data parallel (parallel.EarlyExchange): walking the UNet the way unet_exec's forward builds its tape, the records' own
    parameters (`_own_params`) cover every UNet parameter EXACTLY once except the ResBlock embedding projections (their gradient
    comes from the stacked linear behind the node); with the conditioning MLP those are the parameters that go out with the
    optimizer step.  Checked on the CPU-built module tree + arena of an efficient and a non-efficient UNet, then driven through
    EarlyExchange's bookkeeping (tail-first readiness, nothing reported twice, every chunk accounted for)."""
    import torch
    import torch.nn as nn

    from joligen_amd import parallel
    from joligen_amd.arena import ParamArena
    from joligen_amd.models.palette_model import define_G
    from joligen_amd.modules import unet_exec as ue
    from joligen_amd.modules.unet_generator_attn import AttentionBlock, ResBlock
    from joligen_amd.options import opt_from_json

    for efficient, mults, nres in ((True, [1, 2], [1, 1]), (False, [1, 2, 2], [2, 1, 1])):
        opt = opt_from_json({}, dict(G_ngf=32, G_unet_mha_channel_mults=mults, G_unet_mha_res_blocks=nres, G_unet_mha_attn_res=[16],
                                     G_unet_mha_vit_efficient=efficient, data_crop_size=32, gpu_ids="0"))
        net = define_G(**vars(opt))
        arena = ParamArena(net, torch.device("cpu"), torch.bfloat16)
        u = net.denoise_fn.model
        recs = [dict(kind="stem", m=list(u.input_blocks[0])[0].meta)]
        blocks = [list(b) for b in list(u.input_blocks)[1:]] + [list(u.middle_block)] + [list(b) for b in u.output_blocks]
        for layers in blocks:
            for layer in layers:
                if isinstance(layer, ResBlock):
                    recs.append(dict(kind="res", rb=layer, identity=isinstance(layer.skip_connection, nn.Identity)))
                else:
                    assert isinstance(layer, AttentionBlock), type(layer)
                    recs.append(dict(kind="attn", blk=layer))
        recs.append(dict(kind="head", gn=u.out[0].norm, m=u.out[2].meta))
        name_of = {id(p): n for n, p in net.named_parameters()}
        reported = [id(p) for rec in recs for p in ue._own_params(rec)]
        assert len(reported) == len(set(reported))                                    # nothing twice
        assert all(i in name_of for i in reported)
        left = sorted(n for i, n in name_of.items() if i not in set(reported))
        assert left and all(("emb_layers" in n) or ("cond_embed" in n) for n in left), left   # only the embedding path is outside the node
        # the bookkeeping: report in backward (reverse tape) order
        ex = parallel.EarlyExchange.__new__(parallel.EarlyExchange)
        launched = []
        ex._launch = lambda c, ex=ex: (ex.sent.__setitem__(c, True), launched.append(c))
        parallel.EarlyExchange.__init__(ex, arena, list(net.named_parameters()), n_chunks=8)
        for rec in reversed(recs):
            for p in ue._own_params(rec):
                ex.mark(p)
        early = list(launched)
        assert len(early) >= len(ex.bounds) - 3, (early, len(ex.bounds))              # the priority (embedding) group sits at the head
        assert early == sorted(early, reverse=True) or len(set(early)) == len(early)  # tail-first, each chunk once
        assert all(ex.left[c] == 0 for c in early) and all(ex.left[c] > 0 or ex.total[c] == 0 for c in range(len(ex.bounds)) if c not in early)
        for k in list(parallel._EARLY):                                                # keep the module-level registry clean for other tests
            if parallel._EARLY[k] is ex:
                del parallel._EARLY[k]


def test_fp16_loss_scale_policy_polls_every_step_after_growth():
    """BaseModel.poll_overflow (host half of GradScaler, reference base_model.py:89-90,1268-1274): the dropped-step counter is
    read every `jg_overflow_poll` optimizer steps, and on EVERY step of the window that follows a growth event (an overflowing probe costs
    one update, not fifty); `jg_loss_scale_growth_interval <= 0` never grows; the step count of a dropped step is given back."""
    from types import SimpleNamespace

    from joligen_amd.models.base_model import BaseModel

    class Arena:
        def __init__(self):
            self.overflow, self.step = torch.zeros(2, dtype=torch.int64), 0

    def model(growth, every=10):
        m = object.__new__(BaseModel)
        m.opt = SimpleNamespace(jg_overflow_poll=every, train_iter_size=1, jg_loss_scale_growth_interval=growth)
        m.act_dtype, m.niter, m.loss_scale = torch.float16, 0, 1024.0
        a = Arena()
        m.optimizers = [SimpleNamespace(arena=a, grad_scale=1.0 / 1024.0)]
        return m, a

    m, a = model(growth=20)
    for _ in range(20):                       # 20 clean steps: polled at 10 and 20, grows at 20
        m.niter += 1; a.step += 1
        m.poll_overflow()
    assert m.loss_scale == 2048.0 and m.optimizers[0].grad_scale == 1.0 / 2048.0
    m.niter += 1; a.step += 1
    a.overflow[1] += 1                        # the very next step overflows on the doubled scale ...
    m.poll_overflow()                         # ... and is seen at once (step 21 is not a multiple of 10)
    assert m.loss_scale == 1024.0 and a.step == 20, (m.loss_scale, a.step)
    for _ in range(8):                        # back to the sparse schedule: an overflow at step 22 waits for the poll at step 30
        m.niter += 1; a.step += 1
        if m.niter == 22:
            a.overflow[1] += 1
        m.poll_overflow()
        assert m.loss_scale == 1024.0
    m.niter += 1; a.step += 1
    m.poll_overflow()
    assert m.niter == 30 and m.loss_scale == 512.0
    m, a = model(growth=0)                    # static scale: never grows
    for _ in range(200):
        m.niter += 1; a.step += 1
        m.poll_overflow()
    assert m.loss_scale == 1024.0


def test_hip_graphs_safe_flag():
    """joligen_amd/__init__.py: the package switches ROCm's graph AQL-packet capture off when it still can (variable unset, HIP runtime not yet
    initialised) and records whether replays can be trusted; an explicit user setting is respected either way."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import os, joligen_amd; print(joligen_amd.HIP_GRAPHS_SAFE, os.environ.get('DEBUG_CLR_GRAPH_PACKET_CAPTURE'))"

    def run(value):
        env = {k: v for k, v in os.environ.items() if k != "DEBUG_CLR_GRAPH_PACKET_CAPTURE"}
        if value is not None:
            env["DEBUG_CLR_GRAPH_PACKET_CAPTURE"] = value
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120).stdout.split()

    assert run(None) == ["True", "0"]
    assert run("0") == ["True", "0"]
    assert run("1") == ["False", "1"]


def test_cut_gate_truth_table(monkeypatch):
    """models/cut_step.gate: an option under its environment variable, read at call time.  `=0` always switches off; `=1` forces the path on
    over a false option only for the tri-state gates (JG_FORK_GAN / JG_GRAPH_G / JG_GRAPH_D), not for the switch-off-only ones."""
    from types import SimpleNamespace

    from joligen_amd.models.cut_step import gate

    absent = object()
    for force in (False, True):
        for option in (True, False, absent):
            for default in (True, False):
                for env in (None, "0", "1"):
                    opt = SimpleNamespace() if option is absent else SimpleNamespace(jg_x=option)
                    monkeypatch.delenv("JG_X", raising=False) if env is None else monkeypatch.setenv("JG_X", env)
                    value = default if option is absent else option
                    want = env != "0" and (value or (force and env == "1"))
                    got = gate(opt, "jg_x", "JG_X", default, force=force)
                    assert got is want, (force, option, default, env, got)
    monkeypatch.delenv("JG_X", raising=False)
    assert gate(SimpleNamespace(), "jg_x", "JG_X") is True          # an absent option defaults to on


def test_cut_captured_half_bookkeeping(monkeypatch):
    """models/cut_step.CapturedHalf with a fake capture function and no GPU: at most three captured states, a failure is sticky (the capture
    function is never called again) and leaves the warning and the note the tests and bench.py grep for, and the snapshot is written back
    without a version bump (the frozen-BN tables key on tensor versions)."""
    import warnings
    from types import SimpleNamespace

    import joligen_amd
    from joligen_amd.models.cut_step import CapturedHalf

    monkeypatch.setattr(joligen_amd, "HIP_GRAPHS_SAFE", True)
    for v in ("JG_GRAPH_G", "JG_GRAPH_D", "JG_DBG_GRAPH_CANARY_FAIL"):
        monkeypatch.delenv(v, raising=False)

    def fake_model():
        return SimpleNamespace(opt=SimpleNamespace(), act_dtype=torch.bfloat16, niter=3, step_driver_note="", device=torch.device("cpu"))

    def fake_net():
        buf = torch.arange(4.0)
        return SimpleNamespace(arena=SimpleNamespace(g=torch.ones(8), p=torch.zeros(8)), training=True, buffers=lambda: [buf], buf=buf)

    def halves(m):
        return (CapturedHalf(m, "jg_graph_G", "JG_GRAPH_G", "generator", "generator graph dropped", "G"),
                CapturedHalf(m, "jg_graph_D", "JG_GRAPH_D", "discriminator", "graph dropped", "1", "HIP_GRAPHS_SAFE is False (test)"))

    # the gate and the shared guards
    m = fake_model()
    g, d = halves(m)
    assert g.ready() and d.ready()
    m.niter = 2
    assert not g.ready()
    m.niter, m.act_dtype = 3, torch.float16
    assert not d.ready()
    m.act_dtype = torch.bfloat16
    monkeypatch.setenv("JG_GRAPH_D", "0")
    assert g.ready() and not d.ready()
    monkeypatch.delenv("JG_GRAPH_D")
    m.opt.jg_graph_G = False
    assert not g.ready()
    monkeypatch.setenv("JG_GRAPH_G", "1")
    assert g.ready()
    monkeypatch.setattr(joligen_amd, "HIP_GRAPHS_SAFE", False)
    assert not g.ready() and m.step_driver_note == ""              # only the discriminator half says why
    assert not d.ready() and "HIP_GRAPHS_SAFE" in m.step_driver_note
    monkeypatch.setattr(joligen_amd, "HIP_GRAPHS_SAFE", True)

    # a passing capture: cached per key, three keys at most, touched state restored without a version bump
    m = fake_model()
    g, d = halves(m)
    net, calls = fake_net(), []
    versions = (net.arena.g._version, net.buf._version)

    def capture(restore):
        calls.append(restore)
        net.arena.g.data.mul_(3.0)                                 # what two replays of a canary do to the state
        net.buf.data.add_(1.0)
        d.check(torch.tensor(2.0), torch.tensor(2.0 + 1e-4), 1e-3, "an untouched graph")
        d.check(torch.tensor([2.0, 5.0]), torch.tensor([2.001, 5.1]), torch.tensor([5e-3, 5e-2]), "the generator graphs")
        return "state%d" % len(calls)

    assert d.get(("a",), [net], capture) == "state1" and d.get(("a",), [net], capture) == "state1" and len(calls) == 1
    assert torch.equal(net.arena.g, torch.ones(8)) and torch.equal(net.buf, torch.arange(4.0))
    assert (net.arena.g._version, net.buf._version) == versions
    net.arena.g.data.fill_(7.0)
    calls[0]()                                                     # the restore handed to the capture function, on its own
    assert torch.equal(net.arena.g, torch.ones(8)) and net.arena.g._version == versions[0]
    assert d.get(("b",), [net], capture) == "state2" and d.get(("c",), [net], capture) == "state3"
    assert d.get(("d",), [net], capture) is None and len(calls) == 3 and len(d.cache) == 3       # a fourth distinct key is refused ...
    assert not d.failed and m.step_driver_note == "" and d.get(("b",), [net], capture) == "state2"   # ... and is no failure
    net.training = False                                           # the networks' mode and arena address are part of the key
    assert d.get(("a",), [net], capture) is None and len(calls) == 3

    # the canary's comparison: relative tolerance, non-finite values, the forced failure of the tests
    for first, second, tol in ((torch.tensor(2.0), torch.tensor(2.01), 1e-3), (torch.tensor(2.0), torch.tensor(float("nan")), 1e-3),
                               (torch.tensor([2.0, 5.0]), torch.tensor([2.0, 5.5]), torch.tensor([5e-3, 5e-2]))):
        with pytest.raises(RuntimeError, match="disagree after interleaved eager launches"):
            d.check(first, second, tol, "an untouched graph")
    monkeypatch.setenv("JG_DBG_GRAPH_CANARY_FAIL", "G")
    d.check(torch.tensor(2.0), torch.tensor(2.0), 1e-3, "an untouched graph")          # "G" targets the generator half only
    with pytest.raises(RuntimeError):
        g.check(torch.tensor(2.0), torch.tensor(2.0), 1e-3, "the generator graphs")
    monkeypatch.setenv("JG_DBG_GRAPH_CANARY_FAIL", "1")
    g.check(torch.tensor(2.0), torch.tensor(2.0), 1e-3, "the generator graphs")
    with pytest.raises(RuntimeError):
        d.check(torch.tensor(2.0), torch.tensor(2.0), 1e-3, "an untouched graph")

    # failing captures: warning, note, sticky flag, state restored; both halves append to the note
    m = fake_model()
    g, d = halves(m)
    net, calls = fake_net(), []

    def failing(half):
        def capture(restore):
            calls.append(half.option)
            net.arena.g.data.mul_(3.0)
            half.check(torch.tensor(2.0), torch.tensor(2.0), 1e-3, "an untouched graph")          # JG_DBG_GRAPH_CANARY_FAIL=1 / G
            return "state"
        return capture

    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert d.get(("a",), [net], failing(d)) is None
        monkeypatch.setenv("JG_DBG_GRAPH_CANARY_FAIL", "G")
        assert g.get(("a",), [net], failing(g)) is None
        monkeypatch.delenv("JG_DBG_GRAPH_CANARY_FAIL")
        for _ in range(3):                                         # sticky: the capture function is never called again
            assert d.get(("a",), [net], failing(d)) is None and g.get(("b",), [net], failing(g)) is None
            assert not d.ready() and not g.ready()
    assert calls == ["jg_graph_D", "jg_graph_G"] and d.failed and g.failed and not d.cache and not g.cache
    texts = [str(w.message) for w in rec]
    assert len(texts) == 2 and texts[0].startswith("jg_graph_D: the discriminator half stays eager")
    assert texts[1].startswith("jg_graph_G: the generator half stays eager")
    assert m.step_driver_note.startswith("graph dropped: ") and "; generator graph dropped: " in m.step_driver_note
    assert torch.equal(net.arena.g, torch.ones(8)) and net.arena.g._version == versions[0]
