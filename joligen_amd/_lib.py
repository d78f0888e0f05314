"""ctypes binding of libjg355.so (the C ABI declared in include/jg355.h).

The library is built in-tree with hipcc for gfx950 (`build()`) and loaded once.  The header is the single statement of the ABI: it is
parsed at import, and the argtypes / restype of every entry point, the ctypes mirrors of its structs and every JG_* constant come from
it.  There is NO fallback: if the shared object is missing or a symbol is absent, importing the ops fails loudly, and a declaration the
parser does not understand is an error, never a guess.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libjg355.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "jg355.h")
SOURCES = ["attention.hip", "gemm_nt.hip", "conv_halo.hip", "conv_kxk.hip", "reflect_border.hip", "conv_p64.hip", "conv1x1.hip", "gemm_tn.hip", "wgrad_halo.hip", "wgrad_sw.hip", "wgrad_kxk.hip", "nce.hip", "segformer.hip", "vit.hip", "projected_d.hip", "effnet.hip", "norm.hip", "gn_fused.hip", "elementwise.hip", "d_aug.hip", "context.hip", "d_diffusion.hip", "dropout.hip", "sem_cls.hip", "resize_aa.hip", "optim.hip", "capi.hip"]
# -fno-slp-vectorize: the SLP vectoriser packs independent fp32 chains into v_pk_* pairs (register tuples: gn_fused.hip went from 150 spilled
# registers to none without it) -- "an anti-lever beside MFMAs" in the MI355X guide; same-box A/B of the whole step: 52.2 -> 52.0 ms
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics", "-fno-slp-vectorize"]

FILE_FLAGS = {}      # per-source extra flags

c_i32, c_i64, c_f32, c_p = C.c_int32, C.c_int64, C.c_float, C.c_void_p

_SCALARS = {"int": c_i32, "int32_t": c_i32, "int64_t": c_i64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": c_f32, "jg_stream_t": c_p}


def _ctype(decl: str, structs: dict, where: str):
    """ctypes type of the declaration `type [name]`; the closed type map of the ABI, anything else raises"""
    tok = re.findall(r"\w+|\*", decl)
    if len(tok) > 1 and tok[-1] != "*":
        tok = tok[:-1]          # the parameter / field name
    if not tok or re.sub(r"[\w\s*]", "", decl):
        raise TypeError(f"jg355.h: cannot parse `{decl.strip()}` in `{where}`")
    if "*" not in tok:
        if len(tok) == 1 and tok[0] in _SCALARS:
            return _SCALARS[tok[0]]
        raise TypeError(f"jg355.h: type `{' '.join(tok)}` of `{decl.strip()}` in `{where}` is outside the ABI's type map")
    if tok == ["const", "char", "*"]:
        return C.c_char_p
    if len(tok) == 3 and tok[0] == "const" and tok[1] in structs and tok[2] == "*":
        return C.POINTER(structs[tok[1]])
    return c_p


def parse_header(text: str):
    """(constants, structs, signatures, restypes) of a header in the dialect of include/jg355.h: enums with explicit values,
    `#define JG_X n`, typedef structs of scalars and pointers, prototypes `type jg_x(type name, ...);`.  Whatever else it finds raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts, structs, sigs, restypes = {}, {}, {}, {}
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(JG_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M):
        consts[name] = int(val)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    text = re.sub(r"typedef\s+void\s*\*\s*jg_stream_t\s*;", " ", text)

    def enum(m):
        for item in m.group(1).split(","):
            im = re.fullmatch(r"\s*(JG_\w+)\s*=\s*(-?\d+)\s*", item)
            if not im:
                raise TypeError(f"jg355.h: enumerator `{item.strip()}` needs the form JG_X = n")
            consts[im.group(1)] = int(im.group(2))
        return " "

    def struct(m):
        fields = []
        for decl in filter(str.strip, m.group(1).split(";")):
            first, *more = decl.split(",")
            ct = _ctype(first, structs, m.group(2))
            if ct not in _SCALARS.values() and more:
                raise TypeError(f"jg355.h: one pointer per declaration, `{decl.strip()}` in `{m.group(2)}`")
            fields += [(re.findall(r"\w+", d)[-1], ct) for d in [first] + more]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return " "

    def proto(m):
        ret, name, params = m.group(1), m.group(2), m.group(3)
        restypes[name] = _ctype(ret + " " + name, structs, name)
        sigs[name] = [] if params.strip() == "void" else [_ctype(p, structs, name) for p in params.split(",")]
        return " "

    text = re.sub(r"enum\s*\{([^}]*)\}\s*;", enum, text)
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"([\w\s*]+?)\b(jg_\w+)\s*\(([^()]*)\)\s*;", proto, text)
    if text.strip():
        raise TypeError(f"jg355.h: not understood: `{' '.join(text.split())[:200]}`")
    return consts, structs, sigs, restypes


with open(HEADER) as _f:
    CONSTANTS, STRUCTS, SIGNATURES, RESTYPES = parse_header(_f.read())      # name -> value / Structure class / argtypes / restype
globals().update(CONSTANTS)         # JG_OK, JG_F16, JG_ACT_SILU, JG_OUT_STORE_T, JG_D_AUG_MAX, ...
ConvArgs, WgradArgs = STRUCTS["jg_conv_args"], STRUCTS["jg_wgrad_args"]


def build(force: bool = False, verbose: bool = False, jobs: int = 0) -> str:
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU) into csrc/libjg355.so.
    One object per source under csrc/build/ (compiled in parallel, rebuilt when the source or any header is newer), then one link.
    csrc/build/BUILD_INFO.json records what was compiled by this call."""
    import json
    import time
    from concurrent.futures import ThreadPoolExecutor

    hdrs = [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + [HEADER]
    hdr_time = max(os.path.getmtime(h) for h in hdrs)
    bdir = os.path.join(CSRC, "build")
    os.makedirs(bdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]
    todo, objs = [], []
    for src in SOURCES:
        sp, op = os.path.join(CSRC, src), os.path.join(bdir, src.replace(".hip", ".o"))
        objs.append(op)
        if force or not os.path.exists(op) or os.path.getmtime(op) < max(os.path.getmtime(sp), hdr_time):
            todo.append((sp, op))

    def cc(job):
        sp, op = job
        cmd = [hipcc] + cflags + FILE_FLAGS.get(os.path.basename(sp), []) + ["-c", sp, "-o", op]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=CSRC)

    t0 = time.time()
    if todo:
        with ThreadPoolExecutor(max_workers=jobs or min(len(todo), os.cpu_count() or 4)) as ex:
            list(ex.map(cc, todo))
    relink = bool(todo) or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(o) for o in objs)
    if relink:
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=CSRC)
    if todo or relink:
        with open(os.path.join(bdir, "BUILD_INFO.json"), "w") as f:
            json.dump({"compiled": [os.path.basename(s) for s, _ in todo], "linked": relink, "seconds": round(time.time() - t0, 1),
                       "flags": cflags, "hipcc": hipcc}, f)
    return LIB_PATH


_lib = None


def lib():
    """The loaded library with typed entry points.  Raises if it is missing -- no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  joligen_amd has no CPU / eager fallback."
        )
    L = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the symbol is absent
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    _lib = L
    return L


def set_tuning(name: str, value: int):
    """override a dispatch switch of the library for the rest of the process; returns the previous value"""
    L = lib()
    prev = L.jg_get_tuning(name.encode())
    check(L.jg_set_tuning(name.encode(), int(value)), f"jg_set_tuning({name})")
    return prev


def check(code: int, what: str = ""):
    if code != 0:
        msg = lib().jg_strerror(code).decode()
        raise RuntimeError(f"libjg355 {what} failed: {msg} ({code})")
