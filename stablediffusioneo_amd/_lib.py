"""ctypes binding of libsdeo.so (the C ABI in include/sdeo.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent, loading
raises immediately (the reference silently falls back to PyTorch when a .plan is missing,
`cldm_trt/ddim_hacked.py:22-23,35-36`; we deliberately do not)."""
from __future__ import annotations

import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDEO_LIB") or os.path.join(HERE, "libsdeo.so")     # SDEO_LIB: A/B of two builds on one device
HEADER = os.path.join(os.path.dirname(HERE), "include", "sdeo.h")
INTERNAL_HEADER = os.path.join(HERE, "csrc", "sdeo_internal.h")      # the private hooks of tools/ and tests

_lib = None

MAX_LEVELS = 8


class SdeoConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("hint_channels", C.c_int),
        ("model_channels", C.c_int), ("num_res_blocks", C.c_int),
        ("channel_mult", C.c_int * MAX_LEVELS), ("num_levels", C.c_int),
        ("attention_resolutions", C.c_int * MAX_LEVELS), ("num_attention_resolutions", C.c_int),
        ("num_heads", C.c_int), ("context_dim", C.c_int), ("context_len", C.c_int),
        ("vae_ch", C.c_int), ("vae_out_ch", C.c_int), ("vae_ch_mult", C.c_int * MAX_LEVELS),
        ("vae_num_levels", C.c_int), ("vae_num_res_blocks", C.c_int), ("vae_z_channels", C.c_int),
        ("vae_scale_factor", C.c_float),
    ]


class SdeoConfigExt(C.Structure):
    """sdeo_config_ext of include/sdeo.h (the SD-2.x layout switches of sdeo_create_ex)"""
    _fields_ = [("size", C.c_int), ("num_head_channels", C.c_int), ("use_linear_in_transformer", C.c_int)]


class SdeoClipConfig(C.Structure):
    _fields_ = [("vocab", C.c_int), ("positions", C.c_int), ("width", C.c_int), ("layers", C.c_int), ("heads", C.c_int),
                ("ffn", C.c_int)]


class SdeoClipVisionConfig(C.Structure):
    _fields_ = [("image", C.c_int), ("patch", C.c_int), ("width", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("ffn", C.c_int),
                ("proj", C.c_int)]


class SdeoResamplerConfig(C.Structure):
    _fields_ = [("tokens", C.c_int), ("embed_dim", C.c_int), ("dim", C.c_int), ("depth", C.c_int), ("dim_head", C.c_int), ("heads", C.c_int),
                ("num_queries", C.c_int), ("ffn", C.c_int), ("out_dim", C.c_int)]


class SdeoError(RuntimeError):
    pass


# The binding's description of the C boundary is the two headers themselves: parse_header reads every prototype and struct layout
# out of them and load() types the library with the result.  A parser for these two files, not for C: the vocabulary is closed.
_SCALARS = {"void": None, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "int32_t": C.c_int32, "int64_t": C.c_int64,
            "unsigned long long": C.c_ulonglong}
_DECL = re.compile(r"\s*(.*?)\s*\b(\w+)\s*(?:\[(\w*)\])?\s*")        # type, name, array length (None: not an array)


def _ctype(decl, where):
    """ctypes type of the C type `decl`.  Every pointer but a plain char* is c_void_p, and so is every handle: callers pass ptr(t),
    byref(struct), ctypes arrays and None, and c_void_p takes all of them."""
    base = " ".join(w for w in re.findall(r"\w+", decl) if w != "const")
    if "*" in decl:
        return C.c_char_p if base == "char" and decl.count("*") == 1 else C.c_void_p
    if re.fullmatch(r"sdeo_\w*handle", base):
        return C.c_void_p
    if base not in _SCALARS:
        raise SdeoError(f"{where}: the binding has no mapping for the type '{decl.strip()}'")
    return _SCALARS[base]


def parse_header(text: str):
    """({function: (restype, [argtypes])}, {struct: [(field, scalar ctype, array length or None)]}) of a header's text"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    defines = dict(re.findall(r"^\s*#\s*define\s+(\w+)\s+(\d+)\s*$", text, re.M))
    text = re.sub(r"^\s*#.*$|extern\s+\"C\"\s*\{", "", text, flags=re.M)
    struct = r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;"
    structs = {}
    for body, name in re.findall(struct, text, re.S):
        fields = structs[name] = []
        for stmt in filter(str.strip, body.split(";")):                  # `int a, b[8], c`: one type, several declarators
            first = _DECL.fullmatch(stmt.split(",")[0])
            ctype = _ctype(first.group(1), f"struct {name}")
            for m in map(_DECL.fullmatch, stmt[first.end(1):].split(",")):
                fields.append((m.group(2), ctype, None if m.group(3) is None else int(defines.get(m.group(3), m.group(3)))))
    text = re.sub(struct + r"|typedef[^;{]*;|\}", "", text, flags=re.S)   # what is left: prototypes (and extern "C"'s brace)
    protos = {}
    for stmt in filter(str.strip, text.split(";")):
        m = re.fullmatch(r"\s*(.*?)\b(sdeo_\w+)\s*\((.*)\)\s*", stmt, re.S)
        if not m:
            raise SdeoError(f"cannot read the declaration '{' '.join(stmt.split())}'")
        name, params = m.group(2), [] if m.group(3).strip() == "void" else map(_DECL.fullmatch, m.group(3).split(","))
        protos[name] = (_ctype(m.group(1), name), [C.c_void_p if p.group(3) is not None else _ctype(p.group(1), name) for p in params])
    return protos, structs


def prototypes(header: str):
    """{name: (restype, [argtypes])} of every function the header at this path declares"""
    return parse_header(open(header).read())[0]


def header_constant(name: str, header: str = HEADER) -> int:
    """The integer `#define name <digits>` of a header: SDEO_ABI_VERSION, SDEO_MAX_TABLE_STEPS, ... are read, never restated"""
    m = re.search(rf"^\s*#\s*define\s+{re.escape(name)}\s+(\d+)\s*$", open(header).read(), re.M)
    if not m:
        raise SdeoError(f"{header} does not define the integer constant {name}")
    return int(m.group(1))


def declared_symbols(header: str = HEADER):
    """Names of every function include/sdeo.h declares (used by the CPU export test)."""
    return sorted(prototypes(header))


def load(path: str = LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SdeoError(f"{path} not found: build it with `python -m stablediffusioneo_amd.build` "
                        f"(there is no CPU / PyTorch fallback for the HIP path)")
    # Load order: PyTorch ships its own libamdhip64 / libhsa-runtime64 and libsdeo.so is linked against /opt/rocm's.  Whichever
    # is loaded first owns the soname; with libsdeo first, torch ends up with two HSA runtimes in the process and every later
    # HIP call fails with "no ROCm-capable device".  This host uses torch for device memory and streams, so torch goes first.
    import torch  # noqa: F401
    lib = C.CDLL(path)
    missing = []
    for header in (HEADER, INTERNAL_HEADER):
        for name, (restype, argtypes) in prototypes(header).items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
            else:
                missing.append(name)
    if missing:
        raise SdeoError(f"{path} does not export {missing}")
    want = header_constant("SDEO_ABI_VERSION")
    if lib.sdeo_version() != want:
        raise SdeoError(f"{path} reports ABI version {lib.sdeo_version()}, include/sdeo.h declares {want}: rebuild the library "
                        f"(operand semantics changed between versions)")
    _lib = lib
    load_tuned_plans(lib)
    return lib


TUNED_PLANS = os.path.join(HERE, "tuned_plans_gfx950.json")


def load_tuned_plans(lib, path: str = TUNED_PLANS) -> int:
    """Push the committed (tile, split-K) table into the library; returns the number of entries."""
    import json
    env = os.environ.get("SDEO_TUNED_PLANS", "1")      # 0: re-measure everything (tools/tune_plans.py); a path: that table instead
    if env not in ("0", "1"):
        path = env
    if not os.path.exists(path) or env == "0":
        return 0
    rows = json.load(open(path))
    for r in rows:
        lib.sdeo_set_tuned_gemm_plan((C.c_int * 10)(*r[:10]), r[10], r[11])
    return len(rows)


def dump_tuned_plans(lib=None):
    import json
    lib = lib or load()
    return json.loads(lib.sdeo_tuned_gemm_plans_json().decode())


def check(rc: int, what: str = "sdeo"):
    if rc != 0:
        msg = load().sdeo_last_error().decode(errors="replace")
        raise SdeoError(f"{what} failed: {msg}")


def ptr(t):
    """Raw device (or host) pointer of a torch tensor as c_void_p; None -> NULL."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
