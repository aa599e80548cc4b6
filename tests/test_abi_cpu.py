"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports exactly what include/sdeo.h and
csrc/sdeo_internal.h declare, and the ctypes binding is typed from those two headers (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

from stablediffusioneo_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_exports_every_declared_symbol(lib):
    names = _lib.declared_symbols()
    assert len(names) >= 25 and "sdeo_groupnorm_nhwc_f16" in names and "sdeo_unet_forward" in names
    for n in names:
        assert hasattr(lib, n), n


def test_version_and_error_string(lib):
    assert lib.sdeo_version() == 101          # include/sdeo.h SDEO_ABI_VERSION; _lib.load() refuses a library that disagrees with the header
    assert isinstance(lib.sdeo_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    """Shape validation runs on the host before any launch, so it is testable without a device."""
    rc = lib.sdeo_layernorm_f16(None, None, None, None, ctypes.c_int(4), ctypes.c_int(64), ctypes.c_float(1e-5), None)
    assert rc != 0 and b"layernorm" in lib.sdeo_last_error()
    rc = lib.sdeo_attention_f16(ctypes.c_void_p(16), 64, ctypes.c_void_p(16), 64, ctypes.c_void_p(16), 64, ctypes.c_void_p(16),
                                64, 1, 1, 8, 8, 8, 8, 12, ctypes.c_float(1.0), None)
    assert rc != 0 and b"head dim" in lib.sdeo_last_error()


def _declared():
    """{name: (restype, [argtypes])} of both headers, parsed independently of load()"""
    return {**_lib.prototypes(_lib.HEADER), **_lib.prototypes(_lib.INTERNAL_HEADER)}


def test_every_declared_function_is_typed(lib):
    protos = _declared()
    assert len(protos) >= 100
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read() + open(_lib.INTERNAL_HEADER).read(), flags=re.S)
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text).group(1)          # counted without the parser
        assert len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    # const char* sdeo_last_error(void);
    assert lib.sdeo_last_error.restype is ctypes.c_char_p and list(lib.sdeo_last_error.argtypes) == []
    # size_t sdeo_gemm_workspace_bytes(int m, int n, int k);
    assert lib.sdeo_gemm_workspace_bytes.restype is ctypes.c_size_t and list(lib.sdeo_gemm_workspace_bytes.argtypes) == [I, I, I]
    # int sdeo_cfg_ddim_step(float* x_prev, float* pred_x0, const float* x, const float* eps_c, const float* eps_u, const float* noise,
    #                        float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, int64_t n, void* stream);
    assert lib.sdeo_cfg_ddim_step.restype is I and list(lib.sdeo_cfg_ddim_step.argtypes) == [V] * 6 + [F] * 5 + [ctypes.c_int64, V]
    # int sdeo_weight_info(sdeo_handle h, int i, const char** name, int64_t dims[4], int* ndim);
    assert list(lib.sdeo_weight_info.argtypes) == [V, I, V, V, V]
    # const char* sdeo_debug_attention_kernel_name(int B, int H, int Tq, int Tk, int d, int causal);
    assert lib.sdeo_debug_attention_kernel_name.restype is ctypes.c_char_p and list(lib.sdeo_debug_attention_kernel_name.argtypes) == [I] * 6
    # two long prototypes, their parameters counted by hand in the header
    assert len(lib.sdeo_conv2d_nhwc_f16.argtypes) == 19 and len(lib.sdeo_debug_conv2d_gn_f16.argtypes) == 23


def test_nothing_exported_is_undeclared():
    """The defined dynamic function symbols `sdeo_*` of the built library are exactly the functions the two headers declare."""
    path = build.build(verbose=False)
    rocm = os.path.dirname(os.path.dirname(build.HIPCC))
    tools = [t for t in (os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf"), os.path.join(rocm, "llvm", "bin", "llvm-readelf"))
             if os.path.exists(t)]
    assert tools, f"no llvm-readelf below {rocm} (the tree of the hipcc that built the library)"
    out = subprocess.run([tools[0], "--dyn-syms", "--wide", path], capture_output=True, text=True, check=True).stdout
    exported = set()
    for line in out.splitlines():          # Num: Value Size Type Bind Vis Ndx Name
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND" and f[7].startswith("sdeo_"):
            exported.add(f[7].split("@")[0])
    declared = set(_declared())
    assert exported - declared == set(), "exported but declared in neither header"
    assert declared - exported == set(), "declared but not exported"


@pytest.mark.parametrize("text, culprit", [
    ("int sdeo_ok(int a);\nint sdeo_takes_double(void* y, double eps, void* stream);", "sdeo_takes_double"),
    ("typedef struct sdeo_pair { int a, b; } sdeo_pair;\nint sdeo_takes_struct(sdeo_pair p, void* stream);", "sdeo_takes_struct"),
    ("double sdeo_returns_double(void);", "sdeo_returns_double"),
])
def test_parser_refuses_unknown_types(text, culprit):
    with pytest.raises(_lib.SdeoError, match=culprit):
        _lib.parse_header(text)


def test_parser_reads_the_closed_vocabulary():
    protos, structs = _lib.parse_header("""
        /* a comment with sdeo_not_a_function(int) in it */
        #define SDEO_MAX_LEVELS 8
        typedef struct sdeo_x_s* sdeo_x_handle;
        typedef struct sdeo_s { int a, mult[SDEO_MAX_LEVELS], n; float f; int fixed[4]; } sdeo_s;
        const char* sdeo_a(void);
        void sdeo_b(sdeo_x_handle h, const sdeo_s* cfg, const char* name, const char** out, int64_t dims[4], size_t n, int32_t i,
                    unsigned long long* stamps, float* const* outs, float scale);
    """)
    V = ctypes.c_void_p
    assert protos == {"sdeo_a": (ctypes.c_char_p, []),
                      "sdeo_b": (None, [V, V, ctypes.c_char_p, V, V, ctypes.c_size_t, ctypes.c_int32, V, V, ctypes.c_float])}
    assert structs == {"sdeo_s": [("a", ctypes.c_int, None), ("mult", ctypes.c_int, 8), ("n", ctypes.c_int, None),
                                  ("f", ctypes.c_float, None), ("fixed", ctypes.c_int, 4)]}


@pytest.mark.parametrize("mirror, struct", [(_lib.SdeoConfig, "sdeo_config"), (_lib.SdeoConfigExt, "sdeo_config_ext"),
                                            (_lib.SdeoClipConfig, "sdeo_clip_config")])
def test_struct_mirrors_match_the_header(mirror, struct):
    fields = _lib.parse_header(open(_lib.HEADER).read())[1][struct]
    assert len(fields) >= 3
    assert list(mirror._fields_) == [(name, ctype if length is None else ctype * length) for name, ctype, length in fields]


def test_wrong_arguments_fail_in_python(lib):
    with pytest.raises(ctypes.ArgumentError):
        lib.sdeo_layernorm_f16(None, None, None, None, 4, "64", 1e-5, None)
    with pytest.raises(TypeError):
        lib.sdeo_layernorm_f16(None, None, None, None, 4, 64, 1e-5)


def test_product_path_has_no_oracle_import():
    """The oracle is test infrastructure: nothing under stablediffusioneo_amd/ may import it."""
    import os
    import re
    root = os.path.dirname(os.path.abspath(_lib.__file__))
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(dp, f)
