"""CPU: the C-ABI shared library loads and exports every entry point include/uc_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uc_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(uc_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_hot_path_entry_points():
    syms = declared_symbols()
    for must in ("uc_rope2d", "uc_layernorm", "uc_gemm", "uc_attention_fwd", "uc_patch_gather", "uc_bilinear_nhwc",
                 "uc_convt_scatter", "uc_pixel_shuffle", "uc_pointmap_adaptor", "uc_conv1x1_to4", "uc_vt_pack"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    from uniception_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in uc_hip.h but not exported: {missing}"
    # the ctypes signature table covers the same set
    assert sorted(list(_lib.SIGNATURES.keys()) + ["uc_last_error", "uc_build_flavor"]) == declared_symbols()
    loaded = _lib.load()
    assert loaded.uc_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define UC_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert loaded.uc_last_error() is not None


def test_shipped_library_is_the_release_build_without_diagnostics():
    """no wrong-result / allocating path is reachable in the shipped library.  The release build says so, its
    sources read the environment in exactly one place (under std::call_once), and the diagnostics names do not even occur in the
    binary's strings."""
    from uniception_amd import _lib

    lib = _lib.load()
    assert lib.uc_build_flavor() == b"release"
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"UC_GEMM_DBG", b"UC_ATTN_DBG", b"UC_GEMM_TRACE"):
        assert name not in blob, f"{name.decode()} is still compiled into the release library"
    assert b"UC_GEMM_GROUP_M" in blob            # (the tuning knobs are there)
    csrc = os.path.join(ROOT, "uniception_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and re.search(r"\bgetenv\s*\(", open(os.path.join(csrc, f)).read())]
    assert users == ["error.hip"], users
    assert "std::call_once" in open(os.path.join(csrc, "error.hip")).read()
    # run-time switchable knobs: validated, round-trip
    import ctypes as C
    v = C.c_int(0)
    assert lib.uc_tuning_get(b"gemm_variant", C.byref(v)) == 0 and v.value == int(os.environ.get("UC_GEMM_VARIANT", "-3"))
    assert lib.uc_tuning_set(b"gemm_variant", 2) == 0 and lib.uc_tuning_get(b"gemm_variant", C.byref(v)) == 0 and v.value == 2
    assert lib.uc_tuning_set(b"gemm_variant", 5) != 0 and b"gemm_variant" in lib.uc_last_error()
    assert lib.uc_tuning_set(b"gemm_dbg", 64) != 0            # diagnostics are not tuning knobs
    assert lib.uc_tuning_set(b"gemm_variant", -3) == 0


def test_release_library_allocates_nothing():
    """VERDICT r3 #6 / SURVEY section 8b: no hipMalloc* is reachable from any uc_* entry point — the release library does not even
    import one (round 3 kept a lazily grown pool of uncached hand-over buffers inside uc_gemm); workspaces are the caller's:
    uc_gemm_desc.fuse_ws (size from uc_gemm_fuse_ws_bytes), uc_attention_fwd_x3's ws."""
    import subprocess
    from uniception_amd import _lib
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    bad = [ln.split()[-1] for ln in und.splitlines() if re.search(r"hip\w*Malloc\w*|hipMemset|hipFree\b|hipHostAlloc", ln)]
    assert not bad, bad
    lib = _lib.load()
    assert lib.uc_gemm_fuse_ws_bytes() == 128 * 128 * 128 * 4 + 128 * 4
    hdr = open(HEADER).read()
    assert "void* fuse_ws;" in hdr and "uc_gemm_fuse_ws_bytes" in hdr


# C type of a descriptor field -> the ctypes types its mirror may declare (pointers of any kind: c_void_p)
_CTYPES = {"int": (ctypes.c_int,), "int64_t": (ctypes.c_int64,), "float": (ctypes.c_float,),
           "unsigned long long": (ctypes.c_ulonglong, ctypes.c_uint64), "*": (ctypes.c_void_p,)}


def header_struct_fields(name):
    """[(field, C type)] of `typedef struct NAME {...} NAME;` in uc_hip.h, pointers as '*'."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"^(?:const\s+)?(void|float|int64_t|int|unsigned long long)\s*(\*?)\s*(.*)$", decl, flags=re.S)
        assert m, f"{name}: unparsed field declaration {decl!r}"
        for n in m.group(3).split(","):
            n = n.strip()
            fields.append((n.lstrip("*").strip(), "*" if m.group(2) or n.startswith("*") else m.group(1)))
    return fields


def check_descriptor_layout(struct, mirror):
    """Field order, names and types of a ctypes mirror == those of the C descriptor (an int64_t stride mirrored as c_int fails)."""
    from uniception_amd import _lib

    fields = header_struct_fields(struct)
    mirrored = getattr(_lib, mirror)._fields_
    assert [n for n, _ in fields] == [n for n, _ in mirrored]
    wrong = [(n, ctype, t.__name__) for (n, ctype), (_, t) in zip(fields, mirrored) if t not in _CTYPES[ctype]]
    assert not wrong, wrong


def test_gemm_descriptor_layout_matches_header():
    """Field order (and types) of the ctypes mirror == those of struct uc_gemm_desc."""
    check_descriptor_layout("uc_gemm_desc", "GemmDesc")


@pytest.mark.parametrize("struct,mirror", [("uc_attention_desc", "AttnDesc"), ("uc_attention_bwd_desc", "AttnBwdDesc"),
                                           ("uc_gemm_tn_desc", "GemmTnDesc")])
def test_attention_descriptor_layout_matches_header(struct, mirror):
    check_descriptor_layout(struct, mirror)


def test_product_path_fails_loudly_without_gpu():
    import torch
    from uniception_amd import ops
    from uniception_amd._lib import UcHipError

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(UcHipError):
        ops.layernorm(torch.zeros(2, 8), torch.ones(8), torch.zeros(8), 1e-6, torch.float32)
    with pytest.raises(RuntimeError):
        ops.rope_2d_(torch.zeros(1, 2, 1, 64), torch.zeros(1, 2, 2, dtype=torch.int64), 100.0, 1.0)


def test_four_wave_gemm_hands_its_accumulators_over_in_untouched_agprs():
    """gemm_bf16_glds4_kernel: the asm K-loop leaves its accumulators in a0..a255 and 256 single-register asm statements read them
    back for the C++ epilogues.  Sound only if the compiler itself never allocates an AGPR in that kernel — checked on the generated
    code of the two instantiations the forward uses (uniception_amd/check_kernels.py); also: the committed loop text is what the generator
    produces."""
    import subprocess
    import sys
    from concurrent.futures import ThreadPoolExecutor
    from uniception_amd import check_kernels as chk
    with ThreadPoolExecutor(4) as ex:       # all four translation units that instantiate the kernel: the default UC_GEMM_4WAVE=3 routes the f32 and 'all' families too
        reports = list(ex.map(chk.check, chk.TUS))
    seen = 0
    for rep in reports:
        for name, (blocks, bad) in rep.items():
            seen += 1
            assert blocks >= 257 and not bad, (name, blocks, bad[:3])
    assert seen == 4
    # the persistent attention kernel: every MFMA through inline asm — no scratch, no spills, no AGPRs in the generated code
    p64 = chk.check_p64()
    assert len(p64) == 2 and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["agprs"] == 0 and 0 < r["vgprs"] <= 256 for r in p64.values()), p64
    # ... and build() runs the same check whenever it links a new library (a violation fails the build)
    from uniception_amd import build as B
    assert open(B.LIB + ".agpr").read().strip() == B.loaded_fingerprint()
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "uniception_amd", "csrc", "gen", "gen_glds4_loop.py")], capture_output=True, text=True, check=True).stdout
    assert gen == open(os.path.join(ROOT, "uniception_amd", "csrc", "gemm_glds4_loop.inc")).read(), "regenerate gemm_glds4_loop.inc"


def test_package_reaches_no_vendor_blas():
    """nothing in the package may compute a matrix product through PyTorch (rocBLAS / hipBLASLt behind `@`, mm, linear,
    einsum ...), not even in one-time weight preparation — every product is a uc_hip kernel or an elementwise pass.  Static check over the
    package sources (tools/ are offline utilities that compare against torch on purpose)."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uniception_amd")
    pat = re.compile(r"(\s@\s|torch\.(mm|matmul|bmm|addmm|einsum|mv|baddbmm)\(|\.(matmul|mm|bmm|mv)\(|F\.linear\(|F\.conv2d\(|F\.scaled_dot_product_attention\()")
    hits = []
    for d, _, files in os.walk(root):
        if os.sep + "tools" in d:
            continue
        for f in files:
            if f.endswith(".py"):
                for i, line in enumerate(open(os.path.join(d, f)), 1):
                    code = line.split("#")[0]
                    if pat.search(code) and not code.lstrip().startswith(('"', "'")):
                        hits.append(f"{os.path.relpath(os.path.join(d, f), root)}:{i}: {line.strip()}")
    assert not hits, hits


def test_attention_descriptors_are_checked_before_any_launch():
    """uc_attention_fwd / uc_attention_bwd reject a bad descriptor with their own message before they touch the device (the pointers
    below are never dereferenced): the fp32 backward has no RoPE form, the bf16 backward only head_dim 64, drop_p lies in [0, 1)."""
    import ctypes as C
    from uniception_amd import _lib

    lib = _lib.load()

    def bwd(**kw):
        d = _lib.AttnBwdDesc(dtype=_lib.UC_F32, B=1, H=1, Nq=8, Nk=8, D=32, scale=1.0)
        for n in ("Q", "K", "V", "O", "dO", "LSE", "dQ", "dK", "dV", "delta"):
            setattr(d, n, 4096)
        for n, v in kw.items():
            setattr(d, n, v)
        return lib.uc_attention_bwd(C.byref(d), None), lib.uc_last_error().decode()

    status, msg = bwd(rope_qpos=4096, rope_kpos=4096, rope_base=100.0, rope_f0=1.0)
    assert status != 0 and msg.startswith("uc_attention_bwd(f32)") and "RoPE" in msg, msg
    status, msg = bwd(dtype=_lib.UC_BF16)
    assert status != 0 and "head_dim must be 64" in msg, msg
    status, msg = bwd(drop_p=1.0)
    assert status != 0 and "drop_p" in msg, msg
    status, msg = bwd(dtype=_lib.UC_F16)
    assert status != 0 and "unsupported dtype" in msg, msg
    d = _lib.AttnDesc(dtype=_lib.UC_F32, B=1, H=1, Nq=8, Nk=8, D=32, Q=4096, K=4096, V=4096, O=4096, scale=1.0, drop_p=-0.5)
    assert lib.uc_attention_fwd(C.byref(d), None) != 0 and lib.uc_last_error().decode().startswith("uc_attention_fwd: drop_p")


def test_single_dtype_entry_points_reject_other_dtype_codes_before_any_launch():
    """Every streaming entry point that takes ONE storage dtype rejects a code outside its set with UC_ERR_BAD_ARG and
    '<fn>: unsupported dtype <d> (...)' before it launches anything: shapes are valid, the pointers are never dereferenced.  The table
    is written out per entry point: which of them take fp16 (UC_F16 = 2) is part of the ABI, not of the dispatch macro.  Decided
    entirely on the host, so it is skipped where a GPU is visible (a dispatch that wrongly accepted a code would launch on these
    pointers)."""
    import torch
    from uniception_amd import _lib

    if torch.cuda.is_available():
        pytest.skip("GPU present: a wrongly accepted code would launch on invalid pointers")
    lib = _lib.load()
    P = 4096                    # 16-byte aligned, never dereferenced
    D = "DTYPE"
    F32_BF16, WITH_F16 = (2, 3, -1), (3, -1)
    table = [
        ("uc_patch_gather", F32_BF16, (P, P, D, 2, 3, 8, 8, 4, None)),                  # 16-byte pixel quads
        ("uc_patch_gather", F32_BF16, (P, P, D, 2, 3, 6, 10, 2, None)),                 # any patch size
        ("uc_bilinear_nhwc", WITH_F16, (P, P, D, 2, 3, 5, 16, 6, 10, 6, 10, None)),     # x2 upsampling (the several-rows form's range)
        ("uc_bilinear_nhwc", WITH_F16, (P, P, D, 2, 6, 10, 16, 3, 5, 3, 5, None)),      # downsampling
        ("uc_convt_scatter", WITH_F16, (P, P, D, 2, 3, 5, 2, 16, None)),
        ("uc_pixel_shuffle", WITH_F16, (P, D, P, 2, 3, 5, 2, 16, None)),
        ("uc_conv1x1_to4", WITH_F16, (P, D, P, P, P, 30, 16, None)),                    # aligned bias: the cooperative form's range
        ("uc_conv1x1_to4", WITH_F16, (P, D, P, P + 4, P, 30, 16, None)),
        ("uc_bilinear_nhwc_bwd", F32_BF16, (P, P, D, 2, 3, 5, 16, 6, 10, 6, 10, None)),
        ("uc_convt_gather", F32_BF16, (P, P, D, 2, 3, 5, 2, 16, None)),
        ("uc_im2col_t", F32_BF16, (P, P, D, 2, 3, 5, 16, 1, 0, 30, None)),
        ("uc_dilate_nhwc", F32_BF16, (P, P, D, 2, 3, 5, 6, 10, 16, 2, None)),
        ("uc_conv1x1_to4_bwd", F32_BF16, (P, D, P, P, P, P, P, 30, 16, 0, None)),
        ("uc_colsum", F32_BF16, (P, D, 30, 16, 16, P, None)),
        ("uc_act_bwd", F32_BF16, (P, P, P, D, _lib.UC_ACT_RELU, 480, None)),
        ("uc_swiglu", F32_BF16, (P, P, D, 30, 16, None)),
        ("uc_swiglu_bwd", F32_BF16, (P, P, P, D, 30, 16, None)),
        ("uc_pixel_unshuffle", F32_BF16, (P, P, D, 2, 3, 5, 2, 16, None)),
        ("uc_token_pool", WITH_F16, (P, D, 16, P, P, 2, 15, 16, None)),
        ("uc_token_pool_bwd", WITH_F16, (P, P, 16, P, 16, D, 2, 15, 16, None)),
    ]
    converted = {"uc_patch_gather", "uc_bilinear_nhwc", "uc_convt_scatter", "uc_pixel_shuffle", "uc_conv1x1_to4", "uc_bilinear_nhwc_bwd",
                 "uc_convt_gather", "uc_im2col_t", "uc_dilate_nhwc", "uc_conv1x1_to4_bwd", "uc_colsum", "uc_act_bwd", "uc_swiglu",
                 "uc_swiglu_bwd", "uc_pixel_unshuffle", "uc_token_pool", "uc_token_pool_bwd"}
    assert {name for name, _, _ in table} == converted
    for name, rejected, args in table:
        assert len(args) == len(_lib.SIGNATURES[name]) and args.count(D) == 1, name
        for code in rejected:
            status = getattr(lib, name)(*[code if a is D else a for a in args])
            msg = lib.uc_last_error().decode()
            assert status != 0 and msg.startswith(name + ":") and f"unsupported dtype {code} " in msg, (name, code, status, msg)
