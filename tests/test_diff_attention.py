"""CPU: the differential attention feature is declared, exported, mirrored and checked before any launch; the new modules carry the
reference's state_dict keys and shapes (tests/golden/diff_attention.npz, written by tests/golden/make_golden_diff_attention.py); the
geometry outside the kernels (Q/K head_dim 64 with V head_dim 128) raises the documented error."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.golden.diff_cases import CASES, KEY_ONLY, resolve
from tests.helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uc_diff_attention_fwd", "uc_diff_attention_combine_bwd", "uc_diff_attention_combine_ws_bytes")


def _lib_or_build():
    from uniception_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib, _lib.load()


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uc_hip.h")).read(), flags=re.S)
    _lib, lib = _lib_or_build()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/uc_hip.h"
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.uc_abi_version() >= 17
    assert lib.uc_diff_attention_combine_ws_bytes(1) > 0


def test_descriptor_mirror_matches_header():
    from tests.test_abi import check_descriptor_layout
    check_descriptor_layout("uc_diff_attention_desc", "DiffAttnDesc")


def _desc(_lib, **kw):
    d = _lib.DiffAttnDesc(dtype=_lib.UC_BF16, v_layout=_lib.UC_V_PACKED_T, B=1, H=2, Nq=64, Nk=64, Dqk=32, scale=1.0, lambda_full=0.5,
                          rms_eps=1e-5, out_scale=0.5)
    for n in ("Q", "K", "V", "O", "subln_w"):       # never dereferenced: every call below is rejected before any launch
        setattr(d, n, 4096)
    d.q_sb, d.q_sn, d.q_sh = 64 * 128, 128, 32
    d.k_sb, d.k_sn, d.k_sh = 64 * 128, 128, 32
    d.o_sb, d.o_sn, d.o_sh = 64 * 128, 128, 64
    for n, v in kw.items():
        setattr(d, n, v)
    return d


@pytest.mark.parametrize("kw,needle", [
    (dict(dtype=2), "unsupported dtype 2"),
    (dict(Dqk=64), "Q/K head_dim 64 with V head_dim 128 is not supported"),
    (dict(q_sn=129), "Q/K strides must be multiples of 8"),
    (dict(k_sh=36), "Q/K strides must be multiples of 8"),
    (dict(training=1), "training needs the four saves"),
    (dict(training=1, lse1=4096, lse2=4096, A1=4096), "training needs the four saves"),
    (dict(lse1=4096), "come together or not at all"),
    (dict(v_layout=0), "packed VT layout"),
    (dict(dtype=0, v_layout=0, Dqk=18), "multiple of 4"),
    (dict(Q=None), "null pointer"),
])
def test_forward_descriptor_is_checked_before_any_launch(kw, needle):
    _lib, lib = _lib_or_build()
    status = lib.uc_diff_attention_fwd(C.byref(_desc(_lib, **kw)), None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith("uc_diff_attention_fwd") and needle in msg, msg


def test_combine_backward_arguments_are_checked_before_any_launch():
    _lib, lib = _lib_or_build()
    p = 4096

    def call(dtype=0, D=64, dw=p):
        st = lib.uc_diff_attention_combine_bwd(p, p, p, p, p, p, dw, p, p, dtype, 1, 8, 2, D, 1024, 128, 64, 0.5, 1e-5, 0.5, None)
        return st, lib.uc_last_error().decode()

    for kw, needle in ((dict(dtype=2), "unsupported dtype"), (dict(D=128), "at most 64"), (dict(D=30), "multiple of 4"), (dict(dw=None), "null pointer")):
        st, msg = call(**kw)
        assert st != 0 and msg.startswith("uc_diff_attention_combine_bwd") and needle in msg, msg


def _build(kind, kw):
    from uniception_amd.models import info_sharing
    from uniception_amd.models.libs.croco.pos_embed import RoPE2D
    from uniception_amd.models.utils import transformer_blocks as TB
    cls = getattr(TB, kind, None) or getattr(info_sharing, kind)
    return cls(**resolve(kw, RoPE2D))


@pytest.mark.parametrize("name", list(CASES) + list(KEY_ONLY))
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    kind, kw = (CASES.get(name) or KEY_ONLY[name])
    gold = np.load(os.path.join(GOLDEN_DIR, "diff_attention.npz"))
    want = str(gold[f"{name}/keys"]).split("\n")
    got = [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in _build(kind, kw).state_dict().items()]
    assert got == want


def test_rmsnorm_and_lambda_init_follow_the_reference():
    from uniception_amd.models.utils.transformer_blocks import RMSNorm, lambda_init_fn
    assert lambda_init_fn(0) == pytest.approx(0.2) and lambda_init_fn(3) == pytest.approx(0.8 - 0.6 * np.exp(-0.9))
    n = RMSNorm(8, eps=1e-5)
    x = torch.arange(16.0).view(2, 8)
    torch.testing.assert_close(n(x), x / (x.pow(2).mean(-1, keepdim=True) + 1e-5).sqrt())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_head_dim_64_raises_the_documented_error(mode):
    """dim 768 with 12 heads (the reference's default): the differential layer has Q/K head_dim 64 and V head_dim 128.  Construction
    works (the state_dict loads); calling it raises UcHipError naming the head dims — before any tensor is touched, so also without a GPU."""
    from uniception_amd import engine
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.utils.transformer_blocks import DiffCrossAttention, DiffCrossAttentionBlock
    layer = DiffCrossAttention(dim=768, depth=0, num_heads=6)
    block = DiffCrossAttentionBlock(dim=768, depth=0, num_heads=6)
    x = torch.zeros(1, 4, 768)
    with engine.precision(mode), torch.no_grad():
        for call in (lambda: layer(x, x, x), lambda: block(x, x)):
            with pytest.raises(UcHipError, match=r"Q/K head_dim 64 and V head_dim 128 is not supported.*head_dim-128"):
                call()


def test_unsupported_options_name_themselves():
    from uniception_amd import engine
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.utils.transformer_blocks import DiffAttention
    x = torch.zeros(1, 4, 192)
    with engine.precision("fp32"), torch.no_grad():
        with pytest.raises(UcHipError, match="qk_norm"):
            DiffAttention(dim=192, depth=0, num_heads=3, qk_norm=True)(x)
        with pytest.raises(UcHipError, match="attn_drop"):
            DiffAttention(dim=192, depth=0, num_heads=3, attn_drop=0.1).train()(x)
