"""Tensor-level wrappers over the C ABI (include/uc_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every function below
hands raw device pointers + sizes/strides to libuc_hip.so.  Nothing in this module computes with
torch ops, and nothing falls back to the CPU: tensors must live on a HIP device.
"""
import ctypes as C
import weakref
from typing import Optional, Tuple

import contextlib

import torch

from . import _lib
from ._lib import (AttnBwdDesc, AttnDesc, DiffAttnDesc, GemmDesc, GemmTnDesc, UC_A_CONV3X3, UC_A_DENSE, UC_ACT_GELU_ERF, UC_ACT_NONE, UC_ACT_RELU,
                   UC_BF16, UC_F16, UC_F32, UC_V_PACKED_T, UC_V_ROWMAJOR, UcHipError)

_DT = {torch.float32: UC_F32, torch.bfloat16: UC_BF16, torch.float16: UC_F16}
ACT = {None: UC_ACT_NONE, "none": UC_ACT_NONE, "gelu": UC_ACT_GELU_ERF, "relu": UC_ACT_RELU}


def _dt(t: torch.dtype) -> int:
    try:
        return _DT[t]
    except KeyError:
        raise UcHipError(f"dtype {t} is not supported by the HIP kernels")


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise UcHipError(
                "uniception_amd kernels run on a HIP device only (got a CPU tensor); there is no CPU fallback. "
                "Use the reference implementation or oracle/ for CPU execution."
            )


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def tuning_set(name: str, value: int) -> None:
    """Run-time switchable tuning knobs of libuc_hip.so (uc_tuning_set): "gemm_variant" (-3 automatic, -1 register-staged kernel,
    0..3 / 6 / 7 tile variants of the direct-to-LDS bf16 GEMM), "gemm_stagger" (-1 launcher policy), "attn_role_split", "attn_p64" (persistent 64-queries-per-wave attention forward: 0 never, 1 policy, 2 wherever the shape allows), "attn_bwd64" (64-rows-per-wave attention backward kernels: 0 never, 1 policy, 2 wherever the shape allows; bitwise the same results), "conv_rows" (row-walking 3x3
    conv kernels: 0 never, 1 where they win, 2 the 256-pixel one wherever the shape allows, 3 the eight-wave 512-pixel one wherever the shape allows), "conv_rows_flat" (1: the eight-wave kernel's flat form also takes maps whose rows do not tile 512 pixels; 0: those stay on the implicit-GEMM kernel), "small_m_split" (smallest K for which a dense launch on at most half
    the CUs splits K in two inside the kernel; 0: never — results are then bit-identical across batch sizes).  Every value selects a correct
    kernel; everything else the library reads from the environment, once (csrc/knobs.h)."""
    _lib.check(_lib.load().uc_tuning_set(name.encode(), int(value)), f"uc_tuning_set({name})")
    if name == "small_m_split":
        _small_m_cache[0] = int(value)


def tuning_get(name: str) -> int:
    import ctypes
    v = ctypes.c_int(0)
    _lib.check(_lib.load().uc_tuning_get(name.encode(), ctypes.byref(v)), f"uc_tuning_get({name})")
    return v.value


@contextlib.contextmanager
def tuning(name: str, value: int):
    "Scoped tuning_set (tests, micro-benchmarks: run one tile variant, then restore)."
    prev = tuning_get(name)
    tuning_set(name, value)
    try:
        yield
    finally:
        tuning_set(name, prev)


# --------------------------------------------------------------------------------------------
def rope_2d_(tokens: torch.Tensor, positions: torch.Tensor, base: float, fwd: float) -> None:
    """In-place RoPE-2D on tokens [B,N,H,D] (any strides with stride(3)==1); positions [B,N,2] int64.
    Same contract as curope.rope_2d (curope.cpp:49-69)."""
    if tokens.dim() != 4:
        raise RuntimeError("tokens must have 4 dimensions")
    if positions.dim() != 3:
        raise RuntimeError("positions must have 3 dimensions")
    if tokens.size(0) != positions.size(0):
        raise RuntimeError("batch size differs between tokens & positions")
    if tokens.size(1) != positions.size(1):
        raise RuntimeError("seq_length differs between tokens & positions")
    if positions.size(2) != 2:
        raise RuntimeError("positions.shape[2] must be equal to 2")
    if tokens.is_cuda != positions.is_cuda:
        raise RuntimeError("tokens and positions are not on the same device")
    _need_gpu(tokens, positions)
    if tokens.stride(3) != 1:
        raise RuntimeError("tokens are not contiguous in the last dimension")
    if positions.dtype != torch.int64 or not positions.is_contiguous():
        raise RuntimeError("positions must be a contiguous int64 tensor")
    B, N, H, D = tokens.shape
    lib = _lib.load()
    _lib.check(lib.uc_rope2d(tokens.data_ptr(), positions.data_ptr(), B, N, H, D, tokens.stride(0), tokens.stride(1),
                             tokens.stride(2), float(base), float(fwd), _dt(tokens.dtype), _stream()), "uc_rope2d")


def rope_axial_(q: torch.Tensor, k: Optional[torch.Tensor], table_y: torch.Tensor, table_x: torch.Tensor, prefix: int, grid_h: int,
                grid_w: int, inverse: bool = False) -> None:
    """In-place axial RoPE (DINOv3: uc_rope_axial) of q [B,N,H,D] and, when given, k of the same shape — views with stride(3) == 1, e.g.
    the q | k slices of a packed [B,N,3,H,D] projection, which are rotated in ONE launch (k lies a constant offset behind q with the same
    strides; anything else takes one launch per operand).  N == prefix + grid_h * grid_w; the first `prefix` tokens stay as they are.
    table_y [grid_h, D/4, 2], table_x [grid_w, D/4, 2]: fp32 (cos, sin).  inverse: the rotation by the negated angle (gradients)."""
    _need_gpu(q, k, table_y, table_x)
    if q.dim() != 4 or q.stride(3) != 1:
        raise UcHipError("rope_axial_: tokens must be a [B, N, H, D] view with a contiguous last dimension")
    B, N, H, D = q.shape
    for t, n in ((table_y, grid_h), (table_x, grid_w)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (n, D // 4, 2):
            raise UcHipError(f"rope_axial_: a table must be a contiguous fp32 [{n}, {D // 4}, 2] tensor, got {t.dtype} {tuple(t.shape)}")
    lib = _lib.load()

    def run(t, parts, sp):
        _lib.check(lib.uc_rope_axial(t.data_ptr(), B, N, H, D, t.stride(0), t.stride(1), t.stride(2), parts, sp, prefix, grid_h, grid_w,
                                     table_y.data_ptr(), table_x.data_ptr(), int(bool(inverse)), _dt(t.dtype), _stream()), "uc_rope_axial")
    if k is None:
        return run(q, 1, 0)
    if k.shape != q.shape or k.dtype != q.dtype or k.stride(3) != 1:
        raise UcHipError("rope_axial_: q and k must have the same shape and dtype")
    off = k.data_ptr() - q.data_ptr()
    if k.stride() == q.stride() and off > 0 and off % q.element_size() == 0:
        return run(q, 2, off // q.element_size())
    run(q, 1, 0)
    run(k, 1, 0)


_rope_tables = {}


def rope_table(device, npos: int, base: float, F0: float = 1.0) -> torch.Tensor:
    """[npos,16,2] fp32 cos/sin table for the fused GEMM epilogue (head_dim 64 -> Q=16); cached per device."""
    npos = max(64, (npos + 63) // 64 * 64)
    key = (device.index if device.index is not None else torch.cuda.current_device(), npos, float(base), float(F0))
    t = _rope_tables.get(key)
    if t is None:
        t = torch.empty(npos, 16, 2, dtype=torch.float32, device=device)
        _lib.check(_lib.load().uc_rope_table(t.data_ptr(), npos, 16, float(base), float(F0), _stream()), "uc_rope_table")
        t.uc_rope_base, t.uc_rope_f0 = float(base), float(F0)   # travel with the table into uc_gemm's descriptor
        from .engine import BuiltOn
        t.uc_built = BuiltOn()
        _rope_tables[key] = t
    else:
        t.uc_built.sync()       # a consumer on another stream waits for the stream that filled the table
    return t


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, out_dtype: torch.dtype,
              twin: bool = False) -> torch.Tensor:
    """x [..., C] contiguous (fp32|bf16) -> same shape in out_dtype.  twin: a bf16 copy of the result is written in the same
    pass and rides on the returned tensor as ``y.uc_twin`` (for consumers that take bf16 operands)."""
    _need_gpu(x, weight, bias)
    assert x.is_contiguous() and weight.dtype == torch.float32 and bias.dtype == torch.float32
    Cn = x.shape[-1]
    rows = x.numel() // Cn
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    tw = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if twin else None
    _lib.check(_lib.load().uc_layernorm_twin(x.data_ptr(), _dt(x.dtype), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                             _dt(out_dtype), _p(tw), rows, Cn, float(eps), _stream()), "uc_layernorm")
    if twin:
        y.uc_twin = tw
    return y


# ---------------------------------------------------------------------------------------------
# Hand-over buffers of uc_gemm's small-M path (uc_gemm_desc.fuse_ws, ABI 11): the library allocates nothing, the HOST does.
# A buffer is uc_gemm_fuse_ws_bytes() (8 MiB) of UNCACHED device memory — the two halves of a split tile may run on different
# XCDs, whose L2s are not coherent; PyTorch's allocator has no such flavour, so the HIP runtime is called directly (ctypes on the
# libamdhip64 the process already has) — zero-filled once, used by one launch at a time: one per (device, stream), and one per
# (device, stream, graph) for launches recorded into a hipGraph (its replays may overlap eager launches on the same stream handle).
# Allocation is not allowed while a stream is capturing: captures draw from a reserve filled beforehand (fuse_ws_reserve, called by
# graphs.GraphedTwoView); an empty reserve means the launch runs unsplit (uc_gemm's documented behaviour without a buffer).
# ---------------------------------------------------------------------------------------------
_HIP_MALLOC_UNCACHED = 0x3      # hipDeviceMallocUncached
_hip_rt = None
_fuse_ws_sets = {}              # (device, stream handle, capture token | 0) -> device pointer
_fuse_ws_free = {}              # device -> [device pointers not handed out]
_capture_token = 0              # set by capture_scope(): identifies the graph being recorded


def _hip_runtime():
    "The HIP runtime library this process has loaded (PyTorch's): hipExtMallocWithFlags / hipMemset / hipFree."
    global _hip_rt
    if _hip_rt is None:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        _hip_rt = C.CDLL(path or "libamdhip64.so")
        _hip_rt.hipExtMallocWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        _hip_rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        _hip_rt.hipFree.argtypes = [C.c_void_p]
    return _hip_rt


def _fuse_ws_new(device_index: int) -> Optional[int]:
    hip = _hip_runtime()
    nbytes = int(_lib.load().uc_gemm_fuse_ws_bytes())
    ptr = C.c_void_p()
    with torch.cuda.device(device_index):
        if hip.hipExtMallocWithFlags(C.byref(ptr), nbytes, _HIP_MALLOC_UNCACHED) != 0 or not ptr.value:
            return None
        if hip.hipMemset(ptr, 0, nbytes) != 0:        # (synchronous; the flag words must start at zero)
            hip.hipFree(ptr)
            return None
    return ptr.value


def fuse_ws_reserve(n: int = 4, device=None) -> None:
    """Make sure n hand-over buffers are ready to be handed to streams (call OUTSIDE a stream capture, e.g. before recording a graph
    whose small-M launches should split)."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    free = _fuse_ws_free.setdefault(dev, [])
    while len(free) < n:
        ptr = _fuse_ws_new(dev)
        if ptr is None:
            break
        free.append(ptr)


def fuse_ws_release(token: int) -> None:
    "Return the buffers of a destroyed graph (capture token) to the reserve."
    for key in [k for k in _fuse_ws_sets if k[2] == token and token != 0]:
        _fuse_ws_free.setdefault(key[0], []).append(_fuse_ws_sets.pop(key))


def fuse_ws_free_all() -> None:
    "hipFree every hand-over buffer (only when no launch that uses one can still be in flight: synchronizes first)."
    torch.cuda.synchronize()
    hip = _hip_runtime()
    for ptr in list(_fuse_ws_sets.values()) + [p for v in _fuse_ws_free.values() for p in v]:
        hip.hipFree(C.c_void_p(ptr))
    _fuse_ws_sets.clear()
    _fuse_ws_free.clear()


@contextlib.contextmanager
def capture_scope(token: int):
    "Launches recorded inside belong to the graph identified by `token` (their hand-over buffers live as long as it does)."
    global _capture_token
    prev = _capture_token
    _capture_token = token
    try:
        yield
    finally:
        _capture_token = prev


def _fuse_ws_for_launch(M: int, N: int, K: int) -> Optional[int]:
    """The buffer a dense bf16 launch of this shape may use for the in-kernel K split (None: it runs unsplit).  Only shapes uc_gemm
    can split get one (at most 128 tiles of 128 x 128 on at most half the CUs, K at least the small_m_split knob)."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles > 128 or K % 128 != 0:
        return None
    smk = _small_m_k()
    if smk <= 0 or K < smk or 2 * tiles > _num_cus():
        return None
    dev = torch.cuda.current_device()
    capturing = torch.cuda.is_current_stream_capturing()
    # a captured launch belongs to its GRAPH, not to the stream it was recorded on (PyTorch records every graph on a capture stream, and
    # two graphs may be replayed at the same time on different streams): keyed by the capture_scope token, else by the capture's own id
    token = 0
    if capturing:
        if not _capture_token:
            # a capture outside ops.capture_scope has no owner to hand the buffer back when the graph dies (every such graph would
            # keep 8 MiB for good, and once the reserve is drained later captures would silently run unsplit): it runs unsplit,
            # always — wrap captures in ops.capture_scope(token) + fuse_ws_release(token) (uniception_amd.graphs does)
            return None
        token = _capture_token
    key = (dev, _stream(), token)
    ptr = _fuse_ws_sets.get(key)
    if ptr is None:
        free = _fuse_ws_free.setdefault(dev, [])
        if not capturing and len(free) < _FUSE_WS_SPARE + 1:
            fuse_ws_reserve(_FUSE_WS_SPARE + 1, dev)      # this one + spares for the streams a later capture brings along
        if not free:
            return None
        ptr = free.pop()
        _fuse_ws_sets[key] = ptr
    return ptr


_FUSE_WS_SPARE = 3


_small_m_cache = [None]
_num_cus_cache = {}


def _small_m_k() -> int:
    if _small_m_cache[0] is None:
        _small_m_cache[0] = tuning_get("small_m_split")
    return _small_m_cache[0]


def _num_cus() -> int:
    dev = torch.cuda.current_device()
    if dev not in _num_cus_cache:
        _num_cus_cache[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _num_cus_cache[dev]


# ---------------------------------------------------------------------------------------------
# fp16 range guard (TF32-class heads): every launch that can push a value out of fp16's range (GEMM / conv epilogues with fp16
# outputs, conversions into fp16) saturates at +-65504 and ORs 1 into this per-device int32 — the engine polls it (engine.
# head_range_exceeded) and falls back to a wider head format.
# ---------------------------------------------------------------------------------------------
_f16_sat_flags = {}


def f16_sat_flag() -> torch.Tensor:
    dev = torch.cuda.current_device()
    t = _f16_sat_flags.get(dev)
    if t is None:
        t = _f16_sat_flags[dev] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", dev))
    return t


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
         residual: Optional[torch.Tensor] = None, residual2: Optional[torch.Tensor] = None,
         out_dtype: Optional[torch.dtype] = None,
         out: Optional[torch.Tensor] = None, relu_a: bool = False,
         rope: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
         vt: Optional[Tuple[int, torch.Tensor, int]] = None,
         conv: Optional[Tuple[int, int, int, int, int]] = None, preact_out: Optional[torch.Tensor] = None,
         split_k: int = 1, dact: Optional[Tuple[torch.Tensor, str]] = None,
         ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, emit_ln: bool = False,
         tail: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None) -> torch.Tensor:
    """C[M,N] = epilogue(A . W^T).

    a    : dense [M,K] (row stride a.stride(0), unit column stride) or, with conv=(B,H,W,Cin,stride), an NHWC image.
    w    : [N,K] contiguous, same dtype as a (fp32 -> exact fp32 kernel, bf16 -> MFMA kernel).
    rope : (positions [M,2] int64, table, rope_cols) -> fused RoPE-2D on the first rope_cols columns (bf16 only).
    vt   : (vt_col0, vt_out [B,H,64,Npad] bf16, ntok) -> V columns written in the packed VT layout (bf16 only).
    ln   : (stats [M,2] fp32 (mean, rstd), colsum [N] fp32) -> folded LayerNorm: a holds the RAW rows, w has gamma folded in,
           the epilogue computes rstd * (acc - mean * colsum) + bias (bf16 output only).
    tail : (w4 [4,N] fp32, b4 [4] fp32 | None) with N == 128 on a 3x3 convolution — the [M,128] result is not stored; returns
           fp32 [M,4] = b4 + act(acc + bias) . w4^T (the DPT regressor's conv3x3 -> ReLU -> conv1x1(128 -> 4) in one kernel).
    emit_ln : also write per-row 64-column-block statistics and, for an fp32 output, a bf16 twin of it (a bf16 output — the bf16
           residual stream — is its own twin); they ride on the returned tensor as ``out.uc_ln`` (an LnSide: twin, partial,
           finalized-stats cache) for the consumer's ``ln=``.
    """
    _need_gpu(a, w, bias, residual)
    assert a.dtype == w.dtype and w.is_contiguous() and w.dim() == 2
    cd = _dt(a.dtype)
    N, K = w.shape
    if (cd == UC_F32 and fp32_matmul_hook() == "bf16x3" and rope is None and vt is None and preact_out is None
            and (split_k <= 1 or (conv is None and bias is None and act in (None, "none") and residual is None and not relu_a))
            and dact is None and ln is None and not emit_ln and (K // (9 if conv is not None else 1)) % 8 == 0 and a.is_contiguous()):
        # fp32-class product on the bf16 matrix pipe: [hi | hi | lo] rows against [Wh | Wl | Wh] weights (uc_split_bf16x3)
        # (split_k > 1, round 6: the weight gradients of the fp32-class heads — a handful of output tiles, millions of reduction steps —
        #  return fp32 slabs [split_k, M, N] like the bf16 path's)
        a3 = split_bf16x3(a, relu=relu_a)
        conv3 = None if conv is None else (conv[0], conv[1], conv[2], 3 * conv[3], conv[4])
        return gemm(a3, split_weight_bf16x3(w, 9 if conv is not None else 1), bias, act=act, residual=residual, residual2=residual2,
                    out_dtype=out_dtype or torch.float32, out=out, conv=conv3, tail=tail, split_k=split_k)
    d = GemmDesc()
    d.compute_dtype = cd
    d.relu_a = 1 if relu_a else 0
    d.A, d.W = a.data_ptr(), w.data_ptr()
    if conv is None:
        assert a.dim() == 2 and a.stride(1) == 1 and a.shape[1] == K
        M = a.shape[0]
        d.a_mode, d.lda = UC_A_DENSE, a.stride(0)
    else:
        Bc, Hc, Wc, Cin, s = conv
        assert a.is_contiguous() and a.numel() == Bc * Hc * Wc * Cin and K == 9 * Cin
        Ho, Wo = (Hc - 1) // s + 1, (Wc - 1) // s + 1
        M = Bc * Ho * Wo
        d.a_mode, d.lda = UC_A_CONV3X3, 0
        d.conv_B, d.conv_H, d.conv_W, d.conv_Cin, d.conv_stride, d.conv_Ho, d.conv_Wo = Bc, Hc, Wc, Cin, s, Ho, Wo
    d.M, d.N, d.K = M, N, K
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N
    d.bias = _p(bias)
    d.act = ACT[act]
    if residual is not None:
        assert residual.dim() == 2 and residual.stride(1) == 1 and residual.shape == (M, N)
        d.residual, d.res_dtype, d.ldr = residual.data_ptr(), _dt(residual.dtype), residual.stride(0)
        if residual2 is not None:
            assert residual2.shape == residual.shape and residual2.stride() == residual.stride() and residual2.dtype == residual.dtype
            d.residual2 = residual2.data_ptr()
    n_out = N
    d.vt_col0 = -1
    if vt is not None:
        vt_col0, vt_out, ntok = vt
        assert vt_out.dtype == torch.bfloat16 and vt_out.is_contiguous()
        d.vt_col0, d.vt_out, d.vt_ntok, d.vt_npad = vt_col0, vt_out.data_ptr(), ntok, vt_out.shape[-1]
        n_out = vt_col0
    if rope is not None:
        pos, table, rope_cols = rope
        assert pos.dtype == torch.int64 and pos.is_contiguous() and pos.numel() == 2 * M
        d.rope_cols, d.rope_pos, d.rope_table, d.rope_npos = rope_cols, pos.data_ptr(), table.data_ptr(), table.shape[0]
        d.rope_base, d.rope_f0 = table.uc_rope_base, table.uc_rope_f0
    if tail is not None:
        w4, b4 = tail
        assert conv is not None and N == 128 and out is None and residual is None and rope is None and vt is None and split_k <= 1
        assert w4.dtype == torch.float32 and w4.is_contiguous() and w4.shape == (4, N)
        assert b4 is None or (b4.dtype == torch.float32 and b4.is_contiguous() and b4.numel() == 4)
        out4 = torch.empty((M, 4), dtype=torch.float32, device=a.device)
        d.tail_w, d.tail_b, d.tail_out = w4.data_ptr(), _p(b4), out4.data_ptr()
        d.C, d.out_dtype, d.ldc = None, (UC_F16 if cd == UC_F16 else UC_BF16), N      # (nothing is stored: the storage dtype of the operands)
        if cd == UC_F16:
            d.sat_flag = _p(f16_sat_flag())
        _lib.check(_lib.load().uc_gemm(C.byref(d), _stream()), "uc_gemm")
        return out4
    if out is None and split_k > 1:
        out = torch.empty((split_k, M, N), dtype=torch.float32, device=a.device)
        d.C, d.out_dtype, d.ldc = out.data_ptr(), _dt(out.dtype), N
    elif out is None:
        out = torch.empty((M, n_out), dtype=out_dtype or a.dtype, device=a.device)
    elif split_k > 1:   # workspace of split_k [M,N] fp32 slabs
        assert out.shape == (split_k, M, N) and out.is_contiguous() and out.dtype == torch.float32
        d.C, d.out_dtype, d.ldc = out.data_ptr(), _dt(out.dtype), N
    else:
        assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == M and out.shape[1] >= n_out
    if split_k <= 1 or out.dim() == 2:
        d.C, d.out_dtype, d.ldc = out.data_ptr(), _dt(out.dtype), out.stride(0)
    if preact_out is not None:
        assert preact_out.shape == out.shape and preact_out.stride() == out.stride() and preact_out.dtype == out.dtype
        d.preact_out = preact_out.data_ptr()
    d.split_k = int(split_k)
    if dact is not None:   # fused activation backward: out *= act'(u)
        u, act_name = dact
        assert u.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and u.shape == out.shape and u.stride() == out.stride()
        d.dact_u, d.dact_act = u.data_ptr(), ACT[act_name]
    if ln is not None:
        st, cs = ln
        assert cs.dtype == torch.float32 and cs.is_contiguous() and cs.numel() == N
        if isinstance(st, LnPartial):     # block partials merged in this GEMM's epilogue (small batches: no finalize launch)
            pt = st.partial
            assert pt.dtype == torch.float32 and pt.is_contiguous() and pt.shape == (K // 64, M, 2)     # block-major
            d.ln_stats, d.ln_nblk, d.ln_eps = pt.data_ptr(), K // 64, float(st.eps)
        else:
            assert st.dtype == torch.float32 and st.is_contiguous() and st.shape == (M, 2)
            d.ln_stats = st.data_ptr()
        d.ln_colsum = cs.data_ptr()
    side = None
    if emit_ln:
        assert out.dim() == 2 and N % 64 == 0 and vt is None
        partial = torch.empty((N // 64, M, 2), dtype=torch.float32, device=a.device)     # block-major: [N/64][M] (sum, M2) pairs
        if out.dtype == torch.bfloat16:      # bf16 residual stream: the stored rows are their own twin
            assert out.is_contiguous() and (residual is None or residual.dtype == torch.bfloat16)
            side = LnSide(out, partial)
            d.stats_out = partial.data_ptr()
        else:
            assert out.dtype == torch.float32
            side = LnSide(torch.empty((M, N), dtype=torch.bfloat16, device=a.device), partial)
            d.twin_out, d.ldt, d.stats_out = side.twin.data_ptr(), N, side.partial.data_ptr()
    if cd == UC_F16:
        d.sat_flag = _p(f16_sat_flag())
    if cd != UC_F32 and split_k <= 1:      # small-M path: hand uc_gemm a hand-over buffer when this launch can split K inside the kernel
        ws = _fuse_ws_for_launch(M, N, K)
        if ws is not None:
            d.fuse_ws = ws
    _lib.check(_lib.load().uc_gemm(C.byref(d), _stream()), "uc_gemm")
    if side is not None:
        out.uc_ln = side
    return out


# fp32 GEMMs: "exact" (fp32 FMA chain, the verification kernels) or "bf16x3" (split operands on the bf16 MFMA pipe); the
# engine installs a hook that answers per call (precision context, head policy)
fp32_matmul_hook = lambda: "exact"   # noqa: E731


def split_bf16x3(x: torch.Tensor, relu: bool = False) -> torch.Tensor:
    """fp32 [..., C] contiguous -> bf16 [..., 3C] = [hi | hi | lo] (uc_split_bf16x3)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 8 == 0
    Cn = x.shape[-1]
    out = torch.empty(x.shape[:-1] + (3 * Cn,), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().uc_split_bf16x3(x.data_ptr(), out.data_ptr(), x.numel() // Cn, Cn, 1 if relu else 0, _stream()),
               "uc_split_bf16x3")
    return out


_w3_cache = {}   # id(weight tensor) -> (weakref, stamp, split copy); entries die with their tensor


def split_weight_bf16x3(w: torch.Tensor, taps: int = 1) -> torch.Tensor:
    """fp32 weight [N, taps*Cin] -> bf16 [N, taps*3*Cin] with every tap's block laid out [Wh | Wl | Wh]; cached per tensor."""
    key = id(w)
    hit = _w3_cache.get(key)
    stamp = (w._version, w.data_ptr(), taps)
    if hit is not None and hit[0]() is w and hit[1] == stamp:
        hit[3].sync()
        return hit[2]
    with torch.no_grad():
        N = w.shape[0]
        w32 = w.detach().float().view(N, taps, -1)
        hi = w32.bfloat16()
        lo = (w32 - hi.float()).bfloat16()
        w3 = torch.cat([hi, lo, hi], dim=2).reshape(N, -1).contiguous()
    from .engine import BuiltOn
    _w3_cache[key] = (weakref.ref(w, lambda _r, k=key: _w3_cache.pop(k, None)), stamp, w3, BuiltOn())
    return w3


class LnPartial:
    "ln= argument of gemm(): the producer's per-block row statistics, merged into (mean, rstd) inside the consumer's epilogue."
    __slots__ = ("partial", "eps")

    def __init__(self, partial, eps):
        self.partial, self.eps = partial, eps


# rows up to which the consumer GEMMs merge the LayerNorm block statistics themselves (uc_gemm_desc.ln_nblk) instead of reading the
# output of a uc_ln_stats_finalize launch.  Measured (512x512 pairs, ms per batch at 1 / 2 / 4 / 8 pairs): eager 12.8 / 13.7 / 15.0 /
# 25.1 -> 11.6 / 10.8 / 16.5 / 27.0 — the eager forward of 1-2 pairs is HOST-bound (~640 launches through ctypes), so 120 fewer
# launches are worth 1-3 ms there; replayed from a hipGraph (GPU-bound) 8.2 / 9.8 / 14.8 / 24.5 -> 8.4 / 10.3 / 16.3 / 26.9: every
# column tile of a row panel repeats the merge at the head of its epilogue, which costs more than the 4-us launches it saves.  Hence:
# up to 2048 rows (two pairs per stream), and never while a graph is being captured.
LN_MERGE_IN_EPILOGUE_MAX_ROWS = int(__import__("os").environ.get("UNICEPTION_AMD_LN_MERGE_ROWS", "2048"))


class LnSide:
    """What a producer GEMM leaves next to its fp32 output rows for the folded LayerNorm of the consumer: a bf16 copy of the
    rows and their per-block statistics; (mean, rstd) per row are finalized on first use, per eps."""
    __slots__ = ("twin", "partial", "_stats")

    def __init__(self, twin, partial):
        self.twin, self.partial, self._stats = twin, partial, {}

    def stats_arg(self, eps: float):
        """What the consumer GEMM gets as its LayerNorm statistics: the block partials themselves for small batches (merged in its
        epilogue: same bits, no launch), the finalized (mean, rstd) rows otherwise."""
        if (self.partial.shape[1] <= LN_MERGE_IN_EPILOGUE_MAX_ROWS and eps not in self._stats
                and not torch.cuda.is_current_stream_capturing()):
            return LnPartial(self.partial, eps)
        return self.stats(eps)

    def stats(self, eps: float) -> torch.Tensor:
        st = self._stats.get(eps)
        if st is None:
            nblk, M, _ = self.partial.shape
            st = torch.empty((M, 2), dtype=torch.float32, device=self.partial.device)
            _lib.check(_lib.load().uc_ln_stats_finalize(self.partial.data_ptr(), M, nblk, float(eps), st.data_ptr(), _stream()),
                       "uc_ln_stats_finalize")
            self._stats[eps] = st
        return st


def vt_buffer(B: int, H: int, ntok: int, device) -> torch.Tensor:
    npad = (ntok + 63) // 64 * 64
    vt = torch.empty((B, H, 64, npad), dtype=torch.bfloat16, device=device)
    if npad != ntok:
        # pad key positions must be finite (the attention kernel multiplies them by P = 0).  Keys are permuted inside every
        # group of 16 positions, so the pads of a ragged group are interleaved with its keys: clear the whole last group(s)
        vt[..., (ntok // 16) * 16:].zero_()
    return vt


def vt_pack(v: torch.Tensor) -> torch.Tensor:
    """v: [B,N,H,D] bf16 view (stride(3)==1) -> packed VT [B,H,D,Npad]."""
    _need_gpu(v)
    B, N, H, D = v.shape
    assert v.dtype == torch.bfloat16 and v.stride(3) == 1
    npad = (N + 63) // 64 * 64
    out = torch.empty((B, H, D, npad), dtype=torch.bfloat16, device=v.device)
    _lib.check(_lib.load().uc_vt_pack(v.data_ptr(), out.data_ptr(), B, H, N, D, v.stride(0), v.stride(1), v.stride(2),
                                      _stream()), "uc_vt_pack")
    return out


def vt_pack_fp8(v: torch.Tensor) -> torch.Tensor:
    """v: [B,N,H,64] bf16 view -> e4m3 V^T [B,H,64,Npad] (uint8) in the k-slot order of the fp8 attention kernel."""
    _need_gpu(v)
    B, N, H, D = v.shape
    assert v.dtype == torch.bfloat16 and v.stride(3) == 1 and D == 64
    npad = (N + 63) // 64 * 64
    out = torch.empty((B, H, D, npad), dtype=torch.uint8, device=v.device)
    _lib.check(_lib.load().uc_vt_pack_fp8(v.data_ptr(), out.data_ptr(), B, H, N, D, v.stride(0), v.stride(1), v.stride(2),
                                          _stream()), "uc_vt_pack_fp8")
    return out


def k_pack_fp8(k: torch.Tensor) -> torch.Tensor:
    """k: [B,N,H,64] bf16 view -> e4m3 rows [B,H,Npad,64] (uint8), zero padded: the K operand of the DMA-staged fp8 kernel."""
    _need_gpu(k)
    B, N, H, D = k.shape
    assert k.dtype == torch.bfloat16 and k.stride(3) == 1 and D == 64
    npad = (N + 63) // 64 * 64
    out = torch.empty((B, H, npad, D), dtype=torch.uint8, device=k.device)
    _lib.check(_lib.load().uc_k_pack_fp8(k.data_ptr(), out.data_ptr(), B, H, N, k.stride(0), k.stride(1), k.stride(2), _stream()),
               "uc_k_pack_fp8")
    return out


def attention_fp8(q: torch.Tensor, k: torch.Tensor, vt8: torch.Tensor, scale: float, prepack_k: Optional[bool] = None) -> torch.Tensor:
    """q [B,Nq,H,64], k [B,Nk,H,64] bf16 views; vt8 from vt_pack_fp8.  Returns O [B,Nq,H,64] bf16.
    prepack_k (default: whenever Nk % 64 == 0): convert K once (k_pack_fp8) and run the LDS-DMA kernel
    (uc_attention_fwd_fp8_k8); otherwise the kernel converts K tiles while staging them (uc_attention_fwd_fp8)."""
    _need_gpu(q, k, vt8)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    assert q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and D == 64 and q.stride(3) == 1 and k.stride(3) == 1
    assert vt8.dtype == torch.uint8 and vt8.is_contiguous() and vt8.shape == (B, H, 64, (Nk + 63) // 64 * 64)
    out = torch.empty((B, Nq, H, D), dtype=torch.bfloat16, device=q.device)
    if prepack_k is None:
        prepack_k = Nk % 64 == 0
    if prepack_k:
        k8 = k_pack_fp8(k)
        _lib.check(_lib.load().uc_attention_fwd_fp8_k8(
            q.data_ptr(), k8.data_ptr(), vt8.data_ptr(), out.data_ptr(), B, H, Nq, Nk, q.stride(0), q.stride(1), q.stride(2),
            out.stride(0), out.stride(1), out.stride(2), float(scale), _stream()), "uc_attention_fwd_fp8_k8")
        return out
    _lib.check(_lib.load().uc_attention_fwd_fp8(
        q.data_ptr(), k.data_ptr(), vt8.data_ptr(), out.data_ptr(), B, H, Nq, Nk, q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2), out.stride(0), out.stride(1), out.stride(2), float(scale), _stream()),
        "uc_attention_fwd_fp8")
    return out


# head dims beyond 64 that the bf16 attention kernels serve (csrc/attention_wide.hip); fp32 runs every head_dim up to the last one
WIDE_HEAD_DIMS = (80, 96)


def attention_served(dtype: torch.dtype, head_dim: int, dropout: bool = False, rope: bool = False, qk_norm: bool = False) -> None:
    """The Python side's one statement of which attention the HIP kernels serve (the library's own is csrc/attention_plan.h): raises
    UcHipError, naming the head_dim, for what has no kernel — so that a model is refused before any GEMM or pack is launched.
    bf16 runs head_dim 64, and 80 / 96 on the wide-head kernels, which have no dropout, RoPE or qk_norm form; every other compute
    dtype runs the fp32 kernels, head_dim <= 96.  Attention dropout exists at head_dim <= 64 only, in every dtype.
    dropout: attention dropout is on.  rope: the layer has a positional encoding (a backward: inverse-RoPE positions).  qk_norm: the
    layer normalises q / k."""
    if dtype == torch.bfloat16 and head_dim != 64 and head_dim not in WIDE_HEAD_DIMS:
        raise UcHipError(f"bf16 attention needs head_dim 64 (got {head_dim}), or 80 / 96 without dropout, RoPE and qk_norm; use fp32 precision for this model")
    if dtype != torch.bfloat16 and head_dim > WIDE_HEAD_DIMS[-1]:
        raise UcHipError(f"fp32 attention needs head_dim <= {WIDE_HEAD_DIMS[-1]} (got {head_dim})")
    if dropout and head_dim > 64:
        raise UcHipError(f"attn_drop > 0 has no HIP path at head_dim {head_dim} (attention dropout is head_dim <= 64 only)")
    if dtype == torch.bfloat16 and head_dim > 64:
        if qk_norm:
            raise UcHipError(f"qk_norm has no HIP path at head_dim {head_dim} in bf16 (head_dim 64 only); use fp32 precision for this model")
        if rope:
            raise UcHipError(f"RoPE has no HIP path at head_dim {head_dim} (the rotation kernels are head_dim 64); this model cannot run in bf16")


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, v_packed: bool = False,
              out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None, dropout=None) -> torch.Tensor:
    """q [B,Nq,H,D], k [B,Nk,H,D] strided views (stride(3)==1); v same, or packed VT [B,H,D,Npad] when v_packed.
    Returns O [B,Nq,H,D] contiguous (== [B,Nq,H*D]).
    dropout = (p, seed): dropout of the attention probabilities inside the kernel (uc_attention_fwd with drop_p > 0: a counter-based keep
    function of (seed, batch, head, query, key); attention_drop_mask materialises it; the backward takes the same pair)."""
    _need_gpu(q, k, v)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    assert q.stride(3) == 1 and k.stride(3) == 1 and q.dtype == k.dtype == v.dtype
    if out is None:
        out = torch.empty((B, Nq, H, D), dtype=q.dtype, device=q.device)
    if v_packed:
        vs = (0, 0, 0)
        assert v.is_contiguous() and v.shape[-1] == (Nk + 63) // 64 * 64
    else:
        assert v.stride(3) == 1
        vs = (v.stride(0), v.stride(1), v.stride(2))
    d = AttnDesc()
    d.dtype, d.v_layout = _dt(q.dtype), UC_V_PACKED_T if v_packed else UC_V_ROWMAJOR
    d.B, d.H, d.Nq, d.Nk, d.D = B, H, Nq, Nk, D
    d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.q_sb, d.q_sn, d.q_sh = q.stride(0), q.stride(1), q.stride(2)
    d.k_sb, d.k_sn, d.k_sh = k.stride(0), k.stride(1), k.stride(2)
    d.v_sb, d.v_sn, d.v_sh = vs
    d.o_sb, d.o_sn, d.o_sh = out.stride(0), out.stride(1), out.stride(2)
    d.scale, d.lse = float(scale), _p(lse)
    if dropout is not None and float(dropout[0]) > 0.0:
        d.drop_p, d.seed = float(dropout[0]), int(dropout[1])
    _lib.check(_lib.load().uc_attention_fwd(C.byref(d), _stream()), "uc_attention_fwd")
    return out


def attention_x3(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None,
                 lse: Optional[torch.Tensor] = None, rope: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """fp32-class attention on the matrix pipe (uc_attention_fwd_x3: split bf16 operands, three MFMA products per product, fp32
    softmax).  q [B,Nq,H,64], k / v [B,Nk,H,64]: fp32 strided views with stride(3) == 1.  Returns fp32 O [B,Nq,H,64] contiguous.
    rope = (q positions [B*Nq, 2] int64, k positions [B*Nk, 2] int64, table from rope_table): q and k are rotated by RoPE-2D inside the
    operand split (the arithmetic of rope_2d_), instead of in a pass of their own."""
    _need_gpu(q, k, v)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    assert D == 64 and q.dtype == k.dtype == v.dtype == torch.float32
    assert q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1 and k.shape == v.shape
    if out is None:
        out = torch.empty((B, Nq, H, D), dtype=torch.float32, device=q.device)
    qp = kp = tab = None
    npos = 0
    if rope is not None:
        qp, kp, tab = rope
        assert qp.dtype == kp.dtype == torch.int64 and qp.is_contiguous() and kp.is_contiguous() and qp.numel() == B * Nq * 2 and kp.numel() == B * Nk * 2
        assert tab.dtype == torch.float32 and tab.is_contiguous() and tab.numel() % 32 == 0
        npos = tab.numel() // 32
    lib = _lib.load()
    ws = torch.empty(int(lib.uc_attention_x3_workspace_bytes(B, H, Nq, Nk)), dtype=torch.uint8, device=q.device)
    _lib.check(lib.uc_attention_fwd_x3(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ws.data_ptr(), B, H, Nq, Nk,
                                       q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                                       v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1), out.stride(2), float(scale),
                                       _p(lse), _p(qp), _p(kp), _p(tab), npos, _stream()), "uc_attention_fwd_x3")
    return out


def patch_gather(img: torch.Tensor, P: int, out_dtype: torch.dtype) -> torch.Tensor:
    _need_gpu(img)
    assert img.dtype == torch.float32 and img.is_contiguous() and img.dim() == 4
    B, Cin, H, W = img.shape
    cols = torch.empty((B * (H // P) * (W // P), Cin * P * P), dtype=out_dtype, device=img.device)
    _lib.check(_lib.load().uc_patch_gather(img.data_ptr(), cols.data_ptr(), _dt(out_dtype), B, Cin, H, W, P, _stream()),
               "uc_patch_gather")
    return cols


def nchw_to_nhwc(x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """x [B,C,H,W] contiguous -> [B,H,W,C] contiguous in out_dtype."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dim() == 4
    B, Cn, H, W = x.shape
    y = torch.empty((B, H, W, Cn), dtype=out_dtype, device=x.device)
    _lib.check(_lib.load().uc_nchw_to_nhwc(x.data_ptr(), _dt(x.dtype), y.data_ptr(), _dt(out_dtype), B, Cn, H, W, _stream()),
               "uc_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """x [B,H,W,C] contiguous -> [B,C,H,W] contiguous in out_dtype."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dim() == 4
    B, H, W, Cn = x.shape
    y = torch.empty((B, Cn, H, W), dtype=out_dtype, device=x.device)
    _lib.check(_lib.load().uc_nhwc_to_nchw(x.data_ptr(), _dt(x.dtype), y.data_ptr(), _dt(out_dtype), B, Cn, H, W, _stream()),
               "uc_nhwc_to_nchw")
    return y


def convert(x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    _need_gpu(x)
    assert x.is_contiguous()
    if x.dtype == out_dtype:
        return x
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _lib.check(_lib.load().uc_convert(x.data_ptr(), _dt(x.dtype), y.data_ptr(), _dt(out_dtype), x.numel(),
                                      _p(f16_sat_flag()) if out_dtype == torch.float16 else None, _stream()), "uc_convert")
    return y


def bilinear_nhwc(x: torch.Tensor, Ho: int, Wo: int, crop: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """align_corners=True bilinear resize of NHWC x to (Ho,Wo), optionally keeping only the top-left crop."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dim() == 4
    B, Hi, Wi, Cn = x.shape
    ch, cw = crop if crop is not None else (Ho, Wo)
    y = torch.empty((B, ch, cw, Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_bilinear_nhwc(x.data_ptr(), y.data_ptr(), _dt(x.dtype), B, Hi, Wi, Cn, Ho, Wo, ch, cw, _stream()),
               "uc_bilinear_nhwc")
    return y


def convt_scatter(x: torch.Tensor, B: int, h: int, w: int, k: int, Cout: int) -> torch.Tensor:
    _need_gpu(x)
    assert x.is_contiguous() and x.shape == (B * h * w, k * k * Cout)
    y = torch.empty((B, k * h, k * w, Cout), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_convt_scatter(x.data_ptr(), y.data_ptr(), _dt(x.dtype), B, h, w, k, Cout, _stream()),
               "uc_convt_scatter")
    return y


def pixel_shuffle(x: torch.Tensor, B: int, h: int, w: int, P: int, Cout: int) -> torch.Tensor:
    _need_gpu(x)
    assert x.is_contiguous() and x.shape == (B * h * w, Cout * P * P)
    y = torch.empty((B, Cout, P * h, P * w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().uc_pixel_shuffle(x.data_ptr(), _dt(x.dtype), y.data_ptr(), B, h, w, P, Cout, _stream()),
               "uc_pixel_shuffle")
    return y


def pointmap_adaptor(x: torch.Tensor, conf_vmin: float, conf_vmax: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """x: fp32 4-channel map given as a BCHW-shaped tensor (contiguous NCHW or channels-last strides).
    Returns (pts [B,H,W,3], conf [B,H,W,1]) fp32 contiguous."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 4
    B, _, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if sh != W * sw:
        raise UcHipError("pointmap_adaptor: rows of the 4-channel map must be densely packed")
    pts = torch.empty((B, H, W, 3), dtype=torch.float32, device=x.device)
    conf = torch.empty((B, H, W, 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().uc_pointmap_adaptor(x.data_ptr(), sb, sc, sw, pts.data_ptr(), conf.data_ptr(), B, H, W,
                                               float(conf_vmin), float(conf_vmax), _stream()), "uc_pointmap_adaptor")
    return pts, conf


def adaptor_program(x: torch.Tensor, segs, cout: int) -> torch.Tensor:
    """x: fp32 BCHW-shaped map (contiguous NCHW or a channels-last view); segs: list of _lib.AdaptorSeg -> fp32 NHWC [B,H,W,cout]."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.dim() == 4
    B, _, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if sh != W * sw:
        raise UcHipError("adaptor_program: rows of the input map must be densely packed")
    out = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
    arr = (_lib.AdaptorSeg * len(segs))(*segs)
    _lib.check(_lib.load().uc_adaptor_program(x.data_ptr(), sb, sc, sw, out.data_ptr(), B, H, W, cout, arr, len(segs), _stream()),
               "uc_adaptor_program")
    return out


def adaptor_program_bwd(x: torch.Tensor, dout: torch.Tensor, segs) -> torch.Tensor:
    """Gradient of adaptor_program with respect to x: x as in the forward, dout fp32 NHWC [B,H,W,cout] -> dx with x's strides."""
    _need_gpu(x, dout)
    assert x.dtype == torch.float32 and x.dim() == 4 and dout.dtype == torch.float32 and dout.is_contiguous() and dout.dim() == 4
    B, C, H, W = x.shape
    assert dout.shape[:3] == (B, H, W)
    sb, sc, sh, sw = x.stride()
    if sh != W * sw:
        raise UcHipError("adaptor_program_bwd: rows of the input map must be densely packed")
    dx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    arr = (_lib.AdaptorSeg * len(segs))(*segs)
    _lib.check(_lib.load().uc_adaptor_program_bwd(x.data_ptr(), sb, sc, sw, dout.data_ptr(), dx.data_ptr(), B, H, W, C, dout.shape[3],
                                                  arr, len(segs), _stream()), "uc_adaptor_program_bwd")
    return dx


def conv1x1_to4(feat: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """feat NHWC [B,H,W,Cin]; w fp32 [4,Cin]; b fp32 [4] -> fp32 NHWC [B,H,W,4]."""
    _need_gpu(feat, w, b)
    assert feat.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous() and w.shape[0] == 4
    B, H, W, Cin = feat.shape
    out = torch.empty((B, H, W, 4), dtype=torch.float32, device=feat.device)
    _lib.check(_lib.load().uc_conv1x1_to4(feat.data_ptr(), _dt(feat.dtype), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                                          B * H * W, Cin, _stream()), "uc_conv1x1_to4")
    return out


def add_view_pe_(x: torch.Tensor, pe: torch.Tensor, T: int) -> torch.Tensor:
    """x fp32 [B, L, C] += pe[v] on the T tokens of each of the V = pe.shape[0] views (in place; rows past V*T untouched)."""
    _need_gpu(x, pe)
    assert x.dtype == torch.float32 and pe.dtype == torch.float32 and x.is_contiguous() and pe.is_contiguous() and x.dim() == 3
    B, L, Cn = x.shape
    _lib.check(_lib.load().uc_add_view_pe(x.data_ptr(), pe.data_ptr(), B, L, T, pe.shape[0], Cn, _stream()), "uc_add_view_pe")
    return x


def assemble_tokens(tok: torch.Tensor, cls: torch.Tensor, reg: Optional[torch.Tensor], pos: torch.Tensor) -> torch.Tensor:
    """tok fp32 [B,hw,D], cls [D], reg [R,D]|None, pos [1+hw,D] -> [B, 1+R+hw, D] = [cls+pos0 | reg | tok+pos]."""
    _need_gpu(tok, cls, reg, pos)
    B, hw, D = tok.shape
    R = 0 if reg is None else reg.shape[0]
    for t in (tok, cls, reg, pos):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert cls.numel() == D and pos.shape == (1 + hw, D)
    out = torch.empty((B, 1 + R + hw, D), dtype=torch.float32, device=tok.device)
    _lib.check(_lib.load().uc_assemble_tokens(tok.data_ptr(), cls.data_ptr(), _p(reg), pos.data_ptr(), out.data_ptr(), B, hw, R, D,
                                              _stream()), "uc_assemble_tokens")
    return out


def assemble_prefix(tok: torch.Tensor, prefix: torch.Tensor, pos: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """tok fp32 [B,hw,D], prefix fp32 [P,D], pos fp32 [hw,D] -> [B, P+hw, D] = [prefix | tok+pos] in out_dtype (fp32 / bf16), one pass."""
    _need_gpu(tok, prefix, pos)
    B, hw, D = tok.shape
    for t in (tok, prefix, pos):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert prefix.dim() == 2 and prefix.shape[1] == D and pos.shape == (hw, D)
    out = torch.empty((B, prefix.shape[0] + hw, D), dtype=out_dtype, device=tok.device)
    _lib.check(_lib.load().uc_assemble_prefix(tok.data_ptr(), prefix.data_ptr(), pos.data_ptr(), out.data_ptr(), _dt(out_dtype), B, hw,
                                              prefix.shape[0], D, _stream()), "uc_assemble_prefix")
    return out


def token_slice(src: torch.Tensor, start: int, n: int) -> torch.Tensor:
    """src fp32 [B,Ns,D] -> contiguous [B,n,D] copy of rows start..start+n."""
    _need_gpu(src)
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3
    B, Ns, D = src.shape
    dst = torch.empty((B, n, D), dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().uc_token_slice(src.data_ptr(), dst.data_ptr(), B, Ns, n, start, 0, n, D, _stream()), "uc_token_slice")
    return dst


# --------------------------------------------------------------------------------------------
# training path
# --------------------------------------------------------------------------------------------
def layernorm_bwd(x: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor, eps: float, dgamma: torch.Tensor,
                  dbeta: torch.Tensor, dres: Optional[torch.Tensor] = None, bf16_twin: bool = False):
    """dx (x's dtype: fp32, or bf16 on a bf16 training stream) of y = LN(x); dgamma/dbeta are accumulated into (fp32, caller-zeroed).
    dres: gradient of a parallel residual branch to add into dx (same dtype as x).  bf16_twin (fp32 stream only): also return a bf16
    copy of dx written in the same pass."""
    _need_gpu(x, gamma, dy, dgamma, dbeta, dres)
    assert x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape
    Cn = x.shape[-1]
    rows = x.numel() // Cn
    dx = torch.empty_like(x)
    twin = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if (bf16_twin and x.dtype == torch.float32) else None
    if dres is not None:
        assert dres.dtype == x.dtype and dres.is_contiguous() and dres.shape == x.shape
    _lib.check(_lib.load().uc_layernorm_bwd(x.data_ptr(), _dt(x.dtype), gamma.data_ptr(), dy.data_ptr(), _dt(dy.dtype), _p(dres), dx.data_ptr(),
                                            _p(twin), dgamma.data_ptr(), dbeta.data_ptr(), rows, Cn, float(eps), _stream()),
               "uc_layernorm_bwd")
    return (dx, twin if twin is not None else dx) if bf16_twin else dx


def _gemm_tn_desc(a: torch.Tensor, b: torch.Tensor, conv: Optional[Tuple[int, bool]]) -> GemmTnDesc:
    "Operands and shape of a gemm_tn / gemm_tn_query call as a uc_gemm_tn_desc (outputs and split_k still unset)."
    _need_gpu(a, b)
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1
    T, I = a.shape
    d = GemmTnDesc(A=a.data_ptr(), lda=a.stride(0), B=b.data_ptr(), T=T, I=I)
    if conv is None:
        assert b.dim() == 2 and b.stride(1) == 1 and b.shape[0] == T
        d.J, d.ldb = b.shape[1], b.stride(0)
    else:
        stride, relu = conv
        assert b.dim() == 4 and b.is_contiguous()
        d.conv_B, d.conv_H, d.conv_W, d.conv_Cin = b.shape
        d.J, d.conv_stride, d.relu_b = 9 * b.shape[3], stride, 1 if relu else 0
    return d


def _gemm_tn_query(d: GemmTnDesc) -> Tuple[int, int]:
    tiles, split_k = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().uc_gemm_tn_query(C.byref(d), C.byref(tiles), C.byref(split_k)), "uc_gemm_tn_query")
    return tiles.value, split_k.value


def gemm_tn_query(a: torch.Tensor, b: torch.Tensor, conv: Optional[Tuple[int, bool]] = None) -> Tuple[int, int]:
    "(workgroups one K-slice of gemm_tn(a, b, conv=conv) occupies, the split_k gemm_tn takes when none is given) — uc_gemm_tn_query."
    return _gemm_tn_query(_gemm_tn_desc(a, b, conv))


def gemm_tn(a: torch.Tensor, b: torch.Tensor, split_k: Optional[int] = None, conv: Optional[Tuple[int, bool]] = None,
            colsum: bool = False, colsum_into: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            colsum_out: Optional[torch.Tensor] = None):
    """Weight-gradient contraction over the slow axis: returns fp32 slabs [split_k, I, J] of  sum_t a[t,i] * b[t,j].
    a: [T,I] bf16 (unit column stride).  b: [T,J] bf16, or with conv=(stride, relu) the NHWC input [B,H,W,Cin] of a
    3x3/pad-1 conv whose im2col ([T, 9*Cin], T = output pixels) is formed implicitly.
    split_k=None: the slice count the library recommends for this shape (uc_gemm_tn_query).
    colsum=True: also returns slabs [split_k, I] of sum_t a[t,i] (the bias gradient).
    colsum_into: fp32 [I] buffer that receives += sum_t a[t,i] atomically instead (e.g. the bias's gradient buffer).
    out / colsum_out: caller-provided contiguous fp32 [split_k, I, J] / [split_k, I] (with colsum=True) to write the slabs to, e.g.
    the front of a larger buffer; allocated here when omitted."""
    d = _gemm_tn_desc(a, b, conv)
    d.split_k = _gemm_tn_query(d)[1] if split_k is None else split_k
    if out is None:
        out = torch.empty((d.split_k, d.I, d.J), dtype=torch.float32, device=a.device)
    else:
        _need_gpu(out)
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (d.split_k, d.I, d.J)
    assert colsum_out is None or colsum, "colsum_out goes with colsum=True"
    if colsum_into is not None:
        assert colsum_into.dtype == torch.float32 and colsum_into.is_contiguous() and colsum_into.numel() == d.I and not colsum
        cs, d.colsum_atomic = colsum_into, 1
    elif colsum_out is not None:
        _need_gpu(colsum_out)
        assert colsum_out.dtype == torch.float32 and colsum_out.is_contiguous() and tuple(colsum_out.shape) == (d.split_k, d.I)
        cs = colsum_out
    else:
        cs = torch.empty((d.split_k, d.I), dtype=torch.float32, device=a.device) if colsum else None
    d.C, d.colsum_a = out.data_ptr(), _p(cs)
    _lib.check(_lib.load().uc_gemm_tn(C.byref(d), _stream()), "uc_gemm_tn")
    return (out, cs) if colsum else out


def splitk_reduce(ws: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """ws [sk, M, N] fp32 slabs (uc_gemm split_k / uc_gemm_tn output, or a row range ws_full[:, r0:r1] of them) ->
    out [M,N] (= or += the sum over slabs)."""
    _need_gpu(ws, out)
    assert ws.dtype == torch.float32 and ws.dim() == 3 and ws.stride(2) == 1 and ws.stride(1) == ws.shape[2]
    if out is None:
        assert not accumulate
        out = torch.empty(ws.shape[1:], dtype=torch.float32, device=ws.device)
    assert out.is_contiguous() and out.numel() == ws.shape[1] * ws.shape[2] and out.dtype == torch.float32
    stride = ws.stride(0) if ws.shape[0] > 1 else out.numel()
    _lib.check(_lib.load().uc_splitk_reduce(ws.data_ptr(), ws.shape[0], out.numel(), stride, out.data_ptr(), 1 if accumulate else 0,
                                            _stream()), "uc_splitk_reduce")
    return out


def colsum_(src: torch.Tensor, out: torch.Tensor) -> None:
    """out[n] += sum_m src[m, n] (out fp32)."""
    _need_gpu(src, out)
    assert src.dim() == 2 and src.stride(1) == 1 and out.dtype == torch.float32 and out.numel() == src.shape[1]
    _lib.check(_lib.load().uc_colsum(src.data_ptr(), _dt(src.dtype), src.shape[0], src.shape[1], src.stride(0), out.data_ptr(),
                                     _stream()), "uc_colsum")


def mask_scale(x: torch.Tensor, mask: torch.Tensor, rows_per_mask: int, scale: float, residual: Optional[torch.Tensor] = None,
               out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Dropout / DropPath (training): out [rows, cols] = (residual +) x * (mask ? scale : 0) (uc_mask_scale).  mask uint8: one per element
    (rows_per_mask == 0) or one per group of rows_per_mask rows.  Its own backward when applied to the gradient without residual."""
    _need_gpu(x, mask, residual)
    assert x.dim() == 2 and x.is_contiguous() and mask.dtype == torch.uint8 and mask.is_contiguous() and x.shape[1] % 4 == 0
    rows, cols = x.shape
    assert mask.numel() == (x.numel() if rows_per_mask == 0 else (rows + rows_per_mask - 1) // rows_per_mask)
    od = out_dtype or (residual.dtype if residual is not None else x.dtype)
    if residual is not None:
        assert residual.shape == x.shape and residual.is_contiguous() and residual.dtype == od
    out = torch.empty((rows, cols), dtype=od, device=x.device)
    _lib.check(_lib.load().uc_mask_scale(x.data_ptr(), _dt(x.dtype), mask.data_ptr(), int(rows_per_mask), float(scale), _p(residual),
                                         out.data_ptr(), _dt(od), rows, cols, _stream()), "uc_mask_scale")
    return out


def act_bwd(dg: torch.Tensor, u: torch.Tensor, act: str) -> torch.Tensor:
    _need_gpu(dg, u)
    assert dg.is_contiguous() and u.is_contiguous() and dg.shape == u.shape and dg.dtype == u.dtype
    du = torch.empty_like(dg)
    _lib.check(_lib.load().uc_act_bwd(dg.data_ptr(), u.data_ptr(), du.data_ptr(), _dt(dg.dtype), ACT[act], dg.numel(), _stream()),
               "uc_act_bwd")
    return du


def swiglu(t: torch.Tensor) -> torch.Tensor:
    """t [M, 2H] (= w12(x)) -> silu(t[:, :H]) * t[:, H:]  [M, H]: the gate of DINOv2 giant's SwiGLU FFN.  fp32 / bf16, H % 8 == 0."""
    M, H2 = t.shape
    if not t.is_contiguous() or H2 % 16 != 0 or t.dtype not in (torch.float32, torch.bfloat16):
        raise UcHipError(f"swiglu: contiguous fp32 / bf16 [M, 2H] with H % 8 == 0 expected (got {tuple(t.shape)}, {t.dtype})")
    g = torch.empty((M, H2 // 2), dtype=t.dtype, device=t.device)
    _lib.check(_lib.load().uc_swiglu(t.data_ptr(), g.data_ptr(), _dt(t.dtype), M, H2 // 2, _stream()), "uc_swiglu")
    return g


def swiglu_bwd(dg: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    "Gradient of swiglu with respect to t: dg [M, H], t [M, 2H] -> dt [M, 2H]."
    M, H2 = t.shape
    if not (t.is_contiguous() and dg.is_contiguous()) or dg.shape != (M, H2 // 2) or dg.dtype != t.dtype or H2 % 16 != 0:
        raise UcHipError("swiglu_bwd: contiguous dg [M, H] and t [M, 2H] of one dtype expected")
    dt_ = torch.empty_like(t)
    _lib.check(_lib.load().uc_swiglu_bwd(dg.data_ptr(), t.data_ptr(), dt_.data_ptr(), _dt(t.dtype), M, H2 // 2, _stream()), "uc_swiglu_bwd")
    return dt_


def transpose2d(x: torch.Tensor, out_dtype: Optional[torch.dtype] = None, pad_to: int = 1, with_copy: bool = False):
    """[R,S] contiguous -> [S,Rp] contiguous, Rp = R rounded up to `pad_to` (<= 64; pad columns are zeros).
    with_copy: also return the un-transposed matrix converted to out_dtype (one pass over the source)."""
    _need_gpu(x)
    assert x.dim() == 2 and x.is_contiguous() and 1 <= pad_to <= 64
    out_dtype = out_dtype or x.dtype
    R, S = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    y = torch.empty((S, Rp), dtype=out_dtype, device=x.device)
    c = torch.empty((R, S), dtype=out_dtype, device=x.device) if with_copy else None
    _lib.check(_lib.load().uc_transpose2d(x.data_ptr(), _dt(x.dtype), y.data_ptr(), _dt(out_dtype), _p(c), R, S, Rp, _stream()),
               "uc_transpose2d")
    return (y, c) if with_copy else y


def pointmap_adaptor_bwd(x: torch.Tensor, dpts: Optional[torch.Tensor], dconf: Optional[torch.Tensor], conf_vmin: float,
                         conf_vmax: float) -> torch.Tensor:
    _need_gpu(x, dpts, dconf)
    assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 4
    B, _, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    assert sh == W * sw
    for t in (dpts, dconf):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    dx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    vmax = conf_vmax if conf_vmax != float("inf") else 3.0e38
    _lib.check(_lib.load().uc_pointmap_adaptor_bwd(x.data_ptr(), sb, sc, sw, _p(dpts), _p(dconf), float(conf_vmin), float(vmax),
                                                   dx.data_ptr(), B, H, W, _stream()), "uc_pointmap_adaptor_bwd")
    return dx


def conf_loss(pts: torch.Tensor, conf: torch.Tensor, gt: torch.Tensor, alpha: float, grad_scale: float,
              loss_sum: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _need_gpu(pts, conf, gt, loss_sum)
    for t in (pts, conf, gt):
        assert t.dtype == torch.float32 and t.is_contiguous()
    npix = conf.numel()
    assert pts.numel() == 3 * npix and gt.numel() == 3 * npix
    dpts, dconf = torch.empty_like(pts), torch.empty_like(conf)
    _lib.check(_lib.load().uc_conf_loss(pts.data_ptr(), conf.data_ptr(), gt.data_ptr(), float(alpha), float(grad_scale),
                                        loss_sum.data_ptr(), dpts.data_ptr(), dconf.data_ptr(), npix, _stream()), "uc_conf_loss")
    return dpts, dconf


def pointmap_loss(x: torch.Tensor, gt: torch.Tensor, alpha: float, grad_scale: float, loss_sum: torch.Tensor) -> torch.Tensor:
    """x: fp32 4-channel BCHW-shaped map (dense rows); gt [B,H,W,3] fp32. Adds the summed loss into loss_sum[0] and
    returns d(loss_sum)/dx * grad_scale with the memory layout of x."""
    _need_gpu(x, gt, loss_sum)
    assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 4 and gt.is_contiguous() and gt.dtype == torch.float32
    B, _, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    assert sh == W * sw
    dx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().uc_pointmap_loss(x.data_ptr(), sb, sc, sw, gt.data_ptr(), float(alpha), float(grad_scale),
                                            loss_sum.data_ptr(), dx.data_ptr(), B, H, W, _stream()), "uc_pointmap_loss")
    return dx


def pixel_unshuffle(g: torch.Tensor, P: int, out_dtype: torch.dtype) -> torch.Tensor:
    """g fp32 NCHW [B,Cout,P*h,P*w] contiguous -> [B*h*w, Cout*P*P]."""
    _need_gpu(g)
    assert g.dtype == torch.float32 and g.is_contiguous()
    B, Cout, Hd, Wd = g.shape
    h, w = Hd // P, Wd // P
    y = torch.empty((B * h * w, Cout * P * P), dtype=out_dtype, device=g.device)
    _lib.check(_lib.load().uc_pixel_unshuffle(g.data_ptr(), y.data_ptr(), _dt(out_dtype), B, h, w, P, Cout, _stream()),
               "uc_pixel_unshuffle")
    return y


def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float,
           weight_decay: float, step: int, grad_scale: float = 1.0) -> None:
    _need_gpu(p, g, m, v)
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
    _lib.check(_lib.load().uc_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(beta1),
                                    float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale), _stream()), "uc_adamw")


def attention_drop_mask(B: int, H: int, Nq: int, Nk: int, p: float, seed: int, device) -> torch.Tensor:
    "uint8 [B,H,Nq,Nk] keep mask (1 = kept) of attention(..., dropout=(p, seed)): the function the kernels evaluate, for references."
    mask = torch.empty((B, H, Nq, Nk), dtype=torch.uint8, device=device)
    _need_gpu(mask)
    _lib.check(_lib.load().uc_attention_drop_mask(mask.data_ptr(), B, H, Nq, Nk, float(p), int(seed), _stream()), "uc_attention_drop_mask")
    return mask


def attention_bwd(q, k, v, o, do, lse, scale: float, out=None, rope=None, dropout=None):
    """q,o,do [B,Nq,H,D]; k,v [B,Nk,H,D] (bf16: D = 64, or 80 / 96 on the wide-head kernels; fp32: D <= 96) views (unit last stride); lse fp32 [B,H,Nq].
    dropout = the forward's (p, seed) when it dropped attention probabilities (the kernels re-evaluate the mask).
    Returns dq, dk, dv ([B,N,H,64] bf16): fresh contiguous tensors, or the three views passed as `out`
    (e.g. slices of one fused dqkv buffer).
    rope = (qpos int64 [B*Nq,2], kpos int64 [B*Nk,2], base, F0) (bf16 only): q and k were RoPE-rotated before the forward; dq / dk come
    back as gradients of the un-rotated q / k (the inverse rotation runs inside the backward kernels)."""
    _need_gpu(q, k, v, o, do, lse)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    dt = q.dtype
    if dt not in (torch.bfloat16, torch.float32):
        raise UcHipError(f"attention backward needs bf16 or fp32 operands (got {dt}, head_dim {D})")
    attention_served(dt, D, dropout=dropout is not None and float(dropout[0]) > 0.0, rope=rope is not None)
    assert lse.dtype == torch.float32 and lse.is_contiguous()
    if do.stride() != o.stride() or o.stride(3) != 1:
        o, do = o.contiguous(), do.contiguous()
    if out is None:
        dq = torch.empty((B, Nq, H, D), dtype=dt, device=q.device)
        dk = torch.empty((B, Nk, H, D), dtype=dt, device=q.device)
        dv = torch.empty((B, Nk, H, D), dtype=dt, device=q.device)
    else:
        dq, dk, dv = out
        assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
        assert all(t.dtype == dt and t.stride(3) == 1 for t in out)
    # scratch: fp32 verification kernels [B,H,Nq]; bf16 kernels [B*H][2][Nq rounded up to 128] (ABI 13: the dQ kernel leaves -lse*log2(e)
    # and -rowsum(dO*O) there as the dK / dV kernel's accumulator start values)
    delta = torch.empty((B, H, Nq) if dt == torch.float32 else (B * H, 2, (Nq + 127) // 128 * 128), dtype=torch.float32, device=q.device)
    if rope is not None:
        assert dt == torch.bfloat16 and rope[0].dtype == torch.int64 and rope[1].dtype == torch.int64
        assert rope[0].is_contiguous() and rope[1].is_contiguous() and rope[0].numel() == 2 * B * Nq and rope[1].numel() == 2 * B * Nk
    d = AttnBwdDesc()
    d.dtype, d.B, d.H, d.Nq, d.Nk, d.D = _dt(dt), B, H, Nq, Nk, D
    d.Q, d.K, d.V, d.O, d.dO, d.LSE = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr()
    d.dQ, d.dK, d.dV, d.delta = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    d.q_sb, d.q_sn, d.q_sh = q.stride(0), q.stride(1), q.stride(2)
    d.k_sb, d.k_sn, d.k_sh = k.stride(0), k.stride(1), k.stride(2)
    d.v_sb, d.v_sn, d.v_sh = v.stride(0), v.stride(1), v.stride(2)
    d.o_sb, d.o_sn, d.o_sh = o.stride(0), o.stride(1), o.stride(2)
    d.dq_sb, d.dq_sn, d.dq_sh = dq.stride(0), dq.stride(1), dq.stride(2)
    d.dk_sb, d.dk_sn, d.dk_sh = dk.stride(0), dk.stride(1), dk.stride(2)
    d.dv_sb, d.dv_sn, d.dv_sh = dv.stride(0), dv.stride(1), dv.stride(2)
    d.scale = float(scale)
    if rope is not None:
        d.rope_qpos, d.rope_kpos, d.rope_base, d.rope_f0 = rope[0].data_ptr(), rope[1].data_ptr(), float(rope[2]), float(rope[3])
    if dropout is not None and float(dropout[0]) > 0.0:
        d.drop_p, d.seed = float(dropout[0]), int(dropout[1])
    _lib.check(_lib.load().uc_attention_bwd(C.byref(d), _stream()), "uc_attention_bwd")
    return dq, dk, dv


def bilinear_nhwc_bwd(dy: torch.Tensor, Hi: int, Wi: int, Ho: int, Wo: int) -> torch.Tensor:
    """dy [B,crop_h,crop_w,C] (gradient of bilinear_nhwc's output) -> dx [B,Hi,Wi,C]."""
    _need_gpu(dy)
    assert dy.is_contiguous() and dy.dim() == 4
    B, ch, cw, C = dy.shape
    dx = torch.empty((B, Hi, Wi, C), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().uc_bilinear_nhwc_bwd(dy.data_ptr(), dx.data_ptr(), _dt(dy.dtype), B, Hi, Wi, C, Ho, Wo, ch, cw, _stream()),
               "uc_bilinear_nhwc_bwd")
    return dx


def convt_gather(dy: torch.Tensor, k: int) -> torch.Tensor:
    """dy NHWC [B,k*h,k*w,Cout] -> [B*h*w, k*k*Cout]."""
    _need_gpu(dy)
    assert dy.is_contiguous() and dy.dim() == 4
    B, Hk, Wk, Cout = dy.shape
    h, w = Hk // k, Wk // k
    out = torch.empty((B * h * w, k * k * Cout), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().uc_convt_gather(dy.data_ptr(), out.data_ptr(), _dt(dy.dtype), B, h, w, k, Cout, _stream()), "uc_convt_gather")
    return out


def im2col_t(x: torch.Tensor, stride: int, relu: bool, pad_to: int = 64) -> torch.Tensor:
    """x NHWC [B,H,W,Cin] -> [9*Cin, npix_padded] (see uc_im2col_t)."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dim() == 4
    B, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    npix = B * Ho * Wo
    ld = (npix + pad_to - 1) // pad_to * pad_to
    out = torch.empty((9 * Cin, ld), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_im2col_t(x.data_ptr(), out.data_ptr(), _dt(x.dtype), B, H, W, Cin, stride, 1 if relu else 0, ld, _stream()),
               "uc_im2col_t")
    return out


def dilate_nhwc(src: torch.Tensor, H: int, W: int, stride: int) -> torch.Tensor:
    _need_gpu(src)
    assert src.is_contiguous() and src.dim() == 4
    B, h, w, C = src.shape
    out = torch.empty((B, H, W, C), dtype=src.dtype, device=src.device)
    _lib.check(_lib.load().uc_dilate_nhwc(src.data_ptr(), out.data_ptr(), _dt(src.dtype), B, h, w, H, W, C, stride, _stream()),
               "uc_dilate_nhwc")
    return out


def conv1x1_to4_bwd(feat: torch.Tensor, w: torch.Tensor, dout: torch.Tensor, dw: torch.Tensor, db: torch.Tensor,
                    relu_mask: bool = False) -> torch.Tensor:
    """feat NHWC [...,Cin], w fp32 [4,Cin], dout fp32 [...,4] -> dfeat (feat's dtype); dw/db accumulated (fp32).
    relu_mask: feat is a ReLU's output; its backward (zero where feat <= 0) is applied to dfeat in the same pass."""
    _need_gpu(feat, w, dout, dw, db)
    assert feat.is_contiguous() and dout.is_contiguous() and dout.dtype == torch.float32 and w.is_contiguous()
    Cin = feat.shape[-1]
    npix = feat.numel() // Cin
    dfeat = torch.empty_like(feat)
    _lib.check(_lib.load().uc_conv1x1_to4_bwd(feat.data_ptr(), _dt(feat.dtype), w.data_ptr(), dout.data_ptr(), dfeat.data_ptr(),
                                              dw.data_ptr(), db.data_ptr(), npix, Cin, 1 if relu_mask else 0, _stream()), "uc_conv1x1_to4_bwd")
    return dfeat


# --------------------------------------------------------------------------------------------
# differential attention (uc_diff_attention_fwd / uc_diff_attention_combine_bwd)
def diff_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, lambda_full: float, subln_w: torch.Tensor,
                   rms_eps: float, out_scale: float, out: Optional[torch.Tensor] = None, v_packed: bool = False, save: bool = False):
    """q [B,Nq,2H,hd], k [B,Nk,2H,hd] strided views (unit last stride): head h of softmax 1 is head h, of softmax 2 head H + h;
    v [B,Nk,H,2hd] (fp32, strided) or packed VT [B,H,64,Npad] (bf16, v_packed).  subln_w fp32 [2hd].
    Returns out [B,Nq,H,2hd] (a fresh contiguous tensor, or the strided 4-D view passed as `out`) = RMSNorm(A1 - lambda A2) * out_scale;
    with save also (lse1, lse2, A1, A2): fp32 [B,H,Nq] twice and the two attention outputs, contiguous [B,Nq,H,2hd]."""
    _need_gpu(q, k, v, subln_w)
    B, Nq, H2, hd = q.shape
    Nk, H = k.shape[1], H2 // 2
    if hd > 32 or (q.dtype == torch.bfloat16 and hd != 32) or hd % 4:
        raise UcHipError(f"differential attention with Q/K head_dim {hd} and V head_dim {2 * hd} is not supported: the HIP kernels run "
                         f"Q/K head_dim 32 with V head_dim 64 (fp32 also smaller multiples of 4); head_dim-128 attention does not exist "
                         f"in this library")
    assert H2 == 2 * H and k.shape[2] == H2 and k.shape[3] == hd and q.stride(3) == 1 and k.stride(3) == 1 and q.dtype == k.dtype == v.dtype
    assert subln_w.dtype == torch.float32 and subln_w.is_contiguous() and subln_w.numel() == 2 * hd
    if out is None:
        out = torch.empty((B, Nq, H, 2 * hd), dtype=q.dtype, device=q.device)
    assert out.shape == (B, Nq, H, 2 * hd) and out.stride(3) == 1 and out.dtype == q.dtype
    d = DiffAttnDesc()
    d.dtype, d.v_layout = _dt(q.dtype), UC_V_PACKED_T if v_packed else UC_V_ROWMAJOR
    d.B, d.H, d.Nq, d.Nk, d.Dqk = B, H, Nq, Nk, hd
    if v_packed:
        assert v.is_contiguous() and v.shape == (B, H, 64, (Nk + 63) // 64 * 64)
    else:
        assert v.shape == (B, Nk, H, 2 * hd) and v.stride(3) == 1
        d.v_sb, d.v_sn, d.v_sh = v.stride(0), v.stride(1), v.stride(2)
    d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.q_sb, d.q_sn, d.q_sh = q.stride(0), q.stride(1), q.stride(2)
    d.k_sb, d.k_sn, d.k_sh = k.stride(0), k.stride(1), k.stride(2)
    d.o_sb, d.o_sn, d.o_sh = out.stride(0), out.stride(1), out.stride(2)
    d.scale, d.lambda_full, d.subln_w, d.rms_eps, d.out_scale = float(scale), float(lambda_full), subln_w.data_ptr(), float(rms_eps), float(out_scale)
    saves = None
    if save:
        lse1 = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        lse2 = torch.empty_like(lse1)
        a1 = torch.empty((B, Nq, H, 2 * hd), dtype=q.dtype, device=q.device)
        a2 = torch.empty_like(a1)
        d.training, d.lse1, d.lse2, d.A1, d.A2 = 1, lse1.data_ptr(), lse2.data_ptr(), a1.data_ptr(), a2.data_ptr()
        saves = (lse1, lse2, a1, a2)
    _lib.check(_lib.load().uc_diff_attention_fwd(C.byref(d), _stream()), "uc_diff_attention_fwd")
    return (out, saves) if save else out


def diff_attention_combine_bwd(dy: torch.Tensor, a1: torch.Tensor, a2: torch.Tensor, lambda_full: float, subln_w: torch.Tensor,
                               rms_eps: float, out_scale: float):
    """dy: [B,N,H,D] view addressed like the forward's output (unit last stride); a1, a2: the saved contiguous [B,N,H,D].
    Returns (dA1, dA2 [B,N,H,D] contiguous, dw fp32 [D], dlambda fp32 [1]); dw and dlambda are reduced in a fixed order (bit-reproducible)."""
    _need_gpu(dy, a1, a2, subln_w)
    B, N, H, D = a1.shape
    assert dy.shape == a1.shape and dy.stride(3) == 1 and a1.is_contiguous() and a2.is_contiguous() and dy.dtype == a1.dtype == a2.dtype
    lib = _lib.load()
    da1, da2 = torch.empty_like(a1), torch.empty_like(a2)
    dw = torch.empty(D, dtype=torch.float32, device=a1.device)
    dl = torch.empty(1, dtype=torch.float32, device=a1.device)
    ws = torch.empty(lib.uc_diff_attention_combine_ws_bytes(B * N * H) // 4, dtype=torch.float32, device=a1.device)
    _lib.check(lib.uc_diff_attention_combine_bwd(dy.data_ptr(), a1.data_ptr(), a2.data_ptr(), da1.data_ptr(), da2.data_ptr(), subln_w.data_ptr(),
                                                 dw.data_ptr(), dl.data_ptr(), ws.data_ptr(), _dt(a1.dtype), B, N, H, D, dy.stride(0), dy.stride(1),
                                                 dy.stride(2), float(lambda_full), float(rms_eps), float(out_scale), _stream()),
               "uc_diff_attention_combine_bwd")
    return da1, da2, dw, dl


def token_pool(x: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """x [B*T, C] (fp32 / bf16 / fp16, unit column stride, row stride >= C) -> fp32 [B, C], the mean over each sample's T rows
    (uc_token_pool: fp32 accumulation, chunk partials added in a fixed order — bit-reproducible)."""
    _need_gpu(x)
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != B * T or B <= 0 or T <= 0:
        raise UcHipError(f"token_pool: [B*T, C] rows with unit column stride expected (got {tuple(x.shape)}, strides {x.stride()}, B={B}, T={T})")
    Cn = x.shape[1]
    lib = _lib.load()
    out = torch.empty((B, Cn), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.uc_token_pool_ws_bytes(B, T, Cn) // 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.uc_token_pool(x.data_ptr(), _dt(x.dtype), x.stride(0), out.data_ptr(), ws.data_ptr(), B, T, Cn, _stream()), "uc_token_pool")
    return out


def token_pool_bwd(g: torch.Tensor, T: int, out_dtype: torch.dtype, gate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g fp32 [B, C] -> [B*T, C] in out_dtype: g[b] / T on each of the sample's T rows, zeroed where gate <= 0 (gate [B*T, C] in
    out_dtype: the pre-activation or the output of the ReLU that fed the pooled sum)."""
    _need_gpu(g, gate)
    if g.dim() != 2 or g.dtype != torch.float32 or not g.is_contiguous() or T <= 0:
        raise UcHipError(f"token_pool_bwd: contiguous fp32 [B, C] gradient expected (got {tuple(g.shape)}, {g.dtype})")
    B, Cn = g.shape
    if gate is not None and (gate.shape != (B * T, Cn) or gate.dtype != out_dtype or gate.stride(1) != 1):
        raise UcHipError(f"token_pool_bwd: gate must be [B*T, C] in {out_dtype} with unit column stride (got {tuple(gate.shape)}, {gate.dtype})")
    vec = 4 if out_dtype == torch.float32 else 8
    ld = (Cn + vec - 1) // vec * vec        # 16-byte rows; the caller sees the [B*T, C] view
    buf = torch.empty((B * T, ld), dtype=out_dtype, device=g.device)
    _lib.check(_lib.load().uc_token_pool_bwd(g.data_ptr(), _p(gate), 0 if gate is None else gate.stride(0), buf.data_ptr(), ld, _dt(out_dtype),
                                             B, T, Cn, _stream()), "uc_token_pool_bwd")
    return buf if ld == Cn else buf[:, :Cn]


# =================================================================================================================
# MoGe head: GroupNorm, replicate pad / crop, half-pixel resize on NHWC maps
# =================================================================================================================
def _nhwc4(x: torch.Tensor):
    _need_gpu(x)
    assert x.is_contiguous() and x.dim() == 4
    return x.shape


def group_norm_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, G: int, eps: float, relu: bool = False):
    """(y, mean [B,G] fp32, rstd [B,G] fp32) of GroupNorm(G) on NHWC x, y = act((x - mean) rstd gamma + beta) in x's dtype
    (uc_group_norm_nhwc: fp32 statistics from per-chunk (mean, M2) merged in a fixed order — bit-reproducible)."""
    B, H, W, Cn = _nhwc4(x)
    _need_gpu(gamma, beta)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.is_contiguous() and beta.is_contiguous()
    assert gamma.numel() == Cn and beta.numel() == Cn
    lib = _lib.load()
    y = torch.empty_like(x)
    mean = torch.empty((B, G), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, G), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.uc_group_norm_nhwc_ws_bytes(B, H, W, Cn, G) // 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.uc_group_norm_nhwc(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      ws.data_ptr(), _dt(x.dtype), B, H, W, Cn, G, float(eps), 1 if relu else 0, _stream()), "uc_group_norm_nhwc")
    return y, mean, rstd


def group_norm_nhwc_bwd(dy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor,
                        gate: Optional[torch.Tensor] = None):
    """(dx in x's dtype, dgamma fp32 [C], dbeta fp32 [C]); gate: the forward's output under a fused ReLU (gradient 0 where gate <= 0)."""
    B, H, W, Cn = _nhwc4(x)
    _need_gpu(dy, gate, gamma)
    assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous()
    assert gate is None or (gate.shape == x.shape and gate.dtype == x.dtype and gate.is_contiguous())
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32 and mean.is_contiguous() and rstd.is_contiguous() and mean.shape == rstd.shape
    assert gamma.dtype == torch.float32 and gamma.is_contiguous() and gamma.numel() == Cn
    G = mean.shape[1]
    lib = _lib.load()
    dx = torch.empty_like(x)
    dg = torch.empty(Cn, dtype=torch.float32, device=x.device)
    db = torch.empty(Cn, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.uc_group_norm_nhwc_bwd_ws_bytes(B, H, W, Cn, G) // 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.uc_group_norm_nhwc_bwd(dy.data_ptr(), x.data_ptr(), _p(gate), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                          dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), _dt(x.dtype), B, H, W, Cn, G, _stream()),
               "uc_group_norm_nhwc_bwd")
    return dx, dg, db


def replicate_pad_nhwc(x: torch.Tensor) -> torch.Tensor:
    "[B,H,W,C] -> [B,H+2,W+2,C], the border pixels repeated (F.pad(mode='replicate') by one pixel)."
    B, H, W, Cn = _nhwc4(x)
    y = torch.empty((B, H + 2, W + 2, Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_replicate_pad_nhwc(x.data_ptr(), y.data_ptr(), _dt(x.dtype), B, H, W, Cn, _stream()), "uc_replicate_pad_nhwc")
    return y


def replicate_pad_nhwc_bwd(dy: torch.Tensor) -> torch.Tensor:
    "adjoint of replicate_pad_nhwc: dy [B,H+2,W+2,C] -> dx [B,H,W,C]"
    B, Hp, Wp, Cn = _nhwc4(dy)
    dx = torch.empty((B, Hp - 2, Wp - 2, Cn), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().uc_replicate_pad_nhwc_bwd(dy.data_ptr(), dx.data_ptr(), _dt(dy.dtype), B, Hp - 2, Wp - 2, Cn, _stream()),
               "uc_replicate_pad_nhwc_bwd")
    return dx


def crop_add_nhwc(x: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    "act(x[:, 1:-1, 1:-1] (+ residual)) of a padded map x [B,H+2,W+2,C] -> [B,H,W,C]"
    B, Hp, Wp, Cn = _nhwc4(x)
    H, W = Hp - 2, Wp - 2
    if residual is not None:
        _need_gpu(residual)
        assert residual.shape == (B, H, W, Cn) and residual.dtype == x.dtype and residual.is_contiguous()
    y = torch.empty((B, H, W, Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_crop_add_nhwc(x.data_ptr(), _p(residual), y.data_ptr(), _dt(x.dtype), B, H, W, Cn, 1 if relu else 0, _stream()),
               "uc_crop_add_nhwc")
    return y


def crop_embed_nhwc(dy: torch.Tensor) -> torch.Tensor:
    "adjoint of the crop: dy [B,H,W,C] -> [B,H+2,W+2,C] with a ring of zeros"
    B, H, W, Cn = _nhwc4(dy)
    y = torch.empty((B, H + 2, W + 2, Cn), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().uc_crop_embed_nhwc(dy.data_ptr(), y.data_ptr(), _dt(dy.dtype), B, H, W, Cn, _stream()), "uc_crop_embed_nhwc")
    return y


def resize_bilinear_nhwc(x: torch.Tensor, Ho: int, Wo: int, align_corners: bool) -> torch.Tensor:
    "bilinear resize of NHWC x to (Ho, Wo): PyTorch's half-pixel rule (align_corners=False) or uc_bilinear_nhwc's (True)"
    B, Hi, Wi, Cn = _nhwc4(x)
    y = torch.empty((B, Ho, Wo, Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_resize_bilinear_nhwc(x.data_ptr(), y.data_ptr(), _dt(x.dtype), B, Hi, Wi, Cn, Ho, Wo, 1 if align_corners else 0,
                                                   _stream()), "uc_resize_bilinear_nhwc")
    return y


def resize_bilinear_nhwc_bwd(dy: torch.Tensor, Hi: int, Wi: int, align_corners: bool) -> torch.Tensor:
    "adjoint of resize_bilinear_nhwc: dy [B,Ho,Wo,C] -> dx [B,Hi,Wi,C]"
    B, Ho, Wo, Cn = _nhwc4(dy)
    dx = torch.empty((B, Hi, Wi, Cn), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().uc_resize_bilinear_nhwc_bwd(dy.data_ptr(), dx.data_ptr(), _dt(dy.dtype), B, Hi, Wi, Cn, Ho, Wo,
                                                       1 if align_corners else 0, _stream()), "uc_resize_bilinear_nhwc_bwd")
    return dx


# --------------------------------------------------------------------------------------------
# streaming steps of the non-image input encoders (csrc/input_encoders.hip)
# --------------------------------------------------------------------------------------------
def unshuffle_rows(x: torch.Tensor, P: int, ld: int, out_dtype: torch.dtype) -> torch.Tensor:
    """nn.PixelUnshuffle(P) of x [B,C,h*P,w*P] (fp32 | bf16, contiguous) as rows [B*h*w, ld] in out_dtype: column c*P*P + u*P + v,
    columns [C*P*P, ld) zero (the K padding of the GEMM that reads the rows)."""
    _need_gpu(x)
    assert x.dim() == 4 and x.is_contiguous() and x.shape[2] % P == 0 and x.shape[3] % P == 0 and ld >= x.shape[1] * P * P
    B, Cn, H, W = x.shape
    h, w = H // P, W // P
    y = torch.empty((B * h * w, ld), dtype=out_dtype, device=x.device)
    _lib.check(_lib.load().uc_unshuffle_rows(x.data_ptr(), _dt(x.dtype), y.data_ptr(), _dt(out_dtype), B, Cn, h, w, P, ld, _stream()),
               "uc_unshuffle_rows")
    return y


def unshuffle_rows_bwd(rows: torch.Tensor, B: int, Cn: int, h: int, w: int, P: int) -> torch.Tensor:
    "adjoint of unshuffle_rows: rows [B*h*w, ld] (fp32 | bf16) -> fp32 [B,C,h*P,w*P]"
    _need_gpu(rows)
    assert rows.dim() == 2 and rows.is_contiguous() and rows.shape[0] == B * h * w and rows.shape[1] >= Cn * P * P
    y = torch.empty((B, Cn, h * P, w * P), dtype=torch.float32, device=rows.device)
    _lib.check(_lib.load().uc_unshuffle_rows_bwd(rows.data_ptr(), _dt(rows.dtype), y.data_ptr(), B, Cn, h, w, P, rows.shape[1], _stream()),
               "uc_unshuffle_rows_bwd")
    return y


def act(x: torch.Tensor, name: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    "act(x) for name in ('gelu', 'relu') (exact-erf GELU), fp32 | bf16; out=x works in place"
    _need_gpu(x, out)
    if name not in ("gelu", "relu"):
        raise UcHipError(f"act: {name!r} has no kernel (supported: 'gelu', 'relu')")
    assert x.is_contiguous()
    y = torch.empty_like(x) if out is None else out
    assert y.is_contiguous() and y.shape == x.shape and y.dtype == x.dtype
    _lib.check(_lib.load().uc_act(x.data_ptr(), y.data_ptr(), _dt(x.dtype), ACT[name], x.numel(), _stream()), "uc_act")
    return y


def ln_pe_ln(x: torch.Tensor, B: int, N: int, ln1: Optional[Tuple[torch.Tensor, torch.Tensor, float]], pe: Optional[torch.Tensor],
             ln2: Optional[Tuple[torch.Tensor, torch.Tensor, float]], out_dtype: torch.dtype, want_mid: bool = False):
    """y = LN2(LN1(x) + pe) over rows x [B*N, C] (fp32 | bf16) in one pass; ln1 / ln2: (gamma, beta, eps) fp32 or None (Identity),
    pe: fp32 [N, C] or None.  Returns y, or (y, mid) with want_mid: mid fp32 [B*N, C] is the input of LN2."""
    f32 = [t for n in (ln1, ln2) if n is not None for t in n[:2]] + ([pe] if pe is not None else [])
    _need_gpu(x, *f32)
    Cn = x.shape[-1]
    assert x.dim() == 2 and x.is_contiguous() and x.shape[0] == B * N
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in f32) and all(t.numel() == Cn for n in (ln1, ln2) if n is not None for t in n[:2])
    assert pe is None or pe.shape == (N, Cn)
    y = torch.empty((B * N, Cn), dtype=out_dtype, device=x.device)
    mid = torch.empty((B * N, Cn), dtype=torch.float32, device=x.device) if want_mid else None
    g1, b1, e1 = ln1 if ln1 is not None else (None, None, 0.0)
    g2, b2, e2 = ln2 if ln2 is not None else (None, None, 0.0)
    _lib.check(_lib.load().uc_ln_pe_ln(x.data_ptr(), _dt(x.dtype), _p(g1), _p(b1), float(e1), _p(pe), _p(g2), _p(b2), float(e2), y.data_ptr(),
                                       _dt(out_dtype), _p(mid), B, N, Cn, _stream()), "uc_ln_pe_ln")
    return (y, mid) if want_mid else y


def ln_param_grads(x: torch.Tensor, dy: torch.Tensor, eps: float):
    """(dgamma, dbeta) fp32 [C] of y = LN(x) over rows x [rows, C] with cotangent dy (fp32 | bf16 each), every sum in a fixed order:
    the same bits on every run (uc_layernorm_bwd's atomics do not give that)."""
    _need_gpu(x, dy)
    assert x.dim() == 2 and x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape
    rows, Cn = x.shape
    lib = _lib.load()
    dg = torch.empty(Cn, dtype=torch.float32, device=x.device)
    db = torch.empty(Cn, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(2, lib.uc_ln_param_grads_ws_bytes(rows, Cn) // 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.uc_ln_param_grads(x.data_ptr(), _dt(x.dtype), dy.data_ptr(), _dt(dy.dtype), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), rows, Cn,
                                     float(eps), _stream()), "uc_ln_param_grads")
    return dg, db


# --------------------------------------------------------------------------------------------
# the fused ViT stem (csrc/vit_stem.hip): class token + position table + LayerNorm in one pass, and its backward
# --------------------------------------------------------------------------------------------
def _stem_check(tok, cls, pos, gamma):
    _need_gpu(tok, cls, pos, gamma)
    assert tok.dim() == 3 and tok.is_contiguous() and tok.dtype in (torch.float32, torch.bfloat16)
    B, hw, Cn = tok.shape
    T = hw + (cls is not None)
    for t, shape in ((cls, (Cn,)), (pos, (T, Cn)), (gamma, (Cn,))):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape)
    return B, hw, Cn, T


def vit_stem(tok: torch.Tensor, cls: Optional[torch.Tensor], pos: Optional[torch.Tensor], ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]],
             out_dtype: torch.dtype, want_stats: bool = False):
    """y [B, T, C] = LN(z), z[b, t] = (t < ncls ? cls : tok[b, t - ncls]) + pos[t], T = hw + ncls, ncls = (cls is not None).
    tok [B, hw, C] fp32 | bf16; cls fp32 [C] or None; pos fp32 [T, C] or None; ln: (gamma, beta, eps) fp32 or None (y = z).  Returns y,
    or (y, stats) with want_stats: fp32 [B*T, 2] (mean, rstd) of every row, which vit_stem_bwd needs."""
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    B, hw, Cn, T = _stem_check(tok, cls, pos, g)
    _need_gpu(b)
    assert b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.numel() == Cn)
    y = torch.empty((B, T, Cn), dtype=out_dtype, device=tok.device)
    stats = torch.empty((B * T, 2), dtype=torch.float32, device=tok.device) if (want_stats and ln is not None) else None
    _lib.check(_lib.load().uc_vit_stem(tok.data_ptr(), _dt(tok.dtype), _p(cls), _p(pos), _p(g), _p(b), float(eps), y.data_ptr(), _dt(out_dtype),
                                       _p(stats), B, hw, Cn, _stream()), "uc_vit_stem")
    return (y, stats) if want_stats else y


def vit_stem_bwd(dy: torch.Tensor, tok: torch.Tensor, cls: Optional[torch.Tensor], pos: Optional[torch.Tensor], gamma: Optional[torch.Tensor],
                 stats: Optional[torch.Tensor], need_dtok: bool = True):
    """(dtok, dcls, dpos, dgamma, dbeta) of vit_stem for the cotangent dy [B, T, C] (fp32 | bf16): dtok in tok's dtype (None unless
    need_dtok), the others fp32 and None where the forward had no such input.  Every sum runs in a fixed order: the same bits on
    every call."""
    B, hw, Cn, T = _stem_check(tok, cls, pos, gamma)
    _need_gpu(dy, stats)
    assert dy.is_contiguous() and tuple(dy.shape) == (B, T, Cn) and dy.dtype in (torch.float32, torch.bfloat16)
    assert gamma is None or (stats is not None and stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2 * B * T)
    dev = tok.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
    dtok = torch.empty_like(tok) if need_dtok else None
    dcls = new(Cn) if cls is not None else None
    dpos = new(T, Cn) if pos is not None else None
    dg, db = (new(Cn), new(Cn)) if gamma is not None else (None, None)
    lib = _lib.load()
    ws = new(max(4, lib.uc_vit_stem_ws_bytes(B, T, Cn) // 4))
    _lib.check(lib.uc_vit_stem_bwd(dy.data_ptr(), _dt(dy.dtype), tok.data_ptr(), _dt(tok.dtype), _p(cls), _p(pos), _p(gamma), _p(stats), _p(dtok),
                                   _p(dcls), _p(dpos), _p(dg), _p(db), ws.data_ptr(), B, hw, Cn, _stream()), "uc_vit_stem_bwd")
    return dtok, dcls, dpos, dg, db


# =================================================================================================================
# Cosmos image tokenizer: Haar patcher, GroupNorm + SiLU, Downsample operand rows, nearest x2 upsample, row softmax
# =================================================================================================================
def haar_patch(img: torch.Tensor, out_dtype: torch.dtype, ld: Optional[int] = None, scale: float = 1.0) -> torch.Tensor:
    """fp32 NCHW image [B,C,H,W] (H, W multiples of 4) -> NHWC [B,H/4,W/4,ld] in out_dtype: the two-level Haar transform in the first
    16 C channels (index s2 * 4C + s1 * C + c), zeros in the others (uc_haar_patch)."""
    _need_gpu(img)
    assert img.dim() == 4 and img.is_contiguous() and img.dtype == torch.float32
    B, Cn, H, W = img.shape
    ld = 16 * Cn if ld is None else ld
    y = torch.empty((B, H // 4, W // 4, ld), dtype=out_dtype, device=img.device)
    _lib.check(_lib.load().uc_haar_patch(img.data_ptr(), y.data_ptr(), _dt(out_dtype), B, Cn, H, W, ld, float(scale), _stream()), "uc_haar_patch")
    return y


def haar_unpatch(rows: torch.Tensor, Cn: int, scale: float = 1.0) -> torch.Tensor:
    "NHWC [B,h,w,ld] (ld >= 16 Cn) -> fp32 NCHW [B,Cn,4h,4w]: the inverse of haar_patch, times scale (uc_haar_unpatch)."
    B, h, w, ld = _nhwc4(rows)
    img = torch.empty((B, Cn, 4 * h, 4 * w), dtype=torch.float32, device=rows.device)
    _lib.check(_lib.load().uc_haar_unpatch(rows.data_ptr(), _dt(rows.dtype), img.data_ptr(), B, Cn, 4 * h, 4 * w, ld, float(scale), _stream()),
               "uc_haar_unpatch")
    return img


def group_norm_silu_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, G: int, eps: float):
    "(y, mean [B,G], rstd [B,G]) of y = silu(GroupNorm(x)) on NHWC x: group_norm_nhwc's statistics, SiLU in the apply pass."
    B, H, W, Cn = _nhwc4(x)
    _need_gpu(gamma, beta)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.is_contiguous() and beta.is_contiguous()
    assert gamma.numel() == Cn and beta.numel() == Cn
    lib = _lib.load()
    y = torch.empty_like(x)
    mean = torch.empty((B, G), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, G), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.uc_group_norm_silu_nhwc_ws_bytes(B, H, W, Cn, G) // 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.uc_group_norm_silu_nhwc(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           ws.data_ptr(), _dt(x.dtype), B, H, W, Cn, G, float(eps), _stream()), "uc_group_norm_silu_nhwc")
    return y, mean, rstd


def group_norm_silu_nhwc_bwd(dy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    "(dx, dgamma, dbeta) of group_norm_silu_nhwc; the pre-activation is recomputed from x."
    B, H, W, Cn = _nhwc4(x)
    _need_gpu(dy, gamma, beta)
    assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous()
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32 and mean.is_contiguous() and rstd.is_contiguous() and mean.shape == rstd.shape
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == Cn for t in (gamma, beta))
    G = mean.shape[1]
    lib = _lib.load()
    dx = torch.empty_like(x)
    dg = torch.empty(Cn, dtype=torch.float32, device=x.device)
    db = torch.empty(Cn, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.uc_group_norm_silu_nhwc_bwd_ws_bytes(B, H, W, Cn, G) // 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.uc_group_norm_silu_nhwc_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                               dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), _dt(x.dtype), B, H, W, Cn, G, _stream()),
               "uc_group_norm_silu_nhwc_bwd")
    return dx, dg, db


def down2_gather(x: torch.Tensor) -> torch.Tensor:
    """NHWC x [B,H,W,C] (H, W even) -> operand rows [B*(H/2)*(W/2), 9C], K ordered (ky,kx,c), of the 3x3 / stride-2 convolution padded on
    the right and bottom only (uc_down2_gather)."""
    B, H, W, Cn = _nhwc4(x)
    if H % 2 or W % 2:
        raise UcHipError(f"down2_gather: the Downsample of an odd map ({H} x {W}) has no HIP path")
    rows = torch.empty((B * (H // 2) * (W // 2), 9 * Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_down2_gather(x.data_ptr(), rows.data_ptr(), _dt(x.dtype), B, H, W, Cn, _stream()), "uc_down2_gather")
    return rows


def down2_gather_bwd(drows: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    "adjoint of down2_gather: drows [B*(H/2)*(W/2), 9C] -> dx [B,H,W,C]"
    _need_gpu(drows)
    assert drows.dim() == 2 and drows.is_contiguous() and drows.shape[0] == B * (H // 2) * (W // 2) and drows.shape[1] % 9 == 0
    Cn = drows.shape[1] // 9
    dx = torch.empty((B, H, W, Cn), dtype=drows.dtype, device=drows.device)
    _lib.check(_lib.load().uc_down2_gather_bwd(drows.data_ptr(), dx.data_ptr(), _dt(drows.dtype), B, H, W, Cn, _stream()), "uc_down2_gather_bwd")
    return dx


def upsample2_nhwc(x: torch.Tensor) -> torch.Tensor:
    "[B,H,W,C] -> [B,2H,2W,C], every pixel repeated 2x2 (nearest neighbour)"
    B, H, W, Cn = _nhwc4(x)
    y = torch.empty((B, 2 * H, 2 * W, Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_upsample2_nhwc(x.data_ptr(), y.data_ptr(), _dt(x.dtype), B, H, W, Cn, _stream()), "uc_upsample2_nhwc")
    return y


def upsample2_nhwc_bwd(dy: torch.Tensor) -> torch.Tensor:
    "adjoint of upsample2_nhwc: dy [B,2H,2W,C] -> the sum of every 2x2 block [B,H,W,C]"
    B, H2, W2, Cn = _nhwc4(dy)
    assert H2 % 2 == 0 and W2 % 2 == 0
    dx = torch.empty((B, H2 // 2, W2 // 2, Cn), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().uc_upsample2_nhwc_bwd(dy.data_ptr(), dx.data_ptr(), _dt(dy.dtype), B, H2 // 2, W2 // 2, Cn, _stream()),
               "uc_upsample2_nhwc_bwd")
    return dx


def softmax_rows(s: torch.Tensor, scale: float, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """P = softmax(scale * s) per row.  s: fp32 [rows, N] (unit column stride, any row stride).  Returns P [rows, N] in out_dtype; with
    `out` [rows, ldp >= N] given, P is its first N columns and the others are written as zeros (the K padding of the next product)."""
    _need_gpu(s, out)
    assert s.dim() == 2 and s.stride(1) == 1 and s.dtype == torch.float32
    rows, N = s.shape
    if out is None:
        out = torch.empty((rows, N), dtype=out_dtype, device=s.device)
    assert out.dim() == 2 and out.is_contiguous() and out.shape[0] == rows and out.shape[1] >= N and out.dtype == out_dtype
    _lib.check(_lib.load().uc_softmax_rows(s.data_ptr(), s.stride(0), out.data_ptr(), _dt(out_dtype), out.shape[1], rows, N, float(scale), _stream()),
               "uc_softmax_rows")
    return out


def softmax_rows_bwd(p: torch.Tensor, dp: torch.Tensor, N: int, scale: float) -> torch.Tensor:
    """dS = scale * P * (dP - sum(dP * P)) per row.  p: [rows, ldp] contiguous (P in its first N columns), dp: fp32 [rows, N] (any row
    stride).  Returns dS shaped like p, zeros in the columns beyond N."""
    _need_gpu(p, dp)
    assert p.dim() == 2 and p.is_contiguous() and dp.dim() == 2 and dp.stride(1) == 1 and dp.dtype == torch.float32
    assert dp.shape == (p.shape[0], N) and p.shape[1] >= N
    ds = torch.empty_like(p)
    _lib.check(_lib.load().uc_softmax_rows_bwd(p.data_ptr(), dp.data_ptr(), dp.stride(0), ds.data_ptr(), _dt(p.dtype), p.shape[1], p.shape[0], N,
                                               float(scale), _stream()), "uc_softmax_rows_bwd")
    return ds


# ---- DINOv3 ConvNeXt: depthwise 7x7 convolution and the stage downsample's operand rows (csrc/dwconv.hip) --------------------------
def dwconv7x7_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, flip: bool = False) -> torch.Tensor:
    """Depthwise 7x7 / padding 3 convolution of NHWC x [B,H,W,C] (f32 | bf16 | f16): w fp32 [49, C] tap-major, bias fp32 [C] or None.
    flip: tap 48 - t in place of t — the data gradient of the same convolution (uc_dwconv7x7_nhwc)."""
    B, H, W, Cn = _nhwc4(x)
    _need_gpu(w, bias)
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (49, Cn)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cn)
    y = torch.empty_like(x)
    _lib.check(_lib.load().uc_dwconv7x7_nhwc(x.data_ptr(), w.data_ptr(), _p(bias), y.data_ptr(), _dt(x.dtype), B, H, W, Cn, int(bool(flip)), _stream()),
               "uc_dwconv7x7_nhwc")
    return y


def dwconv7x7_nhwc_wgrad(x: torch.Tensor, dy: torch.Tensor, bias: bool = True, ws: Optional[torch.Tensor] = None):
    """(dw fp32 [49, C], db fp32 [C] | None) of dwconv7x7_nhwc for NHWC x and dy of one dtype (uc_dwconv7x7_nhwc_wgrad).  ws: an fp32
    workspace of at least uc_dwconv7x7_nhwc_wgrad_ws_bytes(B, H, W, C) bytes; allocated here when None."""
    B, H, W, Cn = _nhwc4(x)
    _need_gpu(dy, ws)
    assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous()
    lib = _lib.load()
    need = lib.uc_dwconv7x7_nhwc_wgrad_ws_bytes(B, H, W, Cn)
    if ws is None:
        ws = torch.empty(max(1, need // 4), dtype=torch.float32, device=x.device)
    elif ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() * 4 < need:
        raise UcHipError(f"uc_dwconv7x7_nhwc_wgrad: the workspace holds {ws.numel() * ws.element_size()} bytes of {ws.dtype}, "
                         f"B={B} H={H} W={W} C={Cn} needs {need} bytes of contiguous fp32")
    dw = torch.empty((49, Cn), dtype=torch.float32, device=x.device)
    db = torch.empty(Cn, dtype=torch.float32, device=x.device) if bias else None
    _lib.check(lib.uc_dwconv7x7_nhwc_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _p(db), ws.data_ptr(), _dt(x.dtype), B, H, W, Cn, _stream()),
               "uc_dwconv7x7_nhwc_wgrad")
    return dw, db


def patch2_gather_nhwc(x: torch.Tensor) -> torch.Tensor:
    """NHWC x [B,H,W,C] -> operand rows [B*(H//2)*(W//2), 4C], K ordered (ky,kx,c), of Conv2d(k = 2, stride = 2); an odd last row or
    column is dropped (uc_patch2_gather_nhwc)."""
    B, H, W, Cn = _nhwc4(x)
    rows = torch.empty((B * (H // 2) * (W // 2), 4 * Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().uc_patch2_gather_nhwc(x.data_ptr(), rows.data_ptr(), _dt(x.dtype), B, H, W, Cn, _stream()), "uc_patch2_gather_nhwc")
    return rows


def patch2_gather_nhwc_bwd(drows: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    "adjoint of patch2_gather_nhwc: drows [B*(H//2)*(W//2), 4C] -> dx [B,H,W,C], zero in an odd last row or column"
    _need_gpu(drows)
    assert drows.dim() == 2 and drows.is_contiguous() and drows.shape[0] == B * (H // 2) * (W // 2) and drows.shape[1] % 4 == 0
    Cn = drows.shape[1] // 4
    dx = torch.empty((B, H, W, Cn), dtype=drows.dtype, device=drows.device)
    _lib.check(_lib.load().uc_patch2_gather_nhwc_bwd(drows.data_ptr(), dx.data_ptr(), _dt(drows.dtype), B, H, W, Cn, _stream()),
               "uc_patch2_gather_nhwc_bwd")
    return dx
