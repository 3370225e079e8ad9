"""DINOv3 ViT encoder (reference wrapper: encoders/dinov3.py, `DINOv3Encoder` / `DINOv3IntermediateFeatureReturner`) on the HIP kernels.

The reference obtains the network from `torch.hub.load(<local clone of the DINOv3 repository>, "dinov3_vit{s,s+,b,l,h+}16")`: third-party
code that is NOT under the reference tree and cannot be fetched here.  `DINOv3VisionTransformerParams` therefore restates the PUBLISHED
DINOv3 ViT architecture (patch 16, class token + 4 register ("storage") tokens, NO learned position embedding, axial RoPE on the patch
tokens of q and k, pre-LN blocks with LayerScale, erf-GELU MLP or SwiGLU FFN, LayerNorm eps 1e-5, a q | k | v projection whose K bias
is masked to zero) under the hub checkpoints' parameter names AS FAR AS THEY ARE REMEMBERED — the hub code was not available
when this was written, so these names are UNVERIFIED:
    patch_embed.proj.{weight,bias}, cls_token [1,1,D], storage_tokens [1,4,D], mask_token [1,D] (kept, unused), rope_embed.periods
    (buffer [head_dim/4]), blocks.i.{norm1, attn.qkv.{weight,bias,bias_mask}, attn.proj, ls1.gamma, norm2, mlp.{fc1,fc2} | mlp.{w1,w2,w3},
    ls2.gamma}, norm.
PARITY: pinned to an independent implementation of the same network, transformers' DINOv3ViTModel (tests/golden/dinov3_hf.npz:
outputs and parameter gradients; the RoPE tables bit for bit on the CPU); UNPINNED against the hub code and the hub checkpoints' names.
`uniception_amd.tools.convert_checkpoint --mode dinov3` maps a transformers state_dict onto these names.

Kernel mapping: patch gather + GEMM -> uc_assemble_tokens (cls | registers | patches; there is no position table: zeros) -> per
block: LayerNorm -> QKV GEMM with bias (V through the packed-VT epilogue where the route has one) -> uc_rope_axial on q | k in place
(ONE launch, prefix tokens untouched; csrc/rope_axial.hip) -> flash attention -> proj GEMM with LayerScale folded + residual ->
LayerNorm -> fc1 GEMM + GELU -> fc2 GEMM | w1|w2 GEMM -> uc_swiglu -> w3 GEMM (LayerScale folded) + residual -> final LayerNorm ->
uc_token_slice.  Training: the sub-layers are the HIP forward + backward Functions of autograd.py; the attention backward returns the
gradients of the ROTATED q | k and one uc_rope_axial(inverse) pass over dq | dk turns them back; the token assembly and the output
split are a handful of torch ops on small tensors (cls_token / storage_tokens receive their gradients from autograd).  In train mode
the RoPE coordinates are augmented per forward (libs/dinov3/rope.py) — two tiny tables rebuilt, no kernel work.

DINOv3 ConvNeXt (reference wrapper: `DINOv3ConvNextEncoder` / `DINOv3ConvNextIntermediateFeatureReturner`, hub entries
`dinov3_convnext_{tiny,small,base,large}`).  `DINOv3ConvNextParams` restates the PUBLISHED ConvNeXt: a 4x4 / stride-4 stem convolution
+ LayerNorm, four stages of layers  x + gamma * pwconv2(GELU(pwconv1(LN(dwconv7x7(x)))))  (LayerNorm eps 1e-6, erf-GELU, a LayerScale
`gamma` per layer), LayerNorm + 2x2 / stride-2 convolution between the stages, and a final LayerNorm, under the original ConvNeXt
parameter names AS FAR AS THEY ARE REMEMBERED — the hub code was not available, so these names are UNVERIFIED:
    downsample_layers.0.{0 (conv 4x4 s4), 1 (LayerNorm)}, downsample_layers.{1,2,3}.{0 (LayerNorm), 1 (conv 2x2 s2)},
    stages.i.j.{dwconv, norm, pwconv1, pwconv2}.{weight,bias}, stages.i.j.gamma, norm.
Equally UNVERIFIED is what the hub model does with `model.patch_size` (the wrapper sets it) on intermediate maps: the stage outputs
are handed out at their native strides 4, 8, 16, 32 here; resampling them to the `patch_size` grid is NOT built.
PARITY: pinned to transformers' DINOv3ConvNextModel (tests/golden/dinov3_convnext_hf.npz: final features, the four stage outputs,
parameter gradients); UNPINNED against the hub code and checkpoints.  `convert_checkpoint --mode dinov3_convnext` maps a transformers
state_dict onto these names.

Kernel mapping (every activation stays NHWC, rows [B H W, C], between layers; NCHW only at the public boundary): uc_unshuffle_rows
(the 4x4 patch rows, K = 48 zero-padded to 64) -> stem GEMM -> uc_layernorm -> per layer: uc_dwconv7x7_nhwc (csrc/dwconv.hip) ->
uc_layernorm -> pwconv1 GEMM + GELU -> pwconv2 GEMM with gamma folded into weight and bias and the LAYER INPUT as the epilogue residual
-> between stages: uc_layernorm -> uc_patch2_gather_nhwc -> GEMM with the weight permuted once to (ky, kx, c) -> final norm per pixel
-> uc_nhwc_to_nchw.  The pooled "class" row the hub model prepends is normalised independently of the patch rows and never returned
by the wrapper: it is not computed.  Training: DwConv7x7 (backward = the same kernel with flipped taps + uc_dwconv7x7_nhwc_wgrad),
Patch2Gather, and the existing LayerNorm / linear / MLP Functions; LayerScale and the residual sum are differentiable products there.
"""
from typing import List, Optional, Union

import torch
import torch.nn as nn

from ... import autograd, engine, ops
from ..libs.dinov3.rope import RoPEAxial
from ..utils import sublayers
from ..utils.intermediate_feature_return import IntermediateFeatureReturner, feature_take_indices
from .base import UniCeptionEncoderBase, UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderOutput

# embed dim, depth, heads, FFN kind, FFN hidden width (head_dim 64 throughout)
_SIZES = {"small": (384, 12, 6, "mlp", 1536), "small+": (384, 12, 6, "swiglu", 1536), "base": (768, 12, 12, "mlp", 3072),
          "large": (1024, 24, 16, "mlp", 4096), "huge+": (1280, 32, 20, "swiglu", 5120)}
_UNSERVED = {"7b": (4096, 40, 32)}       # head_dim 128, untied class-token norms
NUM_STORAGE_TOKENS = 4


def resolve_size(size):
    """(embed dim, depth, heads, FFN kind, FFN hidden) of a named size, or of a dict(embed_dim=, depth=, num_heads=, ffn="mlp"|"swiglu",
    ffn_hidden=) — custom-trained variants and the tiny configurations of the tests."""
    if isinstance(size, dict):
        cfg = (size["embed_dim"], size["depth"], size["num_heads"], size.get("ffn", "mlp"), size.get("ffn_hidden", 4 * size["embed_dim"]))
        name = "custom"
    elif size in _UNSERVED:
        D, _, H = _UNSERVED[size]
        raise engine.UcHipError(f"DINOv3 '{size}' has head_dim {D // H} (and untied class-token norms): the attention and RoPE route of this "
                                f"encoder serves head_dim 64; supported sizes: {sorted(_SIZES)}")
    elif size in _SIZES:
        cfg, name = _SIZES[size], size
    else:
        raise engine.UcHipError(f"unknown DINOv3 size '{size}'; supported: {sorted(_SIZES)}")
    D, _, H, ffn, _ = cfg
    if D % H != 0 or D // H != 64:
        raise engine.UcHipError(f"DINOv3 '{name}': head_dim {D / H:g} is not served (head_dim 64 only)")
    if ffn not in ("mlp", "swiglu"):
        raise engine.UcHipError(f"DINOv3 '{name}': unknown FFN kind '{ffn}' (mlp | swiglu)")
    return cfg


class _Lin:
    "What the sub-layer runners read of an nn.Linear (weight, bias, out_features), for weights that are computed from parameters."
    __slots__ = ("weight", "bias", "out_features", "__weakref__")

    def __init__(self, weight, bias):
        self.weight, self.bias, self.out_features = weight, bias, weight.shape[0]


class _KMaskedLinear(nn.Linear):
    "The published LinearKMaskedBias: q | k | v projection whose effective bias is bias * bias_mask, bias_mask = 1 | 0 | 1 (a buffer)."

    def __init__(self, dim):
        super().__init__(dim, 3 * dim, bias=True)
        mask = torch.ones(3 * dim)
        mask[dim:2 * dim] = 0.0
        self.register_buffer("bias_mask", mask)
        object.__setattr__(self, "_served", None)

    def served(self, train: bool) -> _Lin:
        "the linear the kernels see: training — a differentiable product (a new object per forward); inference — prepared once"
        if train:
            return _Lin(self.weight, self.bias * self.bias_mask.to(self.bias.dtype))
        b = engine.prepared(self, "masked_bias", (self.bias, self.bias_mask), lambda: (self.bias.detach().float() * self.bias_mask.float()).contiguous())
        s = self._served
        if s is None or s.weight is not self.weight or s.bias is not b:
            s = _Lin(self.weight, b)
            object.__setattr__(self, "_served", s)
        return s


class _Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = _KMaskedLinear(dim)
        self.proj = nn.Linear(dim, dim, bias=True)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden, bias=True)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim, bias=True)


class _SwiGLUFFN(nn.Module):
    "The published SwiGLUFFN under its parameter names: w3(silu(w1(x)) * w2(x))."

    def __init__(self, dim, hidden):
        super().__init__()
        self.w1 = nn.Linear(dim, hidden, bias=True)
        self.w2 = nn.Linear(dim, hidden, bias=True)
        self.w3 = nn.Linear(hidden, dim, bias=True)
        object.__setattr__(self, "_served", None)

    def w12(self, train: bool) -> _Lin:
        "w1 | w2 as the one concatenated linear sublayers.swiglu takes: training — a differentiable cat; inference — prepared once"
        if train:
            return _Lin(torch.cat([self.w1.weight, self.w2.weight], 0), torch.cat([self.w1.bias, self.w2.bias], 0))
        w, b = engine.prepared(self, "w12", (self.w1.weight, self.w2.weight, self.w1.bias, self.w2.bias),
                               lambda: (torch.cat([self.w1.weight.detach(), self.w2.weight.detach()], 0).contiguous(),
                                        torch.cat([self.w1.bias.detach(), self.w2.bias.detach()], 0).contiguous()))
        s = self._served
        if s is None or s.weight is not w:
            s = _Lin(w, b)
            object.__setattr__(self, "_served", s)
        return s


class _LayerScale(nn.Module):
    def __init__(self, dim, init_values=1.0):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class _Block(nn.Module):
    "x += ls1(attn(norm1(x), rope)); x += ls2(mlp(norm2(x)))  — parameter container; the fused pipeline is in forward_tokens."

    def __init__(self, dim, num_heads, ffn, hidden):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-5)
        self.attn = _Attention(dim, num_heads)
        self.ls1 = _LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-5)
        self.mlp = _SwiGLUFFN(dim, hidden) if ffn == "swiglu" else _Mlp(dim, hidden)
        self.ls2 = _LayerScale(dim)

    def forward_tokens(self, x2d, B, N, dt, rope):
        "rope: the bound axial RoPE of this forward pass (libs/dinov3/rope.py) — the same tables in every block and in a re-computation"
        a, mlp = self.attn, self.mlp
        train = autograd.grad_needed(x2d, *self.parameters())
        x2d = sublayers.self_attn(x2d, self.norm1, a.qkv.served(train), a.proj, B, N, a.num_heads, rope, None, a.scale, dt, train=train,
                                  gamma=sublayers.gamma_of(self.ls1))
        if isinstance(mlp, _SwiGLUFFN):
            return sublayers.swiglu(x2d, self.norm2, mlp.w12(train), mlp.w3, dt, train=train, gamma=sublayers.gamma_of(self.ls2))
        return sublayers.mlp(x2d, self.norm2, mlp.fc1, mlp.fc2, mlp.act, dt, train=train, gamma=sublayers.gamma_of(self.ls2))


class _PatchEmbed(nn.Module):
    def __init__(self, patch_size, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch_size, stride=patch_size)


class _RopeEmbed(nn.Module):
    "Holder of the published `rope_embed.periods` buffer (base^(4j/head_dim)); the tables are built by RoPEAxial from the base itself."

    def __init__(self, head_dim, base):
        super().__init__()
        self.register_buffer("periods", base ** (4 * torch.arange(head_dim // 4, dtype=torch.float32) / head_dim))


class DINOv3VisionTransformerParams(nn.Module):
    "Parameters of a DINOv3 ViT under the hub checkpoints' names (`model.*` inside DINOv3Encoder)."

    def __init__(self, size, patch_size: int = 16, rope_base: float = 100.0, pos_embed_shift: Optional[float] = None,
                 pos_embed_jitter: Optional[float] = None, pos_embed_rescale: Optional[float] = 2.0):
        super().__init__()
        dim, depth, heads, ffn, hidden = resolve_size(size)
        self.embed_dim, self.patch_size, self.num_heads, self.n_storage_tokens = dim, patch_size, heads, NUM_STORAGE_TOKENS
        self.patch_embed = _PatchEmbed(patch_size, dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.storage_tokens = nn.Parameter(torch.zeros(1, NUM_STORAGE_TOKENS, dim))
        self.mask_token = nn.Parameter(torch.zeros(1, dim))          # (masked-image pre-training only: kept so checkpoints load, unused)
        self.rope_embed = _RopeEmbed(dim // heads, rope_base)
        self.blocks = nn.ModuleList([_Block(dim, heads, ffn, hidden) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-5)
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.storage_tokens, std=0.02)
        # (a plain object: no parameters, outside the module tree and the state_dict)
        object.__setattr__(self, "rope", RoPEAxial(dim // heads, base=rope_base, shift=pos_embed_shift, jitter=pos_embed_jitter,
                                                    rescale=pos_embed_rescale))

    @property
    def num_prefix_tokens(self) -> int:
        return 1 + self.n_storage_tokens


class DINOv3Encoder(UniCeptionViTEncoderBase):
    """UniCeption DINOv3 ViT Encoder.  dinov3_repo_dir is accepted and ignored (there is no torch.hub here: the architecture is built
    directly); `weights` is a file holding the network's state_dict under the hub names, `pretrained_checkpoint_path` a
    {"model": state_dict of this wrapper} file.  pos_embed_shift / pos_embed_jitter / pos_embed_rescale: the train-mode augmentation of
    the RoPE coordinates (the published configurations train with rescale 2 only).  size: a name, or a dict (resolve_size)."""

    def __init__(self, name: str, dinov3_repo_dir: Optional[str] = None, data_norm_type: str = "dinov3", patch_size: int = 16,
                 size="large", weights: Optional[str] = None, pretrained_checkpoint_path: str = None,
                 gradient_checkpointing: bool = False, keep_first_n_layers: Optional[int] = None, disable_torch_compile_for_pe=False,
                 pos_embed_shift: Optional[float] = None, pos_embed_jitter: Optional[float] = None,
                 pos_embed_rescale: Optional[float] = 2.0, *args, **kwargs):
        super().__init__(name=name, data_norm_type=data_norm_type, patch_size=patch_size,
                         gradient_checkpointing=gradient_checkpointing, *args, **kwargs)
        self.version = size
        self.enc_embed_dim = resolve_size(size)[0]
        self.model = DINOv3VisionTransformerParams(size, patch_size, pos_embed_shift=pos_embed_shift, pos_embed_jitter=pos_embed_jitter,
                                                   pos_embed_rescale=pos_embed_rescale)
        if weights:
            print(f"Loading DINOv3 weights from {weights}")
            sd = torch.load(weights, map_location="cpu", weights_only=False)
            print(self.model.load_state_dict(sd["model"] if "model" in sd and isinstance(sd["model"], dict) else sd))
        if keep_first_n_layers is not None:
            self.model.blocks = nn.ModuleList(self.model.blocks[:keep_first_n_layers])
        if self.gradient_checkpointing:
            for i in range(len(self.model.blocks)):
                self.model.blocks[i] = self.wrap_module_with_gradient_checkpointing(self.model.blocks[i])
        if pretrained_checkpoint_path:
            print(f"Loading custom pretrained DINOv3 checkpoint from {pretrained_checkpoint_path}")
            ckpt = torch.load(pretrained_checkpoint_path, map_location="cpu", weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    # ---- token-stream core ---------------------------------------------------------------------
    def _check(self, encoder_input):
        self._check_data_normalization_type(encoder_input.data_norm_type)
        assert isinstance(encoder_input.image, torch.Tensor), "Input must be a torch.Tensor"
        assert encoder_input.image.ndim == 4, "Input must be of shape (B, C, H, W)"
        B, C, H, W = encoder_input.image.shape
        assert C == 3, "Input must have 3 channels"
        assert H % self.patch_size == 0 and W % self.patch_size == 0, \
            f"Input shape must be divisible by patch size: {self.patch_size}"
        return B, H // self.patch_size, W // self.patch_size

    def _tokens(self, image, h0, w0):
        "[B, 1 + 4 + h0*w0, D] = [cls | storage tokens | patch tokens] (no position embedding is added: the positions are the RoPE's)"
        m = self.model
        P = self.patch_size
        dt = engine.compute_dtype()
        pdt = dt if (3 * P * P) % 8 == 0 else torch.float32
        img = image.float().contiguous() if (image.dtype != torch.float32 or not image.is_contiguous()) else image
        B = image.shape[0]
        if autograd.grad_needed(image, *m.parameters()):
            tok = autograd.patch_embed(img, m.patch_embed.proj, P, pdt).view(B, h0 * w0, -1)
            x = torch.cat([m.cls_token.float().expand(B, -1, -1), m.storage_tokens.float().expand(B, -1, -1), tok], dim=1)
            return x.contiguous(), dt
        cols = ops.patch_gather(img, P, pdt)
        w, b = engine.patch_weights(m.patch_embed.proj, pdt)
        tok = ops.gemm(cols, w, b, out_dtype=torch.float32).view(B, h0 * w0, -1)
        cls = engine.prepared(m, "cls", (m.cls_token,), lambda: m.cls_token.detach().float().reshape(-1).contiguous())
        reg = engine.prepared(m, "reg", (m.storage_tokens,), lambda: m.storage_tokens.detach().float()[0].contiguous())
        zeros = engine.prepared(m, ("nopos", h0 * w0), (m.cls_token,), lambda: torch.zeros_like(m.cls_token.detach().float()[0]).expand(1 + h0 * w0, -1).contiguous())
        x = ops.assemble_tokens(tok, cls, reg, zeros)
        if engine.stream_dtype(dt, self.enc_embed_dim) == torch.bfloat16:
            x = ops.convert(x, torch.bfloat16)
        return x, dt

    def _rope(self, h0, w0, device):
        m = self.model
        return m.rope.bind(m.num_prefix_tokens, h0, w0, device, training=self.training)

    def _normed_f32(self, x2d, norm: bool):
        if norm and not isinstance(self.model.norm, nn.Identity):
            return engine.layernorm(x2d, self.model.norm, torch.float32)
        return x2d if (x2d.dtype == torch.float32 or x2d.requires_grad) else ops.convert(x2d, torch.float32)

    def _patch_map(self, xn, B, h0, w0):
        "[B, Nt, D] fp32 -> the patch tokens as a BCHW map"
        R = self.model.num_prefix_tokens
        if xn.requires_grad:      # training: a plain (differentiable) slice
            return xn[:, R:].reshape(B, h0, w0, -1).permute(0, 3, 1, 2)
        patches = ops.token_slice(xn, R, h0 * w0)
        return engine.nlc_as_bchw(patches.view(B * h0 * w0, -1), B, h0, w0)

    def forward(self, encoder_input: ViTEncoderInput) -> ViTEncoderOutput:
        "the final-normed patch tokens (the published `forward_features(...)[\"x_norm_patchtokens\"]`) as [B, D, H/P, W/P]"
        B, h0, w0 = self._check(encoder_input)
        x, dt = self._tokens(encoder_input.image, h0, w0)
        Nt, D = x.shape[1], x.shape[2]
        rope = self._rope(h0, w0, x.device)
        x2d = x.view(B * Nt, D)
        for blk in self.model.blocks:
            x2d = blk.forward_tokens(x2d, B, Nt, dt, rope)
        return ViTEncoderOutput(features=self._patch_map(self._normed_f32(x2d, True).view(B, Nt, D), B, h0, w0))


class DINOv3IntermediateFeatureReturner(DINOv3Encoder, IntermediateFeatureReturner):
    "Intermediate Feature Returner for UniCeption DINOv3 ViT Encoder"

    def __init__(self, name: str, dinov3_repo_dir: Optional[str] = None, data_norm_type: str = "dinov3", patch_size: int = 16,
                 size="large", weights: Optional[str] = None, pretrained_checkpoint_path: str = None,
                 gradient_checkpointing: bool = False, keep_first_n_layers: Optional[int] = None, disable_torch_compile_for_pe=False,
                 indices: Optional[Union[int, List[int]]] = 1, norm_intermediate: bool = True, *args, **kwargs):
        DINOv3Encoder.__init__(self, name=name, dinov3_repo_dir=dinov3_repo_dir, data_norm_type=data_norm_type, patch_size=patch_size,
                               size=size, weights=weights, pretrained_checkpoint_path=pretrained_checkpoint_path,
                               gradient_checkpointing=gradient_checkpointing, keep_first_n_layers=keep_first_n_layers,
                               disable_torch_compile_for_pe=disable_torch_compile_for_pe, *args, **kwargs)
        IntermediateFeatureReturner.__init__(self, indices=indices, norm_intermediate=norm_intermediate)

    def forward(self, encoder_input: ViTEncoderInput) -> List[ViTEncoderOutput]:
        """Published `get_intermediate_layers(x, n=indices, reshape=True, norm=norm_intermediate)`: the patch maps of the selected
        blocks' outputs (the last n for an int, the listed ones otherwise), optionally through the final norm."""
        B, h0, w0 = self._check(encoder_input)
        if self.indices is None:
            self.indices = range(len(self.model.blocks))
        take, _ = feature_take_indices(len(self.model.blocks), self.indices)
        x, dt = self._tokens(encoder_input.image, h0, w0)
        Nt, D = x.shape[1], x.shape[2]
        rope = self._rope(h0, w0, x.device)
        x2d = x.view(B * Nt, D)
        outs = []
        for i, blk in enumerate(self.model.blocks):
            x2d = blk.forward_tokens(x2d, B, Nt, dt, rope)
            if i in take:
                outs.append(ViTEncoderOutput(features=self._patch_map(self._normed_f32(x2d, self.norm_intermediate).view(B, Nt, D), B, h0, w0)))
        return outs


# ---------------------------------------------------------------------------------------------------------------------------------
# DINOv3 ConvNeXt
# ---------------------------------------------------------------------------------------------------------------------------------
# stage widths, stage depths (published)
_CONVNEXT_SIZES = {"tiny": ((96, 192, 384, 768), (3, 3, 9, 3)), "small": ((96, 192, 384, 768), (3, 3, 27, 3)),
                   "base": ((128, 256, 512, 1024), (3, 3, 27, 3)), "large": ((192, 384, 768, 1536), (3, 3, 27, 3))}
# the reference wrapper's table (its tiny / small entry is the width of the last stage, 768)
_CONVNEXT_EMBED_DIM = {"tiny": 768, "small": 768, "base": 1024, "large": 1536}
STEM_PATCH, STEM_KPAD = 4, 64


def resolve_convnext_size(size):
    "(widths, depths) of a named size, or of a dict(hidden_sizes=, depths=) — custom variants and the tiny configurations of the tests"
    if isinstance(size, dict):
        widths, depths = tuple(size["hidden_sizes"]), tuple(size["depths"])
    elif size in _CONVNEXT_SIZES:
        widths, depths = _CONVNEXT_SIZES[size]
    else:
        raise engine.UcHipError(f"unknown DINOv3 ConvNeXt size '{size}'; supported: {sorted(_CONVNEXT_SIZES)}")
    if len(widths) != 4 or len(depths) != 4 or any(w <= 0 or w % 8 for w in widths) or any(d < 1 for d in depths):
        raise engine.UcHipError(f"DINOv3 ConvNeXt: four stage widths (multiples of 8: uc_dwconv7x7_nhwc) and four depths >= 1, got {widths} / {depths}")
    return widths, depths


class _ConvNextLayer(nn.Module):
    "x + gamma * pwconv2(act(pwconv1(norm(dwconv(x)))))  — parameter container; the pipeline on NHWC rows is forward_rows."

    def __init__(self, dim, layer_scale_init_value=1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim))

    def forward_rows(self, x, dt):
        "x: NHWC [B, H, W, C] in the stage's stream dtype -> the same"
        C = x.shape[-1]
        if autograd.grad_needed(x, *self.parameters()):
            h = autograd.layer_norm(autograd.dwconv7x7(x, self.dwconv).view(-1, C), self.norm, dt)
            g = self.gamma.float()
            f = autograd.mlp(h, self.pwconv1, _Lin(self.pwconv2.weight * g[:, None], self.pwconv2.bias * g), "gelu", dt)
            return x + f.view(x.shape).to(x.dtype)
        autograd.check_dwconv7x7(self.dwconv)
        w49, b = autograd.dwconv7x7_weights(self.dwconv)
        h = engine.layernorm(ops.dwconv7x7_nhwc(x, w49, b).view(-1, C), self.norm, dt)
        x2d = x.view(-1, C)
        out = engine.mlp(h, self.pwconv1, self.pwconv2, "gelu", x2d, x2d.dtype, fc2_wb=engine.layerscale_lin_weights(self.pwconv2, self.gamma, dt))
        return out.view(x.shape)


def _down2_lin(conv, train: bool, dt) -> _Lin:
    "the [Cout, 4 Cin] linear of Conv2d(k = 2, stride = 2) on uc_patch2_gather_nhwc's rows: K permuted to (ky, kx, c)"
    if train:
        return _Lin(conv.weight.permute(0, 2, 3, 1).reshape(conv.out_channels, -1), conv.bias)
    w, b = engine.prepared(conv, ("p2", dt), (conv.weight, conv.bias),
                           lambda: (conv.weight.detach().permute(0, 2, 3, 1).reshape(conv.out_channels, -1).to(dt).contiguous(),
                                    conv.bias.detach().float().contiguous()))
    return _Lin(w, b)


class DINOv3ConvNextParams(nn.Module):
    "Parameters of a DINOv3 ConvNeXt under the original ConvNeXt names (`model.*` inside DINOv3ConvNextEncoder)."

    def __init__(self, size):
        super().__init__()
        widths, depths = resolve_convnext_size(size)
        self.widths, self.depths = widths, depths
        self.downsample_layers = nn.ModuleList(
            [nn.Sequential(nn.Conv2d(3, widths[0], kernel_size=STEM_PATCH, stride=STEM_PATCH), nn.LayerNorm(widths[0], eps=1e-6))] +
            [nn.Sequential(nn.LayerNorm(widths[i - 1], eps=1e-6), nn.Conv2d(widths[i - 1], widths[i], kernel_size=2, stride=2)) for i in range(1, 4)])
        self.stages = nn.ModuleList([nn.Sequential(*[_ConvNextLayer(widths[i]) for _ in range(depths[i])]) for i in range(4)])
        self.norm = nn.LayerNorm(widths[-1], eps=1e-6)


class DINOv3ConvNextEncoder(UniCeptionEncoderBase):
    """UniCeption DINOv3 ConvNext Encoder.  dinov3_repo_dir and weights are accepted and unused (there is no torch.hub here: the
    architecture is built directly); `pretrained_checkpoint_path` is a {"model": state_dict of this wrapper} file.  size: a name
    (tiny | small | base | large), or a dict(hidden_sizes=, depths=).  The features are the final-normed last stage, [B, C, H/32, W/32]."""

    def __init__(self, name: str, dinov3_repo_dir: Optional[str] = None, data_norm_type: str = "dinov3", patch_size: int = 16,
                 size="large", weights: Optional[str] = None, pretrained_checkpoint_path: Optional[str] = None, *args, **kwargs):
        super().__init__(name=name, data_norm_type=data_norm_type, *args, **kwargs)
        self.patch_size = patch_size
        self.final_layer_patch_size = 32          # DINOv3 ConvNext uses a final patch size of 32
        self.version = size
        widths, _ = resolve_convnext_size(size)
        self.enc_embed_dim = widths[-1] if isinstance(size, dict) else _CONVNEXT_EMBED_DIM[size]
        self.model = DINOv3ConvNextParams(size)
        self.model.patch_size = self.patch_size
        if pretrained_checkpoint_path:
            print(f"Loading custom pretrained DINOv3 checkpoint from {pretrained_checkpoint_path}")
            ckpt = torch.load(pretrained_checkpoint_path, map_location="cpu", weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def _check(self, encoder_input):
        self._check_data_normalization_type(encoder_input.data_norm_type)
        assert isinstance(encoder_input.image, torch.Tensor), "Input must be a torch.Tensor"
        assert encoder_input.image.ndim == 4, "Input must be of shape (B, C, H, W)"
        B, C, H, W = encoder_input.image.shape
        assert C == 3, "Input must have 3 channels"
        assert H % self.patch_size == 0 and W % self.patch_size == 0, \
            f"Input shape must be divisible by patch size: {self.patch_size}"
        if H % STEM_PATCH or W % STEM_PATCH:
            raise engine.UcHipError(f"DINOv3 ConvNeXt: the {STEM_PATCH}x{STEM_PATCH} stem needs H ({H}) and W ({W}) divisible by {STEM_PATCH}")
        return B, H, W

    def _stem(self, image, B, H, W, dt, train):
        "NHWC [B, H/4, W/4, C0] in stage 0's stream dtype: 4x4 patch rows (K = 48 zero-padded to 64) -> GEMM -> LayerNorm"
        conv, ln = self.model.downsample_layers[0]
        C0 = conv.out_channels
        sdt = engine.stream_dtype(dt, C0)
        img = image.float().contiguous() if (image.dtype != torch.float32 or not image.is_contiguous()) else image
        if train:
            rows = autograd.unshuffle_rows(img, STEM_PATCH, STEM_KPAD, dt)
            w = torch.nn.functional.pad(conv.weight.reshape(C0, -1), (0, STEM_KPAD - 3 * STEM_PATCH * STEM_PATCH))
            tok = autograd.linear(rows, w, conv.bias, conv, dt, torch.float32)
            x = autograd.layer_norm(tok, ln, sdt)
        else:
            w, b = engine.patch_weights_padded(conv, dt, STEM_KPAD)
            tok = ops.gemm(ops.unshuffle_rows(img, STEM_PATCH, STEM_KPAD, dt), w, b, out_dtype=torch.float32)
            x = engine.layernorm(tok, ln, sdt)
        return x.view(B, H // STEM_PATCH, W // STEM_PATCH, C0)

    def _downsample(self, x, i, dt, train):
        "stage i - 1's output NHWC -> stage i's input: LayerNorm -> 2x2 / stride-2 patch rows -> GEMM (an odd last row / column is dropped)"
        ln, conv = self.model.downsample_layers[i]
        B, H, W, C = x.shape
        sdt = engine.stream_dtype(dt, conv.out_channels)
        lin = _down2_lin(conv, train, dt)
        if train:
            h = autograd.layer_norm(x.reshape(-1, C), ln, dt).view(B, H, W, C)
            y = autograd.linear(autograd.patch2_gather(h), lin.weight, lin.bias, conv, dt, sdt)
        else:
            h = engine.layernorm(x.view(-1, C), ln, dt).view(B, H, W, C)
            y = ops.gemm(ops.patch2_gather_nhwc(h), lin.weight, lin.bias, out_dtype=sdt)
        return y.view(B, H // 2, W // 2, conv.out_channels)

    def _stage_outputs(self, encoder_input, upto: int = 3):
        "generator of (stage index, NHWC output of that stage) for stages 0..upto"
        B, H, W = self._check(encoder_input)
        image = encoder_input.image
        dt = engine.compute_dtype()
        train = autograd.grad_needed(image, *self.model.parameters())
        x = self._stem(image, B, H, W, dt, train)
        for i in range(upto + 1):
            if i > 0:
                x = self._downsample(x, i, dt, train)
            for layer in self.model.stages[i]:
                x = layer.forward_rows(x, dt)
            yield i, x

    def _to_nchw(self, x, norm: bool):
        "NHWC stage output -> fp32 NCHW, through the final norm (per pixel) when asked"
        B, H, W, C = x.shape
        if norm:
            x = engine.layernorm(x.reshape(-1, C), self.model.norm, torch.float32).view(B, H, W, C)
        if x.requires_grad:           # training: a plain (differentiable) permute
            return x.float().permute(0, 3, 1, 2)
        return ops.nhwc_to_nchw(x.contiguous(), torch.float32)

    def forward(self, encoder_input: ViTEncoderInput) -> ViTEncoderOutput:
        "the final-normed last-stage map (the published `forward_features(...)[\"x_norm_patchtokens\"]` reshaped) as [B, C, H/32, W/32]"
        for i, x in self._stage_outputs(encoder_input):
            pass
        return ViTEncoderOutput(features=self._to_nchw(x, True))


class DINOv3ConvNextIntermediateFeatureReturner(DINOv3ConvNextEncoder, IntermediateFeatureReturner):
    """Intermediate Feature Returner for UniCeption DINOv3 ConvNext Encoder.  `indices` selects among the FOUR stage outputs (None: all,
    an int n: the last n, a list: those); each is handed out as fp32 NCHW at its native stride (4, 8, 16, 32).  norm_intermediate=True
    applies the final `norm` to stage 3 only — the one stage whose width it has; stages 0-2 are handed out as they are.  Resampling the
    stage maps to the `patch_size` grid (what the hub model may do with `model.patch_size`: UNVERIFIED) is not built."""

    def __init__(self, name: str, dinov3_repo_dir: Optional[str] = None, data_norm_type: str = "dinov3", patch_size: int = 16,
                 size="large", weights: Optional[str] = None, pretrained_checkpoint_path: Optional[str] = None,
                 indices: Optional[Union[int, List[int]]] = 1, norm_intermediate: bool = True, *args, **kwargs):
        DINOv3ConvNextEncoder.__init__(self, name=name, data_norm_type=data_norm_type, patch_size=patch_size, size=size,
                                       dinov3_repo_dir=dinov3_repo_dir, weights=weights,
                                       pretrained_checkpoint_path=pretrained_checkpoint_path, *args, **kwargs)
        IntermediateFeatureReturner.__init__(self, indices=indices, norm_intermediate=norm_intermediate)

    def forward(self, encoder_input: ViTEncoderInput) -> List[ViTEncoderOutput]:
        n = len(self.model.downsample_layers)
        if self.indices is None:
            self.indices = range(n)
        take, last = feature_take_indices(n, self.indices)
        outs = []
        for i, x in self._stage_outputs(encoder_input, upto=last):
            if i in take:
                outs.append(ViTEncoderOutput(features=self._to_nchw(x, self.norm_intermediate and i == n - 1)))
        return outs
