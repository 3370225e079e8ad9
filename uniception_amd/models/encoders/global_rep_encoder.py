"""Global representation encoder (reference: encoders/global_rep_encoder.py:14-105) on the HIP kernels: a [B, C] vector (a pose, a
scale factor) through an MLP and a LayerNorm.  Every Linear is one uc_gemm with its activation in the epilogue (autograd.head_linear)
on widths zero-padded to 64 — the input's C columns included —, the last one writes fp32, and the norm is autograd.layer_norm."""
from functools import partial
from typing import Callable, List, Optional, Type, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd, engine, ops
from .base import EncoderGlobalRepInput, EncoderGlobalRepOutput
from .dense_rep_encoder import build_act
from .patch_embedder import build_norm


class GlobalRepresentationEncoder(nn.Module):
    "UniCeption Global Representation Encoder"

    def __init__(
        self,
        name: str,
        in_chans: int = 3,
        enc_embed_dim: int = 1024,
        intermediate_dims: List[int] = [128, 256, 512],
        act_layer: Type[nn.Module] = nn.GELU,
        norm_layer: Union[Type[nn.Module], Callable[..., nn.Module]] = partial(nn.LayerNorm, eps=1e-6),
        pretrained_checkpoint_path: Optional[str] = None,
        *args,
        **kwargs,
    ):
        super().__init__(*args, **kwargs)
        self.name = name
        self.in_chans = in_chans
        self.enc_embed_dim = enc_embed_dim
        self.intermediate_dims = intermediate_dims
        self.pretrained_checkpoint_path = pretrained_checkpoint_path

        self.act_layer, self._act_name = build_act(act_layer)

        # the reference nests one Sequential per layer: the keys are encoder.0.0.0.weight ... encoder.1.weight
        self.encoder = nn.Sequential(
            nn.Linear(self.in_chans, self.intermediate_dims[0]),
            self.act_layer,
        )
        for intermediate_idx in range(1, len(self.intermediate_dims)):
            self.encoder = nn.Sequential(
                self.encoder,
                nn.Linear(self.intermediate_dims[intermediate_idx - 1], self.intermediate_dims[intermediate_idx]),
                self.act_layer,
            )
        self.encoder = nn.Sequential(
            self.encoder,
            nn.Linear(self.intermediate_dims[-1], self.enc_embed_dim),
        )

        self.norm_layer = build_norm(norm_layer, enc_embed_dim, "norm_layer")
        if isinstance(self.norm_layer, nn.LayerNorm):
            nn.init.constant_(self.norm_layer.bias, 0)
            nn.init.constant_(self.norm_layer.weight, 1.0)

        if self.pretrained_checkpoint_path is not None:
            print(
                f"Loading pretrained Global Representation Encoder checkpoint from {self.pretrained_checkpoint_path} ..."
            )
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def linears(self) -> List[nn.Linear]:
        "the Linear layers in the order they are applied (the nested Sequentials are walked depth-first)"
        return [m for m in self.encoder.modules() if isinstance(m, nn.Linear)]

    def forward(self, encoder_input: EncoderGlobalRepInput) -> EncoderGlobalRepOutput:
        input_data = encoder_input.data
        assert input_data.ndim == 2, "Input data must have shape (B, C)"
        assert input_data.shape[1] == self.in_chans, f"Input data must have {self.in_chans} channels"
        ops._need_gpu(input_data)
        dt = engine.compute_dtype()
        E = self.enc_embed_dim
        x = F.pad(input_data.float(), (0, autograd.head_pad(self.in_chans) - self.in_chans))      # [B, 64]: a few hundred bytes
        layers = self.linears()
        for lin in layers[:-1]:
            x = autograd.head_linear(x, (lin,), dt, act=self._act_name)
        x = autograd.head_linear(x, (layers[-1],), dt, out_dtype=torch.float32)
        if x.shape[1] != E:
            x = x[:, :E].contiguous()
        if isinstance(self.norm_layer, nn.LayerNorm):
            x = engine.layernorm(x, self.norm_layer, torch.float32)
        return EncoderGlobalRepOutput(features=x)
