"""Original CroCo v2 / DUSt3R / MASt3R checkpoints -> the state_dict layout of ``uniception_amd.models.factory.DUSt3R``
(and of its sub-modules), so real released weights can be put through the HIP path.

Restates the key maps of the reference's converter (examples/models/dust3r/convert_dust3r_weights_to_uniception.py:20-213):
    decoder_embed.*                      -> info_sharing.proj_embed.*                          (:38-40)
    dec_blocks.N.*  / dec_blocks2.N.*    -> info_sharing.multi_view_branches.{0,1}.N.*         (:41-46); a checkpoint without
                                            dec_blocks2 (CroCo) gets view 0's blocks duplicated (:28-34)
    dec_norm.*                           -> info_sharing.norm.*                                (:47-49)
    downstream_head{h}.dpt.<feature>     -> dpt_feature_head{h}.<feature>                      (:76-79, :176-183)
    downstream_head{h}.dpt.head.{0,2,4}  -> dpt_regressor_head{h}.{conv1, conv2.0, conv2.2}    (:95-109)
    downstream_head{h}.proj.{weight,bias}-> head{h}.linear.{weight [N,K,1,1], bias}            (:134-151: Linear -> 1x1 Conv2d)
    MASt3R's downstream_head{h}.head_local_features.* has no counterpart and is dropped         (:176-178, :198-202)
and, beyond that script (it only extracts decoder and heads):
    patch_embed.* / enc_blocks.* / enc_norm.*  -> encoder.*  (the CroCoEncoder checkpoint format of encoders/croco.py:101-111)
The reference's script targets an older DPTFeature (it loads the original `act_postprocess.*` names with strict=True, which
today's module — `input_process.i.0.j`, aliased `scratch.layer_rn.i` / `input_process.i.1` — rejects); the maps below produce
today's names INCLUDING every alias key, so ``DUSt3R.load_state_dict(converted, strict=True)`` succeeds:
    dpt.act_postprocess.i.j.X            -> input_process.i.0.j.X
    dpt.scratch.layer{i}_rn.weight       -> scratch.layer{i}_rn.weight == scratch.layer_rn.{i-1}.weight == input_process.{i-1}.1.weight
    dpt.scratch.refinenet4.resConfUnit1  -> dropped (the module deletes that unused unit for DDP, prediction_heads/dpt.py:82-83)
    dpt_feature_head{h}.* == head{h}.0.*,  dpt_regressor_head{h}.* == head{h}.1.*              (factory/dust3r.py:166-192)
Real checkpoints cannot be fetched in the build environment; the maps are exercised on synthetic original-format
checkpoints (tests/test_convert_checkpoint.py: round trip through `uniception_to_original`, strict load, equal outputs).

    python -m uniception_amd.tools.convert_checkpoint ORIGINAL.pth OUT.pth [--per-module-dir DIR]

--mode perception_encoder --pe-config PE-Core-L14-336: an original Perception Encoder checkpoint (the bare state_dict, or under
"state_dict" / "weights", with optional "module." and "visual." prefixes; of a CLIP checkpoint only the "visual." entries are kept —
the prefix handling of the reference's VisionTransformer.load_ckpt) -> the {"model": {"model." + key: tensor}} file that
PerceptionEncoder(pretrained_checkpoint_path=...) loads.  A missing or unexpected key is an error that names it.

--mode dinov3: the state_dict of a transformers DINOv3ViTModel (the bare dict, or under "state_dict" / "model") -> the
{"model": {"model." + key: tensor}} file that DINOv3Encoder(pretrained_checkpoint_path=...) loads: q / k / v packed into attn.qkv
(a missing key bias becomes zeros), attn.qkv.bias_mask (1 | 0 | 1) and rope_embed.periods synthesised, layer_scale*.lambda1 ->
ls*.gamma, register_tokens -> storage_tokens, gate_proj / up_proj / down_proj -> w1 / w2 / w3 (up_proj / down_proj -> fc1 / fc2
without a gate).  An unexpected key is an error that names it.

--mode dinov3_convnext: the state_dict of a transformers DINOv3ConvNextModel -> the {"model": {"model." + key: tensor}} file that
DINOv3ConvNextEncoder(pretrained_checkpoint_path=...) loads: model.stages.i.downsample_layers.k -> downsample_layers.i.k,
model.stages.i.layers.j.{depthwise_conv, layer_norm, pointwise_conv1, pointwise_conv2, gamma} -> stages.i.j.{dwconv, norm, pwconv1,
pwconv2, gamma}, layer_norm -> norm.  An unexpected key is an error that names it.
"""
import argparse
import os
import re
from typing import Dict, Optional, Tuple

import torch

REG_HEAD_MAP = {"0": "conv1", "2": "conv2.0", "4": "conv2.2"}
_DROPPED_PREFIXES = ("mask_token", "dec_pos_embed", "enc_pos_embed", "prediction_head.")


def detect_head_type(sd: Dict[str, torch.Tensor]) -> Optional[str]:
    if any(k.startswith("downstream_head1.dpt.") for k in sd):
        return "dpt"
    if any(k.startswith("downstream_head1.proj.") for k in sd):
        return "linear"
    return None


def _dpt_feature_keys(rest: str):
    """Names (relative to a DPTFeature) that an original `dpt.<rest>` entry fills — aliases included — or () when dropped."""
    m = re.match(r"act_postprocess\.(\d+)\.(\d+)\.(.+)$", rest)
    if m:
        return (f"input_process.{m.group(1)}.0.{m.group(2)}.{m.group(3)}",)
    m = re.match(r"scratch\.layer(\d)_rn\.(.+)$", rest)
    if m:
        i = int(m.group(1))
        return (f"scratch.layer{i}_rn.{m.group(2)}", f"scratch.layer_rn.{i - 1}.{m.group(2)}", f"input_process.{i - 1}.1.{m.group(2)}")
    if rest.startswith("scratch.refinenet4.resConfUnit1."):
        return ()
    if rest.startswith("scratch."):
        return (rest,)
    raise KeyError(f"unexpected DPT key dpt.{rest}")


def original_to_uniception(sd: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, str]]:
    """(state_dict in the DUSt3R factory's namespace incl. alias keys, {original key: reason} for everything dropped)."""
    out, dropped = {}, {}
    two_decoders = any(k.startswith("dec_blocks2.") for k in sd)
    for k, v in sd.items():
        if k.startswith(("patch_embed.", "enc_blocks.", "enc_norm.")):
            out["encoder." + k] = v
        elif k.startswith("decoder_embed."):
            out["info_sharing.proj_embed." + k[len("decoder_embed."):]] = v
        elif k.startswith("dec_blocks2."):
            out["info_sharing.multi_view_branches.1." + k[len("dec_blocks2."):]] = v
        elif k.startswith("dec_blocks."):
            out["info_sharing.multi_view_branches.0." + k[len("dec_blocks."):]] = v
            if not two_decoders:   # CroCo: one decoder, both views start from it
                out["info_sharing.multi_view_branches.1." + k[len("dec_blocks."):]] = v
        elif k.startswith("dec_norm."):
            out["info_sharing.norm." + k[len("dec_norm."):]] = v
        elif re.match(r"downstream_head[12]\.", k):
            h = k[len("downstream_head")]
            rest = k[len("downstream_headN."):]
            if rest.startswith("head_local_features."):
                dropped[k] = "MASt3R local-feature head: no counterpart in the DUSt3R factory"
            elif rest.startswith("proj."):
                t = v.reshape(v.shape[0], v.shape[1], 1, 1) if rest == "proj.weight" else v
                out[f"head{h}.linear.{rest[len('proj.'):]}"] = t
            elif rest.startswith("dpt.head."):
                idx, leaf = rest[len("dpt.head."):].split(".", 1)
                if idx not in REG_HEAD_MAP:
                    raise KeyError(f"unexpected regressor layer in {k}")
                for pre in (f"dpt_regressor_head{h}.", f"head{h}.1."):
                    out[pre + f"{REG_HEAD_MAP[idx]}.{leaf}"] = v
            elif rest.startswith("dpt."):
                names = _dpt_feature_keys(rest[len("dpt."):])
                if not names:
                    dropped[k] = "refinenet4.resConfUnit1 is unused and deleted by the module"
                for n in names:
                    out[f"dpt_feature_head{h}.{n}"] = v
                    out[f"head{h}.0.{n}"] = v
            else:
                raise KeyError(f"unexpected head key {k}")
        elif k.startswith(_DROPPED_PREFIXES):
            dropped[k] = "not part of the two-view regression path"
        else:
            raise KeyError(f"unexpected key {k} in an original CroCo / DUSt3R / MASt3R checkpoint")
    return out, dropped


def uniception_to_original(sd: Dict[str, torch.Tensor], two_decoders: bool = True) -> Dict[str, torch.Tensor]:
    """Inverse map (canonical names only): a DUSt3R-factory state_dict written with the original checkpoint's key names.
    Used to synthesize original-format checkpoints for tests and to export weights trained here."""
    out = {}
    for k, v in sd.items():
        if k.startswith("encoder."):
            out[k[len("encoder."):]] = v
        elif k.startswith("info_sharing.proj_embed."):
            out["decoder_embed." + k[len("info_sharing.proj_embed."):]] = v
        elif k.startswith("info_sharing.multi_view_branches.0."):
            out["dec_blocks." + k[len("info_sharing.multi_view_branches.0."):]] = v
        elif k.startswith("info_sharing.multi_view_branches.1."):
            if two_decoders:
                out["dec_blocks2." + k[len("info_sharing.multi_view_branches.1."):]] = v
        elif k.startswith("info_sharing.norm."):
            out["dec_norm." + k[len("info_sharing.norm."):]] = v
        elif re.match(r"dpt_feature_head[12]\.", k):
            h, rest = k[len("dpt_feature_head")], k[len("dpt_feature_headN."):]
            m = re.match(r"input_process\.(\d+)\.0\.(\d+)\.(.+)$", rest)
            if m:
                out[f"downstream_head{h}.dpt.act_postprocess.{m.group(1)}.{m.group(2)}.{m.group(3)}"] = v
            elif re.match(r"scratch\.layer_rn\.|input_process\.\d+\.1\.", rest):
                continue   # aliases of scratch.layer{i}_rn
            else:
                out[f"downstream_head{h}.dpt.{rest}"] = v
        elif re.match(r"dpt_regressor_head[12]\.", k):
            h, rest = k[len("dpt_regressor_head")], k[len("dpt_regressor_headN."):]
            inv = {v_: k_ for k_, v_ in REG_HEAD_MAP.items()}
            name, leaf = rest.rsplit(".", 1)
            out[f"downstream_head{h}.dpt.head.{inv[name]}.{leaf}"] = v
        elif re.match(r"head[12]\.linear\.", k):
            h, leaf = k[len("head")], k.rsplit(".", 1)[1]
            out[f"downstream_head{h}.proj.{leaf}"] = v.reshape(v.shape[0], v.shape[1]) if leaf == "weight" else v
        elif re.match(r"head[12]\.[01]\.", k):
            continue       # aliases of dpt_feature_head / dpt_regressor_head
        else:
            raise KeyError(f"unexpected key {k} in a DUSt3R factory state_dict")
    return out


def split_modules(converted: Dict[str, torch.Tensor], data_norm_type: str = "dust3r", patch_embed_cls: str = "PatchEmbedDust3R"):
    """Per-module checkpoints in the formats the modules' `pretrained_checkpoint_path` arguments read
    (encoders/croco.py:101-111: {"model", "data_norm_type", "patch_embed_cls"}; the others {"model"})."""
    def sub(prefix):
        return {k[len(prefix):]: v for k, v in converted.items() if k.startswith(prefix)}
    mods = {"encoder": {"model": sub("encoder."), "data_norm_type": data_norm_type, "patch_embed_cls": patch_embed_cls},
            "info_sharing": {"model": sub("info_sharing.")}}
    for h in ("1", "2"):
        if any(k.startswith(f"dpt_feature_head{h}.") for k in converted):
            mods[f"dpt_feature_head{h}"] = {"model": sub(f"dpt_feature_head{h}.")}
            mods[f"dpt_regressor_head{h}"] = {"model": sub(f"dpt_regressor_head{h}.")}
        elif any(k.startswith(f"head{h}.linear.") for k in converted):
            mods[f"linear_feature_head{h}"] = {"model": sub(f"head{h}.")}
    return {k: v for k, v in mods.items() if v["model"]}


def load_original_checkpoint(model: torch.nn.Module, original_sd: Dict[str, torch.Tensor], strict: bool = True):
    """Convert an original-format state_dict and load it into a ``DUSt3R`` factory model (strict by default)."""
    converted, _ = original_to_uniception(original_sd)
    res = model.load_state_dict(converted, strict=strict)
    from .. import engine
    engine.bump_weight_epoch()
    return res


def perception_encoder_keys(config_name: str) -> Dict[str, Tuple[int, ...]]:
    "{key: shape} of the vision tower `config_name`, built on the meta device (nothing is allocated)"
    from ..models.libs.perception_encoder.vision_encoder.pe import VisionTransformer
    with torch.device("meta"):
        tower = VisionTransformer.from_config(config_name)
    return {k: tuple(v.shape) for k, v in tower.state_dict().items()}


def perception_encoder_to_uniception(ckpt: Dict, config_name: str) -> Dict[str, torch.Tensor]:
    """The state_dict of PerceptionEncoder (keys under "model.") from an original PE checkpoint dict; KeyError naming the first
    missing / unexpected key, ValueError for a shape that does not fit `config_name`."""
    sd = ckpt.get("state_dict", ckpt.get("weights", ckpt))
    sd = {k.replace("module.", ""): v for k, v in sd.items()}
    if any(k.startswith("visual.") for k in sd):
        sd = {k.replace("visual.", ""): v for k, v in sd.items() if "visual" in k}
    want = perception_encoder_keys(config_name)
    for k in want:
        if k not in sd:
            raise KeyError(f"missing key {k}: the checkpoint is not a {config_name} vision tower")
    for k, v in sd.items():
        if k not in want:
            raise KeyError(f"unexpected key {k} for a {config_name} vision tower")
        if tuple(v.shape) != want[k]:
            raise ValueError(f"{k} has shape {tuple(v.shape)}, {config_name} expects {want[k]}")
    return {"model." + k: sd[k] for k in want}


_DINOV3_BLOCK = {"norm1.weight": "norm1.weight", "norm1.bias": "norm1.bias", "norm2.weight": "norm2.weight", "norm2.bias": "norm2.bias",
                 "attention.o_proj.weight": "attn.proj.weight", "attention.o_proj.bias": "attn.proj.bias",
                 "layer_scale1.lambda1": "ls1.gamma", "layer_scale2.lambda1": "ls2.gamma"}
_DINOV3_FFN = {True: {"gate_proj": "w1", "up_proj": "w2", "down_proj": "w3"}, False: {"up_proj": "fc1", "down_proj": "fc2"}}
_DINOV3_TOP = {"embeddings.cls_token": "cls_token", "embeddings.register_tokens": "storage_tokens",
               "embeddings.patch_embeddings.weight": "patch_embed.proj.weight", "embeddings.patch_embeddings.bias": "patch_embed.proj.bias",
               "norm.weight": "norm.weight", "norm.bias": "norm.bias"}


def dinov3_hf_to_uniception(ckpt: Dict, num_heads: Optional[int] = None, rope_base: float = 100.0, prefix: str = "model.") -> Dict[str, torch.Tensor]:
    """The state_dict of DINOv3Encoder (keys under `prefix`) from a transformers DINOv3ViTModel state_dict.  num_heads: the model's
    head count (rope_embed.periods has head_dim / 4 entries); None: head_dim 64, which every served size has.  KeyError naming the first key without a counterpart."""
    sd = ckpt
    for wrap in ("state_dict", "model"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    out, qkv = {}, {}
    for k, v in sd.items():
        m = re.match(r"(?:model\.)?layer\.(\d+)\.(.+)$", k)
        if k in _DINOV3_TOP:
            out[_DINOV3_TOP[k]] = v
        elif k == "embeddings.mask_token":
            out["mask_token"] = v.reshape(1, -1)
        elif k == "rope_embeddings.inv_freq":
            continue          # (a derived buffer: rope_embed.periods is synthesised below)
        elif m:
            i, rest = m.group(1), m.group(2)
            b = f"blocks.{i}."
            ma = re.match(r"attention\.([qkv])_proj\.(weight|bias)$", rest)
            mf = re.match(r"mlp\.(gate_proj|up_proj|down_proj)\.(weight|bias)$", rest)
            if ma:
                qkv.setdefault(i, {})[ma.group(1) + ma.group(2)] = v
            elif mf:
                gated = any(x.endswith(f"layer.{i}.mlp.gate_proj.weight") for x in sd)
                out[b + f"mlp.{_DINOV3_FFN[gated][mf.group(1)]}.{mf.group(2)}"] = v
            elif rest in _DINOV3_BLOCK:
                out[b + _DINOV3_BLOCK[rest]] = v
            else:
                raise KeyError(f"unexpected key {k} in a transformers DINOv3ViTModel state_dict")
        else:
            raise KeyError(f"unexpected key {k} in a transformers DINOv3ViTModel state_dict")
    for i, p in qkv.items():
        for need in ("qweight", "kweight", "vweight"):
            if need not in p:
                raise KeyError(f"missing key layer.{i}.attention.{need[0]}_proj.weight")
        D = p["qweight"].shape[0]
        zeros = torch.zeros(D, dtype=p["qweight"].dtype)
        out[f"blocks.{i}.attn.qkv.weight"] = torch.cat([p["qweight"], p["kweight"], p["vweight"]], 0)
        out[f"blocks.{i}.attn.qkv.bias"] = torch.cat([p.get("qbias", zeros), p.get("kbias", zeros), p.get("vbias", zeros)], 0)
        mask = torch.ones(3 * D, dtype=p["qweight"].dtype)
        mask[D:2 * D] = 0.0 if "kbias" not in p else 1.0
        out[f"blocks.{i}.attn.qkv.bias_mask"] = mask
    if "cls_token" not in out:
        raise KeyError("missing key embeddings.cls_token: not a transformers DINOv3ViTModel state_dict")
    hd = out["cls_token"].shape[-1] // num_heads if num_heads else 64
    out["rope_embed.periods"] = rope_base ** (4 * torch.arange(hd // 4, dtype=torch.float32) / hd)
    return {prefix + k: v for k, v in out.items()}


_CONVNEXT_LAYER = {"depthwise_conv": "dwconv", "layer_norm": "norm", "pointwise_conv1": "pwconv1", "pointwise_conv2": "pwconv2"}


def dinov3_convnext_hf_to_uniception(ckpt: Dict, prefix: str = "model.") -> Dict[str, torch.Tensor]:
    """The state_dict of DINOv3ConvNextEncoder (keys under `prefix`) from a transformers DINOv3ConvNextModel state_dict (the bare
    dict, or under "state_dict" / "model").  KeyError naming the first key without a counterpart."""
    sd = ckpt
    for wrap in ("state_dict", "model"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    out = {}
    for k, v in sd.items():
        md = re.match(r"(?:model\.)?stages\.(\d+)\.downsample_layers\.(\d+)\.(weight|bias)$", k)
        ml = re.match(r"(?:model\.)?stages\.(\d+)\.layers\.(\d+)\.(depthwise_conv|layer_norm|pointwise_conv1|pointwise_conv2)\.(weight|bias)$", k)
        mg = re.match(r"(?:model\.)?stages\.(\d+)\.layers\.(\d+)\.gamma$", k)
        mn = re.match(r"layer_norm\.(weight|bias)$", k)
        if md:
            out[f"downsample_layers.{md.group(1)}.{md.group(2)}.{md.group(3)}"] = v
        elif ml:
            out[f"stages.{ml.group(1)}.{ml.group(2)}.{_CONVNEXT_LAYER[ml.group(3)]}.{ml.group(4)}"] = v
        elif mg:
            out[f"stages.{mg.group(1)}.{mg.group(2)}.gamma"] = v
        elif mn:
            out[f"norm.{mn.group(1)}"] = v
        else:
            raise KeyError(f"unexpected key {k} in a transformers DINOv3ConvNextModel state_dict")
    if "norm.weight" not in out:
        raise KeyError("missing key layer_norm.weight: not a transformers DINOv3ConvNextModel state_dict")
    return {prefix + k: v for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("original")
    ap.add_argument("out")
    ap.add_argument("--mode", default="dust3r", choices=("dust3r", "perception_encoder", "dinov3", "dinov3_convnext"))
    ap.add_argument("--num-heads", type=int, default=None, help="dinov3 mode: the model's attention head count (default: embed dim / 64)")
    ap.add_argument("--pe-config", default=None, help="perception_encoder mode: the vision tower's config name, e.g. PE-Core-L14-336")
    ap.add_argument("--per-module-dir", default=None, help="also write encoder / info_sharing / head checkpoints there")
    a = ap.parse_args(argv)
    ckpt = torch.load(a.original, map_location="cpu", weights_only=False)
    if a.mode == "perception_encoder":
        if not a.pe_config:
            ap.error("--mode perception_encoder needs --pe-config")
        converted = perception_encoder_to_uniception(ckpt, a.pe_config)
        torch.save({"model": converted}, a.out)
        print(f"wrote {a.out}: {len(converted)} entries of {a.pe_config}")
        return
    if a.mode == "dinov3":
        converted = dinov3_hf_to_uniception(ckpt, a.num_heads)
        torch.save({"model": converted}, a.out)
        print(f"wrote {a.out}: {len(converted)} entries of a DINOv3 ViT")
        return
    if a.mode == "dinov3_convnext":
        converted = dinov3_convnext_hf_to_uniception(ckpt)
        torch.save({"model": converted}, a.out)
        print(f"wrote {a.out}: {len(converted)} entries of a DINOv3 ConvNeXt")
        return
    sd = ckpt["model"] if "model" in ckpt else ckpt
    converted, dropped = original_to_uniception(sd)
    for k, why in dropped.items():
        print(f"dropped {k}: {why}")
    torch.save({"model": converted, "head_type": detect_head_type(sd)}, a.out)
    print(f"wrote {a.out}: {len(converted)} entries ({len(sd)} in the original)")
    if a.per_module_dir:
        os.makedirs(a.per_module_dir, exist_ok=True)
        for name, c in split_modules(converted).items():
            torch.save(c, os.path.join(a.per_module_dir, name + ".pth"))
            print(f"wrote {os.path.join(a.per_module_dir, name + '.pth')}")


if __name__ == "__main__":
    main()
