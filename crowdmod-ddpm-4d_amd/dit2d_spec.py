"""Structural description of the reference DiT2D denoiser (models/backbones/DiT2D.py of the reference), the backbone of
arch "FM-DiT".

`param_shapes` lists the `state_dict` names and shapes in the reference's order (own parameters first --
spatial_pos_embed, temporal_pos_embed, DiT2D.py:196-201 -- then the child modules in registration order:
time_embeddings, time_proj, patch_embed, blocks, final_layer), and `init_params` gives seeded NON-ZERO weights from the
repo PRNG with the ranges of `dit_spec.init_params`.  The reference zero-initialises adaLN_modulation and the final
layer (AdaLN-Zero, DiT2D.py:98-99,120-123); with those weights the output is identically 0.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from . import prng
from .spec import TIME_TABLE_ROWS, sinusoid_table


@dataclass(frozen=True)
class DiT2DConfig:
    """Hyper-parameters of the reference `DiT2D` ctor (DiT2D.py:152-168) plus the frame counts of the tensors it is
    called with (the reference reads them off `past` / `future`)."""
    input_channels: int = 4
    output_channels: int = 4
    grid_rows: int = 12
    grid_cols: int = 36
    past_len: int = 5
    future_len: int = 3
    patch_size: int = 4
    hidden_size: int = 256
    depth: int = 6
    num_heads: int = 4
    mlp_ratio: float = 4.0
    dropout_rate: float = 0.1
    time_multiple: int = 4
    condition: str = "Past"
    t_max: int = 8

    @property
    def n_s(self) -> int:
        return (self.grid_rows // self.patch_size) * (self.grid_cols // self.patch_size)

    @property
    def t_p(self) -> int:
        return self.past_len + self.future_len

    @property
    def qs(self) -> int:
        return self.past_len

    @property
    def tokens(self) -> int:
        return self.t_p * self.n_s

    @property
    def mlp_hidden(self) -> int:
        return int(self.hidden_size * self.mlp_ratio)   # DiT2D.py:89


def param_shapes(cfg: DiT2DConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    D, tx, p = cfg.hidden_size, cfg.hidden_size * cfg.time_multiple, cfg.patch_size
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    out["spatial_pos_embed"] = (1, cfg.n_s, D)
    out["temporal_pos_embed"] = (1, cfg.t_max, D)
    out["time_embeddings.time_blocks.0.weight"] = (TIME_TABLE_ROWS, D)
    out["time_embeddings.time_blocks.1.weight"] = (tx, D)
    out["time_embeddings.time_blocks.1.bias"] = (tx,)
    out["time_embeddings.time_blocks.3.weight"] = (tx, tx)
    out["time_embeddings.time_blocks.3.bias"] = (tx,)
    out["time_proj.0.weight"] = (D, tx)
    out["time_proj.0.bias"] = (D,)
    out["patch_embed.proj.weight"] = (D, cfg.input_channels, p, p)
    out["patch_embed.proj.bias"] = (D,)
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        out[b + "attn.in_proj_weight"] = (3 * D, D)
        out[b + "attn.in_proj_bias"] = (3 * D,)
        out[b + "attn.out_proj.weight"] = (D, D)
        out[b + "attn.out_proj.bias"] = (D,)
        out[b + "mlp.0.weight"] = (cfg.mlp_hidden, D)
        out[b + "mlp.0.bias"] = (cfg.mlp_hidden,)
        out[b + "mlp.3.weight"] = (D, cfg.mlp_hidden)
        out[b + "mlp.3.bias"] = (D,)
        out[b + "adaLN_modulation.1.weight"] = (6 * D, D)
        out[b + "adaLN_modulation.1.bias"] = (6 * D,)
    nout = cfg.output_channels * p * p
    out["final_layer.linear.weight"] = (nout, D)
    out["final_layer.linear.bias"] = (nout,)
    out["final_layer.adaLN_modulation.1.weight"] = (2 * D, D)
    out["final_layer.adaLN_modulation.1.bias"] = (2 * D,)
    return out


def init_params(cfg: DiT2DConfig, seed: int = 42) -> Dict[str, np.ndarray]:
    """Non-zero fp32 weights from the repo PRNG: Linear / Conv weights and biases ~ U(+-1/sqrt(fan_in)), MHA
    in-projection Xavier-uniform with bias U(+-0.02), position embeddings U(+-0.02), the frozen sinusoid table exact."""
    shapes = param_shapes(cfg)
    params: Dict[str, np.ndarray] = OrderedDict()
    for name, shp in shapes.items():
        n = int(np.prod(shp))
        if name == "time_embeddings.time_blocks.0.weight":
            params[name] = sinusoid_table(cfg.hidden_size)
            continue
        u = prng.uniform_pm1(seed, name, n).reshape(shp)
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith("pos_embed") or leaf == "in_proj_bias":
            bound = 0.02
        elif leaf == "in_proj_weight":
            bound = np.sqrt(6.0 / (shp[0] + shp[1]))
        elif leaf == "weight":
            bound = 1.0 / np.sqrt(int(np.prod(shp[1:])))
        else:
            bound = 1.0 / np.sqrt(int(np.prod(shapes[name[: -len("bias")] + "weight"][1:])))
        params[name] = (np.float32(bound) * u).astype(np.float32)
    return params
