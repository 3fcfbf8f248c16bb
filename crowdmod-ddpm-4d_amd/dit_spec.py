"""Structural description of the reference DiT4D_V4 denoiser (/root/reference/models/backbones/DiT4D_V4.py).

`param_shapes` lists the `state_dict` names and shapes in the reference's order (own parameters first --
spatial_pos_embed, temporal_pos_embed, DiT4D_V4.py:289-295 -- then the child modules in registration order), and
`init_params` gives seeded NON-ZERO weights from the repo PRNG.  The reference zero-initialises adaLN_modulation and
the final layer (AdaLN-Zero, DiT4D_V4.py:138-139,218-221); with those weights the output is identically 0, so the
synthetic weights here use torch's default Linear ranges everywhere instead.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from . import prng
from .spec import TIME_TABLE_ROWS, sinusoid_table


@dataclass(frozen=True)
class DiTConfig:
    """Hyper-parameters of the reference `DiT4D_V4` ctor (DiT4D_V4.py:235-254)."""
    input_channels: int = 4
    output_channels: int = 4
    grid_rows: int = 12
    grid_cols: int = 36
    past_len: int = 5
    future_len: int = 3
    t_patch_size: int = 2
    patch_size: int = 4
    hidden_size: int = 256
    depth: int = 6
    num_heads: int = 4
    mlp_ratio: float = 4.0
    dropout_rate: float = 0.1
    time_multiple: int = 4
    condition: str = "Past"
    T_max: int = 32

    @property
    def n_s(self) -> int:
        return (self.grid_rows // self.patch_size) * (self.grid_cols // self.patch_size)

    @property
    def t_p(self) -> int:
        return (self.past_len + self.future_len) // self.t_patch_size

    @property
    def qs(self) -> int:
        return self.past_len // self.t_patch_size

    @property
    def mlp_hidden(self) -> int:
        return int(self.hidden_size * self.mlp_ratio)   # DiT4D_V4.py:127


def param_shapes(cfg: DiTConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    D, tx, p, pt = cfg.hidden_size, cfg.hidden_size * cfg.time_multiple, cfg.patch_size, cfg.t_patch_size
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    out["spatial_pos_embed"] = (1, cfg.n_s, D)
    out["temporal_pos_embed"] = (1, cfg.T_max // pt, D)
    out["dif_time_embeddings.time_blocks.0.weight"] = (TIME_TABLE_ROWS, D)
    out["dif_time_embeddings.time_blocks.1.weight"] = (tx, D)
    out["dif_time_embeddings.time_blocks.1.bias"] = (tx,)
    out["dif_time_embeddings.time_blocks.3.weight"] = (tx, tx)
    out["dif_time_embeddings.time_blocks.3.bias"] = (tx,)
    out["time_proj.0.weight"] = (D, tx)
    out["time_proj.0.bias"] = (D,)
    out["patch_embed.proj.weight"] = (D, cfg.input_channels, pt, p, p)
    out["patch_embed.proj.bias"] = (D,)
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        for attn in ("spatial_attn", "temporal_attn"):
            out[b + attn + ".in_proj_weight"] = (3 * D, D)
            out[b + attn + ".in_proj_bias"] = (3 * D,)
            out[b + attn + ".out_proj.weight"] = (D, D)
            out[b + attn + ".out_proj.bias"] = (D,)
        out[b + "mlp.0.weight"] = (cfg.mlp_hidden, D)
        out[b + "mlp.0.bias"] = (cfg.mlp_hidden,)
        out[b + "mlp.3.weight"] = (D, cfg.mlp_hidden)
        out[b + "mlp.3.bias"] = (D,)
        out[b + "adaLN_modulation.1.weight"] = (9 * D, D)
        out[b + "adaLN_modulation.1.bias"] = (9 * D,)
    nout = pt * cfg.output_channels * p * p
    out["final_layer.linear.weight"] = (nout, D)
    out["final_layer.linear.bias"] = (nout,)
    out["final_layer.adaLN_modulation.1.weight"] = (2 * D, D)
    out["final_layer.adaLN_modulation.1.bias"] = (2 * D,)
    return out


def init_params(cfg: DiTConfig, seed: int = 42) -> Dict[str, np.ndarray]:
    """Non-zero fp32 weights from the repo PRNG: Linear / Conv weights and biases ~ U(+-1/sqrt(fan_in)), MHA
    in-projection Xavier-uniform with bias U(+-0.02), position embeddings U(+-0.02), the frozen sinusoid table exact."""
    shapes = param_shapes(cfg)
    params: Dict[str, np.ndarray] = OrderedDict()
    for name, shp in shapes.items():
        n = int(np.prod(shp))
        if name == "dif_time_embeddings.time_blocks.0.weight":
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
