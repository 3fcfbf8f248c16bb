"""Shapes, names and deterministic initial weights of the reference's ConvRNN forecaster (models/convRNN/forecaster.py,
encoder.py, convGRUCell.py, convLSTMCell.py; arch "ConvRNN").  Pure numpy: shared by the native binding, the float64
oracle of the tests and the fixture generator."""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from . import prng

CELLS = ("ConvGRUCell", "ConvLSTMCell")   # CELL_REGISTRY of convRNN.py:17-20
ENC_KERNELS = (3, 3, 3, 3, 3, 3)
FORC_KERNELS = (3, 4, 3, 4, 3, 3, 3)


@dataclass(frozen=True)
class ConvRNNConfig:
    rows: int = 12
    cols: int = 36
    input_channels: int = 4
    enc_hidden: Tuple[int, ...] = (16, 64, 64, 96, 96, 96)
    forc_hidden: Tuple[int, ...] = (96, 96, 96, 96, 96, 64, 16)
    enc_kernels: Tuple[int, ...] = ENC_KERNELS
    forc_kernels: Tuple[int, ...] = FORC_KERNELS
    cell: str = "ConvGRUCell"
    past_len: int = 5
    future_len: int = 3

    @property
    def gru(self) -> bool:
        return self.cell == "ConvGRUCell"

    def layers(self):
        """(prefix, kind, declared input channels, output / hidden channels, level) in state_dict order; level 0 is the
        quarter-resolution hidden state, 2 the full-resolution one."""
        E, F, C = self.enc_hidden, self.forc_hidden, self.input_channels
        enc = [("conv", C, E[0], 2), ("cell", E[0], E[1], 2), ("down", E[1], E[2], 1), ("cell", E[1], E[3], 1),
               ("down", E[3], E[4], 0), ("cell", E[3], E[5], 0)]
        forc = [("cell", F[0], F[1], 0), ("up", F[1], F[2], 1), ("cell", F[2], F[3], 1), ("up", F[3], F[4], 2),
                ("cell", F[4], F[5], 2), ("conv", F[5], F[6], 2), ("conv", F[6], C, 2)]
        return [(f"encoder.encoder_cell_list.{i}", *l) for i, l in enumerate(enc)] + \
               [(f"forecaster_cell_list.{i}", *l) for i, l in enumerate(forc)]


def param_shapes(cfg: ConvRNNConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """state_dict names and shapes of Forecaster(..., bias=False): weights only."""
    if cfg.cell not in CELLS:
        raise ValueError(f"Unsupported cell class: {cfg.cell}")
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for prefix, kind, cin, cout, _ in cfg.layers():
        if kind == "cell" and cfg.gru:
            for g in ("reset_gate", "update_gate", "conv_cand"):
                out[f"{prefix}.{g}.weight"] = (cout, cin + cout, 3, 3)
        elif kind == "cell":
            out[f"{prefix}.conv.weight"] = (4 * cout, cin + cout, 3, 3)
        elif kind == "up":
            out[f"{prefix}.weight"] = (cin, cout, 4, 4)      # ConvTranspose2d: [in, out, kH, kW]
        else:
            out[f"{prefix}.weight"] = (cout, cin, 3, 3)
    return out


GAIN = 3.0   # three times PyTorch's default range: the recurrence registers and the fp32 reference stays well conditioned


def init_params(cfg: ConvRNNConfig, seed: int = 42) -> Dict[str, np.ndarray]:
    """fp32 weights from the repo PRNG, U(+-GAIN / sqrt(fan_in)); fan_in as torch counts it (shape[1] * kH * kW, which for
    a ConvTranspose2d weight is out_channels * 16)."""
    params: Dict[str, np.ndarray] = OrderedDict()
    for name, shp in param_shapes(cfg).items():
        bound = np.float32(GAIN / np.sqrt(int(np.prod(shp[1:]))))
        params[name] = (bound * prng.uniform_pm1(seed, name, int(np.prod(shp))).reshape(shp)).astype(np.float32)
    return params
