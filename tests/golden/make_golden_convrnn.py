#!/usr/bin/env python3
"""Generate tests/golden/convrnn.npz from the reference's own Forecaster and ConvRNN_model._generate_convRNN.

    python tests/golden/make_golden_convrnn.py

Imports the reference's modules the way make_golden.py does (and reuses its placeholder imports).  Weights
(crowdmod_ddpm_4d_amd.convrnn_spec.init_params) and inputs (tests/convrnn_cases.py) are regenerated from the integer PRNG
on both sides, not stored.  e = max |ref32 - oracle64| / max |oracle64| against tests/convrnn_oracle.py throughout.
Captured, per <key> = <case>/<cell>/tf<0|1>:
  <key>/out                    the reference's fp32 forecast [B,4,H,W,Ft]
  <key>/e_ref                  e of the output
  <key>/e_ref_h<l>, _c<l>      e of the final hidden (and, ConvLSTM, cell) state of level l = 0 quarter, 1 half, 2 full
  tiny/...: <key>/h<l>, /c<l>  the state tensors themselves
  atc/<cell>/names, /shapes    state_dict names and shapes of the reference model
  gen/atc/gru                  ConvRNN_model._generate_convRNN(past, target, teacher_forcing=False): exp on channels 0 and 3
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path)
import convrnn_cases as CC  # noqa: E402


def ref_model(cfg, params):
    from models.convRNN.convGRUCell import ConvGRUCell
    from models.convRNN.convLSTMCell import ConvLSTMCell
    from models.convRNN.forecaster import Forecaster
    net = Forecaster((cfg.rows, cfg.cols), cfg.input_channels, list(cfg.enc_hidden), list(cfg.forc_hidden),
                     list(cfg.enc_kernels), list(cfg.forc_kernels), torch.device("cpu"),
                     ConvGRUCell if cfg.gru else ConvLSTMCell, bias=False)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return net.eval()


def ref_states(net, past, target, tf):
    """The reference's forward with its final hidden states: _init_hidden's list is updated in place by the forward."""
    held = []
    init = net._init_hidden

    def capture(batch_size, device):
        hs = init(batch_size=batch_size, device=device)
        held.append(hs)
        return hs
    net._init_hidden = capture
    try:
        with torch.no_grad():
            y = net(torch.from_numpy(past), torch.from_numpy(target), tf).numpy()
    finally:
        net._init_hidden = init
    return y, [(h.numpy(), None if c is None else c.numpy()) for h, c in held[0]]


def main():
    torch.manual_seed(0)
    d = {}
    for case, cell, tf in CC.keys():
        key = CC.key_id(case, cell, tf)
        cfg, params = CC.config(case, cell), CC.params(case, cell)
        past, target = CC.inputs(case)
        net = ref_model(cfg, params)
        if case == "atc" and not tf:
            sd = net.state_dict()
            assert sum(v.numel() for v in sd.values()) == (2747520 if cfg.gru else 3521664)
            d[f"atc/{cell}/names"] = np.array(list(sd.keys()))
            d[f"atc/{cell}/shapes"] = np.array([list(v.shape) for v in sd.values()], dtype=np.int64)
        y, st = ref_states(net, past, target, tf)
        y64, st64 = CC.oracle(case, cell, tf)
        d[f"{key}/out"] = y
        d[f"{key}/e_ref"] = np.float64(CC.rel_err(y, y64))
        line = [f"e_ref {d[f'{key}/e_ref']:.2e}"]
        for l, ((h, c), (h64, c64)) in enumerate(zip(st, st64)):
            for nm, a, a64 in (("h", h, h64), ("c", c, c64)):
                if a is None:
                    continue
                d[f"{key}/e_ref_{nm}{l}"] = np.float64(CC.rel_err(a, a64))
                line.append(f"{nm}{l} {d[f'{key}/e_ref_{nm}{l}']:.2e}")
                if case == "tiny":
                    d[f"{key}/{nm}{l}"] = a
        print(key, y.shape, f"max|ref| {float(np.abs(y).max()):.3f}", " ".join(line))
        # the conditioning rule of the DiT fixtures: a case the fp32 reference itself cannot hold is ill-conditioned
        assert all(float(v) <= 1e-5 for k, v in d.items() if k.startswith(key + "/e_ref")), key
    # _generate_convRNN reads nothing of its object but the network
    MG._placeholders()
    for name in ("tqdm", "matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].tqdm = None
    from models.convRNN import convRNN as RC
    cfg, params = CC.config("atc", "gru"), CC.params("atc", "gru")
    past, target = CC.inputs("atc")
    holder = types.SimpleNamespace(convRNN=ref_model(cfg, params))
    d["gen/atc/gru"] = RC.ConvRNN_model._generate_convRNN(holder, torch.from_numpy(past), torch.from_numpy(target), False).numpy()
    np.savez_compressed(os.path.join(HERE, "convrnn.npz"), **d)
    print("wrote convrnn.npz", os.path.getsize(os.path.join(HERE, "convrnn.npz")), "bytes")


if __name__ == "__main__":
    main()
