"""torch.optim.Adam.state_dict() of a native trainer's optimizer store, and its inverse: what the reference saves under
a checkpoint's "opt" entry (utils/utils.py:140-147).  "state" maps the position of every parameter that has received an
update to {"step", "exp_avg", "exp_avg_sq"} (and "max_exp_avg_sq" under amsgrad=True); a parameter with requires_grad
False keeps its position in "params" and never gets state.  UNet, DiT2D and Forecaster build and read it here."""
from __future__ import annotations

import numpy as np

ADAM_KEYS = ("exp_avg", "exp_avg_sq")
AMSGRAD_KEYS = ADAM_KEYS + ("max_exp_avg_sq",)


def _array(v) -> np.ndarray:
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def dump(names, frozen, keys, lr, betas, eps, weight_decay, get, step: int) -> dict:
    """names: model.parameters() order; frozen: those without state; get(name, which): the array behind keys[which]."""
    names, state = list(names), {}
    if step > 0:
        for i, name in enumerate(names):
            if name not in frozen:
                state[i] = {"step": np.float32(step), **{key: get(name, which) for which, key in enumerate(keys)}}
    group = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps),
             "weight_decay": float(weight_decay), "amsgrad": "max_exp_avg_sq" in keys, "maximize": False, "foreach": None,
             "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False,
             "params": list(range(len(names)))}
    return {"state": state, "param_groups": [group]}


def load(opt: dict, names, keys, put) -> int:
    """Every moment of `opt` (arrays or torch tensors) to put(name, which, float32 array); returns the step to resume
    from, the maximum over the entries (torch writes the same step into each)."""
    names, step = list(names), 0
    for i, st in opt.get("state", {}).items():
        for which, key in enumerate(keys):
            put(names[int(i)], which, np.ascontiguousarray(_array(st[key]), dtype=np.float32))
        step = max(step, int(_array(st["step"]).reshape(-1)[0]))
    return step
