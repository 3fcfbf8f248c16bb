"""models/guidance.py:44-69 of the reference through the C ABI.

`preservationMassNumericalGradientOptimal` keeps the reference's name, argument order and defaults.  The reference
perturbs every element in turn and re-evaluates the whole energy (N = C*H*W*L energy evaluations per call); here
cm_mass_preservation_grad evaluates the same forward-difference quotient in closed form on the device (the residual is
linear in each single element, so each quotient touches at most four residual cells).  The
sampling loop applies the guidance on the device by itself (cm_sample_opts.guidance = GUIDANCE_MASS_PRESERVATION);
this function is the stand-alone form.
"""
from __future__ import annotations

import numpy as np

from . import native


def _device_index(device) -> int:
    """None -> 0; an int; or anything with an `.index` / a "cuda:N" string (the reference passes a torch.device)."""
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    idx = getattr(device, "index", None)
    if idx is not None:
        return int(idx)
    s = str(device)
    return int(s.split(":", 1)[1]) if ":" in s else 0


def preservationMassNumericalGradientOptimal(x, device=None, delta_t=0.5, delta_l=1.0, eps=0.01) -> np.ndarray:
    """(E(x + eps e_i) - E(x)) / eps for every element i of x [B, C, H, W, L] (C >= 3), E = compute_energy(x, delta_t,
    delta_l).  Returns a float32 array of x's shape; channels >= 3 are 0."""
    x = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
    if x.ndim != 5:
        raise ValueError(f"x has shape {x.shape}: expected [B, C, H, W, L]")
    B, C_, H, W, L = (int(n) for n in x.shape)
    out = np.empty_like(x)
    if x.size == 0:
        return out
    dev = _device_index(device)
    dx = native.DeviceBuffer.from_array(x, dev)
    dg = native.DeviceBuffer(x.nbytes, dev)
    try:
        native.check(native.lib().cm_mass_preservation_grad(dev, dx.ptr, B, C_, H, W, L, float(delta_t), float(delta_l),
                                                            float(eps), dg.ptr, None))
        native.check(native.lib().cm_device_synchronize(dev))
        return dg.download(x.shape)
    finally:
        dx.free()
        dg.free()
