"""One conv launch of the UNet plan against a plain host evaluation: the reference every kernel-level conv test shares
(tests/test_gpu_six_term_hostile.py, tests/test_gpu_h2.py, tests/test_gpu_conv_layers_exact.py, tests/test_conv_oracle_cpu.py).
Data and numpy only; the two helpers that talk to a handle (_find, _run) import the native binding when they are called.

conv_ref evaluates what cm_debug_conv_io launches -- one Conv3d of the reference's models/backbones/layers.py:30-43,84,93-96,
bias kept, nothing else -- in the INTERNAL layout, from what cm_debug_conv_info prints (parse_info):

  x0 [B][Zs][Ys][Xs][C0] and, for a decoder conv_1 / match_input, x1 [..][C1]: the two halves of torch.cat([h, skip], dim=1)
    (unet.py:160) -- x0 is h, the tensor that came up the decoder, x1 the popped encoder tensor (csrc/cm_model.cpp: build_ops
    hands res_block (h, skip) in that order), so the weight's input channels are [x0's C0 | x1's C1];
  w: the state_dict tensor [Co][Ci][kH][kW][kL] -- tap (dz, dy, dx) = element [dy][dx][dz] (Z = frames = L, Y = rows = H,
    X = cols = W) -- or [Co][Ci] (the attention projections).  Ci may be smaller than C0 + C1: the first conv's source is padded to
    8 channels, the weight covers in_channels only, and the padding channels carry weight zero;
  ntaps 27 or 1 (the info line's 8 = the parity form of an upsample conv: 27 reference taps), stride 1 or 2 with padding 1,
  par: nearest x2 upsample (F.interpolate(scale_factor=2, mode="nearest")) followed by the 3x3x3 conv, padding 1.

It returns (y, S): y the convolution with its bias, S = sum |x| |w| + |bias| per output, the backward-error scale of the dot
product.  float64 for real operands.  For INTEGER operands both are int64 and exact: the products run as float64 matrix products
of integer-valued arrays, which no summation order can round while max S < 2^53 (asserted), and are converted back;
tests/test_conv_oracle_cpu.py holds that path to a pure int64 einsum.

The integer operands (int_source, int_state_dict) are the ones with which every kernel, tile, operand form and K split of the plan
must return conv_ref's integers bit for bit: x in [-3, 3], weights 4 k with k in [-2, 2] (the 4 keeps G g G^T of the in-plane
F(2x2, 3x3) Winograd transform integral, at most 18 in magnitude), biases in [-8, 8].  Then every product and partial sum of
every form is an integer below 2^24 -- fp32 accumulation in any order, the bf16 three-way and f16 two-way splits (hi alone) and
the power-of-two scales of the h2 forms are all exact -- provided 16 max S < 2^24 (EXACT_LIMIT; 16 >= the Winograd
intermediates' 9 x, with margin), which the tests assert from S itself."""
import ctypes as C
import zlib

import numpy as np

from crowdmod_ddpm_4d_amd import spec

INFO_FIELDS = ("ntaps", "stride", "par", "Ci", "Co", "Zo", "Yo", "Xo", "NB", "MB", "bz", "by", "bx", "ks", "flags", "out_C", "C0", "C1", "wino")
EXACT_LIMIT = 2 ** 24
X_MAX, W_STEP, W_KMAX, B_MAX = 3, 4, 2, 8
INT_CONVS = ("first", "conv_1", "conv_2", "match_input", "downsample", "upsample.1", "final.2")   # the leaves int_state_dict replaces


def parse_info(line):
    """cm_debug_conv_info's "conv <label> ntaps stride par Ci Co Zo Yo Xo NB MB bz by bx ks flags out_C C0 C1 wino kernel form
    [tail]" as a dict (integers, `label`, `kernel`, `form`, plus the derived `taps` -- the reference's 1 or 27 -- and `src`, the
    (Zs, Ys, Xs) of the sources); None for any other line."""
    f = line.split()
    if not f or f[0] != "conv":
        return None
    if len(f) < 23:
        raise ValueError(f"cm_debug_conv_info: unexpected line {line!r}")
    g = {"label": f[1], "kernel": f[21], "form": int(f[22])}
    g.update({k: int(v) for k, v in zip(INFO_FIELDS, f[2:21])})
    g["taps"] = 1 if g["ntaps"] == 1 else 27
    zyx = (g["Zo"], g["Yo"], g["Xo"])
    # (the plan admits only grids that halve exactly at every level, cm_model.cpp: build_ops)
    g["src"] = tuple(v // 2 for v in zyx) if g["par"] else tuple(v * g["stride"] for v in zyx)
    if g["par"] and any(v % 2 for v in zyx):
        raise ValueError(f"upsample conv with an odd output extent: {line!r}")
    return g


def conv_ops(net):
    """[parse_info dict + idx] of every op the handle reports as a conv, in plan order."""
    from crowdmod_ddpm_4d_amd import native
    L, h = native.lib(), net._handle
    cnt = C.c_int32()
    native.check(L.cm_debug_conv_count(h, C.byref(cnt)))
    buf = C.create_string_buffer(512)
    out = []
    for i in range(cnt.value):
        native.check(L.cm_debug_conv_info(h, i, buf, len(buf)))
        g = parse_info(buf.value.decode())
        if g is not None:
            g["idx"] = i
            out.append(g)
    return out


def _find(net, label):
    """(op index, parse_info dict) of the conv whose weight is `label`."""
    for g in conv_ops(net):
        if g["label"] == label:
            return g["idx"], g
    raise KeyError(label)


def _run(net, idx, mode, x, out_shape, x1=None):
    """cm_debug_conv_io on host sources x [B][Zs][Ys][Xs][C0] (and x1 [..][C1]); out_shape's last extent is the channel stride
    of the output tensor (out_C of the info line)."""
    from crowdmod_ddpm_4d_amd import native
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x1 is not None:
        x1 = np.ascontiguousarray(x1, dtype=np.float32)
        assert x1.shape[:-1] == x.shape[:-1], (x.shape, x1.shape)
    out = np.empty(out_shape, dtype=np.float32)
    native.check(native.lib().cm_debug_conv_io(net._handle, idx, mode, x.ctypes.data, x1.ctypes.data if x1 is not None else None,
                                               out.ctypes.data, x.shape[0]))
    return out


def _taps(w, Ci, taps):
    """The weight as [taps][Ci][Co] float64 in the internal tap order (dz, dy, dx), zero rows for source channels past the weight's."""
    w = np.asarray(w)
    Co, Cw = w.shape[0], w.shape[1]
    if Cw > Ci:
        raise ValueError(f"weight has {Cw} input channels, the sources {Ci}")
    w = w.reshape(Co, Cw, 1, 1, 1) if taps == 1 else w
    k = 1 if taps == 1 else 3
    if w.shape[2:] != (k, k, k):
        raise ValueError(f"weight {w.shape} is not a {taps}-tap kernel")
    t = np.zeros((taps, Ci, Co))
    t[:, :Cw] = np.transpose(w.astype(np.float64), (4, 2, 3, 1, 0)).reshape(taps, Cw, Co)   # [kL = dz][kH = dy][kW = dx][Ci][Co]
    return t


def _sweep(x, t, bias, taps, stride, dtype=np.float64):
    """bias + sum over taps of (shifted, zero-padded, strided view of x) @ t[tap], accumulated in `dtype`."""
    Bn, Z, Y, X, Ci = x.shape
    if taps == 1:
        if stride != 1:
            raise ValueError("a 1x1x1 conv has stride 1")
        return (np.zeros((Bn, Z, Y, X, t.shape[2]), dtype) + bias.astype(dtype) + x.astype(dtype) @ t[0].astype(dtype)).astype(dtype)
    Zo, Yo, Xo = ((n - 1) // stride + 1 for n in (Z, Y, X))      # floor((n + 2 - 3) / s) + 1 (layers.py:84), odd extents included
    xp = np.zeros((Bn, Z + 2, Y + 2, X + 2, Ci), dtype)
    xp[:, 1:-1, 1:-1, 1:-1] = x
    y = np.zeros((Bn, Zo, Yo, Xo, t.shape[2]), dtype) + bias.astype(dtype)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                v = xp[:, dz:dz + stride * (Zo - 1) + 1:stride, dy:dy + stride * (Yo - 1) + 1:stride, dx:dx + stride * (Xo - 1) + 1:stride]
                y = y + (v @ t[(dz * 3 + dy) * 3 + dx].astype(dtype)).astype(dtype)
    return y


def conv_ref(x0, w, bias, x1=None, ntaps=27, stride=1, par=0):
    """(y, S) of one launch, see the module text.  int64 when x0, x1, w and bias are all integer arrays, float64 otherwise."""
    arrs = [np.asarray(a) for a in (x0, w, bias) + ((x1,) if x1 is not None else ())]
    exact = all(np.issubdtype(a.dtype, np.integer) for a in arrs)
    x = np.asarray(x0, np.float64)
    if x1 is not None:
        x = np.concatenate([x, np.asarray(x1, np.float64)], axis=-1)          # torch.cat([h, skip], dim=1)
    taps = 1 if ntaps == 1 else 27
    if par:
        if taps != 27 or stride != 1:
            raise ValueError("the upsample conv is 3x3x3, stride 1")
        x = x.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)
    t = _taps(w, x.shape[-1], taps)
    b = np.asarray(bias, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = _sweep(x, t, b, taps, stride)
        S = _sweep(np.abs(x), np.abs(t), np.abs(b), taps, stride)
    if exact:
        assert float(S.max()) < 2.0 ** 53, "integer operands too large for an exact float64 evaluation"
        return np.rint(y).astype(np.int64), np.rint(S).astype(np.int64)
    return y, S


def conv_ref32(x0, w, bias, x1=None, ntaps=27, stride=1, par=0):
    """The same launch in float32, tap by tap (float32 matrix products, float32 running sum): the CPU reference's own fp32
    rounding on the same data, the yardstick e_ref of the real-valued device pass."""
    x = np.asarray(x0, np.float32)
    if x1 is not None:
        x = np.concatenate([x, np.asarray(x1, np.float32)], axis=-1)
    taps = 1 if ntaps == 1 else 27
    if par:
        x = x.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)
    with np.errstate(invalid="ignore", over="ignore"):
        return _sweep(x, _taps(w, x.shape[-1], taps).astype(np.float32), np.asarray(bias, np.float32), taps, stride, np.float32)


def _ref64(x, w, bias, ups):
    """fp64 evaluation of a single-source 3x3x3 launch (the form tests/test_gpu_six_term_hostile.py and test_gpu_h2.py ask in)."""
    return conv_ref(np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64), par=1 if ups else 0)


def ref_of(g, x0, x1, w, bias, ref=conv_ref):
    """conv_ref (or conv_ref32) with the launch facts of a parse_info dict."""
    return ref(x0, w, bias, x1=x1, ntaps=g["ntaps"], stride=g["stride"], par=g["par"])


# ---- integer operands -------------------------------------------------------------------------------------------------------
def _rng(seed, tag):
    return np.random.default_rng([int(seed), zlib.crc32(tag.encode())])


def int_source(shape, seed, tag, valid=None):
    """int64 source [B][Z][Y][X][C] in [-3, 3]; channels from `valid` on (the first conv's padding) are zero.  Sample b's data
    depends on (seed, tag, b) alone, so a batch's sample b is the B = 1 source of the same tag shifted to b."""
    x = np.stack([_rng(seed, f"{tag}/{b}").integers(-X_MAX, X_MAX + 1, size=shape[1:]) for b in range(shape[0])]).astype(np.int64)
    if valid is not None:
        x[..., valid:] = 0
    return x


def int_weight(shape, seed, name):
    return (W_STEP * _rng(seed, name).integers(-W_KMAX, W_KMAX + 1, size=shape)).astype(np.int64)


def int_bias(shape, seed, name):
    return _rng(seed, name).integers(-B_MAX, B_MAX + 1, size=shape).astype(np.int64)


def is_int_conv(name):
    """Is state_dict entry `name` a weight or bias that int_state_dict replaces?"""
    stem, leaf = name.rsplit(".", 1)
    return leaf in ("weight", "bias") and any(stem == c or stem.endswith("." + c) for c in INT_CONVS)


def int_state_dict(cfg, seed):
    """spec.init_params(cfg, seed) with every conv weight and bias (INT_CONVS) replaced by float32 copies of int_weight /
    int_bias; GroupNorm affines, the time MLP and the attention projections stay as initialised."""
    params = dict(spec.init_params(cfg, seed))
    for name, v in params.items():
        if is_int_conv(name):
            gen = int_weight if name.endswith(".weight") else int_bias
            params[name] = gen(v.shape, seed, name).astype(np.float32)
    return params


def real_source(kind, shape, seed, tag, valid=None):
    """float32 sources of the real-valued pass: "unit" SiLU of a standard normal (the operating point), "wide" log-uniform
    1e-30 .. 1e30 with random signs, "cancel" 1e6 + a standard normal."""
    rng = _rng(seed, f"{kind}/{tag}")
    if kind == "unit":
        v = rng.standard_normal(shape)
        x = v / (1.0 + np.exp(-v))
    elif kind == "wide":
        x = rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-30, 30, size=shape)
    elif kind == "cancel":
        x = 1.0e6 + rng.standard_normal(shape)
    else:
        raise KeyError(kind)
    x = x.astype(np.float32)
    if valid is not None:
        x[..., valid:] = 0
    return x


def conv_shapes(cfg):
    """[(weight name, Ci, Co, taps)] of every conv int_state_dict makes integer, from spec.param_shapes (= spec.make_plan's
    channel counts)."""
    return [(n, s[1], s[0], int(np.prod(s[2:]))) for n, s in spec.param_shapes(cfg).items() if n.endswith(".weight") and is_int_conv(n)]


def worst_case_S(Ci, taps):
    """The largest S any output of a conv over Ci channels can reach with the integer operands: every tap inside the volume."""
    return taps * Ci * X_MAX * W_STEP * W_KMAX + B_MAX

