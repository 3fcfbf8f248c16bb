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
intermediates' 9 x, with margin), which the tests assert from S itself.

THE REDUCED-PRECISION PLAN (tests/test_gpu_f16_layers.py).  conv_ref / conv_ref32 take three optional additions, the tail of an
inference launch that cm_debug_conv_tail keeps: the block's fused 1x1x1 skip conv (x_s0, x_s1 [B][Zo][Yo][Xo][C]: its raw sources,
centre tap; w_skip [Co][Cs] or [Co][Cs][1][1][1], b_skip), a residual [B][Zo][Yo][Xo][Co], and store_f16: the result rounded to f16
(f16_round: float64 -> np.float16, round to nearest even, overflow to +-inf; y is then float64 even for integer operands, S is
never rounded).  The integer operands above are exact in f16 (|x| <= 3, |w| <= 8, |residual| <= 3) and every partial sum is an
integer below 2^24, so an f16-operand kernel with fp32 accumulation must return f16_round(exact int64) BIT FOR BIT: integers up to
2048 unchanged, larger ones on f16's grid (spacing 2 up to 4096, then 4: ties to even, 2049 -> 2048, 2051 -> 2052, 4102 -> 4104).
For real operands the caller rounds what the kernel rounds (f16_round of the sources, the weights, an f16-stored residual) and the
only thing left between the oracle and the device is the order of an fp32 sum.  `fold` (a rounding function) evaluates an upsample
conv in the parity form the kernels run -- per output parity class 2 x 2 x 2 taps on the SOURCE grid, each the float64 sum of the
reference taps that fall on one source voxel, rounded to float32 and then by `fold` (cm_pack.h: parity_weights, pack_ups_f16) --
because there the f16 operand is the folded weight, not the reference tap."""
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
    (Zs, Ys, Xs) of the sources; of the tail cm_debug_conv_info_ext appends: `h16` the product launch's f16-tensor mask, `res` the residual's channels, `skip`
    (C0, C1) of the fused skip conv's sources, `f16d` / `upst` (bz, by, bx, mbw) the tile of the direct f16 / stage-once upsample
    kernel, `alone` (kernel, form) the route the hook launches an absorbed skip conv on, each where present); None for any other line."""
    f = line.split()
    if not f or f[0] != "conv":
        return None
    if len(f) < 23:
        raise ValueError(f"cm_debug_conv_info: unexpected line {line!r}")
    g = {"label": f[1], "kernel": f[21], "form": int(f[22])}
    g.update({k: int(v) for k, v in zip(INFO_FIELDS, f[2:21])})
    g["taps"] = 1 if g["ntaps"] == 1 else 27
    tail = f[23:]
    for key, n in (("h16", 1), ("res", 1), ("skip", 2), ("f16d", 4), ("upst", 4)):      # trailing tokens, where the line carries them
        if key in tail:
            i = tail.index(key)
            v = tuple(int(a) for a in tail[i + 1:i + 1 + n])
            g[key] = v[0] if n == 1 else v
    if "alone" in tail:
        g["alone"] = (tail[tail.index("alone") + 1], int(tail[tail.index("alone") + 2]))
    zyx = (g["Zo"], g["Yo"], g["Xo"])
    # (the plan admits only grids that halve exactly at every level, cm_model.cpp: build_ops)
    g["src"] = tuple(v // 2 for v in zyx) if g["par"] else tuple(v * g["stride"] for v in zyx)
    if g["par"] and any(v % 2 for v in zyx):
        raise ValueError(f"upsample conv with an odd output extent: {line!r}")
    return g


def conv_ops(net, ext=False):
    """[parse_info dict + idx] of every op the handle reports as a conv, in plan order; ext: through cm_debug_conv_info_ext, the
    line with its trailing tokens (h16, res, skip, f16d / upst, alone)."""
    from crowdmod_ddpm_4d_amd import native
    L, h = native.lib(), net._handle
    cnt = C.c_int32()
    native.check(L.cm_debug_conv_count(h, C.byref(cnt)))
    buf = C.create_string_buffer(512)
    info = native.hook("cm_debug_conv_info_ext") if ext else L.cm_debug_conv_info
    out = []
    for i in range(cnt.value):
        native.check(info(h, i, buf, len(buf)))
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


def f16_round(a):
    """`a` rounded to IEEE binary16 and widened again, as float64: round to nearest even, overflow to +-inf, subnormals kept (a
    device (_Float16) cast of an fp32 value; every fp32 is a float64, and numpy rounds float64 -> float16 once)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


_FOLD = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}   # (output parity, folded tap) -> reference taps, one axis


def _sweep_par(x, t, bias, fold, dtype=np.float64):
    """The upsample conv on the SOURCE x in the kernels' parity form: output voxel 2 s + p reads the source voxels s + p - 1 + u,
    u in {0, 1}, per axis, each through the sum of the reference taps that land on it (folded in float64, rounded to float32,
    then by `fold`)."""
    Bn, Z, Y, X, Ci = x.shape
    t = np.asarray(t, np.float64).reshape(3, 3, 3, Ci, -1)
    xp = np.zeros((Bn, Z + 2, Y + 2, X + 2, Ci), dtype)
    xp[:, 1:-1, 1:-1, 1:-1] = x
    y = np.zeros((Bn, 2 * Z, 2 * Y, 2 * X, t.shape[-1]), dtype) + np.asarray(bias).astype(dtype)
    for pz in range(2):
        for py in range(2):
            for px in range(2):
                for uz in range(2):
                    for uy in range(2):
                        for ux in range(2):
                            wf = t[np.ix_(_FOLD[pz, uz], _FOLD[py, uy], _FOLD[px, ux])].sum(axis=(0, 1, 2))
                            wf = np.asarray(fold(wf.astype(np.float32))).astype(dtype)
                            v = xp[:, pz + uz:pz + uz + Z, py + uy:py + uy + Y, px + ux:px + ux + X]
                            y[:, pz::2, py::2, px::2] = y[:, pz::2, py::2, px::2] + (v @ wf).astype(dtype)
    return y


def _skip_w(w_skip, Cs):
    w2 = np.asarray(w_skip)
    w2 = w2.reshape(w2.shape[0], -1)
    if w2.shape[1] != Cs:
        raise ValueError(f"skip weight has {w2.shape[1]} input channels, its sources {Cs}")
    return w2


def _tail(y, dtype, x_s0, x_s1, w_skip, b_skip, resid, mag=False):
    """y + the fused skip conv (centre tap of its raw sources) + the residual, in `dtype`; mag: of absolute values (for S)."""
    f = np.abs if mag else (lambda a: a)
    if w_skip is not None:
        xs = np.asarray(x_s0, dtype) if x_s1 is None else np.concatenate([np.asarray(x_s0, dtype), np.asarray(x_s1, dtype)], axis=-1)
        if xs.shape[:-1] != y.shape[:-1]:
            raise ValueError(f"skip sources {xs.shape} do not lie on the output grid {y.shape}")
        w2 = _skip_w(w_skip, xs.shape[-1])
        y = (y + (f(xs) @ f(w2.astype(dtype)).T).astype(dtype)).astype(dtype) + f(np.asarray(b_skip).astype(dtype))
    if resid is not None:
        if np.shape(resid) != y.shape:
            raise ValueError(f"residual {np.shape(resid)} against output {y.shape}")
        y = y + f(np.asarray(resid).astype(dtype))
    return y.astype(dtype)


def conv_ref(x0, w, bias, x1=None, ntaps=27, stride=1, par=0, x_s0=None, x_s1=None, w_skip=None, b_skip=None, resid=None,
             store_f16=False, fold=None):
    """(y, S) of one launch, see the module text.  int64 when every operand is an integer array (float64 under store_f16),
    float64 otherwise."""
    if (w_skip is None) != (x_s0 is None) or (w_skip is None) != (b_skip is None) or (x_s1 is not None and x_s0 is None):
        raise ValueError("a fused skip conv needs x_s0, w_skip and b_skip")
    extra = tuple(a for a in (x1, x_s0, x_s1, w_skip, b_skip, resid) if a is not None)
    arrs = [np.asarray(a) for a in (x0, w, bias) + extra]
    exact = all(np.issubdtype(a.dtype, np.integer) for a in arrs)
    x = np.asarray(x0, np.float64)
    if x1 is not None:
        x = np.concatenate([x, np.asarray(x1, np.float64)], axis=-1)          # torch.cat([h, skip], dim=1)
    taps = 1 if ntaps == 1 else 27
    if par and (taps != 27 or stride != 1):
        raise ValueError("the upsample conv is 3x3x3, stride 1")
    if fold is not None and not par:
        raise ValueError("fold is the parity form of an upsample conv")
    t = _taps(w, x.shape[-1], taps)
    b = np.asarray(bias, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if fold is not None:
            y, S = _sweep_par(x, t, b, fold), _sweep_par(np.abs(x), np.abs(t), np.abs(b), lambda a: np.abs(fold(a)))
        else:
            if par:
                x = x.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)
            y = _sweep(x, t, b, taps, stride)
            S = _sweep(np.abs(x), np.abs(t), np.abs(b), taps, stride)
        y = _tail(y, np.float64, x_s0, x_s1, w_skip, b_skip, resid)
        S = _tail(S, np.float64, x_s0, x_s1, w_skip, b_skip, resid, mag=True)
    if exact:
        assert float(S.max()) < 2.0 ** 53, "integer operands too large for an exact float64 evaluation"
        y, S = np.rint(y).astype(np.int64), np.rint(S).astype(np.int64)
    return (f16_round(y) if store_f16 else y), S


def conv_ref32(x0, w, bias, x1=None, ntaps=27, stride=1, par=0, x_s0=None, x_s1=None, w_skip=None, b_skip=None, resid=None,
               store_f16=False, fold=None):
    """The same launch in float32, tap by tap (float32 matrix products, float32 running sum): the CPU reference's own fp32
    rounding on the same data, the yardstick e_ref of the real-valued device pass."""
    x = np.asarray(x0, np.float32)
    if x1 is not None:
        x = np.concatenate([x, np.asarray(x1, np.float32)], axis=-1)
    taps = 1 if ntaps == 1 else 27
    t = _taps(w, x.shape[-1], taps)
    with np.errstate(invalid="ignore", over="ignore"):
        if fold is not None:
            y = _sweep_par(x, t, np.asarray(bias, np.float32), fold, np.float32)
        else:
            if par:
                x = x.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)
            y = _sweep(x, t.astype(np.float32), np.asarray(bias, np.float32), taps, stride, np.float32)
        y = _tail(y, np.float32, x_s0, x_s1, w_skip, b_skip, resid)
    return f16_round(y).astype(np.float32) if store_f16 else y


def _ref64(x, w, bias, ups):
    """fp64 evaluation of a single-source 3x3x3 launch (the form tests/test_gpu_six_term_hostile.py and test_gpu_h2.py ask in)."""
    return conv_ref(np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64), par=1 if ups else 0)


def ref_of(g, x0, x1, w, bias, ref=conv_ref, **tail):
    """conv_ref (or conv_ref32) with the launch facts of a parse_info dict; `tail`: the optional additions."""
    return ref(x0, w, bias, x1=x1, ntaps=g["ntaps"], stride=g["stride"], par=g["par"], **tail)


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
    1e-30 .. 1e30 with random signs, "cancel" 1e6 + a standard normal, "f16wide" log-uniform over binary16's range."""
    rng = _rng(seed, f"{kind}/{tag}")
    if kind == "unit":
        v = rng.standard_normal(shape)
        x = v / (1.0 + np.exp(-v))
    elif kind == "wide":
        x = rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-30, 30, size=shape)
    elif kind == "cancel":
        x = 1.0e6 + rng.standard_normal(shape)
    elif kind == "f16wide":
        # magnitudes log-uniform over binary16's whole range, 2^-24 (the smallest subnormal) .. 65504, random signs
        x = rng.choice([-1.0, 1.0], size=shape) * np.minimum(2.0 ** rng.uniform(-24, 16, size=shape), 65504.0)
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



# ---- the launches of a plan, without a handle ----------------------------------------------------------------------------------
def _out_grid(src, stride, par):
    return tuple(2 * n for n in src) if par else tuple((n - 1) // stride + 1 for n in src)


def plan_convs(cfg, rows, cols, frames):
    """Every conv int_state_dict makes integer, as one launch each, from spec.make_plan alone: [dict(label, C0, C1, Cw, src
    (Zs, Ys, Xs), out (Zo, Yo, Xo), Co, ntaps, stride, par, tail)] in forward order.  tail: what the block adds
    behind its conv_2 -- ("skip", C of the block input, C of the popped encoder tensor) where the widths differ (match_input, which
    the inference plan fuses into conv_2), ("res", Co) where they agree -- else None.  cm_debug_conv_info says the same of a
    handle (launch_of); tests/test_gpu_f16_layers.py holds the two against each other."""
    plan = spec.make_plan(cfg)
    grid = lambda level: (frames >> level, rows >> level, cols >> level)

    def one(label, C0, C1, Co, src, ntaps=27, stride=1, par=0, tail=None, Cw=None):
        return dict(label=label, C0=C0, C1=C1, Cw=C0 + C1 if Cw is None else Cw, Co=Co, src=src, out=_out_grid(src, stride, par),
                    ntaps=ntaps, stride=stride, par=par, tail=tail)
    out = [one("first.weight", 8, 0, cfg.base_channels, grid(0), Cw=cfg.input_channels)]
    for b in plan.encoder + plan.bottleneck + plan.decoder:
        g = grid(b.level)
        if b.kind == "down":
            out.append(one(b.prefix + ".downsample.weight", b.cin, 0, b.cout, g, stride=2))
        elif b.kind == "up":
            out.append(one(b.prefix + ".upsample.1.weight", b.cin, 0, b.cout, g, par=1))
        else:
            h, sk = b.cin - b.skip_channels, b.skip_channels
            out.append(one(b.prefix + ".conv_1.weight", h, sk, b.cout, g))
            if b.cin != b.cout:
                out.append(one(b.prefix + ".match_input.weight", h, sk, b.cout, g, ntaps=1))
            out.append(one(b.prefix + ".conv_2.weight", b.cout, 0, b.cout, g, tail=("skip", h, sk) if b.cin != b.cout else ("res", b.cout)))
    out.append(one("final.2.weight", plan.final_channels, 0, cfg.output_channels, grid(0)))
    return out


def launch_of(g):
    """The same description from a parse_info dict (a handle's own word); Cw is not in the line (None)."""
    tail = ("skip",) + tuple(g["skip"]) if g.get("skip", (0, 0))[0] else ("res", g["res"]) if g.get("res") else None
    return dict(label=g["label"], C0=g["C0"], C1=g["C1"], Cw=None, Co=g["Co"], src=g["src"], out=(g["Zo"], g["Yo"], g["Xo"]),
                ntaps=1 if g["ntaps"] == 1 else 27, stride=g["stride"], par=g["par"], tail=tail)


def skip_names(label):
    """(weight, bias) names of the 1x1x1 skip conv a block fuses into the conv_2 named `label`."""
    stem = label[:-len("conv_2.weight")]
    return stem + "match_input.weight", stem + "match_input.bias"


def int_operands(key, d, B, Cw, seed, tail):
    """The integer operands of launch `d` (plan_convs / launch_of) of row `key` at batch B: (x0, x1, t0, t1), per-sample data
    (int_source); t0 / t1: the residual, or the fused skip conv's sources, when `tail` (and the launch has one), else None."""
    x0 = int_source((B,) + d["src"] + (d["C0"],), seed, f"{key}/{d['label']}/x0", valid=Cw if d["C0"] + d["C1"] > Cw else None)
    x1 = int_source((B,) + d["src"] + (d["C1"],), seed, f"{key}/{d['label']}/x1") if d["C1"] else None
    t0 = t1 = None
    if tail and d["tail"]:
        t0 = int_source((B,) + d["out"] + (d["tail"][1],), seed, f"{key}/{d['label']}/t0")
        if d["tail"][0] == "skip" and d["tail"][2]:
            t1 = int_source((B,) + d["out"] + (d["tail"][2],), seed, f"{key}/{d['label']}/t1")
    return x0, x1, t0, t1


def tail_args(d, t0, t1, params, conv=lambda a: a):
    """conv_ref's keyword arguments for the tail of launch `d` on (t0, t1); conv: how the weights enter (np.rint -> int64, f16_round, ...)."""
    if t0 is None:
        return {}
    if d["tail"][0] == "res":
        return dict(resid=t0)
    wn, bn = skip_names(d["label"])
    return dict(x_s0=t0, x_s1=t1, w_skip=conv(np.asarray(params[wn])), b_skip=params[bn])
