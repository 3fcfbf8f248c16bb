"""Config loading with the reference's surface: `getYamlConfig(cfg.yml, datalist.yml)`
returns an attribute-dict (/root/reference/utils/myparser.py:5-33).

The reference's configs come in three schema generations;
`resolve()` extracts the keys the DDPM-UNet path needs from any of them.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Tuple

import yaml


class AttrDict(dict):
    """Minimal EasyDict: nested dicts become attribute-accessible."""

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v

    def __setitem__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, AttrDict):
            v = AttrDict(v)
        elif isinstance(v, (list, tuple)):
            v = type(v)(AttrDict(i) if isinstance(i, dict) else i for i in v)
        super().__setitem__(k, v)

    __setattr__ = __setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def update(self, d=None, **kw):
        for k, v in dict(d or {}, **kw).items():
            self[k] = v


class YamlParser(AttrDict):
    def __init__(self, cfg_dict=None, config_file=None):
        super().__init__(cfg_dict or {})
        if config_file is not None:
            self.merge_from_file(config_file)

    def merge_from_file(self, config_file):
        if not os.path.isfile(config_file):
            raise FileNotFoundError(config_file)
        with open(config_file, "r") as fo:
            self.update(yaml.safe_load(fo.read()) or {})

    def merge_from_dict(self, config_dict):
        self.update(config_dict)


def get_config(config_file=None):
    return YamlParser(config_file=config_file)


def getYamlConfig(config_yml_file, configList_yml_file=None):
    cfg = get_config()
    cfg.merge_from_file(config_yml_file)
    if configList_yml_file is not None:
        loaded = yaml.safe_load(open(configList_yml_file).read())
        if isinstance(loaded, dict):
            cfg.update(loaded)
    return cfg


@dataclass
class Resolved:
    """The hot path's view of a config, independent of schema generation."""
    rows: int
    cols: int
    past_len: int
    future_len: int
    batch_size: int
    timesteps: int
    scale: float
    sampler: str
    sigma: float
    ddim_divider: int
    guidance: str
    lambda_guidance: float
    num_res_blocks: int
    base_ch: int
    base_ch_mult: Tuple[int, ...]
    apply_attention: Tuple[bool, ...]
    dropout_rate: float
    time_emb_mult: int
    condition: str
    nsamples: int
    nsamples4plots: int
    train: Optional[AttrDict] = None
    dit: Optional["DiTKeys"] = None   # arch DDPM-DiT: the MODEL.DDPM.DIT section; arch FM-DiT: MODEL.FM.DIT
    convrnn: Optional["ConvRNNKeys"] = None   # arch ConvRNN: the MODEL.CONVRNN section


@dataclass
class DiTKeys:
    """MODEL.DDPM.DIT as models/diffusion/ddpm.py:88-104 reads it, or MODEL.FM.DIT as
    models/flow_matching/flow_matching.py:72-84 does (no T_PATCH_SIZE: t_patch_size is None)."""
    patch_size: int
    t_patch_size: Optional[int]
    hidden_size: int
    depth: int
    num_heads: int
    mlp_ratio: float
    time_emb_mult: int
    condition: str
    dropout_rate: float
    train: Optional[AttrDict]
    precision: str = "f32"   # MODEL.DDPM.DIT.PRECISION: "f32" | "f16", the sampling plan of DiT4D_V4.set_precision; MODEL.FM.DIT.PRECISION:
                             # "f32" | "f16a", that of DiT2D.set_precision (absent: "f32")


@dataclass
class ConvRNNKeys:
    """MODEL.CONVRNN as models/convRNN/convRNN.py:29-46,108-109 reads it."""
    cell_class: str
    teacher_forcing: bool
    enc_hidden: Tuple[int, ...]
    forc_hidden: Tuple[int, ...]
    enc_kernels: Tuple[int, ...]
    forc_kernels: Tuple[int, ...]
    epochs: int
    precision: str = "f32"   # MODEL.CONVRNN.PRECISION: "f32" | "f16", the forecast plan of Forecaster.set_precision (absent: "f32")


def resolve_convrnn(cfg) -> ConvRNNKeys:
    node = (cfg.get("MODEL", {}) or {}).get("CONVRNN", None)
    if not node:
        raise KeyError("MODEL.CONVRNN is missing (needed by arch ConvRNN)")

    def req(key):
        if key not in node:
            raise KeyError(f"MODEL.CONVRNN.{key} is missing (needed by arch ConvRNN)")
        return node[key]
    cell = str(req("CELL_CLASS"))
    if cell not in ("ConvGRUCell", "ConvLSTMCell"):
        raise ValueError(f"Unsupported cell class: {cell}")   # convRNN.py:31-34
    train = node.get("TRAIN", None) or {}
    precision = str(node.get("PRECISION", "f32"))
    if precision not in ("f32", "f16"):
        raise ValueError(f"MODEL.CONVRNN.PRECISION {precision!r}: 'f32' or 'f16'")
    return ConvRNNKeys(cell, bool(node.get("TEACHER_FORCING", False)), tuple(int(v) for v in req("ENC_HIDDEN_CH")),
                       tuple(int(v) for v in req("FORC_HIDDEN_CH")), tuple(int(v) for v in req("ENC_KERNELS")),
                       tuple(int(v) for v in req("FORC_KERNELS")), int(train.get("EPOCHS", 0)), precision)


def train_autocast(train) -> bool:
    """TRAIN.AUTOCAST of a resolved TRAIN node (Resolved.train: MODEL.DDPM.UNET.TRAIN or MODEL.DDPM.DIT.TRAIN): the DDPM
    training step on f16 matrix-core operands -- the UNet's Winograd layers, the DiT4D_V4 blocks' token Linears (the
    reference's torch.amp.autocast, ddpm.py:116-120).  Absent = False.  The FM drivers train in fp32 and do not read it."""
    if train is None or not hasattr(train, "get"):
        return False
    v = train.get("AUTOCAST", False)
    if not isinstance(v, (bool, int)) or v not in (0, 1, False, True):
        raise ValueError(f"TRAIN.AUTOCAST must be a bool, not {v!r}")
    return bool(v)


def _first(*vals, default=None):
    for v in vals:
        if v is not None:
            return v
    return default


def resolve(cfg, arch: str = "DDPM-UNet") -> Resolved:
    """Accept MODEL.DDPM.UNET.* (current), MODEL.DDPM.* + MODEL.* (4test) and the flat
    MODEL.* / DIFFUSION.* / TRAIN.* generation."""
    model = cfg.get("MODEL", {})
    convrnn = None
    if arch == "ConvRNN":   # no generator / backbone pair: the UNet and sampler fields below keep their defaults
        gen_key, back_key, convrnn = "CONVRNN", "", resolve_convrnn(cfg)
    else:
        gen_key, back_key = arch.upper().split("-")
    gen = model.get(gen_key, {}) or {}
    back = gen.get(back_key, {}) or {}
    diff = cfg.get("DIFFUSION", {}) or {}

    def bk(key, default=None):
        return _first(back.get(key), gen.get(key), model.get(key), default=default)

    def df(key, default=None):
        return _first(gen.get(key), diff.get(key), model.get(key), default=default)

    train = _first(back.get("TRAIN"), gen.get("TRAIN"), cfg.get("TRAIN"))
    dit = None
    if arch in ("DDPM-DiT", "FM-DiT"):
        # attribute access on the DIT node in the reference (ddpm.py:95-103, flow_matching.py:77-83): a missing key is
        # an error naming it
        def req(key):
            if key not in back:
                raise KeyError(f"MODEL.{gen_key}.{back_key}.{key} is missing (needed by arch {arch})")
            return back[key]
        if arch == "FM-DiT":
            # FM_model does not pass CONDITION on (DiT2D keeps its default "Past"): read, not required
            dit = DiTKeys(int(req("PATCH_SIZE")), None, int(req("HIDDEN_SIZE")), int(req("DEPTH")),
                          int(req("NUM_HEADS")), float(req("MLP_RATIO")), int(req("TIME_EMB_MULT")),
                          str(back.get("CONDITION", "Past")), float(back.get("DROPOUT_RATE", 0.1)), req("TRAIN"),
                          str(back.get("PRECISION", "f32")))
            if dit.precision not in ("f32", "f16a"):
                raise ValueError(f"MODEL.FM.DIT.PRECISION {dit.precision!r}: 'f32' or 'f16a'")
        else:
            dit = DiTKeys(int(req("PATCH_SIZE")), int(req("T_PATCH_SIZE")), int(req("HIDDEN_SIZE")), int(req("DEPTH")),
                          int(req("NUM_HEADS")), float(req("MLP_RATIO")), int(req("TIME_EMB_MULT")),
                          str(req("CONDITION")), float(back.get("DROPOUT_RATE", 0.1)), req("TRAIN"),
                          str(back.get("PRECISION", "f32")))
            if dit.precision not in ("f32", "f16"):
                raise ValueError(f"MODEL.DDPM.DIT.PRECISION {dit.precision!r}: 'f32' or 'f16'")
        if arch == "DDPM-DiT" and dit.condition != "Past":
            raise NotImplementedError(f"DIT.CONDITION {dit.condition!r}: only 'Past' (the configuration every reference config uses)")
    mult = tuple(int(v) for v in bk("BASE_CH_MULT", (1, 2, 4)))
    attn = tuple(bool(v) for v in bk("APPLY_ATTENTION", (False, False, True, False)))
    return Resolved(
        rows=int(cfg.MACROPROPS.ROWS), cols=int(cfg.MACROPROPS.COLS),
        past_len=int(cfg.DATASET.PAST_LEN), future_len=int(cfg.DATASET.FUTURE_LEN),
        batch_size=int(cfg.DATASET.get("BATCH_SIZE", 64)),
        timesteps=int(df("TIMESTEPS", 1000)), scale=float(df("SCALE", 0.5)),
        sampler=str(df("SAMPLER", "DDPM")), sigma=float(df("SIGMA", 0.0)),
        ddim_divider=int(df("DDIM_DIVIDER", 1)), guidance=str(df("GUIDANCE", "None")),
        lambda_guidance=float(df("LAMBDA_GUIDANCE", 0.0)),
        num_res_blocks=int(bk("NUM_RES_BLOCKS", 1)), base_ch=int(bk("BASE_CH", 32)),
        base_ch_mult=mult, apply_attention=attn, dropout_rate=float(bk("DROPOUT_RATE", 0.1)),
        time_emb_mult=int(bk("TIME_EMB_MULT", 4)), condition=str(bk("CONDITION", "Past")),
        nsamples=int(_first(model.get("NSAMPLES"), diff.get("NSAMPLES"), default=1280)),
        nsamples4plots=int(_first(model.get("NSAMPLES4PLOTS"), diff.get("NSAMPLES4PLOTS"), default=20)),
        train=train, dit=dit, convrnn=convrnn,
    )
