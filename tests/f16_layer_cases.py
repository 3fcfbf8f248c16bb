"""Rows of tests/test_gpu_f16_layers.py and tests/test_conv_oracle_cpu.py: the smallest shapes that reach each branch of the UNet's
reduced-precision inference plan (set_precision("f16"); csrc/cm_model.cpp: add_conv, conv_route, plan_h16).  Data only.  A table of
its own: tests/train_limit_cases.py's fixture depends on that file's rows.

What a row does not name is C = 3, base 32, multiples (1, 2, 4), attention at the lowest level, one res block, 5 + 3 frames.
Which branch each row is there for (the routes are asserted from the info lines, not assumed):

  atc            12 x 36: conv_f16d_pick takes the 4 x 6 x 9 tile at full AND half resolution -- 216 rows, no multiple of 32 (24
                 padding rows in the last of 2 x 4 row blocks), mbw 2, with NB 1 (32 channels) and NB 2 (64); half resolution has Z = 4;
                 a decoder conv_1 with two f16 sources (mask 7); fused skip convs over two sources (masks 21 and 53); residual
                 read as f16 (mask 9); both stage-once upsample convs in form F16 (masks 4 and 5); the last conv's f16 form
                 reading an f16 source; the first conv writing one; conv1x1_f16_kernel (the attention in-projection)
  g12x12         12 x 12, B = 3: the 8 x 4 x 4 tile, 128 rows: mbw 1 with NB 1
  base64_12x12   the same grid at base 64, multiples (1, 1, 2), B = 1: mbw 1 with NB 2 (with base 32 the one-row-block tile needs a
                 20 x 32 grid to appear at half resolution); last conv on conv_smalln (64 input channels: off conv_fin)
  frames4_12x36  3 + 1 frames: half resolution has Z = 2, below add_conv's s.out->Z >= 4 for the direct kernel: the Winograd
                 kernel's FORM_F16 on its two-plane tile (sources and output stay fp32 there: plan_h16)
  frames4        8 x 12, 3 + 1 frames: no Winograd tile fits 4 x 8 x 12, so the direct kernel takes no layer and no tensor is stored
                 as f16: the full-resolution skip convs (32 outputs) can run alone, on conv1x1_f16_kernel<1> (<2>: every wider one)
  res2           8 x 12, two res blocks: blocks with equal widths -- a residual without a skip conv, read as f16 (mask 13)
  ch5            8 x 12, C = 5, B = 3: the last conv off conv_fin (Co > 4): conv_smalln reading an f16 source (mask 1)
  cr90           12 x 20, B = 1: the 8 x 6 x 5 / 4 x 6 x 10 tiles, 240 rows (16 padding rows)"""
import collections

Case = collections.namedtuple("Case", "rows cols past future channels base multiples attention res_blocks dropout B")


def _case(rows=8, cols=12, past=5, future=3, channels=3, base=32, multiples=(1, 2, 4), res_blocks=1, B=2):
    return Case(rows, cols, past, future, channels, base, tuple(multiples), (False,) * (len(multiples) - 1) + (True,), res_blocks, 0.1, B)


CASES = {
    "atc": _case(12, 36, B=2),
    "g12x12": _case(12, 12, B=3),
    "base64_12x12": _case(12, 12, base=64, multiples=(1, 1, 2), B=1),
    "frames4_12x36": _case(12, 36, past=3, future=1, B=2),
    "frames4": _case(8, 12, past=3, future=1, B=2),
    "res2": _case(8, 12, res_blocks=2, B=2),
    "ch5": _case(8, 12, channels=5, B=3),
    "cr90": _case(12, 20, B=1),
}
REAL_CASES = ("atc", "base64_12x12", "ch5")


def cfg_of(key):
    from crowdmod_ddpm_4d_amd import spec
    c = CASES[key]
    return spec.UNetConfig(c.channels, c.channels, c.res_blocks, c.base, c.multiples, c.attention + (False,), c.dropout, 4, "Past")
