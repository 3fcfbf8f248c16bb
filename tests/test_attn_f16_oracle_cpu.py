"""tests/attn_f16_oracle.py held on the CPU: the block walk in float64 IS the plain softmax; a numpy emulation of
attn_core_f16_kernel's arithmetic (key blocks of 32, fp32 softmax, probabilities rounded to f16) stays inside EMU_FRACTION of the
derived allowance; and each wrong variant -- as an emulation against the oracle, and as a float64 oracle against the correct
emulation -- lands outside it on data at the operating point, wherever the variant differs from the kernel at all (applicable)."""
import numpy as np
import pytest

import attn_f16_oracle as ao

HEADS, B = 4, 2
SIZES = (1, 31, 32, 33, 64, 65, 216, 640)


@pytest.mark.parametrize("S", SIZES)
def test_emulation_inside_and_wrong_variants_outside_the_allowance(S):
    for kind in ao.KINDS:
        qkv = ao.sources(kind, B, S, HEADS)
        qs, k, v = ao.round_operands(qkv, HEADS)
        ref, R, floor, A = ao.attn_ref(qs, k, v)
        allow = ao.allowance(R, floor, A, S)
        assert ref.shape == (B, S, HEADS * ao.D) and (allow > 0).all()
        walk = ao.attn_online(qs, k, v, emulate=False)
        assert float(np.abs(walk - ref).max()) <= 1e-13 * max(1.0, float(np.abs(ref).max()))
        emu = ao.attn_online(qs, k, v, emulate=True)
        frac = ao.use(emu, ref, allow)
        print(f"S {S} {kind}: emulation uses {frac:.3f} of the allowance (A = {A:.0f})")
        assert frac <= ao.EMU_FRACTION, (S, kind, frac)
        for var in ao.VARIANTS:
            if not ao.applicable(var, S):
                continue
            miss_emu = ao.use(ao.attn_online(qs, k, v, True, var), ref, allow)
            miss_ref = ao.use(emu, ao.attn_online(qs, k, v, False, var), allow)
            print(f"S {S} {kind} {var}: wrong emulation {miss_emu:.2f} x, wrong oracle {miss_ref:.2f} x the allowance")
            if kind == "unit":
                assert miss_emu > 2.0 and miss_ref > 2.0, (S, var, miss_emu, miss_ref)
    if S > 32:      # spread scores and a dominant key are where a dropped correction is a factor, not a fraction
        for kind in ("spread", "dominant") if S > 33 else ("spread",):
            qs, k, v = ao.round_operands(ao.sources(kind, B, S, HEADS), HEADS)
            ref, R, floor, A = ao.attn_ref(qs, k, v)
            assert ao.use(ao.attn_online(qs, k, v, True, "no_corr"), ref, ao.allowance(R, floor, A, S)) > 100.0


def test_every_variant_is_applicable_somewhere_and_the_predicate_is_right():
    for var in ao.VARIANTS:
        assert any(ao.applicable(var, S) for S in SIZES)
    for S in SIZES:
        qs, k, v = ao.round_operands(ao.sources("unit", 1, S, HEADS), HEADS)
        good = ao.attn_online(qs, k, v, False)
        for var in ao.VARIANTS:
            if var == "last_key" and S == 1:
                continue                                    # (no key left at all: not a wrong answer, no answer)
            same = np.array_equal(ao.attn_online(qs, k, v, False, var), good)
            assert same != ao.applicable(var, S), (var, S)


def test_round_operands_rounds_as_the_kernel_and_refuses_boundary_data():
    qkv = ao.sources("unit", 1, 5, HEADS)
    qs, k, v = ao.round_operands(qkv, HEADS)
    q32, k32, v32 = ao.split_heads(qkv, HEADS)
    assert np.array_equal(k, k32.astype(np.float16).astype(np.float64)) and np.array_equal(v, v32.astype(np.float16).astype(np.float64))
    scale = np.float32(1.0) / np.sqrt(np.float32(32))
    assert np.array_equal(qs, (q32 * scale).astype(np.float16).astype(np.float64))
    bad = qkv.copy()
    bad[0, 0, 0] = np.float32((1.0 + 2.0 ** -11) / np.float64(scale))       # q * scale = the midpoint of two f16 values
    with pytest.raises(AssertionError):
        ao.round_operands(bad, HEADS)
