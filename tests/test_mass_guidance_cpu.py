"""mass_preservation guidance without a GPU: the fp64 closed form of tests/mass_oracle.py against the reference's own
finite-difference gradient (tests/golden/mass_guidance.npz, grad/*), and the host-side plumbing of the feature."""
import numpy as np
import pytest

from helpers import load
from mass_oracle import GRAD_SHAPES, energy, grad_cases, grad_input, mass_grad, ref_tolerance, touched_mask

CASES = grad_cases()


@pytest.mark.parametrize("key,name,scale,p", CASES, ids=[c[0] for c in CASES])
def test_closed_form_matches_the_reference_quotient(key, name, scale, p):
    q_ref = load("mass_guidance.npz")[f"grad/{key}/q"]
    x = grad_input(name, scale)
    assert q_ref.shape == x.shape == GRAD_SHAPES[name]
    q = mass_grad(x, *p)
    assert np.all(np.abs(q - q_ref) <= ref_tolerance(x, q_ref, *p)), float(np.abs(q - q_ref).max())
    # the reference's quotient is exactly 0 where no residual cell reaches (channels >= 3 included)
    assert np.all(q_ref[~touched_mask(x.shape)] == 0) and np.all(q[~touched_mask(x.shape)] == 0)
    if name.startswith("degenerate"):
        assert not q_ref.any() and not q.any()


# The eps g^2 term is what separates the reference's quotient from the analytic gradient.  At the function's defaults
# (eps = 0.01) on unit-scale inputs it is 0.2-0.4 % of max |q|, inside the reference's own fp32 noise there; every other
# case shows it above 1 %.
EPS_CASES = [c for c in CASES if not c[1].startswith("degenerate") and not (c[0].endswith("_default") and c[2] == 1.0)]


@pytest.mark.parametrize("key,name,scale,p", EPS_CASES, ids=[c[0] for c in EPS_CASES])
def test_analytic_gradient_misses_the_reference(key, name, scale, p):
    q_ref = load("mass_guidance.npz")[f"grad/{key}/q"]
    dt, dl, _ = p
    q0 = mass_grad(grad_input(name, scale), dt, dl, 0.0)
    assert np.abs(q0 - q_ref).max() > 1e-2 * np.abs(q_ref).max()


def test_energy_restatement_matches_the_metric_one():
    """mass_oracle.energy is the same compute_energy as the package's (checked against energy.npz elsewhere)."""
    from crowdmod_ddpm_4d_amd import metrics
    x = grad_input("atc_c4", 1.0)
    for dt, dl in ((1.0, 1.0), (0.5, 1.0)):
        np.testing.assert_allclose(energy(x, dt, dl), np.asarray(metrics.compute_energy(x, dt, dl), np.float64), rtol=1e-5)


def test_loop_fixture_sees_the_guidance():
    """The guided 20-step loop moves x_0 by far more than the 1e-4 loop tolerance: a parity test against it sees the
    feature."""
    g = load("mass_guidance.npz")
    assert np.abs(g["loop/ddpm20_mass/x0"] - g["loop/ddpm20_none/x0"]).max() > 1e-3
    for key in ("ddpm20_mass", "ddpm20_none", "cr120_ddpm20_mass"):
        assert np.isfinite(g[f"loop/{key}/x0"]).all()
        assert np.array_equal(g[f"loop/{key}/x_after_t0"], g[f"loop/{key}/x0"])


def test_sample_opts_map_mass_preservation():
    """DDPM_model._opts maps GUIDANCE 'mass_preservation' (case-sensitive, like 'Sparsity') onto the C enum; the ABI
    declares the constant and the stand-alone gradient entry point."""
    import os
    import re
    from crowdmod_ddpm_4d_amd import native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crowdmod_hip.h")).read()
    assert re.search(r"CM_GUIDANCE_MASS_PRESERVATION\s*=\s*2", hdr)
    assert native.GUIDANCE_MASS_PRESERVATION == 2
    assert "cm_mass_preservation_grad" in native.SIGNATURES and "int cm_mass_preservation_grad(" in hdr

    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model

    class _Res:
        guidance, lambda_guidance, sigma = "mass_preservation", 0.0, 0.0

    m = DDPM_model.__new__(DDPM_model)
    m.res, m.seed = _Res(), 1
    assert m._opts(native.SAMPLER_DDPM).guidance == native.GUIDANCE_MASS_PRESERVATION
    _Res.guidance = "Mass_Preservation"
    assert m._opts(native.SAMPLER_DDPM).guidance == native.GUIDANCE_NONE
