"""The Hunt-Crossley law of ``point_physics`` regime by regime, in the host emulation of the kernel core (tests/emul).

Every other parity test feeds the law random heights and ``m ~ 1e-3 N(0, 1)`` and asserts nothing about the branches those
states reach: of the 2240 humanoid points of test_system_dynamics_matches_oracle_gpu one slips, none is clamped at lift-off,
none rests, none is shallower than 1e-5 m; general exponents (``vpow``) and mu = 0 never run on the device; and the fp32
metric of the derivative block divides an m_dot row of 0.1 .. 1 m/s by an acceleration of 1e2 .. 1e4.  The cases here
(tests/soft_regime_cases.py) aim every environment at one regime -- stick, slip, lift-off, rest, airborne -- on flat
ground, a tilted plane and the edge height field, with default and general exponents, without friction, on the chunks
behind the first lane group (80 points), through Runge-Kutta stages and on a fixed base; the regimes are asserted on the
inputs with an fp64 classifier that is itself checked against the oracle; and m_dot and the wrenches are measured on
their own scale (``src.own_scale``).  Device twin: tests/test_soft_regimes_gpu.py.

Each of these edits of a scratch copy of jaxsim_amd/csrc/jxs_core.h makes this module fail (the emulation built from the
copy; in brackets whether tests/test_emulation_parity.py failed on it too; profiles/soft_regimes.txt names the cases):
1. ``md_sl`` without ``Kdp * mt[k]``, in the flat branch (16 tests fail here) and in the general branch (36) [both: yes];
2. ``md_st = vt[k]`` without ``- P.K_over_D * mn[k]`` (32) [yes];  3. ``fn`` without ``vmax(zero, .)`` (52) [yes];
4. ``P.p`` <-> ``P.q`` in the ``vpow`` lines (17) [yes];  6. ``in_contact = delta >= zero`` (54, row H among them) [yes];
7. the ``!P.floating`` velocity term without ``vBc`` (4: the fixed-base cases) [NO: only this module sees it];
8. ``contact_chunk``: the deformation of chunks behind the first read as zero (4: the 80-point humanoid) [yes].
5. ``sticking`` without ``no_contact ||`` does NOT fail, and cannot: every reader of ``sticking`` selects on ``no_contact``
first, and the emulation built with the edit returns bit for bit the unedited answers on all 52 cases.
"""

import pathlib

import numpy as np
import pytest

import emul_binding as eb
import helpers
import oracle
import soft_regime_cases as src


def _block(cd):
    return helpers.odata_to_block(cd["model"], cd["d"])


@pytest.mark.parametrize("key", list(src.BY_KEY))
def test_case_reaches_every_regime(models, key):
    """The input conditions of the case (``src.require``, asserted inside ``case_data``), and the recipe's aim: an environment
    that aims at a regime has its deepest point in it."""
    cd = src.case_data(models, key)
    R, case = cd["R"], cd["case"]
    print(f"[soft regimes] counts {key}: {src.counts(R)}")
    deepest = np.argmax(R["h"], axis=1)
    env = np.arange(case.N)
    for r, name in enumerate(src.REGIMES):
        if case.mu0 and name in ("stick", "slip"):
            continue
        if case.pq and case.pq[0] != case.pq[1] and name == "liftoff":
            continue  # (with p != q the damping of a shallow point outweighs 3 v_eq; the count condition holds all the same)
        sel = env[env % 5 == r]
        assert R[name][sel, deepest[sel]].all(), (key, name)


@pytest.mark.parametrize("key", [c.key for c in src.CASES if np.dtype(c.dtype) == np.float64])
def test_classifier_restates_the_oracle(models, key):
    """Forces and rates rebuilt from the classifier's quantities equal the oracle's law to 1e-13 (relative to
    max(1, |.|)): the classifier cannot drift away from the oracle."""
    cd = src.case_data(models, key)
    R, cp = cd["R"], cd["model_ref"].contact_params
    f, md = oracle.refstep.hunt_crossley_contact_model(cd["model_ref"], R["position"], R["velocity"], R["m"], K=cp.K, D=cp.D, mu=cp.mu, p=cp.p, q=cp.q)
    assert helpers.rel_err(R["force"], f) < 1e-13 and helpers.rel_err(R["m_dot"], md) < 1e-13
    assert src.own_scale(R["m_dot"], md, cd["vs"]) < 1e-13
    idx = cd["model_ref"].kin_dyn_parameters.indices_of_enabled_collidable_points
    assert np.array_equal(md, cd["truth"]["m_dot"][:, idx])


@pytest.mark.parametrize("key", src.EULER_KEYS)
def test_dynamics_and_step_per_regime(models, key):
    cd = src.case_data(models, key)
    model, case = cd["model"], cd["case"]
    N = case.N
    xdot, W = eb.run(model, eb.MODE_DYN, _block(cd))
    assert xdot.dtype == case.dtype
    m_dot = src.m_rows(model, xdot)
    step = eb.run(model, eb.MODE_STEP, _block(cd))
    src.check(models, cd, "emul", block=xdot, m_dot=m_dot, W=W.T.reshape(N, -1, 6), step=step)
    src.assert_rest(cd, m_dot)
    assert np.abs(cd["truth"]["W"]).max() > 1.0  # contacts really act


@pytest.mark.parametrize("key", src.RK4_KEYS)
def test_rk4_step_per_regime(models, key):
    cd = src.case_data(models, key)
    step = eb.run(cd["model"], eb.MODE_STEP, _block(cd))
    src.check(models, cd, "emul", step=step)
    euler = oracle.step(helpers.with_params(cd["model_ref"], integrator=0), cd["d64"])
    assert helpers.rel_err(helpers.odata_to_block(cd["model"], euler), cd["truth"]["step"]) > 1e-7  # and it is not the Euler answer


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_point_exactly_on_the_ground(models, dtype):
    """Row H: h == 0 and h one ulp above the ground give no force and relax the spring, m_dot = -(K / D) m; h one ulp inside
    sticks (``in_contact = delta > 0``, not >=)."""
    model, d, expected, touching = src.grazing_case(models, dtype)
    xdot, W = eb.run(model, eb.MODE_DYN, helpers.odata_to_block(model, d))
    src.check_grazing(model, d, expected, touching, src.m_rows(model, xdot), W.T.reshape(4, -1, 6), dtype)


def test_float32_reference_errors_pin_the_states(models):
    """The float32 gates: three times the error of the reference formulation in float32 on these states (never the
    kernel's); on its own scale that error stays below 1e-2 (asserted in ``src.fp32_reference_errors``)."""
    for family in ("box", "anymal", "icub", "fixedcart"):
        ref = src.fp32_reference_errors(models, family)
        assert len(ref["cases"]) >= 2
        for q in src.QUANTITIES:
            src.measured(f"fp32 oracle {q} {family}", ref[q], 3 * ref[q])
            assert 0 < ref[q] < 1e-2


# ---- the kernel descriptions of the device twin ----------------------------------------------------------------------------
def test_every_kernel_of_the_gpu_module_is_in_the_manifest(models):
    """The 'specialised' pass of the GPU suite needs a pre-built object per (model, precision, mode) description; the build
    takes them from tests/spec_manifest.txt.  A missing line is found here, not on the GPU machine."""
    import test_soft_regimes_gpu as gpu_module

    manifest = {ln.strip() for ln in (pathlib.Path(__file__).parent / "spec_manifest.txt").read_text().splitlines() if ln.strip()}
    wanted = gpu_module.kernel_descriptions(models)
    assert len(wanted) >= 40
    missing = sorted(wanted - manifest)
    assert not missing, missing
