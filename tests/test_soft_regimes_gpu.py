"""Device twin of tests/test_soft_regimes_cpu.py (``-m gpu``, through the public API): the Hunt-Crossley law regime by
regime -- stick, slip, lift-off, rest, airborne, asserted on the inputs (tests/soft_regime_cases.py) -- through
js.ode.system_dynamics / system_acceleration, js.contact.link_contact_forces (wrenches and ``aux["m_dot"]``) and
js.model.step, with m_dot and the wrenches measured on their own scale.  The first device runs of general contact
exponents (``vpow``) and of mu = 0, of contact on the chunks behind the first lane group and of a fixed base in soft contact.
"""

import dataclasses

import numpy as np
import pytest

import helpers
from helpers import to_gpu
import jaxsim_amd.api as js
import oracle
import soft_regime_cases as src
from jaxsim_amd import specialize

pytestmark = pytest.mark.gpu

DYN_KEYS = ("base_position", "base_quaternion", "joint_positions", "base_linear_velocity", "base_angular_velocity", "joint_velocities")


def launches(zoo):
    """[(host model, precision, query modes besides those of step / rollout)]: everything this module runs on the device."""
    out = [(src.case_models(zoo, c)[0], c.dtype, [] if c.rk4 else [specialize.MODE_DYN]) for c in src.CASES + src.REP_CASES]
    out += [(src.grazing_case(zoo, dt)[0], dt, [specialize.MODE_DYN]) for dt in (np.float64, np.float32)]
    return out


def gpu_models(zoo):
    """Every model this module launches (the kernels of their descriptions are pre-built from tests/spec_manifest.txt)."""
    return [m for m, _, _ in launches(zoo)]


def kernel_descriptions(zoo) -> set:
    """The description of every kernel the 'specialised' pass of this module asks for (computed on the host)."""
    return {specialize.spec(m, dt, mode) for m, dt, extra in launches(zoo) for mode in specialize.modes_of(m) + list(extra)}


def _device_answers(cd):
    """(derivative block [rows, N], m_dot of link_contact_forces, link wrenches, stepped state block) of the device."""
    model, d = cd["model"], cd["d"]
    g = to_gpu(model, d)
    got = js.ode.system_dynamics(model, g)
    assert np.asarray(got["joint_velocities"]).dtype == d.dtype
    xd = {k: np.asarray(got[k]) for k in DYN_KEYS}
    xd["tangential_deformation"] = np.asarray(got["contact_state"]["tangential_deformation"])
    W, aux = js.contact.link_contact_forces(model, g)
    step = js.model.step(model, g).state_block()
    return g, src.derivative_block(model, xd), np.asarray(aux["m_dot"]), np.asarray(W), step


@pytest.mark.parametrize("key", src.EULER_KEYS + src.REP_KEYS)
def test_dynamics_forces_and_step_per_regime_gpu(models, key):
    cd = src.case_data(models, key)
    model, case = cd["model"], cd["case"]
    g, xdot, m_dot, W, step = _device_answers(cd)
    src.check(models, cd, "gpu", block=xdot, m_dot=m_dot, W=W, step=step)
    src.assert_rest(cd, m_dot)
    rows = src.m_rows(model, xdot)
    if case.dtype == np.float64:
        # aux["m_dot"] is a copy of the rows of m of the derivative block, and the step applies that rate
        assert np.array_equal(m_dot.view(np.uint64), rows.view(np.uint64))
        np.testing.assert_allclose(src.m_rows(model, step), cd["d"].tangential_deformation + model.time_step * rows, rtol=0, atol=1e-12)
    else:
        src.check(models, cd, "gpu dyn rows", m_dot=rows)
    # system_acceleration answers in the data's representation (oracle.refstep.system_acceleration_active)
    vd, sdd, md = oracle.refstep.system_acceleration_active(cd["model_ref"], cd["d64"])
    gvd, gsdd, gcs = js.ode.system_acceleration(model, g)
    err = helpers.rel_err(np.concatenate([np.asarray(gvd), np.asarray(gsdd)], -1), np.concatenate([vd, sdd], -1))
    assert src.measured(f"gpu system_acceleration {key}", err, src.gate(models, case, "block")) < src.gate(models, case, "block")
    own = src.own_scale(gcs["tangential_deformation"], md, cd["vs"])
    assert src.measured(f"gpu system_acceleration m_dot {key}", own, src.gate(models, case, "m_dot")) < src.gate(models, case, "m_dot")


@pytest.mark.parametrize("key", src.RK4_KEYS)
def test_rk4_step_per_regime_gpu(models, key):
    cd = src.case_data(models, key)
    step = js.model.step(cd["model"], to_gpu(cd["model"], cd["d"])).state_block()
    src.check(models, cd, "gpu", step=step)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_point_exactly_on_the_ground_gpu(models, dtype):
    model, d, expected, touching = src.grazing_case(models, dtype)
    W, aux = js.contact.link_contact_forces(model, to_gpu(model, d))
    src.check_grazing(model, d, expected, touching, np.asarray(aux["m_dot"]), np.asarray(W), dtype)
