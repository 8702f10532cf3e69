"""Device twin of tests/test_height_field_edges_cpu.py (``-m gpu``, through the public API): the height-field terrain on an
anisotropic, off-centre grid with delta = 0.004 whose borders the states straddle (tests/height_field_cases.py) -- step,
Runge-Kutta, the rigid contact models, a fused rollout that carries environments across the borders, js.ode.system_dynamics
and js.contact.link_contact_forces, and the known answers that need no oracle -- and the first test of the ``out_mdot``
branch of ``jxs_link_contact_forces`` (a strided device copy of the rows of m out of a scratch derivative block).
"""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import height_field_cases as hfc
import helpers
from helpers import REP, to_gpu
import jaxsim_amd.api as js
import oracle
from jaxsim_amd import _lib, runtime, specialize
from jaxsim_amd.api import model as _m
from jaxsim_amd.api import ode as _ode
from jaxsim_amd.runtime import DeviceArray
from jaxsim_amd.state import StateLayout, untile_block
from oracle import VelRepr
from parity_cases import reduced_qp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DYN_KEYS = ("base_position", "base_quaternion", "joint_positions", "base_linear_velocity", "base_angular_velocity", "joint_velocities")
MDOT_N = 37  # no multiple of any tile: the last tile of the copy is ragged
# (name, enabled points or None for all, RigidContacts parameters or None for SoftContacts, precisions)
MDOT_CASES = {
    "box": ("box", None, None, (np.float64, np.float32)),
    "icub": ("icub", None, None, (np.float64, np.float32)),
    "icub_some_points": ("icub", [0, 3, 5, 8, 13, 21], None, (np.float64,)),
    "anymal4_rigid": ("anymal", helpers.ANYMAL_FEET_4, dict(), (np.float64,)),
}
MDOT_PARAMS = [(key, dt) for key, case in MDOT_CASES.items() for dt in case[3]]


def mdot_model(zoo, key):
    name, idx, rigid, _ = MDOT_CASES[key]
    model = zoo(name)
    if rigid is not None:
        return helpers.rigid_model(model, idx, **rigid)
    return model if idx is None else helpers.enable_points(model, idx)


def launches(zoo):
    """[(host model, precisions, query modes besides those of step / rollout)]: everything this module runs on the device."""
    t, _ = hfc.edge_field()
    both, f64 = (np.float64, np.float32), (np.float64,)
    out = [(helpers.with_params(zoo(name), terrain=t), both, [specialize.MODE_DYN]) for name in ("box", "icub")]
    out.append((hfc.soft_case(zoo, "box", np.float64, rk4=True)[0], f64, []))
    out += [(hfc.contact_case(zoo, kind, key)[0], f64, []) for kind, key in hfc.CONTACT_CASES]
    out.append((helpers.with_params(zoo("box"), terrain=hfc.anisotropic_plane()[1]), f64, []))
    for key, case in MDOT_CASES.items():
        m = mdot_model(zoo, key)
        out.append((m, case[3], [specialize.dyn_mode_of(m)]))
    out.append((zoo("cartpole"), f64, [specialize.MODE_DYN]))
    return out


def gpu_models(zoo):
    """Every model this module launches (the kernels of their descriptions are pre-built from tests/spec_manifest.txt)."""
    return [m for m, _, _ in launches(zoo)]


def kernel_descriptions(zoo) -> set:
    """The description of every kernel the 'specialised' pass of this module asks for (computed on the host)."""
    return {specialize.spec(m, dt, mode) for m, dts, extra in launches(zoo) for dt in dts for mode in specialize.modes_of(m) + list(extra)}


# ---- step parity on edge_field() -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", hfc.SOFT_CASES)
def test_soft_step_and_rollout_on_the_edge_field_gpu(models, name, dtype):
    model, model_ref, d = hfc.soft_case(models, name, dtype)
    _, g = hfc.edge_field()
    tol = helpers.tol_of(dtype, name)
    d64 = helpers.upcast(d, model)
    ref = oracle.step(model_ref, d64)
    out = js.model.step(model, to_gpu(model, d))
    assert out.dtype == dtype
    assert hfc.measured(f"gpu step {name} {np.dtype(dtype).name}", helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)), tol) < tol
    # three steps in one fused launch: the states move on, some collidable points to the other side of a border line
    ref3 = ref
    for _ in range(2):
        ref3 = oracle.step(model_ref, ref3)
    assert hfc.crossings(model, g, d64, ref3) >= 1
    out3 = js.model.rollout(model, to_gpu(model, d), 3)
    err3 = helpers.rel_err(out3.state_block(), helpers.odata_to_block(model, ref3))
    assert hfc.measured(f"gpu rollout3 {name} {np.dtype(dtype).name}", err3, 10 * tol) < 10 * tol


def test_rk4_box_on_the_edge_field_gpu(models):
    model, model_ref, d = hfc.soft_case(models, "box", np.float64, rk4=True)
    _, g = hfc.edge_field()
    ref = oracle.step(model_ref, d)
    assert hfc.crossings(model, g, d, ref) >= 6
    out = js.model.step(model, to_gpu(model, d))
    err = helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref))
    assert hfc.measured("gpu rk4 step box float64", err, helpers.FP64_TOL) < helpers.FP64_TOL


@pytest.mark.parametrize("kind,key", list(hfc.CONTACT_CASES))
def test_rigid_models_on_the_edge_field_gpu(models, reduced_qp, kind, key):
    model, model_ref, d = hfc.contact_case(models, kind, key)
    ref = oracle.step(model_ref, d)
    out = js.model.step(model, to_gpu(model, d))
    tol = 1e-7 if kind == "rigid" else 1e-9
    err = helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref))
    assert hfc.measured(f"gpu {kind} step {key} float64", err, tol) < tol


@pytest.mark.parametrize("name", ["box", "icub"])
def test_system_dynamics_and_link_contact_forces_on_the_edge_field_gpu(models, name):
    """The existing device tests of these two functions run on flat terrain only."""
    model, model_ref, d = hfc.soft_case(models, name, np.float64)
    d = dataclasses.replace(d, velocity_representation=VelRepr.Inertial)
    g = to_gpu(model, d)
    ref = oracle.refstep.system_dynamics(model_ref, d)
    got = js.ode.system_dynamics(model, g)
    worst = max(helpers.rel_err(got[key], ref[key]) for key in DYN_KEYS)
    worst = max(worst, helpers.rel_err(got["contact_state"]["tangential_deformation"], ref["tangential_deformation"]))
    assert hfc.measured(f"gpu system_dynamics {name} float64", worst, 1e-10) < 1e-10
    ref_W, ref_md = oracle.refstep.link_contact_forces(model_ref, d)
    W, aux = js.contact.link_contact_forces(model, g)
    assert hfc.measured(f"gpu link_contact_forces {name} float64", helpers.rel_err(W, ref_W), 1e-10) < 1e-10
    assert helpers.rel_err(aux["m_dot"], ref_md) < 1e-10
    assert np.abs(ref_W[..., :2]).max() > 0.1  # tilted normals: horizontal contact forces


# ---- known answers without the oracle ----------------------------------------------------------------------------------------
def test_anisotropic_plane_equals_plane_terrain_gpu(models):
    hf, plane = hfc.anisotropic_plane()
    box = models("box")
    d = models.random_data("box", 33, seed=3)
    o1 = js.model.step(helpers.with_params(box, terrain=hf), to_gpu(box, d)).state_block()
    o2 = js.model.step(helpers.with_params(box, terrain=plane), to_gpu(box, d)).state_block()
    assert hfc.measured("gpu anisotropic plane", helpers.rel_err(o1, o2), 1e-11) < 1e-11


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_outside_the_grid_the_border_extends_gpu(models, dtype):
    """Two launches of the same kernel on two grids (the second repeats the border row out to the boxes): bit for bit."""
    t, ext, d = hfc.outside_state(models, dtype, N=33)
    box = models("box")
    o1 = js.model.step(helpers.with_params(box, terrain=t), to_gpu(box, d)).state_block()
    o2 = js.model.step(helpers.with_params(box, terrain=ext), to_gpu(box, d)).state_block()
    assert o1.dtype == dtype and np.array_equal(o1, o2)
    flat = js.model.step(box, to_gpu(box, d)).state_block()
    assert helpers.rel_err(flat, o1) > 1e-5  # the terrain acts on these boxes


def test_the_last_sample_belongs_to_the_last_cell_gpu(models):
    t, ext = hfc.last_cell_fields()
    d = hfc.last_cell_state(models)
    box = models("box")
    o1 = js.model.step(helpers.with_params(box, terrain=t), to_gpu(box, d)).state_block()
    o2 = js.model.step(helpers.with_params(box, terrain=ext), to_gpu(box, d)).state_block()
    assert hfc.measured("gpu last cell", helpers.rel_err(o1, o2), 1e-12) < 1e-12


# ---- out_mdot of jxs_link_contact_forces -------------------------------------------------------------------------------------
GUARD_BITS = {4: np.uint32(0x7FC0BEEF), 8: np.uint64(0x7FF8DEADBEEF0123)}  # quiet NaNs with a payload


def _pattern(rows, cols, dtype):
    bits = GUARD_BITS[np.dtype(dtype).itemsize]
    return np.full((rows, cols), bits, dtype=bits.dtype).view(dtype)


def _bits(a):
    return np.ascontiguousarray(a).view(GUARD_BITS[a.dtype.itemsize].dtype)


def _raw_link_contact_forces(model, g, tau, f, rep, mdot_rows, with_mdot=True):
    """``jxs_link_contact_forces`` through ``_lib``: (wrenches [nL * 6, N], rows of m [mdot_rows, N], guard tile as stored,
    the pattern it was filled with).  The m_dot buffer is sized in whole tiles and followed by one more tile of a
    recognisable bit pattern; all of it is filled with that pattern before the call."""
    st = g._state
    dtype, N, tile = st.dtype, st.cols, st.tile
    dm = _m._device_model_fast(model, dtype)
    specialize.ensure_mode(dm, model, specialize.dyn_mode_of(model))
    nL, n = model.number_of_links(), model.dofs()
    f_d = _m._as_device(f, nL * 6, N, dtype, (nL, 6), tile)
    tau_d = _m._as_device(tau, n, N, dtype, (n,), tile)
    W = DeviceArray(nL * 6, N, dtype, tile=tile)
    nt = st.n_tiles
    rows = max(mdot_rows, 1)
    fill = _pattern(rows, (nt + 1) * tile, dtype)
    buf = DeviceArray.from_host(fill, tile=tile)
    _lib.check(
        _lib.load().jxs_link_contact_forces(dm.handle, C.c_void_p(st.ptr), _m._ptr(tau_d), _m._ptr(f_d), int(REP[rep]), _m._ptr(W),
                                            _m._ptr(buf) if with_mdot else None, N, runtime._sp()),
        "jxs_link_contact_forces",
    )  # fmt: skip
    runtime.synchronize()
    raw = buf.to_host_raw()  # [nt + 1, rows, tile]
    md = untile_block(raw[:nt].reshape(-1), rows, N, tile)
    return W.to_host(), md, raw[nt], fill[:, :tile]


@pytest.mark.parametrize("key,dtype", MDOT_PARAMS)
def test_link_contact_forces_out_mdot_gpu(models, key, dtype):
    model = mdot_model(models, key)
    name = MDOT_CASES[key][0]
    N = MDOT_N
    d = models.random_data(name, N, seed=4, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 15, dtype)
    lay = StateLayout.of(model)
    mrows = 3 * lay.n_points
    g = to_gpu(model, d)
    assert N % g._state.tile != 0
    W, md, guard, pattern = _raw_link_contact_forces(model, g, tau, f, d.velocity_representation, mrows)
    # 1. the rows of m of the derivative block jxs_system_dynamics writes for the same inputs: same kernel, a pure copy
    xdot, W_dyn = _ode.system_dynamics_device(model, g, link_forces=f, joint_torques=tau, force_repr=REP[d.velocity_representation],
                                              want_derivative=True, want_link_contact_forces=True)  # fmt: skip
    xdot = xdot.to_host()
    assert xdot.shape[0] == lay.row_m + mrows
    assert np.array_equal(_bits(md), _bits(xdot[lay.row_m :]))
    assert np.array_equal(_bits(W), _bits(W_dyn.to_host()))
    # 2. the oracle's rate of the tangential deformation (zero for disabled points and for the rigid contact models)
    d64 = helpers.upcast(d, model)
    ref_md = np.zeros((N, lay.n_points, 3)) if MDOT_CASES[key][2] is not None else oracle.refstep.link_contact_forces(model, d64)[1]
    if dtype == np.float64:
        err = helpers.rel_err(md, ref_md.reshape(N, -1).T)
        assert hfc.measured(f"gpu out_mdot {key} float64", err, 1e-10) < 1e-10
    if MDOT_CASES[key][2] is None:
        assert np.abs(ref_md).max() > 1e-3  # contacts really act: the rows are not all zero
        en = np.asarray(model.kin_dyn_parameters.contact_enabled, dtype=bool)
        assert (md.T.reshape(N, -1, 3)[:, ~en] == 0).all()
    # 3. the link wrenches of the same call equal those of a call without out_mdot
    W0, untouched, _, pattern0 = _raw_link_contact_forces(model, g, tau, f, d.velocity_representation, mrows, with_mdot=False)
    assert np.array_equal(_bits(W), _bits(W0))
    assert (_bits(untouched) == _bits(pattern0)[0, 0]).all()
    # 4. the tile behind the buffer keeps its bit pattern
    assert np.array_equal(_bits(guard), _bits(pattern))


def test_link_contact_forces_out_mdot_without_points_gpu(models):
    """n_points == 0 (cartpole): the call succeeds, writes zero wrenches and leaves the m_dot buffer untouched."""
    model = models("cartpole")
    assert StateLayout.of(model).n_points == 0
    d = models.random_data("cartpole", MDOT_N, seed=4)
    g = to_gpu(model, d)
    W, md, guard, pattern = _raw_link_contact_forces(model, g, None, None, d.velocity_representation, 0)
    assert (W == 0).all()
    assert (_bits(md) == _bits(pattern)[0, 0]).all() and np.array_equal(_bits(guard), _bits(pattern))
