"""Height-field terrain off the square grid, in the host emulation of the kernel core (tests/emul).

Every other height-field test samples a square, centred grid with the default delta that no point leaves; a transposed
row stride, exchanged spacings or origin coordinates, a wrong clamp, a last sample that belongs to no cell, a delta other
than 0.01 or a wrong rule outside the grid all pass them.  The cases here (tests/height_field_cases.py) run on an
18 x 12 grid with spacing (0.07, 0.11), origin (-0.55, -0.70) and delta 0.004 whose borders the random states straddle --
asserted on the inputs -- against the oracle on ``oracle.refterrain.GridTerrain`` of the same samples, and against three
known answers that need no oracle.  Device twin: tests/test_height_field_edges_gpu.py.

Each of these edits of a scratch copy of the kernel sources makes this module fail (the emulation built from the copy):
``ix * P.hf_ny`` -> ``ix * P.hf_nx``; ``hf_idx`` <-> ``hf_idy`` and ``hf_x0`` <-> ``hf_y0`` in jxs_pack.h; the cell clamp
``hf_nx - 2`` applied to ``fx`` instead of the index; ``hf_inv_2delta`` fixed at 50 (profiles/height_field_edges.txt).
"""

import dataclasses

import numpy as np
import pytest

import emul_binding as eb
import height_field_cases as hfc
import helpers
import oracle
from oracle import VelRepr
from parity_cases import RELAXED_CASES, RIGID_CASES, dyn_err, dyn_reference, reduced_qp  # noqa: F401


def _block(model, d):
    return helpers.odata_to_block(model, d)


def test_edge_field_is_the_stated_grid():
    """18 x 12 samples, last sample lines at x = 0.64 and y = 0.51, delta 0.004; the product's host class and the oracle's
    restatement agree on it inside, on and beyond every border (the sine-field twin of this check is square and centred)."""
    t, g = hfc.edge_field()
    assert t._heights.shape == (18, 12) and t._spacing == (0.07, 0.11) and t._origin == (-0.55, -0.70) and t.delta == 0.004
    np.testing.assert_allclose(hfc.bounds(g), (-0.55, 0.64, -0.70, 0.51), rtol=0, atol=1e-15)
    rng = np.random.default_rng(0)
    x, y = rng.uniform(-1.2, 1.2, 4000), rng.uniform(-1.2, 1.2, 4000)
    x[:200], y[200:400] = 0.64, 0.51  # on the last sample lines
    np.testing.assert_allclose(t.height(x, y), g.height(x, y), rtol=0, atol=1e-15)
    np.testing.assert_allclose(t.normal(x, y), g.normal(x, y), rtol=0, atol=1e-13)
    X, Y = np.meshgrid(-0.55 + 0.07 * np.arange(18), -0.70 + 0.11 * np.arange(12), indexing="ij")
    np.testing.assert_allclose(t.height(X, Y), hfc.edge_fn(X, Y), rtol=0, atol=1e-15)  # x is the outer axis of the samples


def test_contact_cases_are_those_of_the_parity_suite():
    for (kind, key), case in hfc.CONTACT_CASES.items():
        assert case == (RIGID_CASES if kind == "rigid" else RELAXED_CASES)[key]


@pytest.mark.parametrize("name,dtype", hfc.SOFT_CASES)
def test_soft_step_and_dynamics_on_the_edge_field(models, name, dtype):
    model, model_ref, d = hfc.soft_case(models, name, dtype)
    tol = helpers.tol_of(dtype, name)
    ref = oracle.step(model_ref, helpers.upcast(d, model))
    out = eb.run(model, eb.MODE_STEP, _block(model, d))
    assert out.dtype == dtype
    assert hfc.measured(f"emul step {name} {np.dtype(dtype).name}", helpers.rel_err(out, _block(model, ref)), tol) < tol
    # the derivative and the link wrenches of system_dynamics see the same grid (gate rule of test_height_field_terrain_soft)
    d_in = dataclasses.replace(helpers.upcast(d, model), velocity_representation=VelRepr.Inertial)
    ref_blk, ref_W = dyn_reference(model_ref, d_in, None, None)
    xdot, W = eb.run(model, eb.MODE_DYN, _block(model, d))
    tol_dyn = max(tol, 1e-3 if dtype == np.float32 else 0)
    assert hfc.measured(f"emul xdot {name} {np.dtype(dtype).name}", dyn_err(xdot, ref_blk, dtype, env_axis=-1), tol_dyn) < tol_dyn
    ref_W = ref_W.reshape(d.batch_size, -1).T
    assert hfc.measured(f"emul wrenches {name} {np.dtype(dtype).name}", dyn_err(W, ref_W, dtype, env_axis=-1), tol_dyn) < tol_dyn
    assert np.abs(ref_W).max() > 1.0


def test_rk4_box_on_the_edge_field(models):
    """Three of the four stages evaluate the terrain at moved points: eight environments are placed so that their lowest
    corner meets a border line half a step from now (hfc.move_onto_borders)."""
    model, model_ref, d = hfc.soft_case(models, "box", np.float64, rk4=True)
    ref = oracle.step(model_ref, d)
    _, g = hfc.edge_field()
    assert hfc.crossings(model, g, d, ref) >= 6
    out = eb.run(model, eb.MODE_STEP, _block(model, d))
    assert hfc.measured("emul rk4 step box float64", helpers.rel_err(out, _block(model, ref)), helpers.FP64_TOL) < helpers.FP64_TOL
    euler = oracle.step(helpers.with_params(model_ref, integrator=0), d)
    assert helpers.rel_err(_block(model, euler), _block(model, ref)) > 1e-7  # and it is not the Euler answer


@pytest.mark.parametrize("kind,key", list(hfc.CONTACT_CASES))
def test_rigid_models_on_the_edge_field(models, reduced_qp, kind, key):
    model, model_ref, d = hfc.contact_case(models, kind, key)
    ref = oracle.step(model_ref, d)
    out = eb.run(model, eb.MODE_STEP, _block(model, d))
    tol = 1e-7 if kind == "rigid" else 1e-9
    assert hfc.measured(f"emul {kind} step {key} float64", helpers.rel_err(out, _block(model, ref)), tol) < tol


# ---- known answers without the oracle ------------------------------------------------------------------------------------
def test_anisotropic_plane_equals_plane_terrain(models):
    """z = a x + b y + c with a != b on unequal spacings and a shifted origin: the bilinear interpolant of a linear function
    is that function and its central difference the exact slope.  (The ramp of test_emulation_parity has b = 0 on a square
    grid: exchanged spacings pass it.)"""
    hf, plane = hfc.anisotropic_plane()
    box = models("box")
    d = models.random_data("box", 16, seed=3)
    o1 = eb.run(helpers.with_params(box, terrain=hf), eb.MODE_STEP, _block(box, d))
    o2 = eb.run(helpers.with_params(box, terrain=plane), eb.MODE_STEP, _block(box, d))
    flat = eb.run(box, eb.MODE_STEP, _block(box, d))
    assert hfc.measured("emul anisotropic plane", helpers.rel_err(o1, o2), 1e-11) < 1e-11
    assert helpers.rel_err(flat, o2) > 1e-5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_outside_the_grid_the_border_extends(models, dtype):
    """Boxes a metre beyond the last sample line step bit for bit like boxes inside a grid that repeats the border row out
    to them (hfc.outside_fields says why the two heights are the same number, not merely close)."""
    t, ext, d = hfc.outside_state(models, dtype)
    box = models("box")
    o1 = eb.run(helpers.with_params(box, terrain=t), eb.MODE_STEP, _block(box, d))
    o2 = eb.run(helpers.with_params(box, terrain=ext), eb.MODE_STEP, _block(box, d))
    flat = eb.run(box, eb.MODE_STEP, _block(box, d))
    assert o1.dtype == dtype and np.array_equal(o1, o2)
    assert helpers.rel_err(flat, o1) > 1e-5  # the terrain acts on these boxes


def test_the_last_sample_belongs_to_the_last_cell(models):
    """Two bottom corners exactly on x = x_hi (cell nx - 2, t = 1) against the same samples with one more row behind them
    (cell nx - 1, t = 0)."""
    t, ext = hfc.last_cell_fields()
    d = hfc.last_cell_state(models)
    box = models("box")
    o1 = eb.run(helpers.with_params(box, terrain=t), eb.MODE_STEP, _block(box, d))
    o2 = eb.run(helpers.with_params(box, terrain=ext), eb.MODE_STEP, _block(box, d))
    _, g = hfc.edge_field()
    ref = oracle.step(helpers.with_params(box, terrain=g), d)
    assert hfc.measured("emul last cell", helpers.rel_err(o1, o2), 1e-12) < 1e-12
    assert helpers.rel_err(o1, _block(box, ref)) < helpers.FP64_TOL


# ---- the kernel descriptions of the device twin ----------------------------------------------------------------------------
def test_every_kernel_of_the_gpu_module_is_in_the_manifest(models):
    """The 'specialised' pass of the GPU suite needs a pre-built object per (model, precision, mode) description; the build
    takes them from tests/spec_manifest.txt.  A missing line is found here, not on the GPU machine."""
    import pathlib

    import test_height_field_edges_gpu as gpu_module

    manifest = {ln.strip() for ln in (pathlib.Path(__file__).parent / "spec_manifest.txt").read_text().splitlines() if ln.strip()}
    wanted = gpu_module.kernel_descriptions(models)
    assert len(wanted) >= 20
    missing = sorted(wanted - manifest)
    assert not missing, missing
