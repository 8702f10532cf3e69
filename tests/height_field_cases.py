"""TEST INFRASTRUCTURE: the height-field grids and states of tests/test_height_field_edges_cpu.py (host emulation) and
tests/test_height_field_edges_gpu.py (device) -- one statement of every case, so that the two modules run the same inputs.

Every other height-field test of the suite samples a SQUARE grid (nx == ny, one spacing, an origin symmetric about zero, the
default delta = 0.010) wide enough that no collidable point reaches a border.  ``edge_field()`` is unequal in everything: 18 x 12
samples, spacing (0.07, 0.11), origin (-0.55, -0.70), delta = 0.004 -- and so small that the random states of the zoo (base
x, y in [-1, 1]) put penetrating points inside it, beyond each of its four borders and beyond its corners
(``region_counts`` / ``require_regions`` assert that on the inputs, before anything is compared).
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import helpers
import jaxsim_amd as ja
import oracle
import parity_cases as pc
from oracle import refterrain

X_RANGE, Y_RANGE, SPACING, DELTA = (-0.55, 0.62), (-0.70, 0.45), (0.07, 0.11), 0.004
SOFT_N, SOFT_SEED = 70, 23    # SoftContacts and Runge-Kutta cases
RIGID_N, RIGID_SEED = 24, 5   # RigidContacts / RelaxedRigidContacts cases
SOFT_CASES = [(name, dtype) for name in ("box", "icub") for dtype in (np.float64, np.float32)]
# (kind, key) -> (model of the zoo, enabled points, contact parameters): the entries of RIGID_CASES / RELAXED_CASES of
# tests/parity_cases.py under the same keys
CONTACT_CASES = {("rigid", "box4"): pc.RIGID_CASES["box4"], ("relaxed", "box8"): pc.RELAXED_CASES["box8"], ("relaxed", "anymal16"): pc.RELAXED_CASES["anymal16"]}
REGIONS = ("interior", "x<x_lo", "x>x_hi", "y<y_lo", "y>y_hi", "corners")


def edge_fn(x, y):
    return 0.04 * (np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.3 * np.sin(3.3 * y)) + 0.02 * x - 0.015 * y


def restated(t: ja.HeightFieldTerrain) -> refterrain.GridTerrain:
    """The oracle's statement of the grid of a product terrain (same samples, origin, spacing, delta)."""
    return refterrain.GridTerrain(np.array(t._heights), t._origin, t._spacing, t.delta)


@functools.lru_cache(maxsize=None)
def edge_field():
    """(product terrain, oracle GridTerrain of the same samples): anisotropic, off-centre, delta = 0.004."""
    t = ja.HeightFieldTerrain.from_function(edge_fn, x_range=X_RANGE, y_range=Y_RANGE, spacing=SPACING, delta=DELTA)
    assert t._heights.shape == (18, 12)
    return t, restated(t)


def bounds(g: refterrain.GridTerrain):
    """(x_lo, x_hi, y_lo, y_hi): the first and the last sample coordinate of each axis."""
    nx, ny = g.h.shape
    return g.x0, g.x0 + g.dx * (nx - 1), g.y0, g.y0 + g.dy * (ny - 1)


def region_counts(model, g: refterrain.GridTerrain, d) -> dict:
    """Number of PENETRATING enabled collidable points of the reference (grid height above the point) per region of
    the grid: inside it, beyond each border line, and beyond two border lines at once (the four corners together)."""
    d = helpers.upcast(d, model)
    p, _ = oracle.refstep.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    pen = g.height(x, y) - z > 0
    x_lo, x_hi, y_lo, y_hi = bounds(g)
    xl, xh, yl, yh = x < x_lo, x > x_hi, y < y_lo, y > y_hi
    masks = {"interior": ~(xl | xh | yl | yh), "x<x_lo": xl, "x>x_hi": xh, "y<y_lo": yl, "y>y_hi": yh, "corners": (xl | xh) & (yl | yh)}
    return {k: int((masks[k] & pen).sum()) for k in REGIONS}


def require_regions(counts: dict, per_side: int = 5, need: dict | None = None) -> None:
    """The input condition: at least ``per_side`` penetrating points beyond each border line and 5 inside the grid and in
    the corners (``need``: another number for a region).  A case that stops reaching a border fails here, not silently."""
    need = {"interior": 5, "corners": 5, **(need or {})}
    for k in REGIONS:
        assert counts[k] >= need.get(k, per_side), (k, counts)


def _sides(model, g, d):
    p, v = oracle.refstep.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    x_lo, x_hi, y_lo, y_hi = bounds(g)
    return p, v, np.stack([p[..., 0] < x_lo, p[..., 0] > x_hi, p[..., 1] < y_lo, p[..., 1] > y_hi], axis=-1)


def crossings(model, g, d0, d1) -> int:
    """Number of collidable points that are on another side of a border line in state ``d1`` than in ``d0``."""
    return int((_sides(model, g, d0)[2] != _sides(model, g, d1)[2]).any(axis=-1).sum())


def move_onto_borders(model, g, d, n_env: int = 8):
    """Shift the first ``n_env`` environments in x or y so that their lowest collidable point meets a border line (the four
    lines in turn) HALF a time step from now: the stages of a Runge-Kutta step evaluate the terrain on both sides of it."""
    x_lo, x_hi, y_lo, y_hi = bounds(g)
    lines = [(0, x_lo), (0, x_hi), (1, y_lo), (1, y_hi)]
    pos = np.array(d.base_position, dtype=np.float64)
    for _ in range(3):  # (the point's velocity v + w x p moves with the shift: a fixed point in two rounds)
        cur = dataclasses.replace(d, base_position=pos.astype(d.dtype)).update_caches(model)
        p, v, _ = _sides(model, g, helpers.upcast(cur, model))
        for e in range(n_env):
            j, (axis, line) = int(np.argmin(p[e, :, 2])), lines[e % 4]
            pos[e, axis] += (line - 0.5 * model.time_step * v[e, j, axis]) - p[e, j, axis]
    return dataclasses.replace(d, base_position=pos.astype(d.dtype)).update_caches(model)


def soft_case(zoo, name, dtype, rk4: bool = False):
    """(model on the product terrain, the same model on the oracle's grid, state): SoftContacts on ``edge_field()``."""
    t, g = edge_field()
    base = zoo(name)
    if rk4:
        base = pc.rk4(base)  # (a softer ground, as every Runge-Kutta parity case of the suite)
    d = zoo.random_data(name, SOFT_N, seed=SOFT_SEED, dtype=dtype)
    model = helpers.with_params(base, terrain=t)
    if rk4:
        d = move_onto_borders(model, g, d)
    # (icub reaches the two y borders and x < x_lo with 5 points each: 3 per side are asked of it, 5 of the box)
    require_regions(region_counts(model, g, d), per_side=3 if name == "icub" else 5)
    return model, helpers.with_params(base, terrain=g), d


def contact_case(zoo, kind, key):
    """(model on the product terrain, on the oracle's grid, state) of a RigidContacts / RelaxedRigidContacts case."""
    t, g = edge_field()
    name, idx, params = CONTACT_CASES[(kind, key)]
    base = (helpers.rigid_model if kind == "rigid" else helpers.relaxed_model)(zoo(name), idx, **params)
    d = zoo.random_data(name, RIGID_N, seed=RIGID_SEED)
    model = helpers.with_params(base, terrain=t)
    # 24 states of seed 5 hold no full input condition: two penetrating points of the box and none of the quadruped lie
    # beyond x_lo (the three cases together: 4).  Asked of each case: the interior, the other three borders and the corners
    # with 4 points or more (measured: 21 / 13 / 11 / 19 / 7 box4, 6 / 12 / 12 / 4 / 8 anymal16) and, of the box, x < x_lo too.
    require_regions(region_counts(model, g, d), per_side=4, need={"x<x_lo": 2 if name == "box" else 0})
    return model, helpers.with_params(base, terrain=g), d


def measured(key: str, value: float, gate: float) -> float:
    """Print a figure next to its gate before it is asserted (and log it: helpers.note); returns the figure."""
    print(f"[height-field edges] {key}: {value:.3e} (gate {gate:.1e})")
    helpers.note(key, value)
    return value


# ---- known answers that need no oracle ---------------------------------------------------------------------------------
PLANE_ABC = (0.08, -0.05, 0.013)


def anisotropic_plane():
    """(height field, PlaneTerrain) of z = a x + b y + c with a != b, sampled with unequal spacing on an off-centre grid that
    covers every point of the random box states (base x, y in [-1, 1], half diagonal 0.19) by more than delta."""
    a, b, c = PLANE_ABC
    hf = ja.HeightFieldTerrain.from_function(lambda x, y: a * x + b * y + c, x_range=(-1.45, 1.60), y_range=(-1.70, 1.50), spacing=SPACING, delta=DELTA)
    assert hf._heights.shape[0] != hf._heights.shape[1]
    return hf, ja.PlaneTerrain.build(height=c, normal=[-a, -b, 1.0])


def outside_fields():
    """(grid, the same grid extended by 30 repeated border rows in +x): the samples are a plane, all positive and adjacent
    ones within a factor two of each other.  Beyond x_hi the first grid clamps (cell nx - 2, t = 1: a + (c - a) * 1, and
    c - a is exact by Sterbenz's lemma, so the sum IS c); the extended grid interpolates between two equal rows
    (a + 0 * t = a).  Both are the border's height profile, bit for bit, and the x slope is exactly zero in both."""
    fn = lambda x, y: 0.05 + 0.03 * x - 0.02 * y  # noqa: E731
    t = ja.HeightFieldTerrain.from_function(fn, x_range=X_RANGE, y_range=Y_RANGE, spacing=SPACING, delta=DELTA)
    h = np.array(t._heights)
    assert h.min() > 0 and (h[1:] < 2 * h[:-1]).all() and (h[:-1] < 2 * h[1:]).all()
    ext = ja.HeightFieldTerrain.build(np.concatenate([h, np.repeat(h[-1:], 30, axis=0)], axis=0), origin=t._origin, spacing=t._spacing, delta=t.delta)
    return t, ext


def outside_state(zoo, dtype, N=16, seed=3):
    """Boxes placed wholly beyond x_hi (base x = x_hi + 1 .. 1.3), resting on / in the border's height profile."""
    t, ext = outside_fields()
    g = restated(t)
    _, x_hi, _, _ = bounds(g)
    d = zoo.random_data("box", N, seed=seed, dtype=np.float64)
    rng = np.random.default_rng(seed + 50)
    pos = np.array(d.base_position)
    pos[:, 0] = x_hi + 1.0 + rng.uniform(0.0, 0.3, N)
    pos[:, 2] += g.height(pos[:, 0], pos[:, 1])
    kw = {f.name: getattr(d, f.name) for f in dataclasses.fields(d)}
    kw.update(base_position=pos, link_transforms=None, link_velocities=None)
    d = oracle.OracleData(**{k: (v.astype(dtype) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}).update_caches(zoo("box"))
    counts = region_counts(helpers.with_params(zoo("box"), terrain=t), g, d)
    p, _ = oracle.refstep.collidable_points_pos_vel(zoo("box"), link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    assert p[..., 0].min() > x_hi + 0.5 and p[..., 0].max() < x_hi + 2.0  # wholly outside the grid, inside the extended one
    assert counts["x>x_hi"] >= 5 and counts["interior"] == 0
    return t, ext, d


def last_cell_fields():
    """(edge_field's terrain, the same samples with the last row repeated once): on the line x = x_hi the first grid reads
    its last cell at t = 1, the second the cell behind it at t = 0; beyond the line both extend the same row."""
    t, _ = edge_field()
    h = np.array(t._heights)
    ext = ja.HeightFieldTerrain.build(np.concatenate([h, h[-1:]], axis=0), origin=t._origin, spacing=t._spacing, delta=t.delta)
    return t, ext


def last_cell_state(zoo, N=8, seed=11):
    """Axis-aligned boxes (0.3 x 0.2 x 0.1, identity orientation: the corner coordinates are base +- half size, exactly
    rounded) whose two +x bottom corners lie on the last sample line -- (x - x0) / dx reaches nx - 1 = 17 -- and penetrate."""
    t, g = edge_field()
    x_lo, x_hi, _, _ = bounds(g)
    rng = np.random.default_rng(seed)
    bx = x_hi - 0.15
    while ((bx + 0.15) - x_lo) * (1.0 / SPACING[0]) < 17.0:  # (the kernel's own expression of the cell coordinate)
        bx = np.nextafter(bx, np.inf)
    assert abs(bx + 0.15 - x_hi) < 1e-15
    by = rng.uniform(-0.5, 0.3, N)
    hz = np.minimum(g.height(np.full(N, bx + 0.15), by - 0.1), g.height(np.full(N, bx + 0.15), by + 0.1))
    pos = np.stack([np.full(N, bx), by, 0.05 + hz - rng.uniform(0.001, 0.004, N)], axis=1)
    box = zoo("box")
    d = oracle.OracleData.build(box, base_position=pos, base_linear_velocity=0.3 * rng.uniform(-1, 1, (N, 3)),
                                base_angular_velocity=0.3 * rng.uniform(-1, 1, (N, 3)))  # fmt: skip
    p, _ = oracle.refstep.collidable_points_pos_vel(box, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    on_line = (p[..., 0] >= x_hi) & (p[..., 2] < pos[:, None, 2])
    assert (on_line.sum(axis=1) == 2).all() and (np.abs(p[..., 0][on_line] - x_hi) < 1e-15).all()
    assert (g.height(p[..., 0], p[..., 1]) - p[..., 2] > 0)[on_line].all()  # the two corners on the line penetrate
    return d
