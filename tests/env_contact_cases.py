"""TEST INFRASTRUCTURE: the cases the CPU and the GPU tests of the contact sensors share -- sensor tables of the shapes the
feature distinguishes, the three terrains, synthetic link blocks (random rotations, positions and velocities), and the
comparison of two records with the one tolerance the law allows (the slip on a height field)."""

from __future__ import annotations

import numpy as np

import env_contact_ref as ref

DTYPES = (np.float32, np.float64)
# (P, G, N): every P, G and N of the issue; G <= P; groups are unequal, with one of a single point and, from P = 200 on,
# one above 64 points (table())
SHAPES = ((1, 1, 1), (63, 1, 37), (63, 4, 130), (63, 32, 1), (64, 4, 37), (65, 4, 130), (65, 32, 37), (200, 4, 130), (200, 32, 37), (1024, 1, 37),
          (1024, 4, 1), (1024, 32, 130))  # fmt: skip
TILES = (1, 2, 4, 64)
TERRAINS = ("flat", "plane", "field")
# Height-field slip (test_env_contact_cpu.py test_height_field_slip_error_against_float64 measures it): the largest error of the
# harness against the float64 evaluation over the CPU cases, in eps |pd|^2 of the group's points in contact -- 59.38 in float32; in float64 the harness is that
# evaluation, so the one multiple serves both dtypes, each with its own eps -- and the bound of the comparisons, twice that
SLIP_MEASURED_EPS = 60.0
SLIP_BOUND_EPS = 2 * SLIP_MEASURED_EPS


def terrain(kind: str) -> ref.Terrain:
    if kind == "flat":
        return ref.Terrain(ref.FLAT, height=0.07)
    if kind == "plane":
        n = np.array([0.12, -0.2, 1.0])
        return ref.Terrain(ref.PLANE, height=-0.05, normal=tuple((n / np.linalg.norm(n)).tolist()))
    # 5 x 4 samples, unequal spacing, off-centre: x in [-0.3, 1.7], y in [0.1, 2.5]; the blocks reach beyond it on every side
    rng = np.random.default_rng(5)
    return ref.Terrain(ref.FIELD, samples=rng.uniform(-0.2, 0.2, size=(5, 4)), origin=(-0.3, 0.1), spacing=(0.5, 0.8), delta=0.01)


def group_sizes(P: int, G: int) -> list[int]:
    """``G`` unequal sizes summing to ``P``: one group of a single point, one that takes what is left (above 64 points from
    P = 200 on), the others 2, 3, 4 ... where ``P`` allows."""
    if G == 1:
        return [P]
    sizes = [1] * G
    left = P - G
    for g in range(1, G - 1):
        add = min(left, g)
        sizes[g] += add
        left -= add
    sizes[G - 1] += left
    return sizes[1:] + sizes[:1] if G > 2 else sizes  # (the single point last but one place round: not always group 0)


def table(P: int, G: int, n_links: int, seed: int = 0) -> ref.Table:
    rng = np.random.default_rng(1000 * P + G + seed)
    sizes = group_sizes(P, G)
    assert sum(sizes) == P and min(sizes) >= 1
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return ref.Table(np.stack([first, sizes], axis=1).astype(np.int32), rng.integers(0, n_links, size=P).astype(np.int32), rng.uniform(-0.3, 0.3, size=(P, 3)))


def link_blocks(n_links: int, N: int, dtype, seed: int = 0):
    """Untiled ``H [nL*12, N]`` (random rotations; positions x, y in [-1.5, 3.5], z in [-0.3, 0.5], or
    1.5 higher for a whole environment) and ``V [nL*6, N]``."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n_links, N, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = np.moveaxis(q, -1, 0)
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=0).reshape(3, 3, n_links, N)  # fmt: skip
    lifted = np.where(rng.random(N) < 0.4, 1.5, 0.0)  # (four environments in ten are in the air with every link)
    t = np.stack([rng.uniform(-1.5, 3.5, (n_links, N)), rng.uniform(-1.5, 3.5, (n_links, N)), rng.uniform(-0.3, 0.5, (n_links, N)) + lifted])
    H = np.zeros((n_links, 3, 4, N))
    H[:, :, :3] = np.moveaxis(R, 2, 0)
    H[:, :, 3] = np.moveaxis(t, 1, 0)
    V = np.concatenate([rng.normal(0, 1.0, (n_links, 3, N)), rng.normal(0, 2.0, (n_links, 3, N))], axis=1)
    return H.reshape(n_links * 12, N).astype(dtype), V.reshape(n_links * 6, N).astype(dtype)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits_or_both_nan(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def slip_rows(G: int) -> np.ndarray:
    return ref.ROWS * np.arange(G) + ref.SLIP_SQ


def slip_magnitude(tr: ref.Terrain, tb: ref.Table, H: np.ndarray, V: np.ndarray) -> np.ndarray:
    """``[G, N]``: the largest ``|pd|^2`` over the points of each group that are in contact (``c <= 0`` in the block's dtype:
    the only points whose slip can reach the record), in float64: the magnitude of the slip's operands.  0 without one."""
    c, _ = ref.point_samples(tr, tb, H, V)
    _, mag = ref.slip_squared_f64(tr, tb, H, V)
    with np.errstate(invalid="ignore"):
        mag = np.where((c <= 0) & ~np.isnan(mag), mag, 0.0)
    return np.stack([mag[f : f + n].max(axis=0) for f, n in np.asarray(tb.groups)])


def assert_records_equal(got: np.ndarray, want: np.ndarray, G: int, *, slip_tolerance=None, what=""):
    """Untiled records ``[G*8, n]``: bit for bit (two NaNs are equal); the SLIP_SQ rows within ``slip_tolerance [G, n]`` where
    one is given (the height field)."""
    same = same_bits_or_both_nan(got, want)
    if slip_tolerance is not None:
        rows = slip_rows(G)
        with np.errstate(invalid="ignore"):
            same[rows] |= np.abs(got[rows].astype(np.float64) - want[rows].astype(np.float64)) <= slip_tolerance
    bad = np.argwhere(~same)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first (row, env) {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
