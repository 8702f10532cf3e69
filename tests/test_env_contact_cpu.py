"""The contact sensors on the host: the harness (tests/env_contact_emul.py: jxs_contact::sense_env of
jaxsim_amd/csrc/jxs_env_contact.h over every environment) against the NumPy restatement (tests/env_contact_ref.py) -- bit for bit
on flat, tilted-plane and height-field terrain, the slip on the height field within the measured bound --, the NaN rules, the
timers over a sequence of calls, and the validity check of a table."""

import numpy as np
import pytest

import env_contact_cases as cases
import env_contact_emul as emul
import env_contact_ref as ref

N_LINKS = 7
GRID = [pytest.param(P, G, N, cases.TILES[(i + j) % 4], dt, kind, id=f"P{P}-G{G}-N{N}-T{cases.TILES[(i + j) % 4]}-{np.dtype(dt).name}-{kind}")
        for i, (P, G, N) in enumerate(cases.SHAPES) for j, kind in enumerate(cases.TERRAINS) for dt in cases.DTYPES]  # fmt: skip


def run_both(tr, tb, H, V, N, T, dt_step, timers=None, reset=None, fill=np.nan):
    """``(harness record, restatement record, harness timers, restatement timers)`` untiled, the harness's with the padding
    columns.  The padding columns of every block going in hold ``fill``."""
    G = tb.G
    tH, tV = ref.tile_block(H, T, fill), None if V is None else ref.tile_block(V, T, fill)
    tt = None if timers is None else ref.tile_block(timers, T, fill)
    out0 = np.full(8 * G * (-(-N // T) * T), fill, H.dtype)
    rec, tm = emul.contacts(tr, tb, N_LINKS, tH, tV, N, T, dt_step, reset=reset, timers=tt, out=out0)
    want, want_t = ref.sense(tr, tb, H, V, dt_step, timers, reset)
    return ref.untile_block(rec, 8 * G, N, T), want, None if tm is None else ref.untile_block(tm, 2 * G, N, T), want_t


def slip_tolerance(tr, tb, H, V):
    if tr.kind != ref.FIELD or V is None:
        return None
    return cases.SLIP_BOUND_EPS * np.finfo(H.dtype).eps * cases.slip_magnitude(tr, tb, H, V)


@pytest.mark.parametrize("P,G,N,T,dtype,kind", GRID)
def test_harness_equals_the_restatement(P, G, N, T, dtype, kind):
    """Record and timers, bit for bit; NaN in every padding column going in, zero in the record's coming out."""
    tr, tb = cases.terrain(kind), cases.table(P, G, N_LINKS)
    H, V = cases.link_blocks(N_LINKS, N, dtype, seed=P + G)
    rng = np.random.default_rng(N)
    timers = rng.uniform(0.0, 0.4, (2 * G, N)).astype(dtype) * (rng.random((2 * G, N)) < 0.7)
    reset = (rng.random(N) < 0.3).astype(np.uint8)
    got, want, got_t, want_t = run_both(tr, tb, H, V, N, T, 0.002, timers, reset)
    cases.assert_records_equal(got[:, :N], want, G, slip_tolerance=slip_tolerance(tr, tb, H, V), what="record")
    assert (cases.bits(got[:, N:]) == 0).all(), "padding columns of the record are not zero"
    assert (cases.bits(got_t[:, :N]) == cases.bits(want_t)).all()
    assert np.isnan(got_t[:, N:]).all(), "padding columns of the timers were written"
    flag, count = want[ref.FLAG :: 8], want[ref.COUNT :: 8]
    assert ((flag == 1) == (count > 0)).all()
    assert N < 8 or 0 < flag.mean() < 1, "the case does not see both outcomes"


@pytest.mark.parametrize("kind", cases.TERRAINS)
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_without_velocities_and_timers(dtype, kind):
    """NULL velocities: SLIP_SQ is 0; NULL timers: rows 4-7 are 0; the rest as with them."""
    P, G, N, T = 65, 4, 37, 4
    tr, tb = cases.terrain(kind), cases.table(P, G, N_LINKS)
    H, V = cases.link_blocks(N_LINKS, N, dtype, seed=3)
    got, want, got_t, _ = run_both(tr, tb, H, None, N, T, 0.002)
    full, _, _, _ = run_both(tr, tb, H, V, N, T, 0.002, np.zeros((2 * G, N), dtype))
    cases.assert_records_equal(got[:, :N], want, G, what="record")
    assert got_t is None and (got.reshape(G, 8, -1)[:, ref.SLIP_SQ :] == 0).all()
    assert (cases.bits(got.reshape(G, 8, -1)[:, : ref.SLIP_SQ]) == cases.bits(full.reshape(G, 8, -1)[:, : ref.SLIP_SQ])).all()


@pytest.mark.parametrize("kind", cases.TERRAINS)
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_nan_position_is_no_contact_and_keeps_the_min_rule(dtype, kind):
    """Link 2 of every third environment has a NaN position.  Groups: [only link 2] -> no contact, CLEARANCE NaN; [link 2
    first, then a point deep in the ground] -> contact by the second point, CLEARANCE stays NaN (c < NaN is false); [the deep
    point first, then link 2] -> CLEARANCE is the first point's, the NaN is passed over."""
    N, T = 37, 4
    H, V = cases.link_blocks(N_LINKS, N, dtype, seed=11)
    H[12 * 1 + 11] = -5.0  # link 1 far below every terrain
    H[12 * 2 + 3 : 12 * 2 + 12 : 4, ::3] = np.nan
    tb = ref.Table(np.array([[0, 2], [2, 2], [4, 2]], np.int32), np.array([2, 2, 2, 1, 1, 2], np.int32),
                   np.array([[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0, 0, 0], [0, 0, 0], [0.1, 0.1, 0]]))  # fmt: skip
    tr = cases.terrain(kind)
    got, want, _, _ = run_both(tr, tb, H, V, N, T, 0.002, np.zeros((6, N), dtype))
    cases.assert_records_equal(got[:, :N], want, 3, slip_tolerance=slip_tolerance(tr, tb, H, V), what="record")
    r = got[:, :N].reshape(3, 8, N)[:, :, ::3]
    assert (r[0, ref.FLAG] == 0).all() and (r[0, ref.COUNT] == 0).all() and np.isnan(r[0, ref.CLEARANCE]).all() and (r[0, ref.AIR_TIME] > 0).all()
    assert (r[1, ref.FLAG] == 1).all() and (r[1, ref.COUNT] == 1).all() and np.isnan(r[1, ref.CLEARANCE]).all()
    assert (r[2, ref.FLAG] == 1).all() and (r[2, ref.COUNT] == 1).all() and (r[2, ref.CLEARANCE] < -4).all()
    assert np.isfinite(got[:, :N].reshape(3, 8, N)[:, ref.SLIP_SQ]).all()


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_timer_sequence_with_touchdown_lift_off_and_reset(dtype):
    """Eight calls; every environment's links go up and down by its own pattern, so touchdown and lift-off both fire; the
    fourth and fifth calls carry a reset mask; dt = 1e-3 accumulates in the block's dtype, which the comparison of the timers with
    the restatement's, bit for bit at every call, checks."""
    P, G, N, T, dt_step = 20, 4, 37, 4, 1e-3
    tr, tb = cases.terrain("flat"), cases.table(P, G, N_LINKS)
    H0, V = cases.link_blocks(N_LINKS, N, dtype, seed=2)
    rng = np.random.default_rng(8)
    up = np.array([1, 1, 0, 0, 1, 1, 0, 1], bool)[:, None] ^ (rng.random((8, N)) < 0.25)
    timers = np.zeros((2 * G, N), dtype)
    seen = np.zeros((3, G, N), bool)  # touchdown, lift-off (air time restarts from dt), a flight of more than one step
    for call in range(8):
        H = H0.copy()
        H[11::12] += np.where(up[call], 2.0, -2.0).astype(dtype)
        reset = (rng.random(N) < 0.3).astype(np.uint8) if call in (3, 4) else None
        got, want, got_t, want_t = run_both(tr, tb, H, V, N, T, dt_step, timers, reset)
        cases.assert_records_equal(got[:, :N], want, G, what=f"record of call {call}")
        assert (cases.bits(got_t[:, :N]) == cases.bits(want_t)).all(), f"timers of call {call}"
        r = want.reshape(G, 8, N)
        assert ((r[:, ref.FLAG] == 1) == ~up[call]).all()
        if reset is not None:
            assert (r[:, ref.TOUCHDOWN][:, reset != 0] == 0).all()
            assert np.isin(r[:, ref.AIR_TIME : ref.CONTACT_TIME + 1][:, :, reset != 0], (0, dtype(dt_step))).all()
        seen[0] |= r[:, ref.TOUCHDOWN] == 1
        seen[1] |= (r[:, ref.AIR_TIME] == dtype(dt_step)) & (call > 0)
        seen[2] |= r[:, ref.FLIGHT_TIME] > dtype(dt_step)
        assert ((r[:, ref.TOUCHDOWN] == 1) == (r[:, ref.FLIGHT_TIME] > 0)).all()
        timers = want_t
    assert seen[0].any() and seen[1].any() and seen[2].any()


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_height_field_slip_error_against_float64(dtype):
    """The slip on the height field is the one value behind a reciprocal square root (and behind a difference of two heights
    times 1 / (2 delta), which is what the error comes from).  Its bound is taken the way tests/test_env_observe_gpu.py takes
    those of the values behind a square root: a multiple of eps times the magnitude of the operands, the largest |pd|^2 over the
    group's points in contact.  The multiple is
    the worst case of the harness against the float64 evaluation over the height-field cases of this file
    (cases.SLIP_MEASURED_EPS = 60; measured 59.38 in float32, and 0 in float64, where the harness is that evaluation), and the comparisons with the restatement and with the
    device allow twice that, which covers the device's reciprocal square root."""
    worst = 0.0
    for P, G, N in cases.SHAPES:
        tr, tb = cases.terrain("field"), cases.table(P, G, N_LINKS)
        H, V = cases.link_blocks(N_LINKS, N, dtype, seed=P + G)
        rec, _ = emul.contacts(tr, tb, N_LINKS, ref.tile_block(H, 1), ref.tile_block(V, 1), N, 1, 0.002)
        got = ref.untile_block(rec, 8 * G, N, 1)[cases.slip_rows(G)].astype(np.float64)
        c, _ = ref.point_samples(tr, tb, H, V)
        s64, mag = ref.slip_squared_f64(tr, tb, H, V)
        s64 = np.where(c <= 0, s64, 0.0)
        want = np.stack([s64[f : f + n].max(axis=0) for f, n in tb.groups])
        scale = np.finfo(dtype).eps * cases.slip_magnitude(tr, tb, H, V)
        assert (got[scale == 0] == 0).all() and (want[scale == 0] == 0).all()  # (no point in contact: no slip)
        worst = max(worst, float((np.abs(got - want)[scale > 0] / scale[scale > 0]).max(initial=0.0)))
    print(f"height-field slip, {np.dtype(dtype).name}: worst error {worst:.2f} eps |pd|^2")
    assert worst <= cases.SLIP_MEASURED_EPS


def test_create_refusals_report_the_first_bad_entry():
    tb = cases.table(20, 4, N_LINKS)
    ok = lambda **kw: emul.table_error(ref.Table(**{**dict(groups=tb.groups, parent=tb.parent, L_p=tb.L_p), **kw}), N_LINKS)  # noqa: E731
    assert emul.table_error(tb, N_LINKS) == (0, -1)
    for G, P in ((0, 20), (33, 20), (4, 0), (4, 1025)):
        assert emul.table_error(tb, N_LINKS, G=G, P=P) == (1, -1)
    big = cases.table(1024, 32, N_LINKS)
    assert emul.table_error(big, N_LINKS) == (0, -1)
    g = tb.groups.copy()
    g[2, 1] = 0  # an empty group
    assert ok(groups=g) == (2, 2)
    g = tb.groups.copy()
    g[1, 0] -= 1  # overlaps group 0
    assert ok(groups=g) == (2, 1)
    g = tb.groups.copy()
    g[3, 1] += 1  # beyond the table
    assert ok(groups=g) == (2, 3)
    g = tb.groups.copy()
    g[0, 0] = -1
    assert ok(groups=g) == (2, 0)
    g = tb.groups.copy()
    first, count = g[1]
    g[1, 1] -= 1  # its last entry belongs to no group
    assert ok(groups=g) == (3, first + count - 1)
    for bad_parent in (-1, N_LINKS):
        p = tb.parent.copy()
        p[5], p[9] = bad_parent, bad_parent
        assert ok(parent=p) == (4, 5)
    for bad_value in (np.nan, np.inf, -np.inf):
        L = tb.L_p.copy()
        L[7, 1], L[12, 0] = bad_value, bad_value
        assert ok(L_p=L) == (5, 7)
    L = tb.L_p.copy()
    L[3, 2] = 1e300  # finite in float64 only
    assert emul.table_error(ref.Table(tb.groups, tb.parent, L), N_LINKS, np.float32) == (5, 3)
    assert emul.table_error(ref.Table(tb.groups, tb.parent, L), N_LINKS, np.float64) == (0, -1)
    # an uncovered entry in front of a bad parent: the entries are looked at in order
    g, p = tb.groups.copy(), tb.parent.copy()
    g[1, 1] -= 1
    p[0] = -1
    assert emul.table_error(ref.Table(g, p, tb.L_p), N_LINKS) == (4, 0)


def test_harness_refuses_what_the_launch_refuses():
    tr, tb = cases.terrain("flat"), cases.table(5, 1, N_LINKS)
    H, _ = cases.link_blocks(N_LINKS, 3, np.float32)
    for dt_step in (-1e-3, np.nan, np.inf, 1e300):
        assert emul.contacts(tr, tb, N_LINKS, ref.tile_block(H, 1), None, 3, 1, dt_step, rc=True) == -2
    assert emul.contacts(tr, tb, N_LINKS, ref.tile_block(H, 1), None, 0, 1, 1e-3, rc=True) == -2
    assert emul.contacts(tr, tb, N_LINKS, ref.tile_block(H, 1), None, 3, 1, 0.0, rc=True) == 0
