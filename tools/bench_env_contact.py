#!/usr/bin/env python3
"""The contact sensors on the device (jxs_env_contacts; JaxSimModelData.contact_sensors), timed the way
tools/bench_env_observe.py times the observation: blocks resident in HBM, HIP events on the launch stream around `--reps`
launches, 20 warm-up launches, the median of 5 windows.  The 12-DoF quadruped (4 feet x 4 points and a trunk group of 8) and
the 24-link humanoid of the headline (a group per link with collidable points, a trunk group of 8), fp32, N = 1024 and 65 536,
everything in one job.

  (a) the kernel with velocities (slip) and timers;
  (b) the kernel without velocities and timers;
  (c) observe of the link rows (a) reads, as two sources -- the yardstick: the same words read;
  (d) jxs_memcpy_d2d of the link-transform block;
  (e) the host route: js.contact.in_contact (wall clock);
  (f) per loop iteration: jxs_step in place alone, jxs_refresh_kinematics alone, and step + kinematics + sensors.

(a) - (e) run on random states whose base is low enough that part of the points is in contact; (f) steps the benchmark's
synthetic state.

(a) is also run with the launcher's environments-per-wave rule overridden (JXS_CONTACT_ENVS_PER_WAVE), which is what the rule
rests on.

    python tools/bench_env_contact.py [--reps 300] > profiles/env_contact.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from env_timing import set_envs_per_wave, timed, wall  # noqa: E402
import jaxsim_amd as ja  # noqa: E402
import jaxsim_amd.api as js  # noqa: E402
from jaxsim_amd import _lib, robots, runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="*", default=[1024, 65536])
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--envs-per-wave", type=int, nargs="*", default=[2, 4, 8, 16, 32])
args = ap.parse_args()

runtime.require_device()
lib = _lib.load()
stream = runtime.Stream()
runtime.set_stream(stream)
dtype = np.float32
F32 = _lib.dtype_code(dtype)
vp = C.c_void_p


def trunk_points(model):
    return [(model.link_names()[0], (x, y, z)) for x in (-0.2, 0.2) for y in (-0.1, 0.1) for z in (-0.1, 0.1)]


def quadruped():
    model = ja.JaxSimModel.build_from_model_description(robots.anymal12_urdf())
    kdp = model.kin_dyn_parameters
    body = np.asarray(kdp.contact_body)[np.asarray(kdp.indices_of_enabled_collidable_points)]
    children = set(np.asarray(kdp.parent_array).tolist())
    feet = [i for i in sorted(set(body.tolist())) if i not in children][:4]  # the leaf links with collidable points
    point = np.asarray(kdp.contact_point, np.float64)[np.asarray(kdp.indices_of_enabled_collidable_points)]
    tip = {i: point[body == i][0] for i in feet}  # four sensor points 3 cm around the first collidable point of each foot link
    groups = {model.link_names()[i]: dict(points=[(model.link_names()[i], tuple(tip[i] + (x, y, 0.0))) for x in (-0.03, 0.03) for y in (-0.03, 0.03)]) for i in feet}
    groups["trunk"] = dict(points=trunk_points(model))
    return model, groups


def humanoid():
    model = bench.build_model("icub23")
    kdp = model.kin_dyn_parameters
    body = np.asarray(kdp.contact_body)[np.asarray(kdp.indices_of_enabled_collidable_points)]
    groups = {model.link_names()[i]: dict(links=[model.link_names()[i]]) for i in sorted(set(body.tolist()))}
    groups["trunk"] = dict(points=trunk_points(model))
    return model, groups


print(f"# contact sensors, fp32, {args.reps} launches per figure (median [min .. max] of 5 windows), HIP events on the launch stream")
for label, (model, groups) in (("quadruped (anymal12)", quadruped()), ("humanoid (icub23)", humanoid())):
    spec = js.data.ContactSensorSpec.build(model, groups, dtype=dtype)
    dm = runtime.device_model(model, dtype)
    nL, P, G = model.number_of_links(), len(spec.parent), spec.n_groups
    used = sorted(set(spec.parent.tolist()))
    take_H, take_V = [12 * k + r for k in used for r in range(12)], [6 * k + r for k in used for r in range(6)]
    obs = js.data.ObservationSpec.build(model, [("source", dict(name="H", rows=12 * nL, take=take_H)), ("source", dict(name="V", rows=6 * nL, take=take_V))], dtype=dtype)
    print(f"# {label}: {nL} links, P = {P} points on {len(used)} links in G = {G} groups {[int(c) for c in spec.groups[:, 1]]}; the record has {spec.n_rows} rows, "
          f"(c) reads {obs.size} rows")
    for N in args.envs:
        # the sensors are timed on states with a mix of contacts (the base low enough that part of the points is under the
        # ground, so that the slip branch runs); the loop rows (f) step the benchmark's own synthetic state
        data = js.data.random_model_data(model, batch_size=N, seed=0, dtype=dtype, base_pos_bounds=((-1, -1, 0.50), (1, 1, 0.66)),
                                         base_rpy_bounds=((-0.3, -0.3, -np.pi), (0.3, 0.3, np.pi)))
        loop = bench.synthetic_state(model, N, seed=0, dtype=dtype)
        st, lst = data._state, loop._state
        tile = st.tile
        H, V = data.link_kinematics()
        H2, V2 = loop.link_kinematics()
        rec, timers = runtime.DeviceArray(spec.n_rows, N, dtype, tile=tile), spec.new_timers(N)
        out_c = runtime.DeviceMatrix(N, obs.size, dtype)
        copy, work = runtime.DeviceArray.like(H), runtime.DeviceArray.like(lst)
        mask = runtime.DeviceMask(N)
        _lib.check(lib.jxs_memset(vp(mask.ptr), 0, N, stream.handle), "jxs_memset")
        h, table, otable = stream.handle, spec._table(dm), obs._table(dm)
        src = (C.c_void_p * 4)(H.ptr, V.ptr)
        dt = model.time_step

        def sensors(full, Hp=H.ptr, Vp=V.ptr):
            if full:
                return lambda: lib.jxs_env_contacts(dm.handle, table, vp(Hp), vp(Vp), N, dt, vp(mask.ptr), vp(timers.ptr), vp(rec.ptr), h)
            return lambda: lib.jxs_env_contacts(dm.handle, table, vp(Hp), None, N, dt, None, None, vp(rec.ptr), h)

        wp = vp(work.ptr)
        tau = runtime.DeviceArray(max(model.dofs(), 1), N, dtype, tile=tile, zero=True)
        step_only = lambda: lib.jxs_step(dm.handle, wp, wp, vp(tau.ptr), None, int(loop.velocity_representation), N, h)  # noqa: E731
        kin_only = lambda: lib.jxs_refresh_kinematics(dm.handle, wp, vp(H2.ptr), vp(V2.ptr), N, h)  # noqa: E731
        loop_sensors = sensors(True, H2.ptr, V2.ptr)
        print(f"# N = {N}: transforms {H.nbytes / 1e6:.2f} MB + velocities {V.nbytes / 1e6:.2f} MB in {-(-N // tile)} tiles of {tile} columns; (a) reads "
              f"{N * P * 18 * 4 / 1e6:.2f} MB in {P} x 18 row accesses per environment and writes {N * (spec.n_rows + spec.n_timer_rows) * 4 / 1e6:.2f} MB")
        print(f"# {'operation':74s} {'us/launch':>10s} {'[min .. max]':>20s} {'M env/s':>9s} {'vs (c)':>7s} {'vs (d)':>7s}")
        cases = [
            (f"(c) observe of the {obs.size} link rows (a) reads", 0, lambda: lib.jxs_env_observe(dm.handle, otable, vp(st.ptr), src, N, 0, vp(out_c.ptr), F32, obs.size, h)),
            ("(d) jxs_memcpy_d2d of the link-transform block", 0, lambda: lib.jxs_memcpy_d2d(vp(copy.ptr), vp(H.ptr), H.nbytes, h)),
            ("(a) contacts with velocities and timers, the launcher's rule", 0, sensors(True)),
            ("(b) contacts without velocities and timers, the launcher's rule", 0, sensors(False)),
        ]
        for e in args.envs_per_wave:
            if e >= tile:
                cases.append((f"(a) contacts with velocities and timers, {e} environments per wave", e, sensors(True)))
        ref_c = ref_d = None
        for name, epw, call in cases:
            set_envs_per_wave("JXS_CONTACT_ENVS_PER_WAVE", epw)
            us, lo, hi = timed(stream, name, call, args.reps)
            ref_c = us if ref_c is None else ref_c
            ref_d = us if ref_d is None and name.startswith("(d)") else ref_d
            vs_d = "" if ref_d is None else f"{us / ref_d:7.2f}"
            print(f"  {name:74s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {vs_d:>7s}", flush=True)
        set_envs_per_wave("JXS_CONTACT_ENVS_PER_WAVE", 0)
        # (f) per loop iteration, in place on a copy of the state (restored before each figure)
        for name, call in (("(f) jxs_step in place", step_only), ("(f) jxs_refresh_kinematics", kin_only),
                           ("(f) step + link_kinematics + contact_sensors", lambda: step_only() or kin_only() or loop_sensors())):  # fmt: skip
            _lib.check(lib.jxs_memcpy_d2d(wp, vp(lst.ptr), lst.nbytes, h), "jxs_memcpy_d2d")
            us, lo, hi = timed(stream, name, call, args.reps)
            print(f"  {name:74s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {us / ref_d:7.2f}", flush=True)

        # (e) the host route to the flags: a kinematics launch, two downloads, NumPy
        def host_flags():
            data._invalidate_caches()
            return js.contact.in_contact(model, data)

        t = wall(stream, host_flags) * 1e6
        print(f"  {'(e) js.contact.in_contact on the host (wall clock)':74s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.1f} {t / ref_d:7.1f}", flush=True)
        reps = 200
        t = wall(stream, lambda: [data.contact_sensors(spec, kinematics=(H, V), timers=timers, out=rec) for _ in range(reps)]) / reps * 1e6
        print(f"  {'(a) data.contact_sensors(spec, kinematics=, timers=, out=) through Python (wall clock)':74s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.2f} {t / ref_d:7.2f}",
              flush=True)
        # the flags of the groups that are whole links against the host route
        data._invalidate_caches()
        H, V = data.link_kinematics(out=(H, V))
        host_rec = data.contact_sensors(spec, kinematics=(H, V), out=rec).to_host()
        flags = host_rec[spec.rows(None, "flag")].T != 0
        print(f"#   ({int(flags.sum())} of {flags.size} group flags are set, {int((host_rec[spec.rows(None, 'slip_sq')] > 0).sum())} groups have a slipping point)")
        links = [g for g, o in groups.items() if "links" in o]
        if links:
            want = np.asarray(js.contact.in_contact(model, data, link_names=links)).reshape(N, len(links))
            got = flags[:, [spec.group_names.index(g) for g in links]]
            print(f"#   ({int((got != want).sum())} of {want.size} link flags differ between (a) and (e); {int(want.sum())} are set)")
