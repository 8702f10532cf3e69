#!/usr/bin/env python3
"""The reward and the termination flags on the device (jxs_env_evaluate; JaxSimModelData.evaluate), timed the way
tools/bench_env_observe.py times the observation: state resident in HBM, HIP events on the launch stream around `--reps`
launches, 20 warm-up launches, the median of 5 windows.  The 24-link humanoid of the headline (`bench.build_model`), fp32,
N = 1024 and 65 536, everything in one job.  The table is a locomotion-style one over about 60 slots: exp-tracking of the base
linear and angular velocity against a commanded source, squared projected-gravity xy, squared joint velocities, squared last
torques (a source), joint-limit excess, a height window and a tilt condition on projected-gravity z.

  (a) evaluate with reward and done only;
  (b) the same plus terms, fired and steps;
  (c) observe of the same slots -- the yardstick: it reads the same words and writes 4 D bytes per environment instead of 5;
  (d) jxs_memcpy_d2d of the state block;
  (e) the host route: the data object's properties and NumPy (wall clock);
  (f) per loop iteration: jxs_step in place alone, and act + step + evaluate + reset_random_where + observe.

(a) is also run with the launcher's environments-per-wave rule overridden (JXS_EVALUATE_ENVS_PER_WAVE), which is what the
rule rests on.

    python tools/bench_env_evaluate.py [--reps 300] > profiles/env_evaluate.txt
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
from jaxsim_amd import _lib, runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="*", default=[1024, 65536])
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--model", default="icub23")
ap.add_argument("--envs-per-wave", type=int, nargs="*", default=[2, 4, 8, 16, 32])
args = ap.parse_args()

runtime.require_device()
lib = _lib.load()
stream = runtime.Stream()
runtime.set_stream(stream)
model = bench.build_model(args.model)
dtype = np.float32
F32 = _lib.dtype_code(dtype)
n = model.dofs()
body = ja.VelRepr.Body

command = lambda rows: ("source", dict(name="command", rows=6, row=rows))  # noqa: E731
REWARDS = [
    ("track_linear", dict(term="base_linear_velocity", target=command([0, 1, 2]), inner="square", outer="exp", sigma=0.25, weight=1.0)),
    ("track_angular", dict(term="base_angular_velocity", target=command([3, 4, 5]), inner="square", outer="exp", sigma=0.25, weight=0.5)),
    ("upright", dict(term="projected_gravity", index=[0, 1], inner="square", weight=-2.0)),
    ("joint_rate", dict(term="joint_velocities", inner="square", weight=-1e-3)),
    ("torques", dict(term=("source", dict(name="tau", rows=n)), inner="square", weight=-1e-4)),
]
TERMINATIONS = [
    ("height", dict(term="base_height", below=0.3, above=1.5)),
    ("tilt", dict(term="projected_gravity", index=2, above=-0.5)),
]
kdp = model.kin_dyn_parameters
if np.isfinite(np.asarray(kdp.position_limits_min, float)).all() and np.isfinite(np.asarray(kdp.position_limits_max, float)).all():
    REWARDS.append(("limits", dict(term="joint_positions", inner="excess", weight=-5.0)))
else:  # (a model without finite limits: a window of one radian around zero)
    REWARDS.append(("limits", dict(term="joint_positions", inner="excess", weight=-5.0, offset=0.0, scale=1.0)))
spec = js.data.RewardSpec.build(model, REWARDS, TERMINATIONS, termination_reward=-10.0, dtype=dtype, velocity_representation=body)
D, K = spec.slots.shape[0], spec.n_terms
# the same slots as an observation: the yardstick
obs_same = js.data.ObservationSpec(spec.layout, dtype, dtype, body, spec.slots, spec.offset, spec.scale, {}, spec.source_names, spec.source_rows)
obs_loop = js.data.ObservationSpec.build(model, ["joint_positions", "joint_velocities", "base_orientation", "base_velocity", "projected_gravity", "base_height"],
                                         dtype=dtype, velocity_representation=body)  # fmt: skip
act_spec = js.data.ActionSpec.build(model, dtype=dtype, kp=40.0, kd=2.0, scale=0.5, action_clip=1.0, torque_limit=80.0)
dist = js.data.RandomStateDistribution.build(model, dtype=dtype)
print(f"# reward and termination flags, {args.model} synthetic humanoid, fp32, D = {D} slots, K = {K} terms, C = {spec.n_conditions} conditions, "
      f"{args.reps} launches per figure (median [min .. max] of 5 windows), HIP events on the launch stream")
dm = runtime.device_model(model, dtype)
vp = C.c_void_p
for N in args.envs:
    data = bench.synthetic_state(model, N, seed=0, dtype=dtype)
    st = data._state
    rows, tile = st.rows, st.tile
    rng = np.random.default_rng(0)
    cmd = runtime.DeviceArray.from_host(rng.uniform(-1, 1, (6, N)).astype(dtype), tile=tile)
    tau = runtime.DeviceArray.from_host(rng.uniform(-20, 20, (n, N)).astype(dtype), tile=tile)
    actions = runtime.DeviceMatrix.from_host(rng.normal(0, 1, (N, n)).astype(np.float32))
    sources = {"command": cmd, "tau": tau}
    ptrs = (C.c_void_p * 4)(*[sources[name].ptr for name in spec.source_names])
    reward, done = runtime.DeviceMatrix(N, 1, dtype), runtime.DeviceMask(N)
    terms, fired = runtime.DeviceMatrix(N, K, dtype), runtime.DeviceWords(N)
    steps = runtime.DeviceIndices.from_host(np.zeros(N, np.int64))
    out_same, out_loop = runtime.DeviceMatrix(N, D, dtype), runtime.DeviceMatrix(N, obs_loop.size, dtype)
    copy, work = runtime.DeviceArray.like(st), runtime.DeviceArray.like(st)
    sp, h = vp(st.ptr), stream.handle
    table, otable, ltable, atable = spec._table(dm), obs_same._table(dm), obs_loop._table(dm), act_spec._table(dm)
    none = (C.c_void_p * 4)()

    def evaluate(state_ptr, full):
        if full:
            return lambda: lib.jxs_env_evaluate(dm.handle, table, state_ptr, ptrs, N, int(body), vp(reward.ptr), F32, vp(done.ptr), vp(fired.ptr),
                                                vp(terms.ptr), F32, K, vp(steps.ptr), 1000, h)  # fmt: skip
        return lambda: lib.jxs_env_evaluate(dm.handle, table, state_ptr, ptrs, N, int(body), vp(reward.ptr), F32, vp(done.ptr), None, None, F32, 0, None, 0, h)

    def observe_same():
        return lib.jxs_env_observe(dm.handle, otable, sp, ptrs, N, int(body), vp(out_same.ptr), F32, D, h)

    def step_only():
        return lib.jxs_step(dm.handle, vp(work.ptr), vp(work.ptr), vp(tau.ptr), None, int(data.velocity_representation), N, h)

    wp = vp(work.ptr)
    loop_eval = evaluate(wp, True)

    def iteration():
        rc = lib.jxs_env_act(dm.handle, atable, wp, vp(actions.ptr), F32, n, None, vp(tau.ptr), N, h)
        rc = rc or step_only() or loop_eval()
        rc = rc or lib.jxs_env_randomize(dm.handle, vp(done.ptr), wp, N, dist.bounds_ptr, 0, 1, 0, int(dist.velocity_representation), h)
        return rc or lib.jxs_env_observe(dm.handle, ltable, wp, none, N, int(body), vp(out_loop.ptr), F32, obs_loop.size, h)

    print(f"# N = {N}: state block {st.nbytes / 1e6:.2f} MB = {-(-N // tile)} tiles of {rows} rows x {tile} columns; (a) writes {N * 5 / 1e6:.2f} MB, "
          f"(b) {N * (13 + 4 * K) / 1e6:.2f} MB, (c) {N * D * 4 / 1e6:.2f} MB")
    print(f"# {'operation':74s} {'us/launch':>10s} {'[min .. max]':>20s} {'M env/s':>9s} {'vs (c)':>7s} {'vs (d)':>7s}")
    cases = [
        (f"(c) observe of the same {D} slots", 0, observe_same),
        ("(d) jxs_memcpy_d2d of the state block", 0, lambda: lib.jxs_memcpy_d2d(vp(copy.ptr), sp, st.nbytes, h)),
        ("(a) evaluate, reward and done, the launcher's rule", 0, evaluate(sp, False)),
        ("(b) evaluate with terms, fired and steps, the launcher's rule", 0, evaluate(sp, True)),
    ]
    for e in args.envs_per_wave:
        if e >= tile:
            cases.append((f"(a) evaluate, reward and done, {e} environments per wave", e, evaluate(sp, False)))
    ref_c = ref_d = None
    for name, epw, call in cases:
        set_envs_per_wave("JXS_EVALUATE_ENVS_PER_WAVE", epw)
        us, lo, hi = timed(stream, name, call, args.reps)
        ref_c = us if ref_c is None else ref_c
        ref_d = us if ref_d is None and name.startswith("(d)") else ref_d
        vs_d = "" if ref_d is None else f"{us / ref_d:7.2f}"
        print(f"  {name:74s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {vs_d:>7s}", flush=True)
    set_envs_per_wave("JXS_EVALUATE_ENVS_PER_WAVE", 0)
    # (f) per loop iteration, in place on a copy of the state (restored before each figure)
    for name, call in (("(f) jxs_step in place with a torque block", step_only), ("(f) act + step + evaluate + reset_random_where(done) + observe", iteration)):
        _lib.check(lib.jxs_memcpy_d2d(wp, sp, st.nbytes, h), "jxs_memcpy_d2d")
        us, lo, hi = timed(stream, name, call, args.reps)
        print(f"  {name:74s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {us / ref_d:7.2f}", flush=True)

    # (e) the host route to the same reward and done: one download of the block per property, NumPy
    cmd_h, tau_h = cmd.to_host().T, tau.to_host().T
    off, sc = spec.offset.astype(dtype), spec.scale.astype(dtype)
    first_limits = int(spec.terms[-1][0])

    def host_reward():
        data._invalidate_caches()
        with data.switch_velocity_representation(body):
            v = data.base_velocity.astype(dtype)
        g = -data.base_transform[:, 2, :3].astype(dtype)
        q, qd = data.joint_positions.astype(dtype), data.joint_velocities.astype(dtype)
        z = data.base_position[:, 2].astype(dtype)
        r = np.exp(-(((v[:, :3] - cmd_h[:, :3]) * sc[0]) ** 2).sum(axis=1)) + 0.5 * np.exp(-(((v[:, 3:] - cmd_h[:, 3:]) * sc[3]) ** 2).sum(axis=1))
        r = r - 2.0 * (g[:, :2] ** 2).sum(axis=1) - 1e-3 * (qd**2).sum(axis=1) - 1e-4 * (tau_h**2).sum(axis=1)
        y = (q - off[first_limits : first_limits + n]) * sc[first_limits : first_limits + n]
        r = r - 5.0 * np.maximum(np.abs(y) - 1, 0).sum(axis=1)
        dn = ~((0.3 <= z) & (z <= 1.5)) | ~(g[:, 2] <= -0.5)
        return np.where(dn, r - 10.0, r), dn

    t = wall(stream, host_reward) * 1e6
    print(f"  {'(e) host properties + NumPy (wall clock)':74s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.1f} {t / ref_d:7.1f}", flush=True)
    reps = 200
    t = wall(stream, lambda: [data.evaluate(spec, sources=sources, reward=reward, done=done) for _ in range(reps)]) / reps * 1e6
    print(f"  {'(a) data.evaluate(spec, reward=, done=) through Python (wall clock)':74s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.2f} {t / ref_d:7.2f}", flush=True)
    data.evaluate(spec, sources=sources, reward=reward, done=done)
    got_r, got_d = reward.to_host()[:, 0], done.to_host()
    want_r, want_d = host_reward()
    print(f"#   (largest difference between (a) and (e): reward {float(np.abs(got_r.astype(np.float64) - want_r).max()):.2e}, "
          f"{int(((got_d & 1) != want_d).sum())} done flags differ; {int((got_d != 0).sum())} of {N} environments are done)")
