#!/usr/bin/env python3
"""The action-to-torque law on the device (jxs_env_act; JaxSimModelData.act), timed the way tools/bench_env_observe.py times
the observation: state resident in HBM, HIP events on the launch stream around `--reps` launches, 20 warm-up launches, the
median of 5 windows.  The 24-link humanoid of the headline (`bench.build_model`), fp32, N = 1024 and 65 536, everything in one
job:

  (a) act: 23 position-controlled joints from a float32 [N][23] action tensor;
  (b) the same with a feed-forward block;
  (c) jxs_tile_from_env_major of an [N][23] tensor -- the least any torque input costs today; it moves half of (a)'s bytes;
  (d) jxs_memcpy_d2d of the state block;
  (e) the route a user has today: a PD kernel of their own on an observation (the stand-in tests/policy_kernel.py, which
      writes an environment-major [N][23] tensor) and jxs_tile_from_env_major of its output;
  (f) the host route: data.joint_positions, data.joint_velocities, NumPy, and the upload of the torques (wall clock);
  per step: jxs_step in place with a torque block, alone and behind act.

(a) and (b) are also run with the launcher's environments-per-wave rule overridden (JXS_ACT_ENVS_PER_WAVE), which is how the
rule was chosen.  (profiles/env_act_both_reads.txt is the output of this tool on the build that still had two ways of reading
the action tensor, switched by a knob that went with the slower one: DESIGN.md section 3.)

    python tools/bench_env_act.py [--reps 300] > profiles/env_act.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from env_timing import set_envs_per_wave, timed, wall  # noqa: E402
import jaxsim_amd.api as js  # noqa: E402
import policy_kernel  # noqa: E402  (the stand-in for a user's own PD kernel)
from jaxsim_amd import _lib, runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="*", default=[1024, 65536])
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--model", default="icub23")
ap.add_argument("--envs-per-wave", type=int, nargs="*", default=[2, 4, 8, 16, 32])
args = ap.parse_args()

runtime.require_device()
lib = _lib.load()
policy_kernel.lib()
stream = runtime.Stream()
runtime.set_stream(stream)
model = bench.build_model(args.model)
dtype = np.float32
F32 = _lib.dtype_code(dtype)


print(f"# action-to-torque law, {args.model} synthetic humanoid, fp32, {args.reps} launches per figure (median [min .. max] of 5 windows), HIP events on the launch stream")
dm = runtime.device_model(model, dtype)
n = model.dofs()
spec = js.data.ActionSpec.build(model, dtype=dtype, kp=40.0, kd=2.0, scale=0.5, action_clip=1.0, clip_to_position_limits=True, torque_limit=80.0)
obs_spec = js.data.ObservationSpec.build(model, ["joint_positions", "joint_velocities"], dtype=dtype)
for N in args.envs:
    data = bench.synthetic_state(model, N, seed=0, dtype=dtype)
    st = data._state
    rows, tile = st.rows, st.tile
    rng = np.random.default_rng(0)
    actions = runtime.DeviceMatrix.from_host(rng.normal(0, 1, (N, n)).astype(np.float32))
    ff = runtime.DeviceArray.from_host(rng.uniform(-1, 1, (n, N)).astype(dtype), tile=tile)
    tau = runtime.DeviceArray(n, N, dtype, tile=tile, zero=True)
    major = runtime.DeviceMatrix(N, n, dtype)
    obs = data.observe(obs_spec)
    q0 = runtime.DeviceMatrix.from_host(np.zeros((1, n), np.float32))
    copy, work = runtime.DeviceArray.like(st), runtime.DeviceArray.like(st)
    sp, h = C.c_void_p(st.ptr), stream.handle
    table = spec._table(dm)
    vp = C.c_void_p

    def act(state_ptr, feed_forward):
        fp = None if feed_forward is None else vp(feed_forward.ptr)
        return lambda: lib.jxs_env_act(dm.handle, table, state_ptr, vp(actions.ptr), F32, n, fp, vp(tau.ptr), N, h)

    def tile_in():
        return lib.jxs_tile_from_env_major(vp(major.ptr), vp(tau.ptr), n, N, tile, F32, h)

    def user_route():
        policy_kernel.pd_torque(obs.ptr, obs_spec.size, q0.ptr, n, N, 40.0, 2.0, major.ptr, h)
        return tile_in()

    def step_only():
        return lib.jxs_step(dm.handle, vp(work.ptr), vp(work.ptr), vp(tau.ptr), None, int(data.velocity_representation), N, h)

    def act_and_step():
        rc = lib.jxs_env_act(dm.handle, table, vp(work.ptr), vp(actions.ptr), F32, n, None, vp(tau.ptr), N, h)
        return rc or step_only()

    print(f"# N = {N}: state block {st.nbytes / 1e6:.2f} MB = {-(-N // tile)} tiles of {rows} rows x {tile} columns; (a) reads {N * n * 4 * 3 / 1e6:.2f} MB "
          f"(actions, q, qdot) and writes {N * n * 4 / 1e6:.2f} MB; (c) reads and writes {N * n * 4 / 1e6:.2f} MB each")
    print(f"# {'operation':74s} {'us/launch':>10s} {'[min .. max]':>20s} {'M env/s':>9s} {'vs (c)':>7s} {'vs (e)':>7s}")
    cases = [
        ("(c) jxs_tile_from_env_major of an [N][23] tensor", 0, tile_in),
        ("(d) jxs_memcpy_d2d of the state block", 0, lambda: lib.jxs_memcpy_d2d(vp(copy.ptr), sp, st.nbytes, h)),
        ("(e) a user's PD kernel on an observation + jxs_tile_from_env_major", 0, user_route),
        ("(a) act, 23 position joints, the launcher's rule", 0, act(sp, None)),
        ("(b) act with a feed-forward block, the launcher's rule", 0, act(sp, ff)),
    ]
    for e in args.envs_per_wave:
        if e >= tile:
            cases.append((f"(a) act, {e} environments per wave", e, act(sp, None)))
    for e in args.envs_per_wave:
        if e >= tile:
            cases.append((f"(b) act with feed-forward, {e} environments per wave", e, act(sp, ff)))
    ref_c = ref_e = None
    for name, epw, call in cases:
        set_envs_per_wave("JXS_ACT_ENVS_PER_WAVE", epw)
        us, lo, hi = timed(stream, name, call, args.reps)
        ref_c = us if ref_c is None else ref_c
        ref_e = us if ref_e is None and name.startswith("(e)") else ref_e
        vs_e = "" if ref_e is None else f"{us / ref_e:7.2f}"
        print(f"  {name:74s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {vs_e:>7s}", flush=True)
    set_envs_per_wave("JXS_ACT_ENVS_PER_WAVE", 0)
    # per step: the step alone against act + step, both in place on a copy of the state (restored before each figure)
    for name, call in (("jxs_step in place with a torque block", step_only), ("act + jxs_step in place", act_and_step)):
        _lib.check(lib.jxs_memcpy_d2d(vp(work.ptr), sp, st.nbytes, h), "jxs_memcpy_d2d")
        _lib.check(lib.jxs_memset(vp(tau.ptr), 0, tau.nbytes, h), "jxs_memset")
        us, lo, hi = timed(stream, name, call, args.reps)
        print(f"  {name:74s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {us / ref_e:7.2f}", flush=True)

    # (f) the host route to the same torques: one download of the block per property, NumPy, the upload
    kp, kd, half = dtype(40.0), dtype(2.0), dtype(0.5)
    a_h = actions.to_host()

    def host_torques():
        data._invalidate_caches()
        q, qd = data.joint_positions.astype(dtype), data.joint_velocities.astype(dtype)
        t = np.clip(kp * (np.clip(a_h, -1, 1) * half - q) - kd * qd, -80, 80)
        return runtime.DeviceArray.from_host(np.ascontiguousarray(t.T), tile=tile)

    t = wall(stream, host_torques) * 1e6
    print(f"  {'(f) host properties + NumPy + upload (wall clock)':74s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.1f} {t / ref_e:7.1f}", flush=True)
    reps = 200
    t = wall(stream, lambda: [data.act(spec, actions, out=tau) for _ in range(reps)]) / reps * 1e6
    print(f"  {'(a) data.act(spec, actions, out=) through Python (wall clock)':74s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.2f} {t / ref_e:7.2f}", flush=True)
