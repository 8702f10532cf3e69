#!/usr/bin/env python3
"""The policy observation on the device (jxs_env_observe; JaxSimModelData.observe), timed the way tools/bench_env_random.py
times the random reset: state resident in HBM, HIP events on the launch stream around `--reps` launches, 20 warm-up
launches, the median of 5 windows.  The 24-link humanoid of the headline (`bench.build_model`), fp32, N = 1024 and 65 536:

  (a) a 60-wide proprioceptive observation: q 23, qdot 23, unit quaternion 4, Body velocity 6, projected gravity 3, height 1;
  (b) the same plus the 24 rows of a centroidal record as a source (84 wide);
  (c) jxs_tile_to_env_major of the whole block -- the only device-side exit there was;
  (d) jxs_memcpy_d2d of the block (what "touch every word once" costs);
  (e) the host path: data.joint_positions, joint_velocities, base_orientation, base_velocity, the projected gravity from
      base_transform, the height and the NumPy concatenation (wall clock, with the download).

(a) and (b) are also run with the launcher's environments-per-wave rule overridden (JXS_OBSERVE_ENVS_PER_WAVE), which is how
the rule was chosen.

    python tools/bench_env_observe.py [--reps 300] > profiles/env_observe.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


PROPRIO = ["joint_positions", "joint_velocities", "base_orientation", "base_velocity", "projected_gravity", "base_height"]
print(f"# policy observation, {args.model} synthetic humanoid, fp32, {args.reps} launches per figure (median [min .. max] of 5 windows), HIP events on the launch stream")
dm = runtime.device_model(model, dtype)
spec_a = js.data.ObservationSpec.build(model, PROPRIO, dtype=dtype, velocity_representation=ja.VelRepr.Body)
spec_b = js.data.ObservationSpec.build(model, PROPRIO + [("source", dict(name="centroidal", rows=js.com.ROWS))], dtype=dtype,
                                       velocity_representation=ja.VelRepr.Body)  # fmt: skip
for N in args.envs:
    data = bench.synthetic_state(model, N, seed=0, dtype=dtype)
    st = data._state
    rows, tile = st.rows, st.tile
    rec = js.com.centroidal_quantities(model, data)
    out_a, out_b = runtime.DeviceMatrix(N, spec_a.size, dtype), runtime.DeviceMatrix(N, spec_b.size, dtype)
    major = runtime.DeviceMatrix(N, rows, dtype)
    copy = runtime.DeviceArray.like(st)
    sp, h = C.c_void_p(st.ptr), stream.handle
    src_b = (C.c_void_p * 4)(rec.ptr)
    none = (C.c_void_p * 4)()
    body = int(ja.VelRepr.Body)

    def observe(spec, out, sources):
        table, optr = spec._table(dm), C.c_void_p(out.ptr)
        return lambda: lib.jxs_env_observe(dm.handle, table, sp, sources, N, body, optr, F32, spec.size, h)

    print(f"# N = {N}: block {st.nbytes / 1e6:.2f} MB = {-(-N // tile)} tiles of {rows} rows x {tile} columns; (a) writes {N * spec_a.size * 4 / 1e6:.2f} MB "
          f"({spec_a.size} columns), (b) {N * spec_b.size * 4 / 1e6:.2f} MB ({spec_b.size} columns), (c) {N * rows * 4 / 1e6:.2f} MB")
    print(f"# {'operation':66s} {'us/launch':>10s} {'[min .. max]':>20s} {'M env/s':>9s} {'vs (c)':>7s} {'vs (d)':>7s}")
    cases = [
        ("(c) jxs_tile_to_env_major of the whole block", None, lambda: lib.jxs_tile_to_env_major(sp, C.c_void_p(major.ptr), rows, N, tile, F32, h)),
        ("(d) jxs_memcpy_d2d of the whole block", None, lambda: lib.jxs_memcpy_d2d(C.c_void_p(copy.ptr), sp, st.nbytes, h)),
        ("(a) observe, 60 wide, the launcher's rule", None, observe(spec_a, out_a, none)),
        ("(b) observe, 84 wide with a 24-row source, the launcher's rule", None, observe(spec_b, out_b, src_b)),
    ]
    for e in args.envs_per_wave:
        if e >= tile:
            cases.append((f"(a) observe, 60 wide, {e} environments per wave", e, observe(spec_a, out_a, none)))
    for e in args.envs_per_wave:
        if e >= tile:
            cases.append((f"(b) observe, 84 wide, {e} environments per wave", e, observe(spec_b, out_b, src_b)))
    ref_c = ref_d = None
    for name, knob, call in cases:
        set_envs_per_wave("JXS_OBSERVE_ENVS_PER_WAVE", knob)
        us, lo, hi = timed(stream, name, call, args.reps)
        ref_c = us if ref_c is None else ref_c
        ref_d = us if ref_d is None and name.startswith("(d)") else ref_d
        vs_d = "" if ref_d is None else f"{us / ref_d:7.2f}"
        print(f"  {name:66s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / ref_c:7.2f} {vs_d:>7s}", flush=True)
    set_envs_per_wave("JXS_OBSERVE_ENVS_PER_WAVE", None)

    # (e) the host path to the same 60 numbers per environment: one download of the block, the properties, the concatenation
    def host_observation():
        data._invalidate_caches()
        with data.switch_velocity_representation(ja.VelRepr.Body):
            v = data.base_velocity
        R = data.base_transform[:, :3, :3]
        return np.concatenate([data.joint_positions, data.joint_velocities, data.base_orientation, v, -R[:, 2, :], data.base_position[:, 2:3]], axis=1)

    t = wall(stream, host_observation) * 1e6
    print(f"  {'(e) host properties + NumPy concatenation (wall clock)':66s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.1f} {t / ref_d:7.1f}", flush=True)
    reps = 200
    t = wall(stream, lambda: [data.observe(spec_a, out=out_a) for _ in range(reps)]) / reps * 1e6
    print(f"  {'(a) data.observe(spec, out=) through Python (wall clock)':66s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / ref_c:7.2f} {t / ref_d:7.2f}", flush=True)
    got, want = out_a.to_host(), host_observation()
    print(f"#   (largest difference between (a) and (e): {float(np.abs(got.astype(np.float64) - want).max()):.2e})")
