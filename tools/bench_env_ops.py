#!/usr/bin/env python3
"""The episode loop around `step`: reset, scatter and flag environments of a batch on the device (jxs_env_select,
jxs_env_copy, jxs_env_flags; JaxSimModelData.reset_where / put / env_flags), timed the way tools/bench_queries.py times
the query kernels: state resident in HBM, HIP events on the launch stream around `--reps` launches, 20 warm-up
launches, the median of 5 windows.  The 24-link humanoid of the headline (`bench.build_model`), fp32, N = 1024 and 65 536.

Two yardsticks stand next to the figures: a jxs_memcpy_d2d of the whole block (what "touch every word once" costs),
and the host round trip that was the only way to reset before (download, np.where per field, data.replace, upload:
wall clock with a device synchronisation).  The last lines are loops through the Python API, wall clock:
step(inplace=True) alone, and step + env_flags + reset_where(inplace=True) with the flags as the mask.

    python tools/bench_env_ops.py [--reps 300] [--loop-steps 2000] > profiles/env_ops.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from env_timing import timed, wall  # noqa: E402
import jaxsim_amd.api as js  # noqa: E402
from jaxsim_amd import _lib, runtime  # noqa: E402
from jaxsim_amd.model import VelRepr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="*", default=[1024, 65536])
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--loop-steps", type=int, default=2000)
ap.add_argument("--model", default="icub23")
args = ap.parse_args()

runtime.require_device()
lib = _lib.load()
stream = runtime.Stream()
runtime.set_stream(stream)
model = bench.build_model(args.model)
dtype = np.float32
F32 = _lib.dtype_code(dtype)


print(f"# per-environment operations, {args.model} synthetic humanoid, fp32, {args.reps} launches per figure (median [min .. max] of 5 windows), HIP events on the launch stream")
for N in args.envs:
    data = bench.synthetic_state(model, N, seed=0, dtype=dtype)
    fresh = bench.synthetic_state(model, N, seed=1, dtype=dtype)
    st, fr = data._state, fresh._state
    rows, tile = st.rows, st.tile
    block_mb = st.nbytes / 1e6
    rng = np.random.default_rng(0)
    K = max(1, N // 100)
    chosen = np.sort(rng.permutation(N)[:K])
    sparse_h = np.zeros(N, bool)
    sparse_h[chosen] = True
    sparse, full, none = (runtime.DeviceMask.from_host(m) for m in (sparse_h, np.ones(N, bool), np.zeros(N, bool)))
    idx = runtime.DeviceIndices.from_host(chosen)
    few = fresh.take(chosen)  # the K fresh states a scatter writes into the batch
    out = runtime.DeviceArray.like(st)
    flags = runtime.DeviceMask(N)
    dm = runtime.device_model(model, dtype)
    sp, fp, op, h = C.c_void_p(st.ptr), C.c_void_p(fr.ptr), C.c_void_p(out.ptr), stream.handle

    def select(mask, dst):
        return lambda: lib.jxs_env_select(C.c_void_p(mask.ptr), fp, sp, dst, rows, N, tile, F32, h)

    tiles = -(-N // tile)
    touched = len(np.unique(chosen // tile))
    print(f"# N = {N}: block {block_mb:.2f} MB = {tiles} tiles of {rows} rows x {tile} columns ({rows * tile * 4} B); the 1 % mask sets {K} environments in {touched} tiles")
    print(f"# {'operation':58s} {'us/launch':>10s} {'[min .. max]':>20s} {'M env/s':>9s} {'vs d2d':>7s}")
    cases = [
        ("jxs_memcpy_d2d of the whole block (yardstick)", lambda: lib.jxs_memcpy_d2d(op, sp, st.nbytes, h)),
        ("reset_where in place, no mask byte set", select(none, sp)),
        ("reset_where in place, 1 % of the mask set", select(sparse, sp)),
        ("reset_where in place, 100 % of the mask set", select(full, sp)),
        ("reset_where out of place, 1 % of the mask set", select(sparse, op)),
        ("put of 1 % of the environments (in place)",
         lambda: lib.jxs_env_copy(C.c_void_p(few._state.ptr), K, few._state.tile, None, sp, N, tile, C.c_void_p(idx.ptr), rows, K, F32, h)),
        ("env_flags", lambda: lib.jxs_env_flags(dm.handle, sp, N, C.c_void_p(flags.ptr), h)),
    ]
    d2d = None
    for name, call in cases:
        us, lo, hi = timed(stream, name, call, args.reps)
        d2d = us if d2d is None else d2d
        print(f"  {name:58s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / d2d:7.2f}", flush=True)

    # the way there was before: the whole block through the host (download, np.where per field, data.replace, upload)
    def host_reset():
        data._invalidate_caches()
        fresh._invalidate_caches()
        f, g = data._fields(), fresh._fields()
        pick = {k: np.where(sparse_h.reshape((-1,) + (1,) * (f[k].ndim - 1)), g[k], f[k]) for k in f}
        with data.switch_velocity_representation(VelRepr.Inertial):
            return data.replace(model, joint_positions=pick["joint_positions"], joint_velocities=pick["joint_velocities"],
                                base_quaternion=pick["base_quaternion"], base_linear_velocity=pick["base_linear_velocity"],
                                base_angular_velocity=pick["base_angular_velocity"], base_position=pick["base_position"],
                                contact_state={"tangential_deformation": pick["tangential_deformation"]})  # fmt: skip

    t = wall(stream, host_reset) * 1e6
    print(f"  {'data.replace round trip of the 1 % reset (host, wall clock)':58s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / d2d:7.0f}", flush=True)

    # loops through the Python API, wall clock: the bare step loop and the episode loop
    steps = args.loop_steps if N <= 4096 else max(50, args.loop_steps // 10)
    run = data.copy()

    def bare():
        for _ in range(steps):
            js.model.step(model, run, inplace=True)

    def episode():
        for _ in range(steps):
            js.model.step(model, run, inplace=True)
            run.reset_where(run.env_flags(), fresh, inplace=True)

    t_bare, t_epi = wall(stream, bare), wall(stream, episode)
    print(f"  {f'loop of {steps}: step(inplace=True)':58s} {t_bare / steps * 1e6:10.2f} {'':>20s} {N * steps / t_bare / 1e6:9.1f}")
    print(f"  {f'loop of {steps}: step + env_flags + reset_where(inplace=True)':58s} {t_epi / steps * 1e6:10.2f} {'':>20s} {N * steps / t_epi / 1e6:9.1f}", flush=True)
    bad = int(run.nonfinite_mask().sum())
    print(f"#   (after the loops {bad} of {N} environments are non-finite; every flagged one was reset from the fresh batch as it appeared)")
