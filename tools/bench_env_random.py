#!/usr/bin/env python3
"""Random resets on the device (jxs_env_randomize; JaxSimModelData.reset_random_where) next to the reset from a fresh
block (jxs_env_select; reset_where), timed the way tools/bench_env_ops.py times the per-environment operations: state
resident in HBM, HIP events on the launch stream around `--reps` launches, 20 warm-up launches, the median of 5 windows.
The 24-link humanoid of the headline (`bench.build_model`), fp32, N = 1024 and 65 536, 0 %, 1 % and 100 % of the mask set.

Yardsticks measured in the same job: a jxs_memcpy_d2d of the whole block (what "touch every word once" costs), and the
host way to a randomised 1 % reset (random_model_data on the host, upload, reset_where: wall clock with a device
synchronisation).

    python tools/bench_env_random.py [--reps 300] > profiles/env_random.txt
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

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="*", default=[1024, 65536])
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--model", default="icub23")
args = ap.parse_args()

runtime.require_device()
lib = _lib.load()
stream = runtime.Stream()
runtime.set_stream(stream)
model = bench.build_model(args.model)
dtype = np.float32
F32 = _lib.dtype_code(dtype)


print(f"# random resets, {args.model} synthetic humanoid, fp32, {args.reps} launches per figure (median [min .. max] of 5 windows), HIP events on the launch stream")
dist = js.data.RandomStateDistribution.build(model, dtype=dtype)
dm = runtime.device_model(model, dtype)
for N in args.envs:
    data = bench.synthetic_state(model, N, seed=0, dtype=dtype)
    fresh = js.data.random_model_data_device(model, batch_size=N, dist=dist, seed=1)
    st, fr = data._state, fresh._state
    rows, tile = st.rows, st.tile
    rng = np.random.default_rng(0)
    K = max(1, N // 100)
    sparse_h = np.zeros(N, bool)
    sparse_h[np.sort(rng.permutation(N)[:K])] = True
    sparse, full, none = (runtime.DeviceMask.from_host(m) for m in (sparse_h, np.ones(N, bool), np.zeros(N, bool)))
    out = runtime.DeviceArray.like(st)
    sp, fp, op, bp, h = C.c_void_p(st.ptr), C.c_void_p(fr.ptr), C.c_void_p(out.ptr), C.c_void_p(dist.bounds_ptr), stream.handle
    draw = [0]

    def randomize(mask):
        def call():
            draw[0] += 1  # (a new draw per launch, as an episode loop passes it)
            return lib.jxs_env_randomize(dm.handle, None if mask is None else C.c_void_p(mask.ptr), sp, N, bp, 7, draw[0], 0, int(dist.velocity_representation), h)

        return call

    def select(mask):
        return lambda: lib.jxs_env_select(C.c_void_p(mask.ptr), fp, sp, sp, rows, N, tile, F32, h)

    print(f"# N = {N}: block {st.nbytes / 1e6:.2f} MB = {-(-N // tile)} tiles of {rows} rows x {tile} columns ({rows * tile * 4} B); the 1 % mask sets {K} environments; "
          f"{13 + 2 * dm.layout.n_joints} of the {rows} rows are sampled, the others are written as zero")
    print(f"# {'operation':62s} {'us/launch':>10s} {'[min .. max]':>20s} {'M env/s':>9s} {'vs d2d':>7s}")
    cases = [
        ("jxs_memcpy_d2d of the whole block (yardstick)", lambda: lib.jxs_memcpy_d2d(op, sp, st.nbytes, h)),
        ("reset_where in place, no mask byte set", select(none)),
        ("reset_where in place, 1 % of the mask set", select(sparse)),
        ("reset_where in place, 100 % of the mask set", select(full)),
        ("reset_random_where in place, no mask byte set", randomize(none)),
        ("reset_random_where in place, 1 % of the mask set", randomize(sparse)),
        ("reset_random_where in place, 100 % of the mask set", randomize(full)),
        ("reset_random_where in place, mask = None (every environment)", randomize(None)),
    ]
    d2d = None
    for name, call in cases:
        us, lo, hi = timed(stream, name, call, args.reps)
        d2d = us if d2d is None else d2d
        print(f"  {name:62s} {us:10.2f} {f'[{lo:.2f} .. {hi:.2f}]':>20s} {N / us:9.1f} {us / d2d:7.2f}", flush=True)

    # the host way to the same thing: sample on the host (NumPy), pack, tile, upload, then select on the device
    seed = [0]

    def host_reset():
        seed[0] += 1
        data.reset_where(sparse, js.data.random_model_data(model, batch_size=N, seed=seed[0], dtype=dtype), inplace=True)

    t = wall(stream, host_reset) * 1e6
    print(f"  {'host random_model_data + reset_where of the 1 % reset (wall clock)':62s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / d2d:7.0f}", flush=True)

    def device_reset():
        seed[0] += 1
        data.reset_random_where(sparse, dist, draw=seed[0], inplace=True)

    reps = 200
    t = wall(stream, lambda: [device_reset() for _ in range(reps)]) / reps * 1e6
    print(f"  {'reset_random_where of the 1 % reset through Python (wall clock)':62s} {t:10.1f} {'':>20s} {N / t:9.3f} {t / d2d:7.2f}", flush=True)
    bad = int(data.nonfinite_mask().sum())
    print(f"#   (after the resets {bad} of {N} environments are non-finite)")
