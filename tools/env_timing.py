"""The timing loops that tools/bench_env_ops.py, bench_env_random.py, bench_env_observe.py and bench_env_act.py share, so
that their figures (profiles/env_*.txt) are taken the same way."""
import os
import time

import numpy as np

from jaxsim_amd import _lib, runtime


def timed(stream, name, call, reps):
    """us per launch: HIP events around `reps` launches, after 20 warm-up launches; the median of 5 windows."""
    for _ in range(20):
        _lib.check(call(), name)
    stream.synchronize()
    windows = []
    for _ in range(5):
        e0, e1 = runtime.Event(), runtime.Event()
        e0.record(stream)
        for _ in range(reps):
            _lib.check(call(), name)
        e1.record(stream)
        stream.synchronize()
        windows.append(e0.elapsed_ms(e1) / reps * 1e3)
    return float(np.median(windows)), float(min(windows)), float(max(windows))


def wall(stream, loop, repeats=3):
    """Seconds of `loop()` including the device synchronisation behind it; the median of `repeats` after one warm-up."""
    loop()
    stream.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        loop()
        stream.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def set_envs_per_wave(knob_name, value):
    """Override a launcher's environments-per-wave rule (JXS_OBSERVE_ENVS_PER_WAVE, JXS_ACT_ENVS_PER_WAVE); None or 0 gives
    the rule back.  The library reads its knobs once per process, so it is told to read them again."""
    if not value:
        os.environ.pop(knob_name, None)
    else:
        os.environ[knob_name] = str(value)
    _lib.check(_lib.load().jxs_debug_reload_env(), "jxs_debug_reload_env")
