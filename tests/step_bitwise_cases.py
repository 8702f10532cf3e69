"""TEST INFRASTRUCTURE: the cases of the bit-for-bit checks of the step kernels (tests/test_step_bitwise_cpu.py on the
host emulation, tests/test_step_bitwise_gpu.py on the device) and the recorder of their goldens.

A change of the step kernel that claims to leave every floating-point operation alone (integer / address / select /
wait-state glue only) must reproduce the state blocks recorded here from the sources BEFORE that change, bit for bit.
The goldens are not portable between the two backends: the host emulation rounds its transcendental functions with the
host's libm, the device with its own instructions, so each backend is compared with its own record:

    tests/golden/step_bitwise_emul_<case>.npz   python tests/step_bitwise_cases.py emul   (no GPU needed)
    tests/golden/step_bitwise_gpu_<case>.npz    python tests/step_bitwise_cases.py gpu library; ... gpu specialised
                                                (on an MI355X; the two kernel policies of tests/conftest.py)

Every case is a handful of environments whose last wave is partly empty; the humanoid and the quadruped run two waves.
"""

from __future__ import annotations

import pathlib
import sys

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

# name -> (model key, dtype, environments, steps, fused rollout too?)
#   icub:      iCub-23, default URDF (two sole boxes per foot), soft contacts, flat terrain: the description of the headline
#              kernel.  32 lanes per environment: N = 3 is two waves, the second half empty.  MODE_STEP (one launch per
#              step) and MODE_ROLLOUT (the fused loop)
#   quadruped: bench.build_quadruped_rigid (RigidContacts, one point per foot): MODE_STEP_RIGID.  16 lanes per environment:
#              N = 5 leaves the last wave one quarter full
#   cartpole:  fixed base
#   rk4:       the random floating 9-link chain of the zoo with RungeKutta4 (MODE_STEP_RK4)
CASES = {
    "icub_f32": ("icub", np.float32, 3, 3, True),
    "icub_f64": ("icub", np.float64, 3, 3, True),
    "quadruped_rigid_f32": ("quadruped_rigid", np.float32, 5, 2, False),
    "cartpole_f32": ("cartpole", np.float32, 3, 3, False),
    "rk4_chain9f_f32": ("rk4_chain9f", np.float32, 3, 2, False),
}


def build_model(key, zoo):
    import bench
    import parity_cases

    if key == "quadruped_rigid":
        return bench.build_quadruped_rigid()
    if key == "rk4_chain9f":
        return parity_cases.rk4(zoo("chain9f"))  # (a softer ground, inside the stability region of explicit RK4)
    return zoo(key)


def inputs(case, zoo):
    """(model, state block [rows, N], tau [N, n]) of a case: seeded, points in contact, random joint torques."""
    import helpers

    key, dtype, N, _, _ = CASES[case]
    model = build_model(key, zoo)
    zoo_name = {"quadruped_rigid": "anymal", "rk4_chain9f": "chain9f"}.get(key, key)
    d = zoo.random_data(zoo_name, N, seed=41, dtype=dtype)
    tau, _ = helpers.random_inputs(model, N, 42, dtype)
    return model, helpers.odata_to_block(model, d), tau


def run_emul(case, zoo):
    """{"step": state after `steps` single-step launches, "rollout": after one fused launch} on the host emulation."""
    import emul_binding as eb

    _, _, _, steps, fused = CASES[case]
    model, blk, tau = inputs(case, zoo)
    tau_rows = np.ascontiguousarray(tau.T)
    out = {}
    s = blk
    for _ in range(steps):
        s = eb.run(model, eb.MODE_STEP, s, tau=tau_rows)
    out["step"] = s
    if fused:
        out["rollout"] = eb.run(model, eb.MODE_STEP, blk, tau=tau_rows, n_steps=steps)
    return out


def run_gpu(case, zoo):
    """The same through the product on the device (js.model.step / js.model.rollout)."""
    import jaxsim_amd as ja
    import jaxsim_amd.api as js

    _, _, _, steps, fused = CASES[case]
    model, blk, tau = inputs(case, zoo)
    out = {}
    g = js.data.JaxSimModelData.from_state_block(model, blk, ja.VelRepr.Mixed)
    for _ in range(steps):
        g = js.model.step(model, g, joint_force_references=tau)
    out["step"] = g.state_block()
    if fused:
        g = js.data.JaxSimModelData.from_state_block(model, blk, ja.VelRepr.Mixed)
        out["rollout"] = js.model.rollout(model, g, steps, joint_force_references=tau).state_block()
    return out


def golden_path(backend, case):
    return GOLDEN / f"step_bitwise_{backend}_{case}.npz"


def assert_bitwise(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.isfinite(want).all(), what  # (a record of NaNs would compare nothing)
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    differ = got.view(bits) != want.view(bits)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} words differ, first at {tuple(np.argwhere(differ)[0])}"


def record(backend, policy=None, out_dir=None):
    """``emul``: one record per case.  ``gpu <policy>``: the arrays of one kernel policy of tests/conftest.py (`library`:
    the library's own kernels, `specialised`: the model-specialised object, which must have been pre-built), keys
    ``<policy>_step`` / ``<policy>_rollout``, merged into the case's file -- one process per policy.  ``out_dir``: write there instead of tests/golden."""
    import os

    here = pathlib.Path(__file__).resolve().parent
    for p in (str(here.parent), str(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    if backend == "gpu":
        os.environ["JAXSIM_AMD_SPECIALIZE"] = {"library": "0", "specialised": "require"}[policy]
    import helpers

    zoo = helpers.ModelZoo()
    for case in CASES:
        out = (run_emul if backend == "emul" else run_gpu)(case, zoo)
        assert all(np.isfinite(v).all() for v in out.values()), case
        path = pathlib.Path(out_dir or GOLDEN) / golden_path(backend, case).name
        if backend == "gpu":
            out = {f"{policy}_{k}": v for k, v in out.items()}
            if path.exists():
                out = {**dict(np.load(path)), **out}
        np.savez(path, **out)
        print(f"recorded {path.name}: " + ", ".join(f"{k}{v.shape}" for k, v in out.items()))


if __name__ == "__main__":
    record(*sys.argv[1:4])
