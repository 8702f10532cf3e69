"""The step kernels on the host emulation, bit for bit against records made from the sources before the step kernel's
non-arithmetic glue (wait states, register shuffles, address arithmetic, lane-constant selects) was trimmed: none of that
may move a single bit of any state (tests/step_bitwise_cases.py holds the cases and the recorder)."""

import numpy as np
import pytest

import step_bitwise_cases as sbc


@pytest.fixture(scope="module")
def emulated(models):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = sbc.run_emul(case, models)
        return cache[case]

    return get


@pytest.mark.parametrize("case", list(sbc.CASES))
def test_step_is_bitwise_what_it_was(emulated, case):
    want = np.load(sbc.golden_path("emul", case))
    got = emulated(case)
    assert set(got) == set(want.files)
    for key in sorted(got):
        sbc.assert_bitwise(got[key], want[key], f"{case} {key}")


def test_cases_have_the_shapes_they_claim(models):
    """The last wave of every case is partly empty; the humanoid runs two waves with the second half empty (32 lanes per
    environment), the quadruped two with the last one quarter full (16 lanes per environment)."""
    import emul_binding as eb

    per_wave = {case: 64 // eb.layout(sbc.build_model(key, models), dtype).group for case, (key, dtype, *_) in sbc.CASES.items()}
    assert all(sbc.CASES[case][2] % n != 0 for case, n in per_wave.items()), per_wave
    assert per_wave["icub_f32"] == per_wave["icub_f64"] == 2 and sbc.CASES["icub_f32"][2] == 3
    assert per_wave["quadruped_rigid_f32"] == 4 and sbc.CASES["quadruped_rigid_f32"][2] == 5
