"""The step kernels on the device, bit for bit against records made on an MI355X from the sources before the step
kernel's non-arithmetic glue was trimmed (tests/step_bitwise_cases.py: same cases and sizes as the host-emulation test).
Both kernel policies of tests/conftest.py run: the library's own kernels and the pre-built model-specialised objects --
the iCub case is the description of the headline kernel.  A few launches of at most five environments each."""

import numpy as np
import pytest

import step_bitwise_cases as sbc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(sbc.CASES))
def test_step_is_bitwise_what_it_was_gpu(models, kernel_policy, case):
    want = np.load(sbc.golden_path("gpu", case))
    got = sbc.run_gpu(case, models)
    assert {f"{kernel_policy}_{k}" for k in got} <= set(want.files)
    for key in sorted(got):
        sbc.assert_bitwise(got[key], want[f"{kernel_policy}_{key}"], f"{case} {kernel_policy} {key}")
