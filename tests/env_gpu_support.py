"""TEST INFRASTRUCTURE: what the GPU tests of the per-environment operations (tests/test_env_*_gpu.py) share -- bitwise
comparisons, blocks with guard or NaN words around them inside one allocation, the humanoid's state on the device.  No test
and no fixture lives here.  Two namesakes differ on purpose and stay where they are: ``same_words`` of
tests/env_cpu_support.py takes two NaNs for the same word (the contract of the action law), the one here compares every
byte; ``upload_raw`` of tests/test_env_ops_gpu.py fills a tiled block, ``upload_flat`` here a flat one."""

import ctypes as C

import numpy as np

import env_ops_ref as ref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import step_bitwise_cases as sbc
from jaxsim_amd import _lib
from jaxsim_amd.runtime import DeviceArray

DTYPES = (np.float32, np.float64)
MODELS = ("icub", "quadruped_rigid", "cartpole", "box")  # humanoid (T = 2), quadruped, fixed base, no joints
GUARD = 64  # words of pattern in front of and behind a destination block
PAD = 64  # words of NaN in front of and behind a source block
CONTACT = dict(base_pos_bounds=((-1, -1, 0.56), (1, 1, 0.68)), base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3)))  # the humanoid on its feet


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    differ = got.view(ref.bits_dtype(got.dtype)) != want.view(ref.bits_dtype(want.dtype))
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} words differ, first at {int(np.argmax(differ))}"


def same_words(got, want, what):
    """``assert_same_bits`` for words of any size (the done bytes too)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    differ = got.view(np.uint8) != want.view(np.uint8)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} bytes differ, first at {int(np.argmax(differ))}"


def upload_flat(a) -> DeviceArray:
    out = DeviceArray(1, a.size, a.dtype, tile=1)
    _lib.check(_lib.load().jxs_memcpy_h2d(C.c_void_p(out.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, None), "h2d")
    return out


class Guarded:
    """A destination vector of any word size with GUARD words of a pattern (every byte 0xA5) on both sides, all inside one
    allocation."""

    def __init__(self, flat):
        self.dtype, self.n = flat.dtype, flat.shape[0]
        self.pattern = np.full(GUARD * flat.dtype.itemsize, 0xA5, dtype=np.uint8).view(flat.dtype)
        host = np.concatenate([self.pattern, flat, self.pattern])
        self.buf = DeviceArray(1, host.shape[0], flat.dtype, tile=1)
        _lib.check(_lib.load().jxs_memcpy_h2d(C.c_void_p(self.buf.ptr), host.ctypes.data_as(C.c_void_p), host.nbytes, None), "h2d")

    @property
    def ptr(self):
        return self.buf.ptr + GUARD * self.dtype.itemsize

    def block(self):
        """The block, after checking that both guards still hold the pattern."""
        host = self.buf.to_host_raw().reshape(-1)
        same_words(host[:GUARD], self.pattern, "words in FRONT of the destination block were written")
        same_words(host[GUARD + self.n :], self.pattern, "words BEHIND the destination block were written")
        return host[GUARD : GUARD + self.n]


class InNaN:
    """A read-only block inside one allocation whose words in front of and behind it are NaN."""

    def __init__(self, flat):
        nan = np.full(PAD, np.nan, dtype=flat.dtype)
        self.buf = upload_flat(np.concatenate([nan, flat, nan]))
        self.ptr = self.buf.ptr + PAD * flat.dtype.itemsize


def icub_data(models, N, dtype, *, rep=ja.VelRepr.Mixed, seed=41):
    model = sbc.build_model("icub", models)
    blk = helpers.odata_to_block(model, models.random_data("icub", N, seed=seed, dtype=dtype))
    return model, blk, js.data.JaxSimModelData.from_state_block(model, blk, rep)
