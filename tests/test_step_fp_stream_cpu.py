"""The floating-point instruction stream and the resource budget of the headline kernel (iCub-23, soft contacts, flat
terrain, fp32, MODE_STEP, model-specialised), read from its gfx950 disassembly -- no GPU needed, hipcc cross-compiles.

Work on the step kernel's non-arithmetic glue (wait states, register shuffles, address arithmetic, lane-constant selects)
promises to leave every floating-point instruction alone.  This test holds it to that: the multiset of floating-point
opcodes equals the record of tests/golden/step_fp_opcodes_icub23_f32.json, made from the sources before that work
(`python tests/test_step_fp_stream_cpu.py record`), no LDS or global-memory opcode occurs more often than it did (one more
global_load_dwordx4 is allowed: a table load of the prologue), and the kernel keeps the budget that three resident waves
per SIMD at large batches depend on: at most 168 VGPRs, no scratch, the same LDS bytes."""

import collections
import json
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "step_fp_opcodes_icub23_f32.json"
MAX_VGPRS = 168


def _is_fp(op: str) -> bool:
    """v_*_f32 / _f64 / _f16 arithmetic (plain, DPP, packed), reciprocals and square roots, conversions, float compares."""
    return op.startswith("v_") and re.search(r"_f(16|32|64)", op) is not None


def _norm(op: str) -> str:
    return re.sub(r"_e(32|64)$", "", op)  # (the encoding follows the operands' registers, the operation does not)


def headline_figures():
    """{"fp": {opcode: count}, "mem": {ds_* / global_* opcode: count}, "vgprs", "agprs", "scratch", "lds"} of the step kernel
    of the headline description."""
    import helpers
    from jaxsim_amd import isa_lint, specialize

    model = helpers.ModelZoo()("icub")  # default URDF, two sole boxes per foot, flat terrain
    path = specialize.compile(model, np.float32, specialize.MODE_STEP)  # (found in the cache after build())
    found = None
    for elf in isa_lint.code_objects(str(path)):
        for sym, insts in isa_lint.parse(isa_lint.disassemble(elf)).items():
            if "jxs_kernel" in sym and "duo" not in sym:
                assert found is None, "more than one step kernel in " + str(path)
                found = (sym, insts, elf)
    assert found is not None, "no step kernel in " + str(path)
    sym, insts, elf = found
    fp = collections.Counter(_norm(i.op) for i in insts if _is_fp(i.op))
    mem = collections.Counter(i.op for i in insts if i.op.startswith(("ds_", "global_", "buffer_", "flat_", "scratch_")))
    readelf = str(pathlib.Path(isa_lint.OBJDUMP).with_name("llvm-readelf"))
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(elf)
        f.flush()
        notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    # the metadata entry of this kernel: the item of `amdhsa.kernels` that holds `.name: <sym>`
    blocks = [b for b in re.split(r"\n  - ", notes) if re.search(rf"\.name:\s+{re.escape(sym)}\s", b + "\n")]
    assert len(blocks) == 1, (sym, len(blocks))

    def field(key):
        return int(re.search(rf"\.{key}:\s+(\d+)", blocks[0]).group(1))

    return {"fp": dict(sorted(fp.items())), "mem": dict(sorted(mem.items())), "vgprs": field("vgpr_count"), "agprs": field("agpr_count"),
            "scratch": field("private_segment_fixed_size"), "lds": field("group_segment_fixed_size"), "instructions": len(insts)}


@pytest.fixture(scope="module")
def figures():
    from jaxsim_amd import isa_lint, specialize

    if not (specialize.hipcc_available() and isa_lint.available()):
        pytest.skip("no hipcc / llvm-objdump: the headline kernel cannot be cross-compiled here")
    return headline_figures()


def test_fp_opcode_multiset_is_the_recorded_one(figures):
    want = json.loads(GOLDEN.read_text())["fp"]
    got = figures["fp"]
    diff = {op: (want.get(op, 0), got.get(op, 0)) for op in sorted(set(want) | set(got)) if want.get(op, 0) != got.get(op, 0)}
    assert not diff, f"floating-point opcodes (recorded, now): {diff}"


def test_memory_opcodes_do_not_grow(figures):
    want = json.loads(GOLDEN.read_text())["mem"]
    allowed_extra = {"global_load_dwordx4": 1}  # one more wide table load per lane in the prologue
    grown = {op: (want.get(op, 0), n) for op, n in figures["mem"].items() if n > want.get(op, 0) + allowed_extra.get(op, 0)}
    assert not grown, f"LDS / memory opcodes that occur more often (recorded, now): {grown}"


def test_resource_budget(figures):
    want = json.loads(GOLDEN.read_text())
    assert figures["vgprs"] + figures["agprs"] <= MAX_VGPRS, figures
    assert figures["scratch"] == 0, figures
    assert figures["lds"] == want["lds"], (figures["lds"], want["lds"])


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    here = pathlib.Path(__file__).resolve().parent
    sys.path[:0] = [str(here.parent), str(here)]
    GOLDEN.write_text(json.dumps(headline_figures(), indent=1) + "\n")
    print(GOLDEN.read_text())
