"""The ISA of the symmetric sweep for ndim 7..10 (csrc/relax_symm_wide.h), read from `make asm` -- no GPU needed.

Per instance (ndim 7..10 x {threshold-free, threshold} x {plain, ERR}): no scratch, the waves per SIMD the kernel's
header states (two, for all of them), the one-instruction DPP column reduction (three steps on ndim values per half
tile) with its hazard spacing, and the issue priority by work left behind scalar branches -- the checks of
tests/test_symm_sweep_isa.py and tests/test_capi.py on the new names.  The register-tiled kernel keeps its twenty
instances (ndim 2..6): it was not instantiated for the new dims."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCCUPANCY = {dim: 2 for dim in (7, 8, 9, 10)}          # relax_symm_wide.h: "Waves per SIMD"


@pytest.fixture(scope="module")
def asm_text():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True)
    return open(os.path.join(csrc, "topolow_relax.gfx950.s")).read()


@pytest.fixture(scope="module")
def wide_instances(asm_text):
    names = re.findall(r"^(_ZN7topolow22symm_sweep_wide_kernelILi(\d+)ELb([01])ELb([01])E\w+):", asm_text, re.M)
    out = {}
    for name, dim, thr, err in names:
        start = asm_text.index("\n" + name + ":")
        end = asm_text.index(".Lfunc_end", start)
        body = asm_text[start:end]
        lines = [ln.strip() for ln in body.split("\n")[2:]
                 if ln.strip() and not ln.strip().startswith((";", ".")) and not re.match(r"^\S+:", ln.strip())]
        out[name] = dict(dim=int(dim), thr=thr == "1", err=err == "1", lines=lines, tail=asm_text[end:][:3000])
    return out


def test_sixteen_instances_of_the_wide_kernel_and_twenty_of_the_register_tiled_one(asm_text, wide_instances):
    assert len(wide_instances) == 16
    assert sorted({(v["dim"], v["thr"], v["err"]) for v in wide_instances.values()}) == \
        [(d, t, e) for d in (7, 8, 9, 10) for t in (False, True) for e in (False, True)]
    assert len(re.findall(r"^_ZN7topolow17symm_sweep_kernelILi\d+ELb[01]ELb[01]E\w+:", asm_text, re.M)) == 20
    assert len(re.findall(r"^_ZN7topolow19symm64_sweep_kernelILi\d+ELb[01]ELb[01]E\w+:", asm_text, re.M)) == 20


def test_no_scratch_and_the_stated_waves_per_simd(wide_instances):
    for name, v in wide_instances.items():
        assert re.search(r"; ScratchSize: (\d+)", v["tail"]).group(1) == "0", name
        assert int(re.search(r"; Occupancy: (\d+)", v["tail"]).group(1)) >= OCCUPANCY[v["dim"]], name


def test_column_reduction_is_three_dpp_steps_on_ndim_values(wide_instances):
    for name, v in wide_instances.items():
        lines, dim = v["lines"], v["dim"]
        dpp = [k for k, ln in enumerate(lines) if ln.startswith("v_add_f32_dpp")]
        assert dpp and len(dpp) % (3 * dim) == 0, (name, len(dpp))
        for q in range(0, len(dpp), 3 * dim):
            first, last = dpp[q], dpp[q + 3 * dim - 1]
            assert not any(ln.startswith("s_setprio") for ln in lines[first:last + 1]), name
        # DPP hazard: a VGPR written by a vector instruction may be read through DPP only two wait states later; the adds
        # are inline asm, so the compiler neither knows nor pads -- no instruction among the two before a DPP add may
        # write the register it reads through DPP (an s_nop counts as wait states)
        for k in dpp:
            src = int(re.match(r"v_add_f32_dpp v\d+, v(\d+), v\d+", lines[k]).group(1))
            waits = 0
            for prev in reversed(lines[max(0, k - 4):k]):
                if waits >= 2:
                    break
                nop = re.match(r"s_nop (\d+)", prev)
                if nop:
                    waits += int(nop.group(1)) + 1
                    continue
                w = re.match(r"v_\w+ v(\d+)|v_\w+ v\[(\d+):(\d+)\]", prev)
                if w:
                    lo = int(w.group(1) or w.group(2))
                    hi = int(w.group(1) or w.group(3))
                    assert not (lo <= src <= hi), (name, prev, lines[k])
                waits += 1


def test_every_priority_level_sits_behind_a_scalar_branch(wide_instances):
    for name, v in wide_instances.items():
        lines = v["lines"]
        prios = [k for k, ln in enumerate(lines) if ln.startswith("s_setprio")]
        levels = {int(lines[k].split()[1]) for k in prios}
        assert levels == {0, 1, 2, 3}, (name, levels)
        for k in prios:
            assert not any("s_and_saveexec" in ln for ln in lines[max(0, k - 3):k]), (name, lines[max(0, k - 3):k + 1])


def test_a_wave_waits_twice_on_scalar_loads_before_its_first_vector_load(wide_instances):
    vmem = ("buffer_load", "global_load", "flat_load", "buffer_store", "global_store", "flat_store")
    for name, v in wide_instances.items():
        waits, pending = 0, False
        for ln in v["lines"]:
            if ln.startswith(vmem):
                break
            if ln.startswith("s_load_"):
                pending = True
            elif ln.startswith("s_waitcnt") and "lgkmcnt" in ln and pending:
                waits += 1
                pending = False
        else:
            raise AssertionError(name + ": no vector memory instruction")
        assert waits <= 2, (name, waits)
