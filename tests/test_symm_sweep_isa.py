"""The ISA of the fp32 symmetric sweep (csrc/relax_symm.h), read from `make asm` -- no GPU needed.

What is checked, per instance (ndim 2..6 x {threshold-free, threshold} x {plain, ERR}):
  * the issue priority by work left: `s_setprio` with each of the levels 0..3, each behind a SCALAR branch (an
    `s_and_saveexec` in front of one would mean the compiler took the condition for divergent: the s_setprio then runs
    in every wave whatever the condition says);
  * none of them inside a column reduction (between the first and the last DPP add of one): the hazard spacing of the
    adds (tests/test_capi.py) is counted in instructions;
  * the head of a wave: at most two waits on scalar loads before the first vector memory instruction -- the kernel
    arguments in one batch, then the wave's run together with the stop flag (the kernel once had five, each behind the
    one before)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep_instances():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True)
    text = open(os.path.join(csrc, "topolow_relax.gfx950.s")).read()
    names = re.findall(r"^(_ZN7topolow17symm_sweep_kernelILi\d+ELb[01]ELb[01]E\w+):", text, re.M)
    assert len(names) == 20
    out = {}
    for name in names:
        start = text.index("\n" + name + ":")
        body = text[start:text.index(".Lfunc_end", start)]
        # instructions only: no comments, directives or labels
        out[name] = [ln.strip() for ln in body.split("\n")[2:]
                     if ln.strip() and not ln.strip().startswith((";", ".")) and not re.match(r"^\S+:", ln.strip())]
    return out


def test_every_priority_level_sits_behind_a_scalar_branch(sweep_instances):
    for name, lines in sweep_instances.items():
        prios = [k for k, ln in enumerate(lines) if ln.startswith("s_setprio")]
        levels = {int(lines[k].split()[1]) for k in prios}
        assert levels == {0, 1, 2, 3}, (name, levels)
        for k in prios:
            assert not any("s_and_saveexec" in ln for ln in lines[max(0, k - 3):k]), (name, lines[max(0, k - 3):k + 1])


def test_no_priority_change_inside_a_column_reduction(sweep_instances):
    for name, lines in sweep_instances.items():
        dim = int(re.search(r"kernelILi(\d+)E", name).group(1))
        dpp = [k for k, ln in enumerate(lines) if ln.startswith("v_add_f32_dpp")]
        assert dpp and len(dpp) % (3 * dim) == 0, name
        for q in range(0, len(dpp), 3 * dim):          # one reduction: three steps on ndim values
            first, last = dpp[q], dpp[q + 3 * dim - 1]
            assert not any(ln.startswith("s_setprio") for ln in lines[first:last + 1]), name


def test_a_wave_waits_twice_on_scalar_loads_before_its_first_vector_load(sweep_instances):
    vmem = ("buffer_load", "global_load", "flat_load", "buffer_store", "global_store", "flat_store")
    for name, lines in sweep_instances.items():
        waits, pending = 0, False
        for ln in lines:
            if ln.startswith(vmem):
                break
            if ln.startswith("s_load_"):
                pending = True
            elif ln.startswith("s_waitcnt") and "lgkmcnt" in ln and pending:
                waits += 1          # (scalar loads return out of order: any wait on one is a wait on all of them)
                pending = False
        else:
            raise AssertionError(name + ": no vector memory instruction")
        assert waits <= 2, (name, waits)
