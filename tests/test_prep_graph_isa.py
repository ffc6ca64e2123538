"""The resources of the graph kernels (csrc/relax_prep_graph.h), read from `make asm` -- no GPU needed: each of the
four is compiled once, uses no scratch, and fits enough waves on a SIMD that a 256-thread workgroup (one wave per
SIMD) is far from the limit."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("graph_bits_kernel", "graph_jump_kernel", "graph_hook_kernel", "graph_gather_kernel")


@pytest.fixture(scope="module")
def asm_text():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True)
    return open(os.path.join(csrc, "topolow_relax.gfx950.s")).read()


def _kernel(text, name):
    start = text.index("\n" + name + ":")
    end = text.index(".Lfunc_end", start)
    return text[start:end], text[end:][:3000]


@pytest.mark.parametrize("kernel", KERNELS)
def test_graph_kernels_use_no_scratch(asm_text, kernel):
    names = re.findall(r"^(_ZN7topolow\d+%s\w+):" % kernel, asm_text, re.M)
    assert len(names) == 1, names
    _, tail = _kernel(asm_text, names[0])
    assert re.search(r"; ScratchSize: (\d+)", tail).group(1) == "0", kernel
    occ = int(re.search(r"; Occupancy: (\d+)", tail).group(1))
    print(kernel, "vgprs", re.search(r"; NumVgprs: (\d+)", tail).group(1), "sgprs",
          re.search(r"; TotalNumSgprs: (\d+)", tail).group(1), "occupancy", occ)
    assert occ >= 4, kernel                                  # small kernels: latency is hidden by waves, not by unrolling
    lds = int(re.search(r"; LDSByteSize: (\d+)", tail).group(1))
    assert lds <= 16, (kernel, lds)                          # graph_bits_kernel: two words; the others none


def test_the_rounds_hook_with_vector_atomics_and_wait_for_nobody(asm_text):
    body, _ = _kernel(asm_text, re.search(r"^(_ZN7topolow\d+graph_hook_kernel\w+):", asm_text, re.M).group(1))
    assert "global_atomic_smin" in body                      # atomicMin on the larger root's entry
    assert "s_sleep" not in body and "s_barrier" not in body # no spinning, no barrier: a line's wave works alone
    body, _ = _kernel(asm_text, re.search(r"^(_ZN7topolow\d+graph_jump_kernel\w+):", asm_text, re.M).group(1))
    assert "s_sleep" not in body and "s_barrier" not in body and "atomic" not in body
