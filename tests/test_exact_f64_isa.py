"""The ISA of the kernels of precision f64_exact, read from `make asm` -- no GPU needed.

symm64x_sweep_kernel (csrc/relax_symm64.h): twenty instances (ndim 2..6 x {threshold-free, threshold} x {plain, ERR}),
no scratch, the waves per SIMD its header states, the tile one basic block (the branch count of
test_f64_symmetric_sweep_instances_run_without_scratch).  slab_stage_exact_kernel (csrc/relax_exact.h): twenty-four
instances (the twelve tuned coordinate counts x {threshold-free, threshold}), no scratch, and the wait before the chunk
barrier counts exactly the younger loads -- twice the pipe kernel's, words and deltas (the check of
test_stage_kernel_awaits_its_lds_transfers_past_exactly_the_younger_loads on the new name).  The existing kernels keep
their instance counts: the exact forms have names of their own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def asm_text():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True)
    return open(os.path.join(csrc, "topolow_relax.gfx950.s")).read()


def _kernel(text, name):
    start = text.index("\n" + name + ":")
    end = text.index(".Lfunc_end", start)
    return text[start:end], text[end:][:3000]


def sweep_waves(dim):
    """relax_symm64.h: kSym64xWaves."""
    return 2 if dim <= 4 else 1


def test_exact_sweep_instances(asm_text):
    names = re.findall(r"^(_ZN7topolow20symm64x_sweep_kernelILi(\d+)ELb([01])ELb([01])E\w+):", asm_text, re.M)
    assert sorted((int(d), t, e) for _, d, t, e in names) == \
        [(d, t, e) for d in (2, 3, 4, 5, 6) for t in "01" for e in "01"]
    for name, dim, thr, err in names:
        body, tail = _kernel(asm_text, name)
        assert re.search(r"; ScratchSize: (\d+)", tail).group(1) == "0", name
        occ = int(re.search(r"; Occupancy: (\d+)", tail).group(1))
        print(name, "vgprs", re.search(r"; NumVgprs: (\d+)", tail).group(1), "occupancy", occ)
        assert occ >= sweep_waves(int(dim)), name
        assert body.count("s_cbranch") <= 19, (name, body.count("s_cbranch"))     # loops and guards only: the tile has no branch


def test_exact_stage_instances_await_their_lds_transfers_past_exactly_the_younger_loads(asm_text):
    names = re.findall(r"^(_ZN7topolow23slab_stage_exact_kernelILi(\d+)E\w+):", asm_text, re.M)
    assert len(names) == 24
    assert sorted({int(d) for _, d in names}) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16]
    for name, dim in names:
        body, tail = _kernel(asm_text, name)
        body = body.split("\n")
        waits = [q for q, l in enumerate(body) if "s_waitcnt vmcnt(" in l and "ASMSTART" in body[q - 1]]
        counts = [int(re.search(r"vmcnt\((\d+)\)", body[q]).group(1)) for q in waits]
        assert len(waits) == 2 and counts[0] == 0 and counts[1] > 0, (name, counts)   # prologue, loop
        q = waits[1]
        dma = max(i for i in range(q) if "global_load_lds_dwordx4" in body[i])
        assert dma > waits[0]                     # the loop's own transfer, not the prologue's
        younger = sum("buffer_load_dwordx4" in l for l in body[dma:q])
        assert younger == counts[1], (name, younger, counts[1])
        # words and deltas of GPC groups x 2 rows (PipeGeom: GPC = 10240 / (256 x ndim x 8) clamped to 1..4)
        gpc = min(4, max(1, 10240 // (256 * int(dim) * 8)))
        assert counts[1] == gpc * 2 * 2, (name, counts[1], gpc)
        assert re.search(r"; ScratchSize: (\d+)", tail).group(1) == "0", name
        occ = int(re.search(r"; Occupancy: (\d+)", tail).group(1))
        print(name, "vgprs", re.search(r"; NumVgprs: (\d+)", tail).group(1), "occupancy", occ)
        assert occ >= 1, name                     # relax_exact.h: one wave per SIMD, as the f64 pipe kernel


def test_existing_kernels_keep_their_instances(asm_text):
    assert len(re.findall(r"^_ZN7topolow22slab_stage_pipe_kernel\w+:", asm_text, re.M)) == 72
    assert len(re.findall(r"^_ZN7topolow19symm64_sweep_kernelILi\d+ELb[01]ELb[01]E\w+:", asm_text, re.M)) == 20
    assert len(re.findall(r"^_ZN7topolow17symm_sweep_kernelILi\d+ELb[01]ELb[01]E\w+:", asm_text, re.M)) == 20
