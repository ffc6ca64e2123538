"""The degrees and prune entries of a prepared handle without a device: declared, exported, ctypes signatures, the
info struct as a C compiler lays it out, the Python surface, and every TOPOLOW_ERR_BAD_ARGUMENT case -- each found
before any device call, so this runs on a box with or without a GPU.  As in tests/test_subsample_capi.py the argument
rules read one thing of a handle, its n, the first field of the struct: the stand-in handle is zeroed memory with n
written at its start, which nothing else may read."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from topolow_amd import _native, prune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_layout_prep_degrees", "topolow_layout_prep_prune")
BAD = _native.ERR_BAD_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    for k, name in enumerate(("CONVERGED", "MIN_POINTS", "MAX_ITERATIONS", "ALL_REMOVED"), start=1):
        assert re.search(r"#define TOPOLOW_PRUNE_%s %d\b" % (name, k), header) and getattr(prune, name) == k
    assert re.search(r"#define TOPOLOW_PRUNE_MAX_ATTEMPTS %d\b" % _native.PRUNE_MAX_ATTEMPTS, header)
    assert prune.MAX_ATTEMPTS == _native.PRUNE_MAX_ATTEMPTS == 10


def test_ctypes_signatures_and_the_python_surface():
    lib = _native.load()
    assert len(lib.topolow_layout_prep_degrees.argtypes) == 7
    assert len(lib.topolow_layout_prep_prune.argtypes) == 9
    for name in SYMBOLS:
        assert getattr(lib, name).restype is C.c_int
    for name in ("degrees", "prune"):
        assert callable(getattr(_native.PreparedHandle, name)), name


def test_info_struct_matches_the_header(tmp_path):
    """344 bytes: 8 int32, 2 int64, 3 doubles, 4 x 10 int32, 10 int64, 4 int64 reserved -- in the ctypes twin and in
    the header as a C compiler reads it, with the offsets of a field of every group."""
    T = _native.TopolowPruneInfo
    assert C.sizeof(T) == 8 * 4 + 2 * 8 + 3 * 8 + 4 * 10 * 4 + 10 * 8 + 4 * 8 == 344
    fields = ("stop_reason", "last_remove", "original_cells", "seconds", "attempt_iterations", "attempt_final_size",
              "attempt_final_cells", "reserved")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "topolow_relax.h"\n'
                   'int main(void) { printf("%zu", sizeof(topolow_prune_info));\n'
                   + "".join('printf(" %%zu", offsetof(topolow_prune_info, %s));\n' % f for f in fields)
                   + 'return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["344"] + [str(getattr(T, f).offset) for f in fields]


def test_the_kernels_live_in_a_header_of_their_own_that_the_library_includes():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "relax_prep_prune.h"))
    sources = glob.glob(os.path.join(csrc, "*.hip"))   # exactly one source compiles the kernels
    assert sum('#include "relax_prep_prune.h"' in open(s).read() for s in sources) == 1


class _StandIn:
    """Zeroed memory with `n` at its start, and the arguments of the two entries around it."""

    def __init__(self, n):
        self.lib = _native.load()
        self.mem = np.zeros(4096, dtype=np.int32)
        self.mem[0] = n
        self.handle = self.mem.ctypes.data_as(C.c_void_p)
        self.err = C.create_string_buffer(256)
        self.deg = np.zeros(max(n, 1), dtype=np.int32)
        self.cells = C.c_int64(0)
        self.kept = np.zeros(max(n, 1), dtype=np.uint8)
        self.info = _native.TopolowPruneInfo()

    def degrees(self, subset, m=None, handle="own", deg="own", cells="own"):
        a = np.ascontiguousarray(subset, dtype=np.int32) if subset is not None else None
        self.err.value = b""
        self._keep = a
        return self.lib.topolow_layout_prep_degrees(
            self.handle if handle == "own" else None, _native._ip(a) if a is not None else None,
            (a.shape[0] if a is not None else 0) if m is None else m, _native._ip(self.deg) if deg == "own" else None,
            C.byref(self.cells) if cells == "own" else None, self.err, len(self.err))

    def prune(self, min_connections=4, target=float("nan"), max_iterations=100, min_points=10, handle="own", kept="own",
              info="own"):
        self.err.value = b""
        return self.lib.topolow_layout_prep_prune(
            self.handle if handle == "own" else None, min_connections, target, max_iterations, min_points,
            self.kept.ctypes.data_as(C.POINTER(C.c_uint8)) if kept == "own" else None,
            C.byref(self.info) if info == "own" else None, self.err, len(self.err))


def test_null_arguments():
    s = _StandIn(20)
    for kw in (dict(handle=None), dict(deg=None), dict(cells=None)):
        assert s.degrees([3, 1, 2], **kw) == BAD, kw
        assert b"NULL" in s.err.value, kw
    assert s.degrees(None, handle=None) == BAD
    for kw in (dict(handle=None), dict(kept=None), dict(info=None)):
        assert s.prune(**kw) == BAD, kw
        assert b"NULL" in s.err.value, kw


@pytest.mark.parametrize("subset,m,word", [
    ([4], None, b"between 2 and"),
    ([4, 5], 1, b"between 2 and"),
    ([4, 5], -3, b"between 2 and"),
    (list(range(10)) + [0], None, b"between 2 and"),
    ([0, 10], None, b"out of range"),
    ([0, -1], None, b"out of range"),
    ([7, 2, 2 ** 31 - 1], None, b"out of range"),
    ([1, 2, 1], None, b"repeated"),
])
def test_degrees_checks_the_subset_before_any_device_call(subset, m, word):
    s = _StandIn(10)
    assert s.degrees(subset, m) == BAD
    assert word in s.err.value, s.err.value


@pytest.mark.parametrize("kw,text", [
    (dict(min_connections=0), b"min_connections must be a positive integer"),
    (dict(min_connections=-4), b"min_connections must be a positive integer"),
    (dict(target=0.0), b"target_completeness must be between 0 and 1"),
    (dict(target=-0.25), b"target_completeness must be between 0 and 1"),
    (dict(target=1.0000001), b"target_completeness must be between 0 and 1"),
    (dict(target=float("inf")), b"target_completeness must be between 0 and 1"),
    (dict(min_points=21), b"Matrix size (20) is smaller than min_points (21)"),
    (dict(min_points=21, min_connections=0, target=5.0), b"Matrix size (20) is smaller than min_points (21)"),
    (dict(min_connections=0, target=5.0), b"min_connections must be a positive integer"),
])
def test_prune_checks_its_arguments_before_any_device_call(kw, text):
    s = _StandIn(20)
    assert s.prune(**kw) == BAD
    assert s.err.value == text
    assert not s.kept.any() and s.info.original_size == 0          # nothing was written


def test_python_argument_errors_need_no_device():
    class Fake:
        n = 7

    D = np.zeros((12, 12))
    with pytest.raises(ValueError, match="handle holds a matrix of another size"):
        prune.prune_sparse_matrix(D, handle=Fake(), verbose=False)
    with pytest.raises(ValueError, match="handle holds a matrix of another size"):
        prune.analyze_network_structure(D, handle=Fake())
    with pytest.raises(ValueError, match="smaller than min_points"):   # the reference's checks come first
        prune.prune_sparse_matrix(np.zeros((5, 5)), handle=Fake(), verbose=False)


def test_the_handle_route_is_taken_exactly_when_a_handle_is_passed():
    """A stand-in handle that records its calls: mask and stats come from .prune, the connectivity check from
    .connectivity(kept), the child from .subsample(kept, preserve_order=True); want_matrix=False skips the gather."""
    log = []

    class Given:
        n = 12

        def prune(self, min_connections, target, max_iterations, min_points):
            log.append(("prune", min_connections, target, max_iterations, min_points))
            kept = np.ones(12, dtype=bool)
            kept[[3, 7]] = False
            return kept, dict(attempts=1, attempt_iterations=[2], attempt_stop_reason=[prune.CONVERGED],
                              attempt_last_remove=[0], attempt_final_size=[10], attempt_final_cells=[90],
                              original_cells=100, min_connections_used=min_connections)

        def connectivity(self, subset):
            log.append(("connectivity", list(subset)))
            return 1, 90, np.zeros(10, dtype=np.int32)

        def subsample(self, indices, preserve_order=False):
            log.append(("subsample", list(indices), preserve_order))
            return "child"

        def degrees(self):
            log.append(("degrees",))
            return np.full(12, 11, dtype=np.int32), 132

    kept = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]
    D = np.ones((12, 12)) - np.eye(12)
    out = prune.prune_sparse_matrix(D, min_connections=5, handle=Given(), verbose=False, want_matrix=False)
    assert log == [("prune", 5, None, 100, 10), ("connectivity", kept), ("subsample", kept, True)]
    assert out["handle"] == "child" and out["pruned_matrix"] is None
    assert out["kept_indices"].tolist() == kept and out["removed_indices"].tolist() == [3, 7]
    s = out["stats"]
    assert (s["final_size"], s["iterations"], s["final_measurements"], s["original_measurements"]) == (10, 2, 45.0, 50.0)
    assert s["final_completeness"] == 1.0 and s["is_connected"] is True and s["min_connections_used"] == 5
    del log[:]
    out = prune.prune_sparse_matrix(D, handle=Given(), verbose=False, ensure_connected=False)
    assert [e[0] for e in log] == ["prune", "subsample"] and out["pruned_matrix"].shape == (10, 10)
    del log[:]
    net = prune.analyze_network_structure(D, handle=Given())
    assert log == [("degrees",)] and net["adjacency"] is None and net["summary"]["n_measurements"] == 66.0
    assert prune.analyze_network_structure(D, handle=Given(), want_adjacency=True)["adjacency"].sum() == 132
