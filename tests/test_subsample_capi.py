"""The two graph entries of a prepared handle without a device: declared, exported, ctypes signatures, the Python
surface, and every TOPOLOW_ERR_BAD_ARGUMENT case -- each found before any device call, so this runs on a box with or
without a GPU.  The subset rules read one thing of a handle, its n, the first field of the struct: the stand-in
handle here is zeroed memory with n written at its start, which nothing else may read."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from topolow_amd import _native, cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_layout_prep_connectivity", "topolow_layout_prep_subsample")
BAD = _native.ERR_BAD_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS + ("topolow_layout_prep_graph_stats",):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_ctypes_signatures_and_the_python_surface():
    lib = _native.load()
    assert len(lib.topolow_layout_prep_connectivity.argtypes) == 8
    assert len(lib.topolow_layout_prep_subsample.argtypes) == 9
    for name in SYMBOLS:
        assert getattr(lib, name).restype is C.c_int
    for name in ("connectivity", "subsample", "graph_stats"):
        assert callable(getattr(_native.PreparedHandle, name)), name


def test_the_kernels_live_in_a_header_of_their_own_that_the_library_depends_on():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "relax_prep_graph.h"))
    sources = glob.glob(os.path.join(csrc, "*.hip"))   # exactly one source compiles the kernels
    assert sum('#include "relax_prep_graph.h"' in open(s).read() for s in sources) == 1
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HDR\s*=.*\$\(wildcard \*\.h\)", make, re.M)          # every header of csrc is a dependency
    assert re.search(r"^%\.o:.*\$\(HDR\)", make, re.M)                        # ... of every object
    assert re.search(r"^libtopolow_relax\.so:.*\$\(OBJ\)", make, re.M)        # ... which the library is linked from


class _StandIn:
    """Zeroed memory with `n` at its start, and the arguments of the two entries around it."""

    def __init__(self, n):
        self.lib = _native.load()
        self.mem = np.zeros(4096, dtype=np.int32)
        self.mem[0] = n
        self.handle = self.mem.ctypes.data_as(C.c_void_p)
        self.err = C.create_string_buffer(256)
        self.nc, self.cells = C.c_int32(0), C.c_int64(0)
        self.out = C.c_void_p(None)
        self.info = _native.TopolowLayoutPrepInfo()

    @staticmethod
    def _sub(subset):
        if subset is None:
            return None, 0
        a = np.ascontiguousarray(subset, dtype=np.int32)
        return a, a.shape[0]

    def connectivity(self, subset, m=None, handle="own", nc="own", cells="own"):
        a, k = self._sub(subset)
        self.err.value = b""
        self._keep = a
        return self.lib.topolow_layout_prep_connectivity(
            self.handle if handle == "own" else None, _native._ip(a) if a is not None else None, k if m is None else m,
            C.byref(self.nc) if nc == "own" else None, C.byref(self.cells) if cells == "own" else None, None, self.err,
            len(self.err))

    def subsample(self, subset, m=None, handle="own", out="own", info="own", preserve_order=0, order_in=None):
        a, k = self._sub(subset)
        o = np.ascontiguousarray(order_in, dtype=np.int32) if order_in is not None else None
        self.err.value = b""
        self._keep = (a, o)
        return self.lib.topolow_layout_prep_subsample(
            self.handle if handle == "own" else None, _native._ip(a) if a is not None else None, k if m is None else m,
            preserve_order, _native._ip(o) if o is not None else None, C.byref(self.out) if out == "own" else None,
            C.byref(self.info) if info == "own" else None, self.err, len(self.err))


def test_null_arguments():
    s = _StandIn(10)
    ok_subset = [3, 1, 2]
    for kw in (dict(handle=None), dict(nc=None), dict(cells=None)):
        assert s.connectivity(ok_subset, **kw) == BAD, kw
        assert b"NULL" in s.err.value, kw
    for kw in (dict(handle=None), dict(out=None), dict(info=None)):
        assert s.subsample(ok_subset, **kw) == BAD, kw
        assert b"NULL" in s.err.value, kw
    assert s.connectivity(None, handle=None) == BAD and s.subsample(None, handle=None) == BAD


@pytest.mark.parametrize("entry", ["connectivity", "subsample"])
@pytest.mark.parametrize("subset,m,word", [
    ([4], None, b"between 2 and"),                       # m < 2
    ([4, 5], 1, b"between 2 and"),
    ([4, 5], 0, b"between 2 and"),
    ([4, 5], -3, b"between 2 and"),
    (list(range(10)) + [0], None, b"between 2 and"),     # m > n
    ([0, 10], None, b"out of range"),                    # one past the end
    ([0, -1], None, b"out of range"),
    ([7, 2, 2 ** 31 - 1], None, b"out of range"),
    ([1, 2, 1], None, b"repeated"),
])
def test_subset_rules_are_checked_before_any_device_call(entry, subset, m, word):
    s = _StandIn(10)
    rc = getattr(s, entry)(subset, m)
    assert rc == BAD
    assert word in s.err.value, s.err.value
    assert s.out.value is None


def test_a_valid_subset_passes_the_rules_and_only_then_is_order_in_judged():
    """subsample checks order_in after the subset and still before any device call: a valid subset with a bad order_in
    is BAD_ARGUMENT with create()'s message, relative to the child's m points."""
    s = _StandIn(10)
    assert s.subsample([9, 0, 4], order_in=[0, 1, 3]) == BAD            # 3 is no point of a 3-point child
    assert b"permutation" in s.err.value
    assert s.subsample([9, 0, 4], order_in=[0, 0, 1]) == BAD
    assert s.subsample(None, order_in=list(range(9)) + [11]) == BAD      # NULL subset: the child has the parent's n
    assert b"permutation" in s.err.value
    assert s.subsample([9, 9, 4], order_in=[0, 0, 1]) == BAD and b"repeated" in s.err.value   # the subset comes first


def test_python_argument_errors_need_no_device():
    h = _native.PreparedHandle.__new__(_native.PreparedHandle)
    h.n = 5
    with pytest.raises(ValueError, match="one entry per selected point"):
        _native.PreparedHandle.subsample(h, [0, 1, 2], order_in=[0, 1])
    D = np.zeros((4, 4))
    sets = [dict(N=2, k0=1.0, cooling_rate=0.01, c_repulsion=0.01)]
    for path in ("sparse", "sparse-calls", "dense", "session"):
        with pytest.raises(ValueError, match="handle is taken by path = 'resident' only"):
            cv.likelihood_sweep(D, sets, 10, 1e-4, folds=2, path=path, handle=object())


def test_likelihood_sweep_judges_a_handle_before_it_uses_it():
    class Fake:
        def __init__(self, n, route, open_=True, declined=False):
            self.n, self._h, self.declined = n, open_, declined
            self.info = dict(order_route=route)

    D = np.ones((4, 4)) - np.eye(4)
    sets = [dict(N=2, k0=1.0, cooling_rate=0.01, c_repulsion=0.01)]
    for fake in (Fake(4, _native.ORDER_DEVICE_GAP), Fake(4, _native.ORDER_PRESERVED, open_=False),
                 Fake(4, _native.ORDER_PRESERVED, declined=True)):
        with pytest.raises(ValueError, match="open PreparedHandle created with preserve_order=True"):
            cv.likelihood_sweep(D, sets, 10, 1e-4, folds=2, path="resident", handle=fake)
    with pytest.raises(ValueError, match="another size"):
        cv.likelihood_sweep(D, sets, 10, 1e-4, folds=2, path="resident", handle=Fake(5, _native.ORDER_PRESERVED))


def test_a_given_handle_is_used_and_left_open(monkeypatch):
    """_sweep_resident with a handle: no PreparedHandle is opened, cv_sweep runs on the given one, close is not called."""
    log = []

    class Given:
        n, _h, declined = 4, True, False
        info = dict(order_route=_native.ORDER_PRESERVED)

        def cv_sweep(self, named, preserve_order, nd, *a, **k):
            log.append(("sweep", len(nd)))
            f = len(nd)
            return (np.ones(f), np.ones(f, np.int64), np.ones(f, np.int32), np.ones(f, np.int32),
                    np.zeros(f, np.int32), 0.5, np.zeros(f, np.int32))

        def close(self):
            log.append(("close",))

    class Forbidden:
        def __init__(self, *a, **k):
            raise AssertionError("a handle was opened")

    monkeypatch.setattr(_native, "PreparedHandle", Forbidden)
    D = np.ones((4, 4)) - np.eye(4)
    sets = [dict(N=2, k0=1.0, cooling_rate=0.01, c_repulsion=0.01)]
    out = cv.likelihood_sweep(D, sets, 10, 1e-4, folds=2, path="resident", rng=np.random.default_rng(0), handle=Given())
    assert log == [("sweep", 2)] and out[1] == 0.5 and out[2] == 2 and out[3] == 0
