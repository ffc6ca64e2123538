"""The resident embedding without a device: the three C entries (declared, exported, ctypes signatures, argument
errors before any device call), the routing of core.euclidean_embedding() with the native calls replaced, and the
`.Call` entry of the R shim on the test double of R's C API (registration, argument-type errors)."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from tests import resident_helpers as rh
from topolow_amd import _native, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_session_load_prepared", "topolow_layout_prep_optimize", "topolow_layout_prep_post_metrics")


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS + ("topolow_layout_prep_order", "topolow_layout_prep_resident_seconds"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_ctypes_signatures_load():
    lib = _native.load()
    assert len(lib.topolow_session_load_prepared.argtypes) == 4
    assert len(lib.topolow_layout_prep_optimize.argtypes) == 20
    assert len(lib.topolow_layout_prep_post_metrics.argtypes) == 8
    for name in SYMBOLS:
        assert getattr(lib, name).restype is C.c_int
    for name in ("optimize", "post_metrics", "fetch", "order", "info") + ("close", "__enter__", "__exit__"):
        assert hasattr(_native.PreparedHandle, name) or name == "info", name
    assert hasattr(_native.Session, "load_prepared")


def test_null_arguments_are_refused_before_any_device_call():
    """TOPOLOW_ERR_BAD_ARGUMENT on a box with or without a GPU: every NULL is found before the handle (here a pointer
    to zeroed memory that nothing may read) is looked at, and before the first device call."""
    lib = _native.load()
    err = C.create_string_buffer(256)
    scratch = np.zeros(4096, dtype=np.float64)        # stands for a non-NULL handle / session / array
    some = scratch.ctypes.data_as(C.c_void_p)
    dp = scratch.ctypes.data_as(C.POINTER(C.c_double))
    ip = scratch.ctypes.data_as(C.POINTER(C.c_int32))
    i64 = scratch.ctypes.data_as(C.POINTER(C.c_int64))
    bad = _native.ERR_BAD_ARGUMENT

    assert lib.topolow_session_load_prepared(None, None, err, len(err)) == bad
    assert lib.topolow_session_load_prepared(None, some, err, len(err)) == bad
    assert lib.topolow_session_load_prepared(some, None, err, len(err)) == bad
    assert err.value

    def optimize(p=some, init=dp, out=dp, conv=ip, iters=ip, mae=dp, k=dp):
        return lib.topolow_layout_prep_optimize(p, init, 2, 10, 5.0, 0.01, 0.01, 1e-4, 5, 3, 0, None, out, conv, iters,
                                                mae, k, None, err, len(err))

    for kw in (dict(p=None), dict(init=None), dict(out=None), dict(conv=None), dict(iters=None), dict(mae=None),
               dict(k=None)):
        err.value = b""
        assert optimize(**kw) == bad, kw
        assert err.value, kw

    def post(p=some, pos=dp, s=dp, c=i64, ndim=2):
        return lib.topolow_layout_prep_post_metrics(p, pos, ndim, None, s, c, err, len(err))

    for kw in (dict(p=None), dict(pos=None), dict(s=None), dict(c=None), dict(ndim=0)):
        assert post(**kw) == bad, kw
    assert lib.topolow_layout_prep_order(None, ip, ip) == bad
    assert lib.topolow_layout_prep_resident_seconds(None, dp) == bad


# ---- core routing, the native calls replaced ----------------------------------------------------------------------

def _matrix(n=8, seed=3):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 2))
    return np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))


ARGS = dict(ndim=2, mapping_max_iter=10, k0=5.0, cooling_rate=0.01, c_repulsion=0.01)


def test_the_environment_and_the_gate_select_the_route(monkeypatch):
    D = np.zeros((8, 8))
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    monkeypatch.delenv("TOPOLOW_RESIDENT", raising=False)
    monkeypatch.setattr(core, "_RESIDENT_MIN_N", None)
    assert not core._resident_wanted(D)
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")
    assert core._resident_wanted(D)
    monkeypatch.setenv("TOPOLOW_RESIDENT", "0")
    monkeypatch.setattr(core, "_RESIDENT_MIN_N", 2)
    assert not core._resident_wanted(D)
    monkeypatch.delenv("TOPOLOW_RESIDENT")
    monkeypatch.setattr(core, "_RESIDENT_MIN_N", 8)
    assert core._resident_wanted(D) and core._resident_wanted(core.RMatrix(D))
    assert not core._resident_wanted(D[:7, :7])
    # the rule of the device prep comes first: where the matrix is prepared on the host nothing is resident
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "0")
    assert not core._resident_wanted(D)
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")
    assert not core._resident_wanted(D)


def test_euclidean_embedding_takes_the_selected_route(monkeypatch):
    seen = []
    monkeypatch.setattr(core, "_embed_resident", lambda *a, **k: seen.append("resident") or "R")
    monkeypatch.setattr(core, "_embed_with", lambda *a, **k: seen.append("present") or "P")
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")
    assert core.euclidean_embedding(_matrix(), **ARGS) == "R"
    monkeypatch.setenv("TOPOLOW_RESIDENT", "0")
    assert core.euclidean_embedding(_matrix(), **ARGS) == "P"
    monkeypatch.delenv("TOPOLOW_RESIDENT")
    monkeypatch.setattr(core, "_RESIDENT_MIN_N", 8)
    assert core.euclidean_embedding(_matrix(), **ARGS) == "R"
    monkeypatch.setattr(core, "_RESIDENT_MIN_N", 9)
    assert core.euclidean_embedding(_matrix(), **ARGS) == "P"
    assert seen == ["resident", "present", "resident", "present"]


@pytest.mark.parametrize("code", [_native.ERR_UNSUPPORTED, _native.ERR_NO_DEVICE])
def test_a_handle_that_cannot_be_made_falls_back_with_the_same_arguments(monkeypatch, code):
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")
    made = []

    class Refusing:
        def __init__(self, *a, **k):
            made.append(1)
            raise _native.NativeError(code, "no")

    monkeypatch.setattr(_native, "PreparedHandle", Refusing)
    got = {}
    monkeypatch.setattr(core, "_embed_with", lambda *a, **k: got.update(a=a, k=k) or "P")
    D = _matrix()
    init = np.zeros((8, 2))
    assert core.euclidean_embedding(D, initial_positions=init, verbose=False, preserve_order=True, **ARGS) == "P"
    assert made == [1]
    a = got["a"]
    assert a[0] is _native.optimize_layout_exact and a[1] is _native.est_distances
    assert a[2] is D and a[3:8] == (2, 10, 5.0, 0.01, 0.01) and a[10] is init and a[15] is True
    assert got["k"]["post_fn"] is core.device_post and got["k"]["prepare_fn"] is core._prepare_layout_call_auto

    class Broken:
        def __init__(self, *a, **k):
            raise _native.NativeError(_native.ERR_HIP, "a HIP call failed")

    monkeypatch.setattr(_native, "PreparedHandle", Broken)
    with pytest.raises(_native.NativeError):     # any other error is the caller's to see
        core.euclidean_embedding(D, **ARGS)


def test_what_the_device_form_does_not_take_never_reaches_the_device(monkeypatch):
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")

    class Forbidden:
        def __init__(self, *a, **k):
            raise AssertionError("the device was reached")

    monkeypatch.setattr(_native, "PreparedHandle", Forbidden)
    monkeypatch.setattr(core, "_embed_with", lambda *a, **k: "P")
    chars = np.array([["0", ">3"], ["<1", "0"]], dtype=object)
    assert core.euclidean_embedding(chars, **ARGS) == "P"                       # a character matrix
    assert core.euclidean_embedding(_matrix(), **dict(ARGS, ndim=0)) == "P"     # _validate rejects it: the host form raises
    assert core.euclidean_embedding(_matrix(), **dict(ARGS, cooling_rate=1.5)) == "P"
    assert core.euclidean_embedding(np.zeros((3, 4)), **ARGS) == "P"
    assert core.euclidean_embedding(_matrix(), initial_positions=np.zeros((7, 2)), **ARGS) == "P"
    monkeypatch.setitem(_native.options, "devices", [0, 0])                    # a sharded run keeps the present route
    assert core.euclidean_embedding(_matrix(), **ARGS) == "P"
    with pytest.raises(TypeError, match='argument "k0" is missing'):
        core.euclidean_embedding(_matrix(), 2)


class _FakeHandle:
    """PreparedHandle's surface over NumPy: reverses the order of the points, "optimizes" by returning the start."""
    log = []

    def __init__(self, values, codes=None, preserve_order=False, order=None, layout=None, device=None):
        self.n = values.shape[0]
        self.values = values
        reorder = not preserve_order
        self._order = np.arange(self.n - 1, -1, -1, dtype=np.int32) if reorder else None
        self.info = dict(n_edges=self.n * (self.n - 1) // 2, n_finite_nonzero=int(np.sum(np.isfinite(values) & (values != 0))),
                         n_infinite=0, n_negative=0, numeric_max=float(np.nanmax(values)), reordered=int(reorder),
                         order_route=_native.ORDER_DEVICE_GAP if reorder else _native.ORDER_PRESERVED, exact_sums=0)
        _FakeHandle.log.append(("create", preserve_order))

    order = property(lambda self: self._order)

    def optimize(self, init, ndim, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, window, freq, verbose,
                 **opt_kw):
        _FakeHandle.log.append(("optimize", ndim, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, window, freq,
                                verbose, sorted(opt_kw)))
        self.init = np.array(init)
        return _native.NativeResult(np.array(init), True, 9, 0.25, 1.5, dict(schedule="slab"))

    def post_metrics(self, positions, want_est=True):
        _FakeHandle.log.append(("post",))
        return np.full((self.n, self.n), 2.0), 6.0, 4

    def close(self):
        _FakeHandle.log.append(("close",))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def test_the_resident_call_builds_the_topolow_from_the_handle(monkeypatch, capsys):
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")
    monkeypatch.setattr(_native, "PreparedHandle", _FakeHandle)
    monkeypatch.setattr(core, "_embed_with", lambda *a, **k: pytest.fail("the present route ran"))
    _FakeHandle.log = []
    n = 6
    names = ["v%d" % q for q in range(n)]
    D = core.RMatrix(_matrix(n), names)
    init = core.RMatrix(np.arange(2.0 * n).reshape(n, 2), [names[q] for q in (3, 1, 0, 5, 2, 4)])
    _native.set_seed(11)
    out = core.euclidean_embedding(D, initial_positions=init, verbose=True, **ARGS)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Matrix reordered for spectral pattern (largest values in corners)"
    assert lines[1] == "Starting C++ optimization..." and lines[2].startswith("Optimization finished in")
    assert out.names == names[::-1]                                   # reordered from .order
    want = np.array([init.values[[3, 1, 0, 5, 2, 4].index(names.index(nm))] for nm in out.names])
    assert np.array_equal(out.positions, want)                        # start positions picked by row names
    assert out.mae == 1.5 and out.iter == 9 and np.array_equal(out.est_distances, np.full((n, n), 2.0))
    assert out.convergence == dict(achieved=True, error=0.25, final_k=1.5)
    assert out.parameters == dict(ndim=2, k0=5.0, cooling_rate=0.01, c_repulsion=0.01, method="cpp_exact_full_pairwise")
    assert out.native_info == dict(schedule="slab")
    kinds = [e[0] for e in _FakeHandle.log]
    assert kinds == ["create", "optimize", "post", "close"]
    assert _FakeHandle.log[1][1:] == (2, 10, 5.0, 0.01, 0.01, 1e-4, 5, 3, True, ["seed"])

    # no start positions: the random walk from info.numeric_max, the draws of the present route from the same stream
    _native.set_seed(5)
    out = core.euclidean_embedding(D.values, preserve_order=True, **ARGS)
    _native.set_seed(5)
    gen = _native.host_rng()
    step = np.float64(np.nanmax(D.values)) / n
    steps = gen.uniform(0.0, 2.0 * step, size=(2, n - 1)).T
    assert np.array_equal(out.positions, np.vstack([np.zeros((1, 2)), np.cumsum(steps, axis=0)]))
    assert out.names is None

    # _validate's warning is raised once, with the device's count
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        core.euclidean_embedding(D.values, **dict(ARGS, k0=31.0))
    assert [str(x.message) for x in w] == ["High k0 value (> 30) may lead to instability"]


def test_an_optimize_that_declines_hands_start_and_seed_to_the_present_route(monkeypatch):
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    monkeypatch.setenv("TOPOLOW_RESIDENT", "1")

    class Declining(_FakeHandle):
        def optimize(self, init, *a, **opt_kw):
            Declining.seen = (np.array(init), opt_kw["seed"])
            raise _native.NativeError(_native.ERR_UNSUPPORTED, "no device memory")

    monkeypatch.setattr(_native, "PreparedHandle", Declining)
    got = {}

    def prepare(dm, *a):
        got["prepare"] = a
        return core.prepare_layout_call(dm, *a)

    def arrays(*a, **k):
        got["arrays"] = (a, k)
        return _native.NativeResult(np.array(a[0]), False, 3, 0.5, 2.0, {})

    monkeypatch.setattr(core, "_prepare_layout_call_auto", prepare)
    monkeypatch.setattr(_native, "optimize_layout_exact_arrays", arrays)
    monkeypatch.setattr(core, "device_post", lambda call, pos: (np.zeros((6, 6)), 0.75))
    _native.set_seed(3)
    out = core.euclidean_embedding(_matrix(6), preserve_order=True, **ARGS)
    init, seed = Declining.seen
    assert np.array_equal(got["prepare"][7], init) and got["prepare"][8] is False
    assert got["arrays"][1] == dict(seed=seed) and np.array_equal(got["arrays"][0][0], init)
    assert out.mae == 0.75 and out.iter == 3


def _fake_prepare_layout(values, codes=None, preserve_order=False, order=None, **kw):
    """_native.prepare_layout's result over NumPy: the info and the order of a _FakeHandle on the same arguments."""
    h = _FakeHandle(values, codes, preserve_order, order)
    n, o = h.n, h.order
    v = np.ascontiguousarray(values if o is None else values[np.ix_(o, o)])
    ei, ej = np.triu_indices(n, 1)
    return _native.PreparedLayout(
        info=h.info, order=o, degrees=np.full(n, n, dtype=np.int32), edge_i=ei.astype(np.int32),
        edge_j=ej.astype(np.int32), edge_dist=v[ei, ej], edge_thresh=np.zeros(ei.shape[0], dtype=np.int32), dense=v,
        tdense=np.zeros((n, n), dtype=np.int32), values_reordered=None if o is None else v)


def test_the_two_device_routes_say_draw_and_align_the_same(monkeypatch, capsys):
    """prepare_layout_call_device over _native.prepare_layout and _embed_resident over _native.PreparedHandle, each
    replaced by an object that reports the same info and order: the same verbose lines, the same numbers out of
    identically seeded generators, and a named, permuted initial_positions lined up to the same rows."""
    monkeypatch.setattr(_native, "prepare_layout", _fake_prepare_layout)
    monkeypatch.setattr(_native, "PreparedHandle", _FakeHandle)
    monkeypatch.setitem(_native.options, "seed", 4)     # the resident route draws no seed of its own
    n = 6
    names = ["v%d" % q for q in range(n)]
    D = core.RMatrix(_matrix(n), names)
    perm = (3, 1, 0, 5, 2, 4)
    named_init = core.RMatrix(np.arange(2.0 * n).reshape(n, 2), [names[q] for q in perm])

    def both(init, preserve_order):
        ga, gb = np.random.default_rng(17), np.random.default_rng(17)
        capsys.readouterr()
        call = core.prepare_layout_call_device(D, 2, 10, 5.0, 0.01, 0.01, 1e-4, 5, init, True, 3, preserve_order, ga)
        said_a = capsys.readouterr().out.splitlines()
        out = core._embed_resident(D, 2, 10, 5.0, 0.01, 0.01, 1e-4, 5, init, False, None, True, 3, preserve_order, gb)
        said_b = capsys.readouterr().out.splitlines()
        assert len(said_a) == 1 and said_b[:said_b.index("Starting C++ optimization...")] == said_a
        assert out.positions.tobytes() == call.initial_positions.tobytes()      # the fake "optimizes" to its start
        assert out.names == call.names
        assert ga.bit_generator.state == gb.bit_generator.state
        return call, said_a[0], ga

    call, said, gen = both(named_init, False)
    assert said.startswith("Matrix reordered") and call.names == names[::-1]
    assert np.array_equal(call.initial_positions, named_init.values[[perm.index(names.index(nm)) for nm in call.names]])
    assert gen.bit_generator.state == np.random.default_rng(17).bit_generator.state       # nothing was drawn
    call, said, gen = both(None, False)
    assert said.startswith("Matrix reordered")
    assert gen.bit_generator.state != np.random.default_rng(17).bit_generator.state       # the walk was
    assert call.initial_positions.tobytes() == core._start_walk(np.nanmax(D.values), n, 2,
                                                                np.random.default_rng(17)).tobytes()
    call, said, _ = both(None, True)
    assert said.startswith("Preserving original row/column order") and call.names == names
    with pytest.raises(IndexError, match="subscript out of bounds"):
        core.prepare_layout_call_device(D, 2, 10, 5.0, 0.01, 0.01, 1e-4, 5, core.RMatrix(named_init.values, list("abcdef")),
                                        False, 3, False)
    with pytest.raises(IndexError, match="subscript out of bounds"):
        core._embed_resident(D, 2, 10, 5.0, 0.01, 0.01, 1e-4, 5, core.RMatrix(named_init.values, list("abcdef")),
                             False, None, False, 3, False)


# ---- the .Call entry on the test double of R's C API ------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return rh.build_harness(tmp_path_factory.mktemp("resident_harness"))


def test_the_entry_is_registered_with_15_arguments():
    shim = open(os.path.join(ROOT, "topolow_amd", "r", "topolow_shim.c")).read()
    assert re.search(r'\{"_topolow_euclidean_embedding_resident",\s*\(DL_FUNC\)&_topolow_euclidean_embedding_resident,\s*15\}',
                     shim)


@pytest.mark.parametrize("case,message", [
    (dict(bad=1), "values must be a numeric n x n matrix"),
    (dict(bad=5), "values must be a numeric n x n matrix"),
    (dict(bad=2, codes=True), "codes must be NULL or an integer n x n matrix"),
    (dict(codes=True, codes_n=5), "codes must be NULL or an integer n x n matrix"),
    (dict(bad=3, order=True), "order must be NULL or an integer vector of length n (1-based)"),
    (dict(order=True, order_n=5), "order must be NULL or an integer vector of length n (1-based)"),
    (dict(bad=4), "initial_positions must be a numeric n x ndim matrix"),
    (dict(init_shape=(5, 2)), "initial_positions must be a numeric n x ndim matrix"),
    (dict(init_shape=(6, 3)), "initial_positions must be a numeric n x ndim matrix"),
    (dict(values_n=1, init_shape=(1, 2)), "dissimilarity_matrix must have at least 2 rows/columns"),
])
def test_argument_type_errors_are_r_errors_with_balanced_protects(harness, tmp_path, case, message):
    """Each is found before the handle is created, so this runs with or without a device; the harness finds the entry
    by name AND arity 15 (registration "ok"), the R error carries the message, and no PROTECT is left behind."""
    n = case.get("values_n", 6)
    D = _matrix(n) if n > 1 else np.zeros((1, 1))
    codes = np.zeros((case.get("codes_n", n),) * 2, dtype=np.int32) if case.get("codes") else None
    order = np.arange(1, case.get("order_n", n) + 1) if case.get("order") else None
    init = np.zeros(case.get("init_shape", (n, 2)))
    res = rh.run_harness(harness, tmp_path, D, codes, order, init, 2, bad=case.get("bad", 0))
    assert res["registration"] == "ok"
    assert res["error"] == message
    assert res["protect_depth"] == 0
