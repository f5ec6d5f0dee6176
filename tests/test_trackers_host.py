"""The tracker registry (classical_speech_enhancement_amd/trackers.py), the
parts that need no GPU: every record agrees with _lib, with its header and with
the library's own defaults, and the generic helpers (params, check_names) do
for every tracker what the per-tracker code did."""

import ast
import ctypes
import os

import numpy as np
import pytest

from classical_speech_enhancement_amd import _lib, plugins, search, trackers
from classical_speech_enhancement_amd.trackers import TRACKERS

INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
P, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(params=list(TRACKERS))
def tracker(request):
    return TRACKERS[request.param]


def test_registry_order_and_methods():
    assert tuple(TRACKERS) == ("mcra", "spp", "minstat", "imcra")
    assert [t.code for t in TRACKERS.values()] == [3, 4, 5, 6]
    assert tuple(search.NOISE_METHODS) == ("percentile", "min_tracking", "true_noise", "mcra",
                                           "spp", "minstat", "imcra")
    assert [n for n, t in TRACKERS.items() if t.time_constants] == ["minstat", "imcra"]
    assert len(_lib.NOISE) == 7 and sorted(_lib.NOISE.values()) == list(range(7))


def test_module_is_host_only():
    """trackers.py imports neither torch nor the loaded library, like layout.py."""
    tree = ast.parse(open(trackers.__file__).read())
    names = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import)
             for a in n.names}
    names |= {n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names <= {"ctypes", "math", "typing", "numpy", ""}
    assert "load(" not in open(trackers.__file__).read()


def test_record_matches_lib_and_header(tracker):
    name = tracker.name
    assert TRACKERS[name] is tracker
    assert tracker.code == _lib.NOISE[name]
    header = open(os.path.join(INCLUDE, f"cse_{name}.h")).read()
    assert f"#define CSE_NOISE_{name.upper()} {tracker.code} " in header
    assert tracker.struct is getattr(_lib, name.capitalize() + "Params")
    assert (tracker.entry, tracker.default_entry) == (f"cse_noise_{name}",
                                                      f"cse_{name}_default_params")
    assert set(getattr(_lib, "EXPORTS_" + name.upper())) == {tracker.entry, tracker.default_entry}


def test_fields_defaults_and_values_share_one_order(tracker):
    fields = [f for f, _ in tracker.struct._fields_ if f != "reserved"]
    assert fields == list(tracker.defaults)
    assert tracker.values({}) == tuple(tracker.defaults.values())
    # under a prefix the bare names are not read
    assert tracker.values({k: None for k in tracker.defaults}, tracker.name + "_") == \
        tracker.values({})
    assert trackers.tracker_values({"noise_method": tracker.name}) == tracker.values({})
    assert trackers.tracker_values({"noise_method": "percentile"}) == ()


def test_params_equals_the_librarys_defaults(lib, tracker):
    want = tracker.struct()  # zeroed
    getattr(lib, tracker.default_entry)(ctypes.byref(want))
    got = trackers.params(tracker, tracker.values({}))
    assert isinstance(got, tracker.struct)
    assert bytes(got) == bytes(want)


def test_params_writes_every_field(tracker):
    """Values that differ from the defaults in every field arrive, arrays
    included, and ``reserved`` stays zero."""
    def other(d):
        return tuple(other(x) for x in d) if isinstance(d, tuple) else type(d)(d * 0.5 + 3)
    values = tuple(other(d) for d in tracker.defaults.values())
    prm = trackers.params(tracker, values)
    for k, x in zip(tracker.defaults, values):
        got = getattr(prm, k)
        assert (tuple(got) if isinstance(x, tuple) else got) == x, k
    assert getattr(prm, "reserved", 0) == 0


def test_entries_resolve_with_the_shared_signatures(lib, tracker):
    default_entry, entry = getattr(lib, tracker.default_entry), getattr(lib, tracker.entry)
    assert default_entry.restype is None and default_entry.argtypes == [P]
    assert entry.restype is I32 and entry.argtypes == [P, I64, I32, I32, P, F64, P, P]


def test_check_names(tracker):
    trackers.check_names(tracker, {})
    trackers.check_names(tracker, dict(tracker.defaults))
    trackers.check_names(tracker, list(tracker.defaults))
    with pytest.raises(TypeError, match=f"^{tracker.name} takes no parameter 'nope'$"):
        trackers.check_names(tracker, {"nope": 1})
    first = next(iter(tracker.defaults))
    with pytest.raises(TypeError, match=f"^{tracker.name} takes no parameter 'abc'$"):
        trackers.check_names(tracker, {"zzz": 1, first: 0.5, "abc": 2})


PLUGIN_ARGS = {
    "spectral_subtraction": dict(alpha=1.0, beta=0.05),
    "wiener_filter": dict(alpha=0.98, gain_floor=0.1),
    "mmse": dict(alpha=0.98, ksi_min=0.01, gain_min=0.05, gain_max=1.0),
    "advanced_mmse": dict(alpha=0.9, ksi_min=0.01, q=0.4, noise_mu=0.95, gain_floor=0.1),
}


@pytest.mark.parametrize("plugin", list(PLUGIN_ARGS))
def test_plugins_refuse_an_unknown_name_before_any_engine(monkeypatch, plugin, tracker):
    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(plugins, "engine", no_engine)
    noisy = np.zeros(4000)
    with pytest.raises(TypeError, match=f"^{tracker.name} takes no parameter 'nope'$"):
        getattr(plugins, plugin)(noisy, 16000, n_fft=512, hop_length=128, noise_percentile=20.0,
                                 noise_method=tracker.name, **PLUGIN_ARGS[plugin],
                                 **{tracker.name: {"nope": 1}})
