"""Extended STOI, the parts that need no GPU: the numpy restatement's own
properties (tests/_estoi_ref.py, the definition of include/cse_estoi.h), the
three entry points' declarations, exports and argument checks, and the enhance
kernels' source digest, which a header of its own leaves alone."""

import ctypes
import os
import re

import numpy as np
import pytest

import _estoi_ref
from oracle import stoi_ref
from classical_speech_enhancement_amd import _lib
from classical_speech_enhancement_amd.synth import make_pair

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "cse_estoi.h")
# bench.kernel_src_sha() of the commit before cse_estoi.h existed: the committed
# PMC profiles carry it, and bench.py drops their roofline when it changes
PARENT_KERNEL_SRC_SHA = "0294b26e5cf891db"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def pair():
    return make_pair(10, seconds=1.0)


def test_identity_scores_one(pair):
    clean, noisy = pair
    assert 1.0 - _estoi_ref.estoi(clean, clean, 16000) < 1e-12
    assert 1.0 - _estoi_ref.estoi(noisy, noisy, 16000) < 1e-12


def test_gain_invariance(pair):
    clean, noisy = pair
    base = _estoi_ref.estoi(clean, noisy, 16000)
    for a in (0.01, 0.5, 7.0):
        assert abs(_estoi_ref.estoi(clean, a * noisy, 16000) - base) < 1e-12, a


def test_short_pair_scores_1e_5():
    clean, noisy = make_pair(4, seconds=0.4)
    assert _estoi_ref.estoi(clean, noisy, 16000) == 1e-5
    assert _estoi_ref.calculate_estoi(clean[:300], noisy[:300], 16000) is None


def test_differs_from_stoi(pair):
    clean, noisy = pair
    e = _estoi_ref.estoi(clean, noisy, 16000)
    s = stoi_ref.stoi(clean, noisy, 16000)
    assert abs(e - 0.3399) < 5e-5, e
    assert abs(s - 0.7727) < 5e-5, s


def test_zero_test_signal_scores_zero(pair):
    clean, _ = pair
    assert _estoi_ref.estoi(clean, np.zeros_like(clean), 16000) == 0.0


def test_header_declares_the_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(cse_[a-z0-9_]+)\s*\(", text))
    assert names == set(_lib.EXPORTS_ESTOI)
    assert '#include "cse.h"' in text
    assert not set(_lib.EXPORTS_ESTOI) & set(_lib.EXPORTS)
    for n in _lib.EXPORTS_ESTOI:
        assert hasattr(lib, n), n
    assert lib.cse_version() == _lib.ABI_VERSION == 5


def test_argument_checks(lib):
    p, n = ctypes.c_void_p(16), 48000
    rc = lib.cse_estoi_prepare(None, 1, n, 16000, p, None)
    assert rc == -1 and b"cse_estoi_prepare: NULL" in lib.cse_last_error()
    rc = lib.cse_estoi_prepare(p, 1, n, 16000, None, None)
    assert rc == -1 and b"cse_estoi_prepare: NULL" in lib.cse_last_error()
    rc = lib.cse_estoi_prepare(p, 0, n, 16000, p, None)
    assert rc == -1 and b"cse_estoi_prepare: n_sig=0" in lib.cse_last_error()
    rc = lib.cse_estoi_prepare(p, 1, n, 500, p, None)
    assert rc == -1 and b"cse_estoi_prepare: sr=500" in lib.cse_last_error()
    rc = lib.cse_estoi_cells(None, p, None, p, 1, 1, n, 16000, 1, p, p, p, None)
    assert rc == -1 and b"cse_estoi_cells: NULL argument" in lib.cse_last_error()
    rc = lib.cse_estoi_cells(p, p, None, p, 1, 1, n, 16000, 1, p, p, None, None)
    assert rc == -1 and b"cse_estoi_cells: NULL argument" in lib.cse_last_error()
    rc = lib.cse_estoi_cells(p, p, None, p, 1, 0, n, 16000, 1, p, p, p, None)
    assert rc == -1 and b"cse_estoi_cells: n_sig=0" in lib.cse_last_error()
    rc = lib.cse_estoi_cells(p, p, None, p, 1, 1, n, 900000, 1, p, p, p, None)
    assert rc == -1 and b"cse_estoi_cells: sr=900000" in lib.cse_last_error()
    rc = lib.cse_estoi_cells(p, p, None, p, 1, 1, n, 16000, 1, p, None, p, None)
    assert rc == -1 and b"cse_estoi_cells: NULL scratch" in lib.cse_last_error()
    # the per-call cell limit at other rates, as cse_stoi_cells_sr
    rc = lib.cse_estoi_cells(p, p, None, p, 65536, 1, n, 22050, 1, p, p, p, None)
    assert rc == -1 and b"cse_estoi_cells: n_cells=65536" in lib.cse_last_error()
    # nothing to score: checked, nothing launched
    assert lib.cse_estoi_cells(p, p, None, p, 0, 1, n, 16000, 1, p, None, p, None) == 0


def test_workspace_sizes(lib):
    n = 48000
    for sr in (16000, 10000, 22050, 48000):
        for n_sig in (1, 3):
            base = lib.cse_stoi_workspace_bytes_sr(n_sig, n, sr)
            ext = lib.cse_estoi_workspace_bytes(n_sig, n, sr)
            # the plain layout, then 16 bytes per (segment, frame) of every signal
            n10 = -(-n * 10000 // sr)
            jmax = (n10 - 256) // 128 + 1 - 1 - 30 + 1
            assert ext >= base + n_sig * jmax * 30 * 16 > base > 0, (sr, n_sig)
    # too short for a segment: nothing is added
    assert lib.cse_estoi_workspace_bytes(1, 4000, 16000) == lib.cse_stoi_workspace_bytes(1, 4000)
    for sr in (500, 768001, -16000):
        assert lib.cse_estoi_workspace_bytes(1, n, sr) == -1
    assert lib.cse_estoi_workspace_bytes(0, n, 16000) == -1


def test_plain_signatures_keep_their_defaults():
    import inspect
    from classical_speech_enhancement_amd import metrics, search
    for fn in (metrics.StoiPlan.__init__, metrics.stoi, metrics.calculate_stoi, search.run_grid,
               search.optimize_parameters, search.run_sweep):
        assert inspect.signature(fn).parameters["extended"].default is False, fn
    assert inspect.signature(search.engine_compute).parameters["stoi"].default is True
    assert search.NCOL == 6 and search.RECORD_FIELDS[4] == "stoi"
    with pytest.raises(ValueError):
        search.engine_compute([], [], [], [], stoi="estoi")


def test_enhance_kernel_digest_is_the_parents():
    import bench
    assert bench.kernel_src_sha() == PARENT_KERNEL_SRC_SHA
