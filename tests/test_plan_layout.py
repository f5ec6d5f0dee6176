"""The planning code (layout.PlanLayout, engine.GridPlan) on the CPU.

tests/golden/plan_layout.npz holds, for four plans, the uploaded tables, the
buffer sizes and every library call with its arguments as the code computed
them before PlanLayout existed (tests/golden/make_plan_layout.py, which also
builds the cases here).  The kernels dereference these offsets unchecked, so
the comparison has no tolerance and leaves nothing out.
"""

import importlib.util
import json
import os

import numpy as np
import pytest

from classical_speech_enhancement_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_plan_layout",
                                               os.path.join(GOLDEN, "make_plan_layout.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
CASES = ("a", "b", "c", "d")


@pytest.fixture(scope="module")
def pinned():
    return np.load(os.path.join(GOLDEN, "plan_layout.npz"))


def test_cases_are_the_pinned_ones(pinned):
    assert tuple(gen.cases()) == CASES
    assert {k.split("/")[0] for k in pinned.files} == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_tables_sizes_and_calls_equal_the_pinned_ones(pinned, case):
    got = gen.record(*gen.cases()[case])
    assert sorted(f"{case}/{n_fft}/{k}" for n_fft, arrays in got.items() for k in arrays) == \
        sorted(k for k in pinned.files if k.startswith(case + "/"))
    for n_fft, arrays in got.items():
        for k, v in arrays.items():
            want = pinned[f"{case}/{n_fft}/{k}"]
            if k == "calls":
                g, w = json.loads(str(v)), json.loads(str(want))
                assert [c[0] for c in g] == [c[0] for c in w], (n_fft, "call sequence")
                for cg, cw in zip(g, w):
                    # NaN fields (smoothing_factor) compare equal as text
                    assert json.dumps(cg) == json.dumps(cw), (n_fft, cg, cw)
                assert str(v) == str(want)
            else:
                assert v.dtype == want.dtype and v.shape == want.shape, (n_fft, k)
                assert v.tobytes() == want.tobytes(), (n_fft, k)


def test_head_grid_noise_schedule():
    """The HEAD grid's calls per hop: one median, both min-tracking eps in one
    call, the four percentile bases as the quad, one finish with 18 jobs."""
    from classical_speech_enhancement_amd.layout import PlanLayout, specs_by_n_fft
    L, specs, _ = gen.cases()["a"]
    n_fft, items = specs_by_n_fft(gen.S, L, specs, True, False)[0]
    lay = PlanLayout(n_fft, gen.S, L, items, True, False, False, align=True, cells_per_group=16)
    assert n_fft == 512 and list(lay.noise_calls) == lay.hops == [128, 256]
    for hop, calls in lay.noise_calls.items():
        assert [c[0] for c in calls] == ["cse_noise_median", "cse_noise_min_tracking_med",
                                         "cse_noise_percentile_quad", "cse_noise_finish"]
        mt, quad, fin = calls[1][1], calls[2][1], calls[3][1]
        assert (mt[5], mt[7]) == (1e-10, 1e-12)
        assert quad[5:9] == (10.0, 20.0, 1e-12, 1e-10)
        assert fin[1] == 18
        outs = [a.off for a in mt + quad if isinstance(a, tuple) and a.buf == "raw"]
        assert len(outs) == len(set(outs)) == 6


def _layouts(case):
    """(layout, elements of the buffer out_offset points into) per n_fft."""
    from classical_speech_enhancement_amd.layout import PlanLayout, specs_by_n_fft
    L, specs, kw = gen.cases()[case]
    want_y, want_g = kw.get("want_waveforms", False), kw.get("want_gains", False)
    for n_fft, items in specs_by_n_fft(gen.S, L, specs, True, want_g):
        per = _lib.cells_per_group(n_fft) if n_fft in (512, 1024) else None
        lay = PlanLayout(n_fft, gen.S, L, items, True, want_y, want_g, kw.get("align", False),
                         kw.get("true_len"), cells_per_group=per)
        yield lay, (len(specs) * L if want_y else lay.head_elems), (L if want_y else lay.xc_n)


@pytest.mark.parametrize("case", CASES)
def test_every_offset_stays_inside_its_buffer(case):
    for lay, out_elems, out_len in _layouts(case):
        S, L, B = lay.S, lay.L, lay.B
        assert len(lay.packed) == len(lay.order) == sum(lay.split)
        real = lay.order >= 0
        assert sorted(lay.order[real].tolist()) == list(range(len(lay.cells)))
        assert lay.packed[real].tobytes() == lay.cells[lay.order[real]].tobytes()
        c = lay.packed[real]
        T = 1 + L // c["hop"].astype(np.int64)
        assert (c["y_offset"] >= 0).all() and (c["y_offset"] + T * B <= lay.y_elems).all()
        assert (c["noise_offset"] >= 0).all() and (c["noise_stride"] >= 0).all()
        assert (c["noise_offset"] + B + (T - 1) * c["noise_stride"] <= lay.pool_elems).all()
        assert (c["clean_offset"] >= 0).all() and (c["clean_offset"] + L <= S * L).all()
        out = c["out_offset"][c["out_offset"] >= 0]
        assert (c["out_offset"] >= -1).all() and (out + out_len <= out_elems).all()
        assert len(out) in (0, len(c)) and len(set(out.tolist())) == len(out)
        g = c["gain_offset"] >= 0
        assert (c["gain_offset"] >= -1).all()
        assert (c["gain_offset"][g] + (T * B)[g] <= lay.g_elems).all()
        pad = lay.packed[~real]
        assert (pad["algo"] == -1).all()
        assert (pad["out_offset"] == -1).all() and (pad["gain_offset"] == -1).all()
        # padding stages its group's rows: those offsets are dereferenced too
        Tp = 1 + L // pad["hop"].astype(np.int64)
        assert (pad["y_offset"] + Tp * B <= lay.y_elems).all()
        assert (pad["noise_offset"] + B + (Tp - 1) * pad["noise_stride"] <= lay.pool_elems).all()
        assert (pad["clean_offset"] + L <= S * L).all()
        # finish jobs: S signals of src_frames (out_frames) rows each
        j = lay.jobs
        assert sum(n for _, n in lay.hop_jobs.values()) == len(j) == len(lay.keys)
        src, dst = j["src_frames"].astype(np.int64) * B, j["out_frames"].astype(np.int64) * B
        assert (j["src_offset"] >= 0).all() and (j["src_offset"] + S * src <= lay.raw_elems).all()
        assert (j["dst_offset"] >= 0).all() and (j["dst_offset"] + S * dst <= lay.pool_elems).all()
        at = np.argsort(j["dst_offset"])
        ends = (j["dst_offset"] + S * dst)[at]
        assert (ends[:-1] <= j["dst_offset"][at][1:]).all()


def test_validation_errors_stay():
    from classical_speech_enhancement_amd.layout import PlanLayout
    p = dict(alpha=1.0, beta=0.05, n_fft=512, hop_length=128, noise_percentile=20.0,
             noise_method="true_noise")
    items = [(0, 0, "spectralSubtractor", p)]
    for true_len in (0, 8001):
        with pytest.raises(ValueError, match="true_len"):
            PlanLayout(512, 1, 8000, items, True, False, False, true_len=true_len,
                       cells_per_group=16)
    with pytest.raises(ValueError, match="TrueNoiseEstimator requires clean_audio"):
        PlanLayout(512, 1, 8000, items, False, False, False, cells_per_group=16)


def test_layout_module_is_host_only():
    """layout.py imports neither torch nor the loaded library."""
    import ast
    path = os.path.join(os.path.dirname(_lib.__file__), "layout.py")
    tree = ast.parse(open(path).read())
    names = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import)
             for a in n.names}
    names |= {n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert "torch" not in names and names <= {"math", "os", "collections", "numpy", ""}
