"""The loops over the score families (scores.FAMILIES) in search.engine_compute,
run_sweep and optimize_parameters, on the device: every flag at once gives what
each flag alone gives; needs a GPU.  The comparisons are bit-exact, as the
per-family tests' pairwise ones are: the same kernels run on the same inputs
with the same launch arguments, whichever other families are scored beside them.

The job is the smallest that reaches every loop: three pairs of two lengths (two
length batches, so the two waveform plans alternate, and one batch with two
signal slots), and two n_fft, so a run queues its scores twice.
"""

import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALG = "spectralSubtractor"
GRID = {ALG: dict(alpha=[1.0, 2.0], beta=[0.01], n_fft=[512, 1024], hop_length=[128],
                  noise_percentile=[10.0], noise_method=["percentile"])}
FLAGS = ("quality", "distortion", "separation", "wss")
# first column and width of each family's columns after the NCOL = 6 shared ones
COLUMNS = {"quality": (6, 2), "distortion": (8, 2), "separation": (10, 3), "wss": (13, 1)}
ALL = dict.fromkeys(FLAGS, True)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from classical_speech_enhancement_amd import search
    return search


_JOB = {}


def _job(search):
    """The pairs, the specs and the tables of the plain run, the run with every
    flag and the four runs with one flag each, made once."""
    if not _JOB:
        from classical_speech_enhancement_amd.synth import make_pair
        # pair 3: its first 0.75 s hold speech well above the noise (13 dB), so the
        # sweep's SNR scan, which starts at -1 dB, has a winner (pair 2's have -2 dB)
        pairs = [make_pair(0, seconds=1.0), make_pair(1, seconds=1.0), make_pair(3, seconds=0.75)]
        clean, noisy = [c for c, _ in pairs], [n for _, n in pairs]
        specs = search.job_specs(3, [ALG], GRID)
        ids = np.arange(len(specs))
        _JOB.update(clean=clean, noisy=noisy, specs=specs, ids=ids,
                    plain=search.engine_compute(clean, noisy, specs, ids),
                    all=search.engine_compute(clean, noisy, specs, ids, **ALL),
                    one={f: search.engine_compute(clean, noisy, specs, ids, **{f: True})
                         for f in FLAGS})
    return _JOB


def test_engine_compute_every_flag_equals_each_flag_alone(dev):
    job = _job(dev)
    assert len(job["specs"]) == 12 and len({len(c) for c in job["clean"]}) == 2
    table = job["all"]
    assert dev.NCOL == 6 and table.shape == (12, dev.NCOL + 8)
    assert job["plain"].shape == (12, dev.NCOL)
    assert np.array_equal(table[:, :dev.NCOL], job["plain"], equal_nan=True)
    assert (table[:, 2] == 1).all() and np.isfinite(table[:, 3]).all()
    for flag, (first, n) in COLUMNS.items():
        alone = job["one"][flag]
        assert alone.shape == (12, first + n), flag
        assert np.array_equal(alone[:, :dev.NCOL], job["plain"], equal_nan=True), flag
        assert np.isnan(alone[:, dev.NCOL:first]).all(), flag  # what was not asked for
        assert not np.isnan(alone[:, first:first + n]).any(), flag
        assert np.array_equal(table[:, first:first + n], alone[:, first:first + n],
                              equal_nan=True), flag


def test_engine_compute_without_stoi(dev):
    job = _job(dev)
    table = dev.engine_compute(job["clean"], job["noisy"], job["specs"], job["ids"], stoi=False,
                               **ALL)
    assert table.shape == job["all"].shape
    assert np.isnan(table[:, 3]).all()
    rest = [c for c in range(table.shape[1]) if c != 3]
    assert np.array_equal(table[:, rest], job["all"][:, rest], equal_nan=True)


def test_run_sweep_every_flag_equals_each_flag_alone(dev, tmp_path):
    job = _job(dev)
    clean, noisy = [job["clean"][2]], [job["noisy"][2]]
    rows = dev.run_sweep(clean, noisy, ["p02"], str(tmp_path / "all"), grids=GRID, **ALL)
    assert len(rows) == 1
    row = rows[0]
    seen = set()
    for flag in FLAGS:
        alone = dev.run_sweep(clean, noisy, ["p02"], str(tmp_path / flag), grids=GRID,
                              **{flag: True})[0]
        assert set(alone) <= set(row), flag
        for key, value in alone.items():
            assert row[key] == value, (flag, key)
        seen |= set(alone)
    assert seen == set(row)
    assert list(row)[-20:] == [
        "segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best", "best_params_fwsegsnr", "snr_fwsegopt",
        "llr_noisy", "cep_noisy", "llr_best", "best_params_llr", "snr_llropt",
        "sisdr_noisy", "sisdr_best", "sisir_sisdropt", "sisar_sisdropt", "best_params_sisdr",
        "snr_sisdropt", "wss_noisy", "wss_best", "best_params_wss", "snr_wssopt"]
    assert all(row[k] is not None for k in ("fwsegsnr_best", "llr_best", "sisdr_best", "wss_best"))
    for tag in ("snr", "stoi", "fwsegsnr", "llr", "sisdr", "wss"):
        assert os.path.exists(os.path.join(tmp_path, "all", f"results_{ALG}",
                                           f"p02_{ALG}_optimized_{tag}.wav")), tag
    means = json.load(open(os.path.join(tmp_path, "all", "results_summary",
                                        "summary_means.json")))[ALG]
    for key in ("segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best", "snr_fwsegopt",
                "llr_noisy", "cep_noisy", "llr_best", "snr_llropt",
                "sisdr_noisy", "sisdr_best", "sisir_sisdropt", "sisar_sisdropt", "snr_sisdropt",
                "wss_noisy", "wss_best", "snr_wssopt"):
        assert means[key + "_mean"] == row[key], key


def test_optimize_parameters_three_flags_equal_each_flag_alone(dev):
    job = _job(dev)
    clean, noisy = job["clean"][2], job["noisy"][2]
    names = {"quality": ("segsnr", "fwsegsnr"), "distortion": ("llr", "cep"),
             "separation": ("sisdr", "sisir", "sisar")}
    res = dev.optimize_parameters(clean, noisy, 16000, ALG, GRID[ALG],
                                  **dict.fromkeys(names, True))
    assert res["table"].shape == (4, dev.NCOL + 7)
    for flag, objectives in names.items():
        alone = dev.optimize_parameters(clean, noisy, 16000, ALG, GRID[ALG], **{flag: True})
        for name in objectives:
            assert res[name] is not None and res[name] == alone[name], name
            assert (name in res["baseline"]) == (name != "sisir" and name != "sisar"), name
            for part in ("baseline", "improvements"):
                assert (name in res[part]) == (name in alone[part]), (part, name)
                if name in alone[part]:
                    assert res[part][name] == alone[part][name], (part, name)
    assert set(res["baseline"]) == {"snr", "stoi", "segsnr", "fwsegsnr", "llr", "cep", "sisdr"}
    assert "wss" not in res
