"""The optional score families of the sweep, one record each.

A family is a group of per-cell scores behind one keyword (quality=True, ...):
a plan class in metrics.py, a run of table columns after the NCOL every table
has, objectives for select_best, and a group of keys in the result rows and the
summary.  Everything search.py, results.py and metrics.py need to know about
one is its record in FAMILIES, in table order; their loops over the records do
for every family what was once written out per family.  STOI is not a family:
it owns column 3 of every table and the ``extended`` switch.  Host-only, like
trackers.py and layout.py: neither torch nor a loaded library.

A further family touches: its header and .hip file (which starts from
csrc/cse_cells.hpp: the frames, the window, a cell's samples, the frame count,
the trimmed mean and the entry points' argument checks; csrc/cse_segfft.hpp on
top of it for the critical-band transform), the build's source list, a plan
class in metrics.py (with calculate_<name> for each of its names), one record
here, one keyword in each public signature, and its tests and documents.
"""

from collections import OrderedDict
from typing import NamedTuple

NCOL = 6  # the columns every table has (search.RECORD_FIELDS without cell_id)


class Family(NamedTuple):
    flag: str               # the keyword, and the word in select_best's message
    names: tuple            # the objectives, in column order
    first: int              # the first table column
    sign: int               # +1: maximised; -1: minimised (the scan runs on the negated column)
    finite_only: bool       # select_best also skips +-inf, and rows hold None for them
    tolerance: dict         # objective -> step of the best-so-far scan
    plan: str               # the class in metrics
    plan_takes_noisy: bool  # the sweep builds the plan with the batch's noisy signals too
    lead: str               # the objective whose winner run_sweep writes and reports
    tag: str                # that winner's spelling in snr_<tag>opt and <other>_<tag>opt
    baselines: tuple        # the names that get a <name>_noisy
    row_args: tuple         # result_row's keywords, in the row's key order
    all_or_none: bool       # result_row refuses a part of the keywords


# tolerances: segsnr / fwsegsnr (dB) take the reference's step for PESQ, the
# quality objective they stand in for; llr / cep carry that step of 1e-3 on a
# 5-wide scale to a 2-wide and a 10-wide one; sisdr / sisir / sisar (dB) take the
# step of the other dB objectives; wss carries the PESQ step to a scale about
# 100 wide (2e-2), rounded down to a power of ten
FAMILIES = OrderedDict((f.flag, f) for f in (
    # include/cse_segsnr.h: dB values clamped to [-10, 35]
    Family("quality", ("segsnr", "fwsegsnr"), NCOL, +1, False,
           {"segsnr": 1e-3, "fwsegsnr": 1e-3}, "SegSnrPlan", False, "fwsegsnr", "fwseg",
           ("segsnr", "fwsegsnr"),
           ("segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best", "fwsegsnr_params", "snr_fwsegopt"),
           False),
    # include/cse_lpc.h: lower is better
    Family("distortion", ("llr", "cep"), NCOL + 2, -1, False,
           {"llr": 1e-4, "cep": 1e-3}, "LpcPlan", False, "llr", "llr", ("llr", "cep"),
           ("llr_noisy", "cep_noisy", "llr_best", "llr_params", "snr_llropt"), False),
    # include/cse_sisdr.h: unbounded dB values that may be +-inf or NaN; the
    # interference is the pair's own noisy - clean, and the unprocessed input's
    # SI-SIR and SI-SAR carry no meaning
    Family("separation", ("sisdr", "sisir", "sisar"), NCOL + 4, +1, True,
           {"sisdr": 1e-3, "sisir": 1e-3, "sisar": 1e-3}, "SiSdrPlan", True, "sisdr", "sisdr",
           ("sisdr",),
           ("sisdr_noisy", "sisdr_best", "sisir_sisdropt", "sisar_sisdropt", "sisdr_params",
            "snr_sisdropt"), False),
    # include/cse_wss.h: lower is better
    Family("wss", ("wss",), NCOL + 7, -1, False, {"wss": 1e-2}, "WssPlan", False, "wss", "wss",
           ("wss",), ("wss_noisy", "wss_best", "wss_params", "snr_wssopt"), True),
))
# objective -> its family
OBJECTIVES = {name: f for f in FAMILIES.values() for name in f.names}


def requested(**flags):
    """The records whose keyword is set, in table order."""
    return tuple(f for f in FAMILIES.values() if flags.get(f.flag))


def columns(f):
    """objective -> table column."""
    return {name: f.first + k for k, name in enumerate(f.names)}


def width(f):
    """Columns of a table whose last requested family is this one."""
    return f.first + len(f.names)


def row_keys(f):
    """The row's keys for row_args: <x>_params is stored as best_params_<x>."""
    return tuple("best_params_" + a[:-len("_params")] if a.endswith("_params") else a
                 for a in f.row_args)


def summary_keys(f):
    """(summary key, row key) of the family's means: every key but the parameters."""
    return tuple((k + "_mean", k) for k in row_keys(f) if not k.startswith("best_params_"))
