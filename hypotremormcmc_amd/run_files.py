"""The files of a step-5 run, read and written in one place for the driver and for the programs that analyse a finished
run (statistics, diagnose, ellipsoid, density, locate): the window list, the per-rank sample files and their record layout,
the device selection, and the number-or-NaN text field of their output files."""
import os

import numpy as np

from .param import Param


def sample_byte_order(endian=None):
    """'<' or '>' for the unformatted output files.  The reference's stock gfortran Makefile builds with
    -fconvert=big-endian (src/Makefile:7-9), so a step 6 built that way expects big-endian sample files; any other
    build reads native little-endian.  HTM_SAMPLE_ENDIAN=big|little (default little) picks the writer's order."""
    e = (endian or os.environ.get("HTM_SAMPLE_ENDIAN") or "little").strip().lower()
    if e in ("big", "big_endian", "big-endian", ">"):
        return ">"
    if e in ("little", "little_endian", "little-endian", "native", "<"):
        return "<"
    raise ValueError("HTM_SAMPLE_ENDIAN must be big or little, got %r" % e)


def record_dtype(n_val: int, endian=None):
    """stream-unformatted records [int32 iteration][n_val float64] (src/hypo_tremor_mcmc.f90:216-233,:270-280), packed:
    4 + 8 n_val bytes; byte order: sample_byte_order"""
    bo = sample_byte_order(endian)
    return np.dtype([("it", bo + "i4"), ("v", bo + "f8", (n_val,))])


def read_sample_file(path: str, n_val: int, endian=None):
    """iterations [n_rec] int32 and values [n_rec][n_val] float64 of a sample file"""
    a = np.fromfile(path, dtype=record_dtype(n_val, endian))
    return a["it"].astype(np.int32), a["v"].reshape(len(a), n_val).astype(np.float64)


def write_sample_file(path: str, iters, values, endian=None):
    """values [n_rec] or [n_rec][n_val] with their iterations, as the records read_sample_file reads"""
    v = np.asarray(values, dtype=np.float64)
    v = v[:, None] if v.ndim == 1 else v
    a = np.zeros(len(v), dtype=record_dtype(v.shape[1], endian))
    a["it"], a["v"] = iters, v
    a.tofile(path)


def read_window_ids(path: str):
    """the window ids of selected_win.dat or a file like it: the first token, as int, of every line that is neither blank nor
    starts with `#`.  The reference reads `id, dummy` per line (src/hypo_tremor_mcmc.f90:82); the second column is not used."""
    with open(path) as fh:
        return [int(ln.split()[0]) for ln in fh if ln.strip() and not ln.lstrip().startswith("#")]


def device_from_env() -> int:
    """HTM_DEVICE=<n> (default 0): the device of every program"""
    return int(os.environ.get("HTM_DEVICE", "0"))


def field(v, width: int, decimals: int = 6) -> str:
    """a number in `width` characters, or the word NaN in the same width"""
    return "%*s" % (width, "NaN") if np.isnan(v) else "%*.*f" % (width, decimals, v)


class Step5Run:
    """A finished step-5 run: the parameter file `par`, its directory `work` (where the run's files lie), the window ids and
    the device to analyse it on; n_procs, n_sta and n_events follow from them."""

    def __init__(self, par, work, win_id, device=0):
        self.par, self.work, self.win_id, self.device = par, work, win_id, device
        self.n_procs, self.n_sta, self.n_events = par.get_n_procs(), par.n_stations, len(win_id)

    @classmethod
    def open(cls, parameter_file, windows=None):
        """`windows`: a file of window ids (default: selected_win.dat next to the parameter file); the device: HTM_DEVICE"""
        par, work = Param(parameter_file), os.path.dirname(os.path.abspath(parameter_file))
        return cls(par, work, read_window_ids(windows or os.path.join(work, "selected_win.dat")), device_from_env())

    def samples(self, names, likelihood=False):
        """(iters [n_rec], {name: [n_rec][width]}): every rank's NAME.RR.out for every name of `names`, stacked in rank order
        (the reference's gather).  All files of a rank must record the same iterations.  With `likelihood` also
        "likelihood": the part of likelihoodRR.out after the burn-in, which must record them too."""
        width = {"vs": 1, "qs": 1, "t_corr": self.n_sta, "a_corr": self.n_sta, "hypo": 3 * self.n_events}
        its, parts = [], {nm: [] for nm in names}
        for r in range(self.n_procs):
            it_r = None
            for nm in names:
                it, v = read_sample_file(os.path.join(self.work, "%s.%02d.out" % (nm, r)), width[nm])
                if it_r is not None and not np.array_equal(it, it_r):
                    raise ValueError(f"{nm}.{r:02d}.out records other iterations than {names[0]}.{r:02d}.out")
                it_r = it
                parts[nm].append(v)
            if likelihood:
                it, v = read_sample_file(os.path.join(self.work, "likelihood%02d.out" % r), 1)
                keep = it > self.par.get_n_burn()      # the trace also covers the burn-in (src/hypo_tremor_mcmc.f90:270-280)
                if not np.array_equal(it[keep], it_r):
                    raise ValueError(f"likelihood{r:02d}.out records other iterations after the burn-in than {names[0]}.{r:02d}.out")
                parts.setdefault("likelihood", []).append(v[keep])
            its.append(it_r)
        return np.concatenate(its), {nm: np.concatenate(p, axis=0) for nm, p in parts.items()}
