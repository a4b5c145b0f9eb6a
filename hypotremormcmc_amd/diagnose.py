"""Convergence diagnostics of a step-5 run on the GPU: split R-hat and effective sample size of every parameter
step 6 summarises, from the same sample files (Vehtari et al. 2021 / Stan; `diagnose` is without rank normalisation,
DESIGN.md §3.6, kernels in hypotremormcmc_amd/csrc/htm_diag.hpp; `diagnose_rank` is with it, §3.7, htm_rank.hpp).

    python -m hypotremormcmc_amd.diagnose <parameter file> [--max-lag N] [--rhat 1.01] [--rank]

run in the directory of the step-5 outputs, writes `convergence.stat` next to the `.stat` files of
`hypotremormcmc_amd.statistics`: one line per parameter with R-hat, ESS, the autocorrelation time tau (ESS =
samples / tau) and the lag at which Geyer's pair sums went negative (-1: they did not within --max-lag, the ESS is
then an upper bound).  Parameters the job fixes (`solve_vs = F`, ...) are constant and are written as NaN.

With --rank it also writes `convergence_rank.stat`: per parameter the larger of the rank-normalised and the folded
R-hat, the two, the bulk-ESS and the tail-ESS (the smaller ESS of the indicators of the 5 % and the 95 % quantile).  These
see what the plain numbers miss: sequences that differ in scale but not in location, heavy tails, and whether the ends
of the intervals in the `.stat` files were sampled enough.  The column sort works in batches under HTM_RANK_MB MiB of
device memory (default 2048).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import _lib
from .run_files import Step5Run, field
from .statistics import sample_matrix

RANK_STAT_HEADER = "# parameter, R-hat (larger of the next two), rank-normalised R-hat, folded R-hat, bulk-ESS, tail-ESS"
STAT_HEADER = "# parameter, R-hat (split), ESS, tau, lag of the first negative pair sum (-1: none up to the last lag)"


def diagnose(samples, n_seq: int, max_lag: int = 1000, device: int = 0, return_acov: bool = False):
    """[n_par][4] = (rhat, ess, tau, lags) of every column of samples [n_seq * n_draws][n_par], sequence m in rows
    m * n_draws .. (m + 1) * n_draws - 1, on the GPU.  With return_acov also the averaged autocovariances
    [(L + 1)][n_par], L = min(n_draws // 2 - 1, max_lag)."""
    x, n_draws = sample_matrix(samples, "htm_diagnose takes", n_seq=n_seq, max_lag=max_lag)
    if n_draws < 4:
        raise ValueError(f"n_draws = {n_draws}: a sequence needs at least 4 draws to be split")
    n_par = x.shape[1]
    n_lag = min(n_draws // 2 - 1, max_lag) + 1
    out = np.empty((n_par, 4))
    acov = np.empty((n_lag, n_par)) if return_acov else None
    _lib.check(_lib.load().htm_diagnose(device, _lib.ptr(x), int(n_seq), n_draws, n_par, int(max_lag), _lib.ptr(out), _lib.ptr(acov)))
    return (out, acov) if return_acov else out


def rank_normalize(samples, fold: bool = False, return_ranks: bool = False, device: int = 0):
    """z [n_rows][n_par] = Phi^-1((r - 3/8) / (n_rows + 1/4)), r the 1-based average rank of an element within its column
    (of |x - median| with fold), on the GPU.  With return_ranks also r."""
    x, n_rows = sample_matrix(samples, "htm_rank_normalize takes")
    if n_rows < 2:
        raise ValueError(f"n_rows = {n_rows}: ranking needs at least 2 rows")
    z = np.empty_like(x)
    ranks = np.empty_like(x) if return_ranks else None
    _lib.check(_lib.load().htm_rank_normalize(device, _lib.ptr(x), n_rows, x.shape[1], 1 if fold else 0, _lib.ptr(z), _lib.ptr(ranks)))
    return (z, ranks) if return_ranks else z


def diagnose_rank(samples, n_seq: int, max_lag: int = 1000, device: int = 0):
    """[n_par][4] = (rhat_bulk, rhat_folded, ess_bulk, ess_tail) of every column of samples, laid out as for `diagnose`,
    on the GPU.  The R-hat to report is the larger of the first two."""
    x, n_draws = sample_matrix(samples, "htm_diagnose_rank takes", n_seq=n_seq, max_lag=max_lag)
    if n_draws < 4:
        raise ValueError(f"n_draws = {n_draws}: a sequence needs at least 4 draws to be split")
    out = np.empty((x.shape[1], 4))
    _lib.check(_lib.load().htm_diagnose_rank(device, _lib.ptr(x), int(n_seq), n_draws, x.shape[1], int(max_lag), _lib.ptr(out)))
    return out


def sequences_by_iteration(iters, values, k: int):
    """The sequence-major sample matrix `diagnose` takes, from the records of all ranks' sample files.

    iters [n_rec], values [n_rec][n_par]: what `run_files.Step5Run.samples` returns.
    The records are stable-sorted by iteration; every recorded iteration must hold exactly k = n_procs * n_cool
    records (the swaps conserve the multiset of temperatures, so this holds over all ranks although the T = 1 role
    moves between them).  Sequence j is the j-th record of every iteration, so a sequence is a T = 1 *slot*, not one
    chain's trajectory: the diagnostics describe the sample set that step 6 summarises."""
    iters = np.asarray(iters)
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1:
        values = values[:, None]
    if iters.ndim != 1 or len(iters) != len(values):
        raise ValueError(f"{len(iters)} iterations for {len(values)} records")
    order = np.argsort(iters, kind="stable")
    it_u, counts = np.unique(iters[order], return_counts=True)
    bad = np.nonzero(counts != k)[0]
    if len(bad):
        raise ValueError(f"iteration {int(it_u[bad[0]])} holds {int(counts[bad[0]])} records, not n_procs * n_cool = {k}")
    n_it, n_par = len(it_u), values.shape[1]
    return np.ascontiguousarray(values[order].reshape(n_it, k, n_par).transpose(1, 0, 2)).reshape(k * n_it, n_par)


def parameter_names(station_names, win_id):
    names = ["vs", "qs"]
    names += ["t_corr %s" % s.strip() for s in station_names]
    names += ["a_corr %s" % s.strip() for s in station_names]
    names += ["%s %d" % (c, w) for w in win_id for c in "xyz"]
    return names + ["log_likelihood"]


def stat_text(names, out) -> str:
    """the text of convergence.stat for out [n_par][4]; a row of NaN (a constant column) is written as NaN"""
    lines = [STAT_HEADER]
    for name, row in zip(names, np.asarray(out, dtype=np.float64)):
        rhat, ess, tau, lags = row if not np.isnan(row[0]) else [np.nan] * 4
        lines.append("%-24s" % name + field(rhat, 13) + field(ess, 13) + field(tau, 13) + field(lags, 7, 0))
    return "\n".join(lines) + "\n"


def summary_text(names, out, rhat_limit: float) -> str:
    out = np.asarray(out, dtype=np.float64)
    live = np.nonzero(~np.isnan(out[:, 0]))[0]
    if not len(live):
        return "no parameter varies: nothing to diagnose\n"
    worst, small = live[np.argmax(out[live, 0])], live[np.argmin(out[live, 1])]
    return (f"{len(live)} parameters ({len(out) - len(live)} constant)\n"
            f"largest R-hat  {out[worst, 0]:.6f}  ({names[worst]})\n"
            f"smallest ESS   {out[small, 1]:.1f}  ({names[small]})\n"
            f"R-hat > {rhat_limit:g}: {int(np.sum(out[live, 0] > rhat_limit))} parameters\n"
            f"pair sums not negative within the lags examined (ESS is an upper bound): "
            f"{int(np.sum(out[live, 3] < 0))} parameters\n")


def rank_stat_text(names, out) -> str:
    """the text of convergence_rank.stat for out [n_par][4] of `diagnose_rank`; an entry that is NaN is written as NaN"""
    lines = [RANK_STAT_HEADER]
    for name, (rb, rf, eb, et) in zip(names, np.asarray(out, dtype=np.float64)):
        rmax = np.fmax(rb, rf)          # of the two that are defined: |x - med| of a two-valued column can be constant
        lines.append("%-24s" % name + "".join(field(v, 13) for v in (rmax, rb, rf, eb, et)))
    return "\n".join(lines) + "\n"


def rank_summary_text(names, out, rhat_limit: float) -> str:
    """three lines: the largest rank R-hat, the smallest bulk-ESS and tail-ESS, the count above the limit"""
    out = np.asarray(out, dtype=np.float64)
    rmax = np.fmax(out[:, 0], out[:, 1])
    live = np.nonzero(~np.isnan(rmax))[0]
    if not len(live):
        return "no parameter varies: no rank-normalised diagnostics\n"
    worst = live[np.argmax(rmax[live])]
    bulks = np.nonzero(~np.isnan(out[:, 2]))[0]
    bulk = bulks[np.argmin(out[bulks, 2])]
    tails = np.nonzero(~np.isnan(out[:, 3]))[0]
    tail_txt = "none defined" if not len(tails) else "%.1f  (%s)" % (out[tails, 3].min(), names[tails[np.argmin(out[tails, 3])]])
    return (f"largest rank-normalised R-hat  {rmax[worst]:.6f}  ({names[worst]})\n"
            f"smallest bulk-ESS  {out[bulk, 2]:.1f}  ({names[bulk]}), smallest tail-ESS  {tail_txt}\n"
            f"rank-normalised R-hat > {rhat_limit:g}: {int(np.sum(rmax[live] > rhat_limit))} parameters\n")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m hypotremormcmc_amd.diagnose", description=__doc__.split("\n\n")[0])
    ap.add_argument("parameter_file")
    ap.add_argument("--max-lag", type=int, default=1000)
    ap.add_argument("--rhat", type=float, default=1.01, help="R-hat above which a parameter is counted in the summary")
    ap.add_argument("--rank", action="store_true", help="also write convergence_rank.stat: rank-normalised R-hat, bulk- and tail-ESS")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    run = Step5Run.open(args.parameter_file)
    work, k = run.work, run.n_procs * run.par.get_n_cool()
    # one sequence-major matrix: columns vs, qs, t_corr, a_corr, hypo, log-likelihood
    iters, s = run.samples(("vs", "qs", "t_corr", "a_corr", "hypo"), likelihood=True)
    x = sequences_by_iteration(iters, np.concatenate(list(s.values()), axis=1), k)
    out = diagnose(x, k, max_lag=args.max_lag, device=run.device)
    names = parameter_names(run.par.stations, run.win_id)
    with open(os.path.join(work, "convergence.stat"), "w") as fh:
        fh.write(stat_text(names, out))
    sys.stdout.write(summary_text(names, out, args.rhat))
    if args.rank:
        rk = diagnose_rank(x, k, max_lag=args.max_lag, device=run.device)
        with open(os.path.join(work, "convergence_rank.stat"), "w") as fh:
            fh.write(rank_stat_text(names, rk))
        sys.stdout.write(rank_summary_text(names, rk, args.rhat))


if __name__ == "__main__":
    main()
