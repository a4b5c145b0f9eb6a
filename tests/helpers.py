"""Shared helpers for the parity tests (fixtures -> inputs)."""
import os

import numpy as np

from hypotremormcmc_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["c1", "c2", "missing", "timeonly", "amponly", "missing64", "fixedcorr", "rejects", "c3", "c4"]


def load_case(name):
    """Returns (fixture npz, SynthData inputs, params dict). Inputs come from the fixture when stored,
    else from the seeded generator (checksum-verified against what the reference was run on)."""
    import hashlib

    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    E, S = (int(v) for v in fx["in_shape"])
    data = synth.make_synthetic(E, S, int(fx["in_seed"]), int(fx["in_n_missing"]))
    if "in_missing_idx" in fx:          # (event, station) pairs whose t_stdv was set to 0 by hand
        idx = fx["in_missing_idx"]
        data.t_stdv[idx[:, 0], idx[:, 1]] = 0.0
    if "in_t_obs" in fx:
        for key in ("sta_x", "sta_y", "sta_z", "t_obs", "t_stdv", "a_obs", "a_stdv"):
            assert np.array_equal(getattr(data, key), fx["in_" + key]), f"generator drift in {key}"
    h = hashlib.sha256()
    for a in (data.sta_x, data.sta_y, data.sta_z, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv):
        h.update(np.ascontiguousarray(a, dtype="<f8").tobytes())
    assert h.hexdigest() == str(fx["in_checksum"]), "synthetic generator no longer reproduces the fixture inputs"
    params = dict(zip(fx["param_keys"].tolist(), fx["param_vals"].tolist()))
    return fx, data, params


def missing_pattern(E, S):
    """(event, station) pairs placed as fixture `missing64` has them, for any shape: the first station of the first event, the
    last station of the last event, one event with every station but one missing, one station missing in every event"""
    e_thin, s_kept, s_gone = E // 2, (2 * S) // 3, S // 4
    pairs = {(0, 0), (E - 1, S - 1)}
    pairs |= {(e_thin, j) for j in range(S) if j != s_kept}
    pairs |= {(i, s_gone) for i in range(E)}
    return np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)


def with_missing(data):
    """the data set with t_stdv = 0 at missing_pattern's entries (the reference's missing-data rule, src/cls_forward.f90:76-92,
    is keyed on t_stdv alone, for both data types)"""
    idx = missing_pattern(data.n_events, data.n_sta)
    data.t_stdv[idx[:, 0], idx[:, 1]] = 0.0
    return data


def write_run_dir(tmp_path, data, params, win_id, stations=None):
    """the station file, param.in and selected_win.dat of a step-5 run of `data` in tmp_path; returns (the parameter file's
    path, the station names)"""
    stations = ["N.S%02d" % j for j in range(data.n_sta)] if stations is None else list(stations)
    (tmp_path / "station_xy.list").write_text("".join(
        "%s %.6f %.6f %.6f 1.0 1.0\n" % (s, x, y, z) for s, x, y, z in zip(stations, data.sta_x, data.sta_y, data.sta_z)))
    (tmp_path / "selected_win.dat").write_text("".join("%d 0.0\n" % w for w in win_id))
    (tmp_path / "param.in").write_text("".join("%s = %s\n" % kv for kv in dict(params, station_file="station_xy.list").items()))
    return str(tmp_path / "param.in"), stations


def write_fake_samples(tmp_path, rank, iters, values):
    """NAME.RR.out of one rank for every name of values = {name: [n_rec][n_val]}, little-endian"""
    from hypotremormcmc_amd.run_files import write_sample_file

    for name, v in values.items():
        write_sample_file(str(tmp_path / ("%s.%02d.out" % (name, rank))), iters, v, endian="little")


def tf(v):
    return str(v).strip().upper().lstrip(".").startswith("T")


class OracleRank:
    """A rank of the job computed by the CPU oracle, in the shape TorchWorld drives."""

    def __init__(self, job, rank, n_procs):
        import torch

        self.job, self.rank, self.n_procs = job, rank, n_procs
        self._rec = np.zeros(job.record_words())
        self.record = torch.from_numpy(self._rec)   # shares memory

    def step_begin(self):
        self.job.rank_begin(self.rank, self._rec)

    def step_end(self, gathered):
        g = gathered.numpy()
        rc = self.job.rank_end(self.rank, np.ascontiguousarray(g))
        assert rc == 0, f"rank_end returned {rc}"

    def drain(self):
        pass

    def counts(self):
        npr = np.zeros(7, np.int64); nac = np.zeros(7, np.int64)
        for c in range(int(self.job.p.n_chains)):
            st = self.job.chain(self.rank, c)
            npr += st["n_propose"]; nac += st["n_accept"]
        return npr, nac


XCORR_CASES = ["xcorr_overlap", "xcorr_gapped"]


def load_xcorr_case(name):
    """Returns (fixture npz, SynthEnvelopes inputs, generator arguments) of a steps-2/3 fixture: the envelopes come
    from the seeded generator, checksum-verified against what the reference was run on."""
    import ast
    import hashlib

    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    gen = {k: ast.literal_eval(v) for k, v in zip(fx["in_gen_keys"].tolist(), fx["in_gen_vals"].tolist())}
    env = synth.make_tremor_envelopes(**gen)
    h = hashlib.sha256(np.ascontiguousarray(env.amps, dtype="<f8").tobytes()).hexdigest()
    assert h == str(fx["in_checksum"]), "tremor envelope generator no longer reproduces the fixture inputs"
    return fx, env, gen
