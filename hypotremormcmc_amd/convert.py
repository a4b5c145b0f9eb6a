"""Step 1 on the HIP path: `hypo_tremor_convert` (reference src/hypo_tremor_convert.f90, src/cls_convertor.f90,
src/cls_c3_data.f90, src/mod_signal_process.f90) -- raw two-component SAC waveforms to the smoothed envelopes step 2
reads.

    python -m hypotremormcmc_amd.convert <parameter file>

Inputs as the reference reads them (paths relative to the working directory):

  * required keys n_procs station_file data_dir time_id_file cmp1 cmp2 filename_format t_win_conv
    (src/cls_param.f90:113-116); the amplitude factors are columns 5 and 6 of the station file;
  * every line of time_id_file is one time ID, trailing blanks trimmed (src/cls_param.f90:394-425);
  * file names: data_dir + "/" + the "+"-separated tokens of filename_format with $STA, $ID and $CMP replaced
    (src/cls_param.f90:699-740), e.g. `$STA+/+$ID+.+$CMP` -> data/STA/ID.EH1;
  * SAC files (src/cls_c3_data.f90:108-180): delta float32 at byte 0, npts int32 at byte 316, float32 samples from
    byte 632.  A station's files are joined end to end in time-ID order.  dt = dble(delta) of the first time ID; the
    files of later IDs must agree within 1.e-6 (a single-precision literal).  Byte order: each file's own, detected
    from the header version nvhdr (int32 at byte 304; 6 or 7) -- the stock reference build reads big-endian files.

Output: `<sta>.merged.env` in the working directory, (time, value) float64 pairs, little-endian; value k is the merged
envelope at stream sample k n_fac and its time is k (dt n_fac) (src/cls_convertor.f90:262-275).

Constants from dt (src/cls_convertor.f90:104-115, :207-210, :23-26): n = nint(t_win_conv / dt), a multiple of 4;
n_fac = nint(1 / dt); h = int(1.5 / dt); band edges 1, 3, 8, 10 Hz at bins nint(f / df), df = 1 / (n dt).

Everything is computed on the GPU (`htm_convert_dev`: detrend, taper, a packed forward FFT, band and analytic
factor, two backward FFTs, |y/n|, two box smoothings and the merge); there is no CPU fallback.  The segments of a
station go in batches whose workspace stays under HTM_CONVERT_MB MiB of device memory (default 512, at least one
segment per batch); the bytes written do not depend on the batch size.  Files are read lazily, a batch at a time.

Deliberate deviations: every station's files are checked (present, valid header, long enough, equal
npts in both components, delta) before the first transform, where the reference stops partway through the job or, for
unequal npts, prints "invalid npts" and reads out of bounds; t_win_conv too short for the decimation carry (n/2 <
n_fac) or for the smoothing (2h > n) is refused, where the reference's index arithmetic goes wrong.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import check
from .correlate import nint
from .param import Param
from .run_files import device_from_env

DEFAULT_CONVERT_MB = 512
BAND_HZ = (1.0, 3.0, 8.0, 10.0)                 # src/cls_convertor.f90:23-26
SAC_DATA = 632                                  # 158 header words of 4 bytes
DELTA_TOL = float(np.float32(1.0e-6))           # the reference's single-precision literal 1.e-6
MAX_H = 4096                                    # kCvMaxH of htm_convert.hpp


def read_time_ids(path):
    """every line is one ID, trailing blanks trimmed (blank lines included, as the reference counts them)"""
    if not os.path.exists(path):
        raise SystemExit(f"ERROR: cannot open {path}")
    with open(path) as f:
        text = f.read()
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return [ln.rstrip(" ") for ln in lines]


def expand_filename(data_dir, filename_format, sta, tid, cmp):
    """src/cls_param.f90:699-740: data_dir // "/" then every "+" token, $ID / $STA / $CMP replaced"""
    name = data_dir.rstrip(" ") + "/"
    for tok in filename_format.split("+"):
        tok = tok.rstrip(" ")
        name += {"$ID": tid, "$STA": sta, "$CMP": cmp}.get(tok, tok)
    return name


@dataclass
class SacFile:
    path: str
    delta: float        # dble of the float32 header value
    npts: int
    order: str          # "<" or ">"

    def read(self, i0=0, i1=None):
        """float32 samples [i0, i1) in native order"""
        i1 = self.npts if i1 is None else i1
        v = np.fromfile(self.path, dtype=self.order + "f4", count=i1 - i0, offset=SAC_DATA + 4 * i0)
        return v.astype(np.float32)


def read_sac_header(path):
    """-> SacFile; refuses (naming the file) a missing file, a header version that is 6 or 7 in neither byte order,
    and a file shorter than 632 + 4 npts bytes"""
    if not os.path.exists(path):
        raise SystemExit(f"ERROR: cannot open: {path}")
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(SAC_DATA)
    if len(head) < SAC_DATA:
        raise SystemExit(f"ERROR: {path} is shorter than a SAC header ({size} < {SAC_DATA} bytes)")
    order = None
    for o in ("<", ">"):
        if int(np.frombuffer(head, dtype=o + "i4", count=1, offset=304)[0]) in (6, 7):
            order = o
            break
    if order is None:
        raise SystemExit(f"ERROR: {path} is not a SAC file (header version nvhdr is 6 or 7 in neither byte order)")
    delta = float(np.frombuffer(head, dtype=order + "f4", count=1, offset=0)[0])
    npts = int(np.frombuffer(head, dtype=order + "i4", count=1, offset=316)[0])
    if npts < 0 or size < SAC_DATA + 4 * npts:
        raise SystemExit(f"ERROR: {path} holds fewer than npts = {npts} samples ({size} bytes)")
    return SacFile(path, delta, npts, order)


@dataclass
class Constants:
    dt: float
    n: int
    n_fac: int
    h: int
    k_band: tuple

    @property
    def dt_out(self):
        return self.dt * self.n_fac


def constants(dt, t_win):
    """(n, n_fac, h, band bins) of src/cls_convertor.f90:104-115, :207-210, :320-324 from dt = dble(float32 delta)"""
    n = nint(t_win / dt)
    n_fac = nint(1.0 / dt / 1)                 # n_sps = 1
    h = int(1.5 / dt)
    df = 1.0 / (n * dt)
    return Constants(dt, n, n_fac, h, tuple(nint(f / df) for f in BAND_HZ))


def check_constants(c: Constants, n_total: int, name: str = ""):
    """the reference's stops, and this build's refusals of lengths its index arithmetic does not cover"""
    where = f" (station {name})" if name else ""
    if c.n % 2:
        raise SystemExit("ERROR: n2 + n2 /= self%n" + where)
    if c.n % 4:
        raise SystemExit("ERROR: n4 * 4 /= self%n" + where)
    if c.n_fac < 1:
        raise SystemExit(f"ERROR: n_fac = nint(1/dt) = {c.n_fac} < 1 (dt = {c.dt}){where}")
    if n_total < c.n:
        raise SystemExit(f"ERROR: data length is not enough in queue (N = {n_total} < n = {c.n}){where}")
    if c.n // 2 < c.n_fac:
        raise SystemExit(f"ERROR: t_win_conv too short: n/2 = {c.n // 2} < n_fac = {c.n_fac}{where}")
    if 2 * c.h > c.n or c.h > MAX_H:
        raise SystemExit(f"ERROR: smoothing half width h = {c.h} needs 2h <= n = {c.n} and h <= {MAX_H}{where}")


def last_segment(n_total, n):
    """index of the last segment, m + 1 with m = (N - n) / n2"""
    return (n_total - n) // (n // 2) + 1


def kept_range(j, n_total, n):
    """[start, end) of the stream samples segment j keeps (first [0, n-n4), middle [n4, n-n4), last [n4, N - j n2)
    in local samples)"""
    n2, n4 = n // 2, n // 4
    start = 0 if j == 0 else j * n2 + n4
    end = n_total if j == last_segment(n_total, n) else j * n2 + n - n4
    return start, end


def outputs(n_total, n, n_fac, j0, j1):
    """(k_base, count): segments j0..j1 write the values ceil(start(j0)/n_fac) .. ceil(end(j1)/n_fac) - 1"""
    k0 = -(-kept_range(j0, n_total, n)[0] // n_fac)
    k1 = -(-kept_range(j1, n_total, n)[1] // n_fac)
    return k0, k1 - k0


def smooth_length(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def batch_segments(n, mb=None):
    """segments per batch whose device memory (workspace of htm_convert_dev, inputs, outputs) stays under
    HTM_CONVERT_MB MiB; at least one"""
    if mb is None:
        mb = float(os.environ.get("HTM_CONVERT_MB", DEFAULT_CONVERT_MB))
    if smooth_length(n):
        per = 80 * n
    else:
        m = 1
        while m < 2 * n - 1:
            m *= 2
        per = 48 * n + 64 * m
    per += 4 * n + 8 * n                       # two float32 components of n/2 new samples, outputs (at most n)
    return max(1, int(mb * (1 << 20)) // per)


@dataclass
class Station:
    name: str
    files: list                 # [(SacFile cmp1, SacFile cmp2)] in time-ID order
    fac: tuple
    c: Constants
    n_total: int
    starts: list = field(default_factory=list)

    def read(self, g0, g1):
        """float32 components of stream samples [g0, g1), read from the files that hold them"""
        x1 = np.empty(g1 - g0, dtype=np.float32)
        x2 = np.empty(g1 - g0, dtype=np.float32)
        for (f1, f2), s in zip(self.files, self.starts):
            a, b = max(g0, s), min(g1, s + f1.npts)
            if a < b:
                x1[a - g0:b - g0] = f1.read(a - s, b - s)
                x2[a - g0:b - g0] = f2.read(a - s, b - s)
        return x1, x2


def plan_station(name, paths, fac, t_win):
    """headers of every file of one station, checked; -> Station"""
    files, dt = [], None
    for i, (p1, p2) in enumerate(paths):
        f1, f2 = read_sac_header(p1), read_sac_header(p2)
        if i == 0:
            dt = f2.delta              # src/cls_c3_data.f90:126-128: the last component of the first ID sets dt
        else:
            for f in (f1, f2):
                if abs(dt - f.delta) > DELTA_TOL:
                    raise SystemExit(f"ERROR: error in SAC header delta (in {f.path})")
        if f1.npts != f2.npts:
            raise SystemExit(f"ERROR: invalid npts: {f1.path} has {f1.npts} samples, {f2.path} has {f2.npts}")
        files.append((f1, f2))
    if not files:
        raise SystemExit(f"ERROR: no time IDs for station {name}")
    starts = list(np.cumsum([0] + [f1.npts for f1, _ in files[:-1]]).tolist())
    n_total = sum(f1.npts for f1, _ in files)
    c = constants(dt, t_win)
    check_constants(c, n_total, name)
    return Station(name, files, tuple(float(v) for v in fac), c, n_total, starts)


def plan(para: Param):
    """every station's files and constants, all checked before the first transform"""
    g = para.values
    ids = read_time_ids(g["time_id_file"])
    stations = []
    for s, name in enumerate(para.stations):
        paths = [tuple(expand_filename(g["data_dir"], g["filename_format"], name, tid, g[key])
                       for key in ("cmp1", "cmp2")) for tid in ids]
        stations.append(plan_station(name, paths, para.sta_amp_fac[s], g["t_win_conv"]))
    return stations


def convert_station(st: Station, out_path, device=0, mb=None, stats=None):
    """all segments of one station on the GPU, in batches; writes out_path"""
    import torch

    c = st.c
    n, n2 = c.n, c.n // 2
    last = last_segment(st.n_total, n)
    b = batch_segments(n, mb)
    lib = _lib.load()
    dev = torch.device("cuda", device)
    kb = (C.c_int * 4)(*c.k_band)
    stats = {} if stats is None else stats
    with open(out_path, "wb") as f, torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        for j0 in range(0, last + 1, b):
            j1 = min(last, j0 + b - 1)
            t0 = time.perf_counter()
            x1, x2 = st.read(j0 * n2, min(st.n_total, j1 * n2 + n))
            t1 = time.perf_counter()
            d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
            k0, cnt = outputs(st.n_total, n, c.n_fac, j0, j1)
            d_out = torch.empty(cnt, dtype=torch.float64, device=dev)
            stream.synchronize()
            t2 = time.perf_counter()
            check(lib.htm_convert_dev(device, C.c_void_p(d1.data_ptr()), C.c_void_p(d2.data_ptr()), st.n_total, n,
                                      c.n_fac, c.h, kb, st.fac[0], st.fac[1], j0, j1, C.c_void_p(d_out.data_ptr()),
                                      C.c_void_p(stream.cuda_stream)))
            v = d_out.cpu().numpy()
            t3 = time.perf_counter()
            rec = np.empty((cnt, 2), dtype="<f8")
            rec[:, 0] = np.arange(k0, k0 + cnt, dtype=np.float64) * c.dt_out
            rec[:, 1] = v
            rec.tofile(f)
            for key, dt_ in (("read", t1 - t0), ("upload", t2 - t1), ("device", t3 - t2),
                             ("write", time.perf_counter() - t3)):
                stats[key] = stats.get(key, 0.0) + dt_
            stats["segments"] = stats.get("segments", 0) + (j1 - j0 + 1)
    return stats


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit("USAGE: hypo_tremor_convert [parameter file]")
    para = Param(argv[0], verb=True, from_where="convert")
    stations = plan(para)
    device = device_from_env()
    for st in stations:
        print(f" {st.name}: N= {st.n_total} n= {st.c.n} n_fac= {st.c.n_fac} segments= "
              f"{last_segment(st.n_total, st.c.n) + 1}", flush=True)
        convert_station(st, f"{st.name}.merged.env", device=device)


if __name__ == "__main__":
    main()
