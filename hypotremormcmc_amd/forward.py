"""Host mirror of `type forward` (reference src/cls_forward.f90:6-41) over the HIP C ABI.

Same constructor keywords and bound-procedure names / argument order as the reference so that callers
(and the parity tests) read like reference code.  Arrays follow the reference layout: observation arrays
are (n_sta, n_events) column-major, i.e. NumPy shape (n_events, n_sta) C-order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr


def _arr(a, n=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


class ObsArrays:
    """What `obs%get_t_obs() .. get_a_stdv()` return (src/cls_forward.f90:71-74)."""

    def __init__(self, t_obs, t_stdv, a_obs, a_stdv):
        self.t_obs, self.t_stdv, self.a_obs, self.a_stdv = t_obs, t_stdv, a_obs, a_stdv

    def get_t_obs(self): return self.t_obs
    def get_t_stdv(self): return self.t_stdv
    def get_a_obs(self): return self.a_obs
    def get_a_stdv(self): return self.a_stdv


class Forward:
    def __init__(self, n_sta, n_events, sta_x, sta_y, sta_z, obs, use_amp=True, use_time=True, device=0,
                 forward_precision="fp64"):
        self._lib = _lib.load()
        self.n_sta, self.n_events = int(n_sta), int(n_events)
        n = self.n_sta * self.n_events
        arrs = [_arr(sta_x, n_sta), _arr(sta_y, n_sta), _arr(sta_z, n_sta), _arr(obs.get_t_obs(), n),
                _arr(obs.get_t_stdv(), n), _arr(obs.get_a_obs(), n), _arr(obs.get_a_stdv(), n)]
        h = C.c_void_p()
        check(self._lib.htm_forward_create(self.n_sta, self.n_events, *[ptr(a) for a in arrs],
                                           int(bool(use_time)), int(bool(use_amp)), int(device), C.byref(h)))
        self.handle = h
        self.device = device
        self.forward_precision = "fp64"
        self.locate_precision = "fp64"
        if str(forward_precision).lower() in ("fp32", "f32", "single"):
            self.set_precision("fp32")

    def close(self):
        if getattr(self, "handle", None):
            self._lib.htm_forward_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_precision(self, precision: str):
        """"fp32": single-precision forward model with fp64 sums and accept (BASELINE configs[4]); "fp64": the reference's
        arithmetic.  The reference has no such mode; the library's is pinned term by term against a numpy.longdouble
        restatement of it (tests/fp32_restatement.py, tests/test_gpu_fp32_terms.py) and statistically against the fp64 run
        (tests/test_gpu_fp32.py).  For n_sta <= 128: more stations raise HtmError and leave the handle in fp64.  Before
        creating chains."""
        fp32 = str(precision).lower() in ("fp32", "f32", "single")
        check(self._lib.htm_forward_set_precision(self.handle, int(fp32)))
        self.forward_precision = "fp32" if fp32 else "fp64"

    def set_locate_precision(self, precision: str):
        """The arithmetic of `locate.locate`, `locate_marginal` and `draw_evidence` on this object, and of nothing else: "fp32"
        forms the synthetic travel time and amplitude of a (cell, station) in single precision and keeps observations, sums
        and everything behind a cell's term fp64 (pinned by tests/locate_fp32_restatement.py); "fp64", a new
        object's setting, is the arithmetic they have without it, bit for bit.  Independent of `set_precision`, which is step
        5's; any number of stations.  Remembered in `locate_precision`."""
        p = str(precision).lower()
        if p not in ("fp32", "fp64"):
            raise ValueError(f"locate precision {precision!r}: need 'fp32' or 'fp64'")
        check(self._lib.htm_forward_locate_set_precision(self.handle, int(p == "fp32")))
        self.locate_precision = p

    def locate_stack(self, n_draws, t_corr, vs, a_corr, qs, grid9, prior5, layer, n_layer, loc, marg, xy, xz, yz, stack, tally):
        """htm_forward_locate_stack on this object (include/htm_hip.h): contiguous float64 arrays as the
        library takes them, `layer` int32 or None, None for an output that is not asked for.  `locate.stack` prepares them."""
        check(self._lib.htm_forward_locate_stack(self.handle, int(n_draws), ptr(t_corr), ptr(vs), ptr(a_corr), ptr(qs), ptr(grid9), ptr(prior5),
                                                 None if layer is None else layer.ctypes.data_as(_lib.ip), int(n_layer), ptr(loc), ptr(marg),
                                                 ptr(xy), ptr(xz), ptr(yz), ptr(stack), ptr(tally)))

    def locate_residuals(self, t_corr, vs, a_corr, qs, grid9, prior5, loc, marg, res, fit):
        """htm_forward_locate_residuals on this object (include/htm_hip.h): contiguous float64 arrays as the
        library takes them, None for loc or marg that is not asked for.  `locate.residuals` prepares them."""
        check(self._lib.htm_forward_locate_residuals(self.handle, ptr(t_corr), float(vs), ptr(a_corr), float(qs), ptr(grid9), ptr(prior5), ptr(loc),
                                                     ptr(marg), ptr(res), ptr(fit)))

    def obs_pack_bytes(self) -> int:
        """Bytes of the packed per-event observation records (the specialised chain master's; 0: none were built)."""
        n = C.c_int64(0)
        check(self._lib.htm_forward_obs_pack_bytes(self.handle, C.byref(n)))
        return int(n.value)

    def set_stream(self, hip_stream: int):
        """Use the caller's HIP stream (0 = the default stream, e.g. torch.cuda.current_stream().cuda_stream)."""
        check(self._lib.htm_forward_set_stream(self.handle, C.c_void_p(int(hip_stream))))

    def reset_stream(self):
        check(self._lib.htm_forward_reset_stream(self.handle))

    def sync(self):
        check(self._lib.htm_forward_sync(self.handle))

    # -- reference bound procedures -------------------------------------------------------------------
    def calc_log_likelihood(self, hypo, t_corr, vs, a_corr, qs) -> float:
        out = C.c_double()
        check(self._lib.htm_forward_loglik_full(self.handle, ptr(_arr(hypo, 3 * self.n_events)),
                                                ptr(_arr(t_corr, self.n_sta)), float(vs),
                                                ptr(_arr(a_corr, self.n_sta)), float(qs), C.byref(out)))
        return out.value

    def partially_update_log_likelihood(self, evt_id, hypo_old, log_likelihood_old, hypo, t_corr, vs, a_corr,
                                        qs) -> float:
        ho = _arr(hypo_old, 3 * self.n_events)
        hn = _arr(hypo, 3 * self.n_events)
        e = int(evt_id)
        if not 1 <= e <= self.n_events:
            raise ValueError(f"evt_id {e} out of range 1..{self.n_events}")
        xo = np.ascontiguousarray(ho[3 * (e - 1):3 * e])
        xn = np.ascontiguousarray(hn[3 * (e - 1):3 * e])
        out = C.c_double()
        check(self._lib.htm_forward_loglik_partial(self.handle, e, ptr(xo), float(log_likelihood_old), ptr(xn),
                                                   ptr(_arr(t_corr, self.n_sta)), float(vs),
                                                   ptr(_arr(a_corr, self.n_sta)), float(qs), C.byref(out)))
        return out.value

    def calc_travel_time(self, hypo, t_corr, vs) -> np.ndarray:
        out = np.empty((self.n_events, self.n_sta))
        check(self._lib.htm_forward_travel_time(self.handle, ptr(_arr(hypo, 3 * self.n_events)),
                                                ptr(_arr(t_corr, self.n_sta)), float(vs), ptr(out)))
        return out

    def calc_amp(self, hypo, a_corr, qs, vs) -> np.ndarray:
        out = np.empty((self.n_events, self.n_sta))
        check(self._lib.htm_forward_amp(self.handle, ptr(_arr(hypo, 3 * self.n_events)),
                                        ptr(_arr(a_corr, self.n_sta)), float(qs), float(vs), ptr(out)))
        return out

    def calc_travel_time_single(self, evt_id, hypo, t_corr, vs) -> np.ndarray:
        out = np.empty(self.n_sta)
        check(self._lib.htm_forward_travel_time_single(self.handle, int(evt_id), ptr(_arr(hypo, 3 * self.n_events)),
                                                       ptr(_arr(t_corr, self.n_sta)), float(vs), ptr(out)))
        return out

    def calc_amp_single(self, evt_id, hypo, a_corr, qs, vs) -> np.ndarray:
        out = np.empty(self.n_sta)
        check(self._lib.htm_forward_amp_single(self.handle, int(evt_id), ptr(_arr(hypo, 3 * self.n_events)),
                                               ptr(_arr(a_corr, self.n_sta)), float(qs), float(vs), ptr(out)))
        return out

    # -- batched extension ----------------------------------------------------------------------------
    def calc_log_likelihood_batch(self, hypo, t_corr, vs, a_corr, qs) -> np.ndarray:
        vs = _arr(vs)
        n = vs.size
        out = np.empty(n)
        check(self._lib.htm_forward_loglik_full_batch(self.handle, n, ptr(_arr(hypo, n * 3 * self.n_events)),
                                                      ptr(_arr(t_corr, n * self.n_sta)), ptr(vs),
                                                      ptr(_arr(a_corr, n * self.n_sta)), ptr(_arr(qs, n)), ptr(out)))
        return out

    def calc_log_likelihood_batch_dev(self, n, d_hypo, d_t_corr, d_vs, d_a_corr, d_qs, d_out):
        """All arguments are device pointers (ints); asynchronous on the handle's stream."""
        check(self._lib.htm_forward_loglik_full_batch_dev(self.handle, int(n), d_hypo, d_t_corr, d_vs, d_a_corr,
                                                          d_qs, d_out))

    def time_full_batch_dev(self, n, d_hypo, d_t_corr, d_vs, d_a_corr, d_qs, d_out, reps) -> float:
        us = C.c_double()
        check(self._lib.htm_forward_time_full_batch_dev(self.handle, int(n), d_hypo, d_t_corr, d_vs, d_a_corr,
                                                        d_qs, d_out, int(reps), C.byref(us)))
        return us.value
