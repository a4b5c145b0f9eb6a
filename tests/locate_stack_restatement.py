"""A plain numpy restatement of the rule of htm_forward_locate_stack (include/htm_hip.h) for the tests, from
GIVEN log posterior volumes: nothing of the evaluation is restated here (that is tests/locate_restatement.py's).

A window e of layer L_e in 0 .. n_layer - 1 with an included cell puts m_e(c) = exp(lp_e(c) - lp_best,e) / W_e into cell c, W_e
the sum of exp(lp_e - lp_best,e) over its included cells.  The weights and W are formed in numpy.longdouble and the mass is
rounded to double once; a cell's stack is math.fsum over the layer's windows (the exact sum of those doubles, rounded once),
and so is every map cell along its summed axis.  The library's sequential fp64 sums are judged against these by the bounds of
tests/test_gpu_locate_stack.py."""
import math

import numpy as np

from tests import locate_restatement as lr


def masses(vols, lp_best=None):
    """vols [E][nz][ny][nx] -> m [E][nz][ny][nx] (double; zeros for a window without an included cell) and has [E] (whether
    the window has an included cell).  lp_best [E]: the windows' best lp as given (the library's loc[4]); None: the largest
    included lp of the volume"""
    vols = np.asarray(vols, dtype=np.float64)
    m = np.zeros(vols.shape)
    has = np.zeros(vols.shape[0], dtype=bool)
    for e, lp in enumerate(vols):
        inc = lr.included(lp)
        if not inc.any():
            continue
        has[e] = True
        best = np.longdouble(lp[inc].max() if lp_best is None else lp_best[e])
        w = np.zeros(lp.shape, dtype=np.longdouble)
        w[inc] = np.exp(lp[inc].astype(np.longdouble) - best)
        m[e] = (w / w.sum()).astype(np.float64)
    return m, has


def fsum_axis(a, axis):
    """math.fsum along one axis of a"""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
    out = np.empty(a.shape[:-1])
    for idx in np.ndindex(*out.shape):
        out[idx] = math.fsum(a[idx])
    return out


def project(stack):
    """stack [n_layer][nz][ny][nx] -> xy [n_layer][ny][nx], xz [n_layer][nz][nx], yz [n_layer][nz][ny], math.fsum along the
    summed axis"""
    return fsum_axis(stack, 1), fsum_axis(stack, 2), fsum_axis(stack, 3)


def layers_of(layer, n_events, n_layer):
    """the layer of every window, -1 for one that takes no part (None: every window in layer 0, and n_layer must be 1)"""
    if layer is None:
        assert n_layer == 1
        return np.zeros(n_events, dtype=np.int64)
    lay = np.asarray(layer, dtype=np.int64)
    assert lay.shape == (n_events,)
    return np.where((lay >= 0) & (lay < n_layer), lay, -1)


def stack_rule(vols, layer=None, n_layer=1, lp_best=None):
    """the rule: a dict of stack [n_layer][nz][ny][nx], xy, xz, yz, tally [n_layer][2] = windows stacked, windows without an
    included cell, and m [E][nz][ny][nx], the windows' masses (zeros for a window that adds nothing)"""
    m, has = masses(vols, lp_best)
    lay = layers_of(layer, m.shape[0], n_layer)
    m[lay < 0] = 0.0
    stack = np.zeros((n_layer,) + m.shape[1:])
    tally = np.zeros((n_layer, 2))
    for L in range(n_layer):
        sel = lay == L
        tally[L] = [(sel & has).sum(), (sel & ~has).sum()]
        if (sel & has).any():
            stack[L] = fsum_axis(m[sel & has], 0)
    xy, xz, yz = project(stack)
    return {"stack": stack, "xy": xy, "xz": xz, "yz": yz, "tally": tally, "m": m, "layer": lay}
