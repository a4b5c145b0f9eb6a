"""Plain-numpy restatement of step 6's order statistics (htm_quantiles, hypotremormcmc_amd/csrc/htm_select.hpp), in integer
arithmetic only.  It shares no code with the product.

A double is ordered by its uint64 image: the bit pattern with all bits flipped when the sign bit is set, with only the sign
bit flipped otherwise.  As unsigned integers the images order every double, NaN included:

    -NaN < -inf < ... < -DBL_MIN < ... < -5e-324 < -0.0 < +0.0 < +5e-324 < ... < +DBL_MAX < +inf < +NaN

and NaNs among themselves by payload (+NaN: larger payload later; -NaN: larger payload earlier).  On columns without NaN
this is numpy's `<` refined by -0.0 < +0.0.  The r-th smallest of a column is the element whose image is the r-th smallest:
sort the images, take the ranks, map back.  Nothing is rounded, so the result is exact and every comparison against it is
on bits."""
import numpy as np

SIGN = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(x):
    """the uint64 view of a float64 array (a copy: the input keeps its memory)"""
    return np.array(x, dtype=np.float64, order="C").view(np.uint64)


def key(x):
    """uint64 image of doubles: a orders before b  <=>  key(a) < key(b)"""
    b = bits(x)
    return b ^ np.where((b & SIGN) != 0, ONES, SIGN)


def unkey(k):
    """the doubles of uint64 images, bit for bit: unkey(key(x)) has x's bits"""
    k = np.array(k, dtype=np.uint64, order="C")
    return (k ^ np.where((k & SIGN) != 0, SIGN, ONES)).view(np.float64)


def select(x, ranks_1based):
    """[n_par][len(ranks)]: per column of x [n_mod][n_par] (1-D: one column) the elements at the 1-based ranks of the column
    sorted by image"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n_mod = x.shape[0]
    r = [int(v) for v in ranks_1based]
    if n_mod < 1 or any(v < 1 or v > n_mod for v in r):
        raise ValueError(f"ranks {r} outside 1..{n_mod}")
    k = np.sort(key(x), axis=0, kind="stable")              # unsigned integer sort
    return np.ascontiguousarray(unkey(k[[v - 1 for v in r]]).T)
