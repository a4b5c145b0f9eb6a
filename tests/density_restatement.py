"""A plain-numpy restatement of the density maps' binning rule, sharing no code with the product.

On an axis {v0, dv, n}: q = (v - v0) / dv in fp64 (a true division); inside iff 0 <= q < n; the cell is floor(q).  A sample
counts iff its three coordinates are inside, and then once in xy, xz, yz, the volume and its layer's `inside`; a sample of a
window whose layer lies outside 0 .. n_layer - 1 is counted nowhere."""
import numpy as np


def bin_axis(v, v0, dv, n):
    """(inside [bool], cell [int64, 0 where outside]) of coordinates v"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = (np.asarray(v, dtype=np.float64) - np.float64(v0)) / np.float64(dv)
        inside = (q >= 0.0) & (q < np.float64(n))
    cell = np.zeros(q.shape, dtype=np.int64)
    cell[inside] = np.floor(q[inside]).astype(np.int64)
    return inside, cell


def density(hypo, grid, layer=None, n_layer=1, volume=True):
    """hypo [n_mod][3 n_win], grid = x0, dx, nx, y0, dy, ny, z0, dz, nz -> dict of uint64 arrays xy [n_layer][ny][nx],
    xz [n_layer][nz][nx], yz [n_layer][nz][ny], vol [n_layer][nz][ny][nx] (None without `volume`), tally [n_layer][2]"""
    x = np.asarray(hypo, dtype=np.float64)
    n_mod, n_win = x.shape[0], x.shape[1] // 3
    x0, dx, nx, y0, dy, ny, z0, dz, nz = [float(v) for v in grid]
    nx, ny, nz = int(nx), int(ny), int(nz)
    lay = np.zeros(n_win, dtype=np.int64) if layer is None else np.asarray(layer, dtype=np.int64)
    L = np.broadcast_to(lay[None, :], (n_mod, n_win))
    part = (L >= 0) & (L < n_layer)
    inx, ix = bin_axis(x[:, 0::3], x0, dx, nx)
    iny, iy = bin_axis(x[:, 1::3], y0, dy, ny)
    inz, iz = bin_axis(x[:, 2::3], z0, dz, nz)
    inside = part & inx & iny & inz
    outside = part & ~(inx & iny & inz)
    out = {"xy": np.zeros((n_layer, ny, nx), dtype=np.uint64), "xz": np.zeros((n_layer, nz, nx), dtype=np.uint64),
           "yz": np.zeros((n_layer, nz, ny), dtype=np.uint64), "vol": np.zeros((n_layer, nz, ny, nx), dtype=np.uint64) if volume else None,
           "tally": np.zeros((n_layer, 2), dtype=np.uint64)}
    one = np.uint64(1)
    Li, X, Y, Z = L[inside], ix[inside], iy[inside], iz[inside]
    np.add.at(out["xy"], (Li, Y, X), one)
    np.add.at(out["xz"], (Li, Z, X), one)
    np.add.at(out["yz"], (Li, Z, Y), one)
    if volume:
        np.add.at(out["vol"], (Li, Z, Y, X), one)
    np.add.at(out["tally"][:, 0], Li, one)
    np.add.at(out["tally"][:, 1], L[outside], one)
    return out


# ---- edge inputs shared by the CPU and the GPU tests -----------------------------------------------------------------
# origins and power-of-two cell sizes chosen so that every edge v0 + k dv, its two neighbours in fp64 and their differences
# from v0 are exact: what is expected below is then plain geometry
EDGE_GRID = (8.0, 0.5, 6.0, -16.0, 0.25, 5.0, 32.0, 2.0, 3.0)
ZERO_GRID = (0.0, 1.0, 2.0, 0.0, 1.0, 2.0, 0.0, 1.0, 2.0)            # q = -0.0 needs v = -0.0 at the origin 0.0


def edge_axis(v0, dv, n):
    """[(v, inside, cell)]: every edge of the axis, one step below it and one step above it, then NaN and +-inf"""
    out = []
    for k in range(n + 1):
        e = v0 + k * dv
        out.append((e, k < n, k if k < n else 0))                                        # on a lower edge: that cell; on the top edge: outside
        out.append((np.nextafter(e, -np.inf), k > 0, k - 1 if k > 0 else 0))
        out.append((np.nextafter(e, np.inf), k < n, k if k < n else 0))
    return out + [(np.nan, False, 0), (np.inf, False, 0), (-np.inf, False, 0)]


def edge_samples(grid=EDGE_GRID):
    """points [n][3] that walk every axis through edge_axis while the other two coordinates sit in the middle of cell 1,
    with what is expected of each: inside [n], cell [n][3]"""
    g = [float(v) for v in grid]
    mid = [g[3 * a] + 1.5 * g[3 * a + 1] for a in range(3)]
    pts, inside, cell = [], [], []
    for a in range(3):
        for v, ok, k in edge_axis(g[3 * a], g[3 * a + 1], int(g[3 * a + 2])):
            p, c = list(mid), [1, 1, 1]
            p[a], c[a] = v, k
            pts.append(p)
            inside.append(ok)
            cell.append(c if ok else [0, 0, 0])
    return np.array(pts), np.array(inside), np.array(cell)
