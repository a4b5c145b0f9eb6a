"""The map grid of the analysis programs (density, locate): x0, dx, nx, y0, dy, ny, z0, dz, nz -- its checks, its cell centres,
and the --cell / --bounds arguments that make one.  The library's side is hypotremormcmc_amd/csrc/htm_grid.hpp.  density.py
imports all of it, so that density.make_grid, density.MAX_CELLS and the rest stay names of that module for its callers."""
import math

import numpy as np

MAX_CELLS = 4096          # per axis: kMapMaxCells of csrc/htm_grid.hpp (tests/test_density.py keeps them equal)


def grid9(grid):
    """{x0, dx, nx, y0, dy, ny, z0, dz, nz} as the float64 array the library takes, after the checks that can be made here"""
    g = np.array(grid, dtype=np.float64).reshape(-1)
    if g.shape != (9,):
        raise ValueError(f"grid has {g.size} numbers: need x0, dx, nx, y0, dy, ny, z0, dz, nz")
    for a, name in enumerate("xyz"):
        v0, dv, n = g[3 * a:3 * a + 3]
        if not (np.isfinite(v0) and np.isfinite(dv) and dv > 0.0):
            raise ValueError(f"grid axis {name}: origin {v0}, cell size {dv}: need a finite origin and a finite cell size > 0")
        if not (1 <= n <= MAX_CELLS and n == math.floor(n)):
            raise ValueError(f"grid axis {name}: {n} cells: need an integer in 1..{MAX_CELLS}")
    return g


def grid_counts(grid):
    g = grid9(grid)
    return int(g[2]), int(g[5]), int(g[8])


def centres(grid, axis: int):
    """the cell centres of one axis, v0 + (i + 0.5) * dv: one multiplication, then one addition, as the library forms them"""
    g = grid9(grid)
    return g[3 * axis] + (np.arange(int(g[3 * axis + 2])) + 0.5) * g[3 * axis + 1]


def make_grid(bounds, cell):
    """bounds = x0, x1, y0, y1, z0, z1 and cell = dx, dy, dz: the grid from the lower bounds with the fewest cells that reach
    the upper ones"""
    g = []
    for a in range(3):
        lo, hi, dv = float(bounds[2 * a]), float(bounds[2 * a + 1]), float(cell[a])
        if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo and np.isfinite(dv) and dv > 0.0):
            raise ValueError(f"axis {'xyz'[a]}: bounds {lo} .. {hi}, cell {dv}: need lower < upper and a cell size > 0")
        n = max(1, math.ceil((hi - lo) / dv * (1.0 - 1e-12)))
        g += [lo, dv, float(n)]
    return grid9(g)


def default_bounds(par):
    wxy, z0, wz = par.get_prior_width_xy(), par.get_prior_z(), par.get_prior_width_z()
    return [par.sta_x.min() - wxy, par.sta_x.max() + wxy, par.sta_y.min() - wxy, par.sta_y.max() + wxy, z0, z0 + 5.0 * wz]


def add_grid_arguments(ap):
    ap.add_argument("--cell", type=float, nargs="+", required=True, metavar="D", help="cell size: DX, or DX DY DZ")
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("x0", "x1", "y0", "y1", "z0", "z1"))


def grid_from_args(ap, args, par):
    """the grid of --cell and --bounds (default: default_bounds)"""
    if len(args.cell) not in (1, 3):
        ap.error("--cell takes DX, or DX DY DZ")
    return make_grid(args.bounds if args.bounds else default_bounds(par), args.cell * 3 if len(args.cell) == 1 else args.cell)
