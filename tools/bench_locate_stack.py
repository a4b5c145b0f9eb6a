"""What the stacked density of the grid posteriors costs (htm_forward_locate_stack), on the job of
tools/bench_locate.py: 1000 windows x 64 stations, both data types, step 5's prior, on 128 x 128 x 64 and 32 x 32 x 16 cells,
with one layer and with 8 layers (equal runs of windows).  Per grid and layering:

    (a) htm_forward_locate_stack: the maps, loc and the marginals;
    (b) htm_forward_locate without a volume, the same build: (a) - (b) is what stacking adds;
    (c) the yardstick, the only way to the maps without it: htm_forward_locate with every window's volume downloaded, then the
        stack in numpy on the host (the rule of include/htm_hip.h, window after window) -- for --host-windows windows, as many
        as host memory takes comfortably (8 MiB a window on the large grid), scaled per window to the job's number.

Every figure is a synchronous host call under a host clock: one warm-up call, then the median of --reps calls.  The kernels'
shares come from a kernel trace of `--once`, a run of its own.

    python tools/bench_locate_stack.py [--windows 1000] [--stations 64] [--reps 3] [--host-windows 64] [--precision fp64|fp32]
    python tools/bench_locate_stack.py --one        # the measurement in this process
    python tools/bench_locate_stack.py --once       # one stacked call on the large grid, 8 layers, and nothing else

The measurement is a process of its own under `timeout` (the job and the driver: tools/locate_bench_job.py).
"""
import argparse
import sys

sys.path.insert(0, ".")
import locate_bench_job as bj


def host_stack(vol, loc, layer, n_layer):
    """the rule on the host from the downloaded volumes, in plain fp64: stack [n_layer][nz][ny][nx]"""
    import numpy as np

    stack = np.zeros((n_layer,) + vol.shape[1:])
    for e in range(vol.shape[0]):
        if loc[e, 0] < 0 or not 0 <= layer[e] < n_layer:
            continue
        with np.errstate(invalid="ignore"):
            w = np.exp(vol[e] - loc[e, 4])
        w[np.isnan(w)] = 0.0
        stack[layer[e]] += w * (1.0 / w.sum())
    return stack


def measure(args):
    import numpy as np

    from hypotremormcmc_amd import locate as lc

    job = bj.Job(args)
    E, S, prior = job.E, job.S, job.prior
    zero = np.zeros(S)

    def layers(n, n_layer):
        return (np.arange(n) * n_layer // n).astype(np.int32)

    def median(f, reps):
        f()                                                              # the warm-up call
        times, res = bj.timed(f, reps)
        return float(np.median(times)), min(times), max(times), res

    if args.once:
        fwd = job.forward_of(E)
        grid, _ = job.grid("128 x 128 x 64")
        lc.stack(fwd, zero, 3.0, zero, 250.0, grid, prior=prior, layer=layers(E, 8), n_layer=8)
        fwd.close()
        return

    for name in bj.GRIDS:
        grid, cells = job.grid(name)
        fwd = job.forward_of(E)
        tb, lo, hi, _ = median(lambda: lc.locate(fwd, zero, 3.0, zero, 250.0, grid, prior=prior, marginals=False), args.reps)
        print(f"(b) htm_forward_locate{job.tag}, no volume   {E:5d} windows x {S} stations, {name} cells: {tb * 1e3:10.2f} ms per call "
              f"(min {lo * 1e3:.2f}, max {hi * 1e3:.2f})", flush=True)
        n_host = min(E, args.host_windows if cells > 100000 else E)
        host = job.forward_of(n_host)
        for n_layer in (1, 8):
            ta, lo, hi, res = median(lambda: lc.stack(fwd, zero, 3.0, zero, 250.0, grid, prior=prior, layer=layers(E, n_layer), n_layer=n_layer),
                                     args.reps)
            assert res["tally"][:, 0].sum() == E
            print(f"(a) htm_forward_locate_stack{job.tag}, {n_layer} layer(s) {E:5d} windows x {S} stations, {name} cells: {ta * 1e3:10.2f} ms per call "
                  f"(min {lo * 1e3:.2f}, max {hi * 1e3:.2f}); (a) - (b) = {(ta - tb) * 1e3:.2f} ms = {100.0 * (ta - tb) / ta:.1f} % of (a)", flush=True)
            lay = layers(n_host, n_layer)

            def yardstick():
                r = lc.locate(host, zero, 3.0, zero, 250.0, grid, prior=prior[:n_host], marginals=False, volume=True)
                return host_stack(r["vol"], r["loc"], lay, n_layer)

            tc, lo, hi, ref = median(yardstick, args.reps)
            scaled = tc * E / n_host
            print(f"(c) htm_forward_locate with the volumes, numpy stack on the host, {n_layer} layer(s), {n_host} windows: {tc * 1e3:10.2f} ms per call "
                  f"(min {lo * 1e3:.2f}, max {hi * 1e3:.2f}) = {scaled * 1e3:.2f} ms scaled to {E} windows; (c) / (a) = {scaled / ta:.1f}", flush=True)
            if n_host == E:          # the same windows: the two stacks agree
                full = lc.stack(fwd, zero, 3.0, zero, 250.0, grid, prior=prior, layer=layers(E, n_layer), n_layer=n_layer, volume=True)["stack"]
                print(f"    largest |device stack - host stack| / largest cell: {np.abs(full - ref).max() / ref.max():.2e}", flush=True)
        host.close()
        fwd.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    bj.add_arguments(ap)
    ap.add_argument("--host-windows", type=int, default=64, help="windows of the yardstick on the large grid (8 MiB of volume each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args(argv)
    if args.one or args.once:
        measure(args)
        return 0
    return bj.drive(__file__, args, [("the measurement", ["--one", "--host-windows", str(args.host_windows)])], args.out)


if __name__ == "__main__":
    sys.exit(main())
