"""Measurements of music_pipeline's grid mode (profiles/array_grid.txt): the steering-table scan that ends in the
two-dimensional peak pick (array_scan_peaks2d_kernel) against the two launches it replaces (array_scan_kernel, then
find_local_max_2d_kernel), timed IN THE SAME RUN on the same full records, 4096 items per shape:

      N = 8,  72 x 18,  M = 2, wrap        N = 5,  1024 x 1,  M = 2, wrap        N = 16,  64 x 64,  M = 3, no wrap

  kernel   per shape, after one full work_dev call has left valid records in the handle: repetitions of
             (a) the grid handle's scan stage alone (set_stages), storing the spectrum,
             (b) the same, angles only (no row leaves the chip),
             (c) MUSIC_array.work_dev (its eigen launch and array_scan_kernel) and find_local_max_2d.work_dev on the covariance
                 items the handle wrote -- the same items, hence the same records, bit for bit,
           alternating -- for a `rocprofv3 --kernel-trace --stats` run of its own; kernel times come from the trace:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_array_grid.py kernel
               python3 tools/profile_array_grid.py summarize OUT

           `summarize` splits the dispatches of the three kernels, in order, by shape (warm-up dispatches dropped) and prints the
           medians with their spread; the two launches are also summed repetition by repetition, so that the spread of the
           sum is there to judge a difference against.
  step     no profiler: grid-mode work_dev (with and without the spectrum) against autocorrelate -> MUSIC_array ->
           find_local_max_2d by hand on one stream, alternating windows of `--inner` calls, device events around each window.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "python"))

# (N, radius in wavelengths, n_az, n_el, M, wrap, sources (azimuth, elevation from the array normal))
SHAPES = ((8, 0.6, 72, 18, 2, True, ((2.8, 40.2), (250.4, 65.3))),
          (5, 0.45, 1024, 1, 2, True, ((2.8, 65.3), (250.4, 65.3))),
          (16, 1.0, 64, 64, 3, False, ((12.8, 40.2), (250.4, 65.3), (120.1, 20.4))))
EL_RANGE = {1: (65.3, 90.0)}                            # n_el = 1: the azimuth circle at the sources' elevation
ITEMS, K = 4096, 64
FUSED, SCAN, PICK = "array_scan_peaks2d_kernel", "array_scan_kernel", "find_local_max_2d_kernel"


def limits(n_el):
    return (0.0, 360.0) + EL_RANGE.get(n_el, (0.0, 90.0))


def streams(N, radius, sources, snr_db=20.0, seed=7):
    """[N, ITEMS * K] complex64: independent Gaussian sources at `sources` on a circular array, plus noise."""
    import doa
    pos = doa.uca_positions(N, radius)
    A = np.concatenate([doa.planar_steering_table(pos, 1, az, az + 1.0, el) for az, el in sources]).T       # [N, sources]
    rng = np.random.default_rng(seed)
    cplx = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)      # noqa: E731
    n = ITEMS * K
    return np.ascontiguousarray((A @ cplx(len(sources), n) + 10.0 ** (-snr_db / 20.0) * cplx(N, n)).astype(np.complex64))


class Scene:
    """One shape on the device: the grid handle, the two blocks of the chain by hand, and every buffer either needs."""

    def __init__(self, shape):
        import torch
        import doa
        self.N, radius, self.n_az, self.n_el, self.M, self.wrap, sources = shape
        N, M, P = self.N, self.M, self.n_az * self.n_el
        lim = limits(self.n_el)
        table = doa.planar_steering_grid(doa.uca_positions(N, radius), self.n_az, self.n_el, *lim)
        self.st = torch.cuda.current_stream()
        self.x = doa.sim.stream_slab_torch([torch.from_numpy(a).cuda() for a in streams(N, radius, sources)])
        self.ptrs = [t.data_ptr() for t in self.x]
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")                                  # noqa: E731
        self.cov = torch.empty((ITEMS, N * N), dtype=torch.complex64, device="cuda")
        self.spec, self.mx, self.am = f32(ITEMS, P), f32(ITEMS, M), f32(ITEMS, 2 * M)
        self.spec2, self.o = f32(ITEMS, P), [f32(ITEMS, M) for _ in range(3)]
        self.pipe = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=ITEMS)
        self.pipe.set_steering_grid(table, self.n_az, self.n_el, *lim, self.wrap)
        self.k1 = doa.autocorrelate(N, K, 0, 0)
        self.scan = doa.MUSIC_array(M, table)
        self.pick = doa.find_local_max_2d(M, self.n_az, self.n_el, *lim, self.wrap)

    def grid(self, spectrum=True):
        self.pipe.work_dev(ITEMS, self.ptrs, self.cov.data_ptr(), self.spec.data_ptr() if spectrum else 0, self.mx.data_ptr(),
                           self.am.data_ptr(), self.st)

    def chain(self, k1=True):
        if k1:
            self.k1.work_dev(ITEMS, self.ptrs, self.cov.data_ptr(), self.st)
        self.scan.work_dev(ITEMS, self.cov.data_ptr(), self.spec2.data_ptr(), self.st)
        self.pick.work_dev(ITEMS, self.spec2.data_ptr(), *[t.data_ptr() for t in self.o], self.st)

    def check(self):
        """the two ways agree bit for bit on what both wrote last"""
        import torch
        torch.cuda.synchronize()
        M = self.M
        same = lambda a, b: bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))   # noqa: E731
        assert same(self.spec, self.spec2) and same(self.mx, self.o[0]) and same(self.am[:, :M], self.o[1]) and same(self.am[:, M:], self.o[2])
        return int((~torch.isnan(self.mx)).sum().item())


def run_kernel(a):
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"mode": "kernel", "reps": a.reps, "warmup": a.warmup, "items": ITEMS, "shapes": []}
    for shape in SHAPES:
        s = Scene(shape)
        s.grid()                                        # every stage once: covariance items and records are valid from here on
        s.pipe.set_stages(cov=False, evd=False, scan=True)
        for _ in range(a.warmup + a.reps):
            s.grid(True)
            s.grid(False)
            s.chain(k1=False)
        s.grid(True)
        out["shapes"].append({"N": s.N, "n_az": s.n_az, "n_el": s.n_el, "M": s.M, "peaks_reported": s.check()})
    print(json.dumps(out))


def run_step(a):
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    print("step: %d items per call, %d calls per window, %d windows per variant, alternating; device events; us per call" % (
        ITEMS, a.inner, a.reps))
    for shape in SHAPES:
        s = Scene(shape)
        variants = (("grid-mode work_dev, spectrum stored", lambda: s.grid(True)), ("grid-mode work_dev, angles only", lambda: s.grid(False)),
                    ("autocorrelate -> MUSIC_array -> find_local_max_2d", s.chain))
        for _, f in variants:                           # warm-up
            for _ in range(a.warmup):
                f()
        s.grid(True)
        s.chain()
        s.check()
        t = {name: [] for name, _ in variants}
        for _ in range(a.reps):
            for name, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s.st)
                for _ in range(a.inner):
                    f()
                e1.record(s.st)
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1000.0 / a.inner)
        base = statistics.median(t[variants[2][0]])
        for name, _ in variants:
            print("N %2d, grid %4d x %2d, M %d: %-52s %8.2f us median (min %.2f, max %.2f) -> %.3f x the chain by hand" % (
                s.N, s.n_az, s.n_el, s.M, name, statistics.median(t[name]), min(t[name]), max(t[name]), statistics.median(t[name]) / base))


def summarize(a):
    rows = {FUSED: [], SCAN: [], PICK: []}
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for name in rows:
                    if name in r["Kernel_Name"]:
                        rows[name].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    per = a.warmup + a.reps
    for name in rows:
        rows[name].sort()
    # per shape: one full call (fused, with the spectrum), then `per` rounds of fused + fused + the two, then one fused
    assert len(rows[FUSED]) == (2 * per + 2) * len(SHAPES) and len(rows[SCAN]) == len(rows[PICK]) == per * len(SHAPES), (
        {k: len(v) for k, v in rows.items()}, per)
    us = lambda v: [(e - s) / 1000.0 for s, e in v]                                                          # noqa: E731
    fmt = lambda t: "%8.2f us median (min %.2f, max %.2f)" % (statistics.median(t), min(t), max(t))         # noqa: E731
    for k, (N, _, n_az, n_el, M, wrap, _) in enumerate(SHAPES):
        fused = us(rows[FUSED][k * (2 * per + 2) + 1:(k + 1) * (2 * per + 2) - 1])
        stored, lean = fused[0::2][a.warmup:], fused[1::2][a.warmup:]
        scan, pick = us(rows[SCAN][k * per + a.warmup:(k + 1) * per]), us(rows[PICK][k * per + a.warmup:(k + 1) * per])
        both = [x + y for x, y in zip(scan, pick)]
        print("N %2d, grid %4d x %2d (P %5d), M %d, %s, %d items, %d repetitions:" % (N, n_az, n_el, n_az * n_el, M, "wrap" if wrap else "no wrap",
                                                                                   ITEMS, len(both)))
        print("    array_scan_kernel                          %s" % fmt(scan))
        print("    find_local_max_2d_kernel                   %s" % fmt(pick))
        print("    the two, summed per repetition             %s" % fmt(both))
        print("    array_scan_peaks2d_kernel, spectrum stored %s -> %.3f x the two" % (fmt(stored), statistics.median(stored) / statistics.median(both)))
        print("    array_scan_peaks2d_kernel, angles only     %s -> %.3f x the two" % (fmt(lean), statistics.median(lean) / statistics.median(both)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "summarize", "step"))
    ap.add_argument("dir", nargs="?", help="summarize: the rocprofv3 output directory")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10, help="step: calls per timed window")
    a = ap.parse_args()
    {"kernel": run_kernel, "summarize": summarize, "step": run_step}[a.mode](a)


if __name__ == "__main__":
    main()
