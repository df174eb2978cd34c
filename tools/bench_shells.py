"""Host-fed rate of the C++ block shells (not the graded bench): N stream files ->
gr::doa::music_pipeline (or the three chained blocks) under the gnuradio_lite scheduler, wall time inside the
blocks' work() calls only (host buffers in, host buffers out).
usage: python tools/bench_shells.py [--snapshots 16384] [--multiple 256 64 16 1] [--format fc32|sc16]
(--format sc16: gr::doa::music_pipeline_sc16 on the same streams quantised to complex int16, run_flowgraph_sc16)"""
import argparse, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gr-doa_amd", "python")]
ap = argparse.ArgumentParser()
ap.add_argument("--snapshots", type=int, default=16384)
ap.add_argument("--multiple", type=int, nargs="*", default=[1024, 256, 64, 16, 1])
ap.add_argument("--format", default="fc32", choices=["fc32", "sc16"])
a = ap.parse_args()
N, K, M, P, d = 4, 1024, 1, 1024, 0.5
from doa import sim
x, _ = sim.make_batch_streams(N, K, a.snapshots, d, M, 20.0, seed=5)
sc16 = a.format == "sc16"
SCALE = 2.0 ** -12
exe = os.path.join(ROOT, "gr-doa_amd", "lib", "run_flowgraph_sc16" if sc16 else "run_flowgraph")
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
    pre = os.path.join(tmp, "in")
    for k in range(N):
        if sc16:
            sim.to_sc16(x[k], SCALE).tofile(f"{pre}.ch{k}.sc16")
        else:
            x[k].tofile(f"{pre}.ch{k}.c64")
    for mode in (("pipeline",) if sc16 else ("pipeline", "music")):
        for mult in a.multiple:
            env = dict(os.environ, DOA_GR_OUTPUT_MULTIPLE=str(mult), DOA_GR_MIN_OUTPUT_BUFFER=str(max(512, 2 * mult)))
            r = subprocess.run([exe, mode, pre, os.path.join(tmp, "out"), str(N), str(K), "0", "0", str(d), str(M), str(P), "8"] + ([repr(SCALE)] if sc16 else []),
                               capture_output=True, text=True, env=env, timeout=600)
            lines = [l for l in r.stdout.splitlines() if "snapshots_per_s" in l]
            print(f"{mode:9s} output_multiple={mult:5d}:", " | ".join(lines) if r.returncode == 0 else r.stderr[-300:], flush=True)
