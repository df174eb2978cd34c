"""The covariance cases the per-item-count tests share (source_count, MUSIC_lin_array.work_counts, work_dev_auto):
doa.sim.make_streams -> oracle.autocorrelate, computed once per process.  Also the fp64 reference results on them."""
import functools

import numpy as np

import doa
import doa_oracle as oracle
import source_count_ref as ref

# name: (N, source angles, d, K, overlap, forward-backward, SNR dB, n, seed)
TABLE1 = {
    "n4_two_fb": (4, (30.0, 123.0), 0.4, 256, 64, 1, 15.0, 48, 11),
    "n4_one": (4, (57.3,), 0.5, 128, 0, 0, 10.0, 48, 11),
    "n8_three": (8, (35.0, 80.0, 140.0), 0.5, 256, 0, 0, 10.0, 32, 11),
    "n16_three_fb": (16, (40.0, 90.0, 121.0), 0.5, 256, 32, 1, 10.0, 16, 11),
    "n3_two": (3, (50.0, 110.0), 0.45, 200, 0, 0, 20.0, 32, 11),
}
# item counts 37 and 67 leave the last wave partial in all three kernel forms (64, 8 and 1 item per wave)
_T2 = {"n2_one": (2, (70.0,), 0.5, 64, 10.0), "n5_two": (5, (35.0, 140.0), 0.5, 128, 10.0),
       "n9_two": (9, (40.0, 90.0), 0.5, 128, 10.0), "n12_four": (12, (25.0, 60.0, 100.0, 150.0), 0.5, 128, 10.0)}
TABLE2 = {f"{k}_s{seed}": (N, th, d, K, 0, 0, snr, n, seed)
          for k, (N, th, d, K, snr) in _T2.items() for seed, n in ((0, 37), (1, 67))}
CASES = {**TABLE1, **TABLE2}


@functools.lru_cache(maxsize=None)
def streams(name):
    N, th, d, K, ovl, fb, snr, n, seed = CASES[name]
    x = doa.sim.make_streams(N, (n - 1) * (K - ovl) + K, list(th), d, snr_db=snr, seed=seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def covariance(name):
    """[n, N*N] complex64, read-only."""
    N, th, d, K, ovl, fb, snr, n, seed = CASES[name]
    R = oracle.autocorrelate(streams(name), K, ovl, fb, n)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def reference(name, method, kmax=None):
    """(counts, eigenvalues fp64, decided) of tests/source_count_ref.py on the case's covariances, read-only."""
    N, K = CASES[name][0], CASES[name][3]
    out = ref.source_count(covariance(name), N, K, method, kmax)
    for a in out:
        a.setflags(write=False)
    return out
