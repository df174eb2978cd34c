"""numpy restatement of the reference's four calibration blocks, for the tests of the device-side calibration chain
(importable like scenarios.py).  Each function restates what the reference's Python computes, in the reference's order:

  twinrx_phase_offset_est   python/twinrx_phase_offset_est.py:37-94   skiphead -> complex_to_arg -> sub_ff(0, p)
  findmax_and_save          python/findmax_and_save.py:66-78          numpy.amax(input[:samples]), str(value) per line
  average_and_save          python/average_and_save.py:68-80          numpy.mean(input[:samples]), str(value) per line
  save_antenna_calib        python/save_antenna_calib.py:61-72        numpy.mean(G[i::num_inputs]) over all items, "g p" per line

complex_to_arg is GNU Radio's, not the reference's; it is restated as the correctly rounded float arctangent (the float64
angle rounded to float32), which is what the accuracy condition of the device kernel is written against.

It also holds the input generators the calibration tests share (pilot captures with per-channel phase offsets)."""
import numpy as np

_F32 = np.float32


def angle64(x):
    """numpy's double `angle` of the float samples: the exact-to-double phase of what the device reads."""
    x = np.asarray(x)
    return np.arctan2(x.imag.astype(np.float64), x.real.astype(np.float64))


def phase_differences64(x, n_skip_ahead=0):
    """[N-1, T - skip] float64: angle64(x_0) - angle64(x_p), unwrapped: the accuracy yardstick of the streaming form."""
    a = angle64(np.asarray(x)[:, n_skip_ahead:])
    return a[0][None, :] - a[1:]


def twinrx_phase_offset_est(x, n_skip_ahead=0):
    """[N-1, T - skip] float32: the block's outputs for streams x [N, T] (complex_to_arg as a float, one float subtraction)."""
    a = angle64(np.asarray(x)[:, n_skip_ahead:]).astype(_F32)
    return (a[0][None, :] - a[1:]).astype(_F32)


def findmax(streams, samples_to_findmax):
    return np.array([np.amax(np.asarray(s, dtype=_F32)[:samples_to_findmax]) for s in streams], dtype=_F32)


def average(streams, samples_to_average):
    return np.array([np.mean(np.asarray(s, dtype=_F32)[:samples_to_average]) for s in streams], dtype=_F32)


def phase_file_text(values):
    return "".join(str(v) + "\n" for v in values)


def save_antenna_calib(mag_items, phase_items, num_inputs):
    """(gains, phases) float32 [num_inputs]: the mean of every num_inputs-th element of the flattened items."""
    G = np.asarray(mag_items, dtype=_F32).reshape(-1)
    P = np.asarray(phase_items, dtype=_F32).reshape(-1)
    return (np.array([np.mean(G[i::num_inputs]) for i in range(num_inputs)], dtype=_F32),
            np.array([np.mean(P[i::num_inputs]) for i in range(num_inputs)], dtype=_F32))


def antenna_file_text(gains, phases):
    return "".join(str(g) + " " + str(p) + "\n" for g, p in zip(gains, phases))


def circular_mean64(x, n_skip_ahead, samples):
    """(arg(sum x_0 conj(x_p)) [N-1] float64, conditioning |sum| / sum |x_0||x_p| [N-1]) over the first `samples` kept samples."""
    xs = np.asarray(x)[:, n_skip_ahead:n_skip_ahead + samples].astype(np.complex128)
    s = (xs[0][None, :] * np.conj(xs[1:])).sum(axis=1)
    den = (np.abs(xs[0])[None, :] * np.abs(xs[1:])).sum(axis=1)
    return np.angle(s), np.abs(s) / den


def ulp32(v):
    """Spacing of float32 at |v| (at least that of the smallest normal)."""
    return np.spacing(np.maximum(np.abs(np.asarray(v, dtype=_F32)), np.finfo(_F32).tiny)).astype(np.float64)


def apply_offsets(x, phi):
    """Streams 1.. of x [N, T] multiplied by exp(-j phi_p): the constant per-channel phase offset of a TwinRX front end
    (channel 0 is the reference).  complex64 out."""
    g = np.concatenate([[1.0 + 0j], np.exp(-1j * np.asarray(phi, dtype=np.float64))])
    return np.ascontiguousarray((g[:, None] * np.asarray(x).astype(np.complex128)).astype(np.complex64))


def pilot_capture(num_ports, n_samples, phi, snr_db=30.0, seed=0, freq=0.01234):
    """What the X310 calibration flowgraph records: ONE common tone on every channel, channel p carrying the offset
    exp(-j phi_p), plus independent noise per channel (unit-amplitude tone, noise variance 10^(-snr/10))."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples, dtype=np.float64)
    tone = np.exp(2j * np.pi * freq * t)
    x = np.repeat(tone[None, :], num_ports, axis=0)
    if snr_db is not None:
        sigma = 10.0 ** (-float(snr_db) / 20.0)
        x = x + sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) / np.sqrt(2.0)
    return apply_offsets(x, phi)
