"""Host-side mirror of the reference's `doa` Python namespace for the hot-path blocks.

The reference exposes its C++ blocks to Python through SWIG (`swig/doa_swig.i:22-34`) as
`doa.autocorrelate(inputs, snapshot_size, overlap_size, avg_method)`,
`doa.MUSIC_lin_array(norm_spacing, num_targets, inputs, pspectrum_len)`,
`doa.find_local_max(num_max_vals, vector_len, x_min, x_max)` and
`doa.rootMUSIC_linear_array(norm_spacing, num_targets, inputs)` — the make strings of the GRC
descriptors (`grc/doa_*.xml`).  The classes below keep those names and argument orders and forward
every call to the HIP library through its C ABI (include/doa_hip.h); they hold no arithmetic.

Each block offers
  * `general_work` / `work(noutput_items, input_items, output_items)` with the item layouts of the
    GNU Radio buffers (numpy arrays standing in for the scheduler's buffers), used by
    `doa.runtime`'s mini scheduler, and
  * `work_dev(...)` on raw device pointers (ints, e.g. `torch.Tensor.data_ptr()`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check, check_handle, ptr_array

_C64 = np.complex64
_F32 = np.float32
_I16 = np.int16
_I32 = np.int32

# criteria of the source-count estimate (DOA_SOURCE_COUNT_MDL / DOA_SOURCE_COUNT_AIC, include/doa_hip.h)
_COUNT_METHODS = {"mdl": 0, "aic": 1}


def _named(value, table, what, choices, ints=True) -> int:
    """The C constant of a named choice: a name of `table` (any case), or with `ints` the constant itself, which is passed
    on for the library to reject if it is none.  `what` and `choices` word the ValueError."""
    if isinstance(value, str) and value.lower() in table:
        return table[value.lower()]
    if isinstance(value, str) or not ints:
        raise ValueError(f"unknown {what} {value!r} ({choices})")
    return int(value)


def _count_method(method) -> int:
    return _named(method, _COUNT_METHODS, "source-count method", "mdl or aic")


def _selected_bins(fft_len, first_bin, num_bins) -> np.ndarray:
    """The FFT bin of every item of a snapshot, in item order: (first_bin + j) mod fft_len."""
    return (first_bin + np.arange(num_bins)) % fft_len


def _opt_ptr(p) -> C.c_void_p:
    """An optional device pointer: None is NULL.  (The per-item count pointers take it too: a missing one is the library's to
    refuse.)"""
    return C.c_void_p(0 if p is None else int(p))


def _dev_ptr(p) -> C.c_void_p:
    """A required device pointer."""
    return C.c_void_p(int(p))

# estimators of music_pipeline (DOA_ESTIMATOR_MUSIC / DOA_ESTIMATOR_CAPON, include/doa_hip.h)
_ESTIMATORS = {"music": 0, "capon": 1}
_GRIDFREE = {"root_music": 0, "esprit": 1}

# input sample formats of the stream-input blocks (DOA_SAMPLE_FC32 / DOA_SAMPLE_SC16, include/doa_hip.h)
SC16_DEFAULT_SCALE = 2.0 ** -15
_FORMATS = {"fc32": 0, "sc16": 1}


def _vp(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


DETACHED = "detached"      # work_dev_batches(..., stream=DETACHED): no ordering on any caller stream (DOA_STREAM_DETACHED)


def _stream_ptr(stream) -> C.c_void_p:
    """Accept None, an int (hipStream_t), a torch.cuda.Stream or DETACHED."""
    if stream is None:
        return C.c_void_p(0)
    if isinstance(stream, str) and stream == DETACHED:
        return C.c_void_p(2 ** 64 - 1)
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(int(stream.cuda_stream))
    return C.c_void_p(int(stream))


class _Block:
    _destroy = None

    def __init__(self):
        self._h = None

    def close(self):
        if getattr(self, "_h", None):
            type(self)._destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    _set_precision = None

    def set_internal_precision(self, bits: int) -> None:
        """Per-handle internal precision of EVD / scan (32 or 64; include/doa_hip.h); blocks without an EVD have none."""
        if type(self)._set_precision is None:
            raise AttributeError(f"{type(self).__name__} has no internal precision")
        check(type(self)._set_precision(self._h, int(bits)))


class _ItemBlock(_Block):
    """Base of the blocks that take one item stream (covariance items or spectra): the checks of the host `work` arguments.
    Each helper returns the pointer the C entry takes.  A new block's work is these three and one library call."""

    @staticmethod
    def _items_in(arr, dtype, n, width) -> C.c_void_p:
        """n input items of `width` elements: converted to a C-contiguous `dtype` array if need be (the pointer keeps it alive)."""
        a = np.ascontiguousarray(arr, dtype=dtype)
        assert a.size >= n * width
        return a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _items_out(arr, dtype, n, width) -> C.c_void_p:
        """n output items of `width` elements, written in place: the array must already have the dtype and layout."""
        assert arr.dtype == dtype and arr.flags.c_contiguous and arr.size >= n * width
        return _vp(arr)

    @classmethod
    def _opt_out(cls, output_items, index, dtype, n, width) -> C.c_void_p:
        """Output port `index` if the caller passed one, else NULL."""
        if len(output_items) <= index or output_items[index] is None:
            return C.c_void_p(0)
        return cls._items_out(output_items[index], dtype, n, width)

    def _weights(self, weights, n) -> C.c_void_p:
        """The optional per-bin weights of a block that takes snapshots of self.num_bins bins: None is NULL."""
        return C.c_void_p(0) if weights is None else self._items_in(weights, _F32, n, self.num_bins)


class _StreamInput:
    """Input sample format of the blocks that take the antenna streams (autocorrelate and the two pipelines):
    "fc32" (complex64, the default) or "sc16" (complex int16, int16 arrays of shape [n, 2] or flat 2n, real first),
    widened on the device as float32(q) * float32(scale) (doa_*_set_input_format, include/doa_hip.h)."""

    _set_format = None
    input_format, scale = "fc32", 1.0

    def set_input_format(self, fmt, scale=None) -> None:
        """fmt "fc32" or "sc16"; scale None = 2**-15 for sc16 and 1.0 for fc32.  Takes effect from the next work call."""
        if fmt not in _FORMATS:
            raise ValueError(f"unknown input format {fmt!r} (fc32 or sc16)")
        s = (SC16_DEFAULT_SCALE if fmt == "sc16" else 1.0) if scale is None else float(scale)
        check(type(self)._set_format(self._h, _FORMATS[fmt], s))
        self.input_format, self.scale = fmt, s

    def _samples(self, a):
        """A stream as the work entries index it: complex64 [n] or, for sc16, int16 [n, 2]."""
        if self.input_format == "sc16":
            a = np.asarray(a)
            if a.dtype != _I16:
                raise TypeError(f"sc16 streams are int16 arrays, got {a.dtype}")
            return a.reshape(-1, 2)
        return a

    def _host_streams(self, input_items, span):
        arrs = []
        for k in range(self.inputs):
            if self.input_format == "sc16":
                a = np.ascontiguousarray(self._samples(input_items[k]))
            else:
                a = np.ascontiguousarray(input_items[k], dtype=_C64)
            if a.shape[0] < span:
                raise ValueError(f"input {k}: {a.shape[0]} samples, need {span}")
            arrs.append(a)
        return arrs


class autocorrelate(_StreamInput, _Block):
    """doa.autocorrelate(inputs, snapshot_size, overlap_size, avg_method) — gr::block with
    history overlap_size+1 (reference lib/autocorrelate_impl.cc:47-65)."""

    _destroy = staticmethod(lib.doa_autocorrelate_destroy)
    _set_format = staticmethod(lib.doa_autocorrelate_set_input_format)

    def __init__(self, inputs, snapshot_size, overlap_size, avg_method):
        super().__init__()
        self.inputs, self.snapshot_size = int(inputs), int(snapshot_size)
        self.overlap_size, self.avg_method = int(overlap_size), int(avg_method)
        self._h = check_handle(lib.doa_autocorrelate_create(self.inputs, self.snapshot_size,
                                                            self.overlap_size, self.avg_method),
                               "autocorrelate")
        # io signature of the reference block (:49-50)
        self.in_sig = [(_C64, 1)] * self.inputs
        self.out_sig = [(_C64, self.inputs * self.inputs)]

    def history(self) -> int:
        return check(lib.doa_autocorrelate_history(self._h))

    def forecast(self, noutput_items: int) -> int:
        return check(lib.doa_autocorrelate_forecast(self._h, int(noutput_items)))

    def input_span(self, noutput_items: int) -> int:
        return int(lib.doa_autocorrelate_input_span(self._h, int(noutput_items)))

    def general_work(self, noutput_items, input_items, output_items):
        """input_items[k]: complex64 array starting at the first history sample of stream k
        (at least input_span(noutput_items) long); output_items[0]: [>=n, N*N] complex64.
        Returns (items produced, items consumed per input) — the caller applies consume_each."""
        n = int(noutput_items)
        arrs = self._host_streams(input_items, self.input_span(n))
        out = output_items[0]
        assert out.dtype == _C64 and out.flags.c_contiguous and out.size >= n * self.inputs ** 2
        produced = check(lib.doa_autocorrelate_work(self._h, n, ptr_array([a.ctypes.data for a in arrs]),
                                                    _vp(out)))
        return produced, self.forecast(produced)

    def work_dev(self, noutput_items, d_input_ptrs, d_out_ptr, stream=None) -> int:
        return check(lib.doa_autocorrelate_work_dev(self._h, int(noutput_items), ptr_array(d_input_ptrs),
                                                    C.c_void_p(int(d_out_ptr)), _stream_ptr(stream)))

    def fuse_antenna_correction(self, correction) -> None:
        """Fold a doa.antenna_correction block (or an array of complex gains, or None to undo) into
        this block: equivalent to wiring the correction block in front of it."""
        _fuse(lib.doa_autocorrelate_fuse_antenna_correction, self._h, correction, self.inputs)


class autocorrelate_sc16(autocorrelate):
    """doa.autocorrelate_sc16(inputs, snapshot_size, overlap_size, avg_method, scale=2**-15) — autocorrelate on complex
    int16 streams (GNU Radio's sc16 items, 4 bytes: int16 real, int16 imaginary), widened on the device as
    float32(q) * float32(scale); outputs and scheduling as autocorrelate.  Not a block of the reference."""

    def __init__(self, inputs, snapshot_size, overlap_size, avg_method, scale=SC16_DEFAULT_SCALE):
        super().__init__(inputs, snapshot_size, overlap_size, avg_method)
        self.set_input_format("sc16", scale)
        self.in_sig = [(_I16, 2)] * self.inputs


def _periodic_window(name, fft_len) -> np.ndarray:
    """The named windows of channel_covariance: periodic forms, computed in double and rounded to float32."""
    t = 2.0 * np.pi * np.arange(fft_len, dtype=np.float64) / fft_len
    forms = {"rect": lambda: np.ones(fft_len), "hann": lambda: 0.5 - 0.5 * np.cos(t),
             "hamming": lambda: 0.54 - 0.46 * np.cos(t),
             "blackman": lambda: 0.42 - 0.5 * np.cos(t) + 0.08 * np.cos(2.0 * t)}
    if name not in forms:
        raise ValueError(f"unknown window {name!r} (rect, hann, hamming, blackman or an array of fft_len values)")
    return forms[name]().astype(_F32)


class channel_covariance(_StreamInput, _Block):
    """doa.channel_covariance(inputs, snapshot_size, overlap_size, fft_len, window="hann") — one covariance per snapshot and
    frequency bin (the Welch / Bartlett cross-spectral matrix; include/doa_hip.h has the definition): each snapshot is cut
    into snapshot_size / fft_len blocks, every block windowed and Fourier-transformed, and the products averaged over the
    blocks.  Item i * num_bins() + j is the column-major inputs x inputs matrix of bin (first_bin + j) mod fft_len of
    snapshot i, an ordinary covariance item for every block behind it.  Not a block of the reference.
    window: "rect", "hann", "hamming", "blackman" (periodic forms) or an array of fft_len values."""

    _destroy = staticmethod(lib.doa_channel_covariance_destroy)
    _set_format = staticmethod(lib.doa_channel_covariance_set_input_format)

    def __init__(self, inputs, snapshot_size, overlap_size, fft_len, window="hann"):
        super().__init__()
        self.inputs, self.snapshot_size = int(inputs), int(snapshot_size)
        self.overlap_size, self.fft_len = int(overlap_size), int(fft_len)
        if isinstance(window, str):                   # (a bad fft_len is the library's to refuse: it does not read the window then)
            w = _periodic_window(window, max(self.fft_len, 1))
        else:
            w = np.ascontiguousarray(window, dtype=_F32).reshape(-1)
            if w.size != self.fft_len:
                raise ValueError(f"window has {w.size} values, fft_len is {self.fft_len}")
        self.window = w
        self._h = check_handle(lib.doa_channel_covariance_create(self.inputs, self.snapshot_size, self.overlap_size,
                                                                 self.fft_len, _vp(w)), "channel_covariance")
        self.first_bin = 0
        self.in_sig = [(_C64, 1)] * self.inputs
        self.out_sig = [(_C64, self.inputs * self.inputs), (_F32, self.fft_len)]

    def history(self) -> int:
        return check(lib.doa_channel_covariance_history(self._h))

    def forecast(self, noutput_items: int) -> int:
        return check(lib.doa_channel_covariance_forecast(self._h, int(noutput_items)))

    def input_span(self, noutput_items: int) -> int:
        return int(lib.doa_channel_covariance_input_span(self._h, int(noutput_items)))

    def set_bins(self, first_bin, num_bins) -> None:
        """Write only the bins (first_bin + j) mod fft_len, j < num_bins; the power output keeps all fft_len bins."""
        check(lib.doa_channel_covariance_set_bins(self._h, int(first_bin), int(num_bins)))
        self.first_bin = int(first_bin)

    def num_bins(self) -> int:
        return check(lib.doa_channel_covariance_num_bins(self._h))

    def bin_frequencies(self, sample_rate=1.0) -> np.ndarray:
        """Centre frequency of every selected bin, in item order: fftfreq(fft_len) * sample_rate."""
        return np.fft.fftfreq(self.fft_len)[_selected_bins(self.fft_len, self.first_bin, self.num_bins())] * float(sample_rate)

    def general_work(self, noutput_items, input_items, output_items):
        """input_items[k]: stream k from its first history sample (at least input_span(noutput_items) long);
        output_items[0]: [>= n * num_bins(), N*N] complex64; output_items[1] (optional): [>= n, fft_len] float32.
        noutput_items counts snapshots.  Returns (snapshots produced, samples consumed per input)."""
        n = int(noutput_items)
        arrs = self._host_streams(input_items, self.input_span(n))
        cov = output_items[0]
        assert cov.dtype == _C64 and cov.flags.c_contiguous and cov.size >= n * self.num_bins() * self.inputs ** 2
        power = C.c_void_p(0)
        if len(output_items) > 1 and output_items[1] is not None:
            pw = output_items[1]
            assert pw.dtype == _F32 and pw.flags.c_contiguous and pw.size >= n * self.fft_len
            power = _vp(pw)
        produced = check(lib.doa_channel_covariance_work(self._h, n, ptr_array([a.ctypes.data for a in arrs]), _vp(cov), power))
        return produced, self.forecast(produced)

    def work_dev(self, noutput_items, d_input_ptrs, d_cov_ptr, d_power_ptr=None, stream=None) -> int:
        return check(lib.doa_channel_covariance_work_dev(self._h, int(noutput_items), ptr_array(d_input_ptrs),
                                                         _dev_ptr(d_cov_ptr), _opt_ptr(d_power_ptr), _stream_ptr(stream)))


def _fuse(fn, handle, correction, n):
    if correction is None:
        check(fn(handle, C.c_void_p(0)))
        return
    g = correction.gains() if hasattr(correction, "gains") else np.asarray(correction)
    g = np.ascontiguousarray(np.asarray(g, dtype=_C64).reshape(n))
    check(fn(handle, _vp(g)))


class antenna_correction(_Block):
    """doa.antenna_correction(num_inputs, config_filename) — gr::sync_block, N complex streams in
    and out (reference lib/antenna_correction_impl.cc:47-99).  Raises ValueError with the
    reference's std::invalid_argument text for a missing / too long / too short config file."""

    _destroy = staticmethod(lib.doa_antenna_correction_destroy)

    def __init__(self, num_inputs, config_filename):
        super().__init__()
        self.num_ant_ele = int(num_inputs)
        h = lib.doa_antenna_correction_create(self.num_ant_ele, str(config_filename).encode())
        if not h:
            msg = _lib.last_error()
            if msg.startswith(("Cannot find configuration", "Configuration file")):
                raise ValueError(msg)                   # std::invalid_argument in the reference
            raise _lib.DoaError(-1, msg or "antenna_correction: create failed")
        self._h = h
        self.in_sig = [(_C64, 1)] * self.num_ant_ele
        self.out_sig = [(_C64, 1)] * self.num_ant_ele

    def gains(self) -> np.ndarray:
        g = np.empty(self.num_ant_ele, dtype=_C64)
        check(lib.doa_antenna_correction_gains(self._h, _vp(g)))
        return g

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        ins = [np.ascontiguousarray(a, dtype=_C64) for a in input_items]
        for a, o in zip(ins, output_items):
            assert a.size >= n and o.dtype == _C64 and o.flags.c_contiguous and o.size >= n
        return check(lib.doa_antenna_correction_work(self._h, n, ptr_array([a.ctypes.data for a in ins]),
                                                     ptr_array([o.ctypes.data for o in output_items])))

    def work_dev(self, noutput_items, d_in_ptrs, d_out_ptrs, stream=None) -> int:
        return check(lib.doa_antenna_correction_work_dev(self._h, int(noutput_items), ptr_array(d_in_ptrs),
                                                         ptr_array(d_out_ptrs), _stream_ptr(stream)))


def read_phase_config(filename):
    """The phase file of phase_correct_hier, parsed the way python/phase_correct_hier.py:33-45 parses it: every line
    that float() accepts AND whose value is truthy is a phase (so a line reading 0 is dropped, like a comment line)."""
    def ok(text):
        try:
            return float(text)
        except ValueError:
            return False
    with open(filename, "r") as f:
        lines = [line.rstrip("\n") for line in f]
    return [float(t) for t in lines if ok(t)]


class phase_correct_hier(antenna_correction):
    """doa.phase_correct_hier(num_ports, config_filename) -- the reference's hier block (python/phase_correct_hier.py:
    52-104): stream 0 passes through, stream p+1 is multiplied by exp(1j*phase_p), phases read from a text file.  Here one
    launch of the per-stream complex-gain kernel (antenna_correction's), or no launch at all when the gains are folded
    into the covariance kernel (autocorrelate.fuse_antenna_correction(self.gains())).  The reference writes its message to
    stderr and exits; this raises ValueError with the same text."""

    def __init__(self, num_ports=2, config_filename=""):
        _Block.__init__(self)
        self.num_ports = self.num_ant_ele = int(num_ports)
        self.config_filename = config_filename
        try:
            open(config_filename, "r").close()
        except (OSError, IOError):
            raise ValueError("Configuration " + str(config_filename) + ", not valid")
        self.phases = read_phase_config(config_filename)
        if len(self.phases) != self.num_ports - 1:
            raise ValueError("Configuration " + str(config_filename) + ". Not valid number of phase estimates")
        # numpy.exp(1j*phase) in double, handed to multiply_const_vcc as gr_complex (:93-94)
        g = np.array([1.0 + 0.0j] + [np.exp(1j * ph) for ph in self.phases], dtype=np.complex128).astype(_C64)
        h = lib.doa_antenna_correction_create_gains(self.num_ports, _vp(np.ascontiguousarray(g)))
        if not h:
            raise _lib.DoaError(-1, _lib.last_error() or "phase_correct_hier: create failed")
        self._h = h
        self.in_sig = [(_C64, 1)] * self.num_ports
        self.out_sig = [(_C64, 1)] * self.num_ports


class MUSIC_lin_array(_ItemBlock):
    """doa.MUSIC_lin_array(norm_spacing, num_targets, inputs, pspectrum_len) — gr::sync_block
    (reference lib/MUSIC_lin_array_impl.cc:47-87)."""

    _destroy = staticmethod(lib.doa_MUSIC_lin_array_destroy)
    _set_precision = staticmethod(lib.doa_MUSIC_lin_array_set_internal_precision)

    def __init__(self, norm_spacing, num_targets, inputs, pspectrum_len):
        super().__init__()
        self.norm_spacing, self.num_targets = float(norm_spacing), int(num_targets)
        self.num_ant_ele, self.pspectrum_len = int(inputs), int(pspectrum_len)
        self._h = check_handle(lib.doa_MUSIC_lin_array_create(self.norm_spacing, self.num_targets,
                                                              self.num_ant_ele, self.pspectrum_len),
                               "MUSIC_lin_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.pspectrum_len)]

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        return check(lib.doa_MUSIC_lin_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                  self._items_out(output_items[0], _F32, n, self.pspectrum_len)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, stream=None) -> int:
        return check(lib.doa_MUSIC_lin_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                      _dev_ptr(d_out_ptr), _stream_ptr(stream)))

    def work_counts(self, noutput_items, input_items, counts, output_items) -> int:
        """work with a source count PER ITEM (int32 array) in place of num_targets: count 0 gives an all-0.0 dB row, a count
        outside 0..inputs-1 (source_count's -1 status included) a NaN row (doa_MUSIC_lin_array_work_counts)."""
        n = int(noutput_items)
        return check(lib.doa_MUSIC_lin_array_work_counts(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                         self._items_in(counts, _I32, n, 1),
                                                         self._items_out(output_items[0], _F32, n, self.pspectrum_len)))

    def work_dev_counts(self, noutput_items, d_in_ptr, d_counts_ptr, d_out_ptr, stream=None) -> int:
        return check(lib.doa_MUSIC_lin_array_work_dev_counts(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                             _opt_ptr(d_counts_ptr), _dev_ptr(d_out_ptr),
                                                             _stream_ptr(stream)))

    def debug(self, R_items: np.ndarray):
        """(P_N [n, N*N] complex64 column-major items, Q [n, P] float32) for parity tests."""
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, self.num_ant_ele ** 2)
        n = a.shape[0]
        pn = np.empty((n, self.num_ant_ele ** 2), dtype=_C64)
        q = np.empty((n, self.pspectrum_len), dtype=_F32)
        check(lib.doa_MUSIC_lin_array_debug(self._h, n, _vp(a), _vp(pn), _vp(q)))
        return pn, q

    def nout_items_total(self) -> int:
        return int(lib.doa_MUSIC_lin_array_items_total(self._h))


_COMBINE = {"null_mean": 0, "power_sum": 1}     # DOA_WIDEBAND_NULL_MEAN / DOA_WIDEBAND_POWER_SUM (include/doa_hip.h)


def wideband_bin_spacing(norm_spacing, rate_over_carrier, fft_len, bin) -> float:
    """The element spacing in wavelengths at FFT bin `bin`: float32(norm_spacing) * (1 + fftfreq(fft_len)[bin] * rate_over_carrier)
    (doa_wideband_bin_spacing; no device)."""
    return float(lib.doa_wideband_bin_spacing(float(norm_spacing), float(rate_over_carrier), int(fft_len), int(bin)))


class wideband_music(_ItemBlock):
    """doa.wideband_music(norm_spacing, num_targets, inputs, pspectrum_len, fft_len, first_bin=0, num_bins=None,
    rate_over_carrier=0.0, combine="null_mean") — incoherent wideband MUSIC (include/doa_hip.h has the definition): one
    spectrum per snapshot from the num_bins covariance items channel_covariance writes for it, every bin with its own noise
    subspace and a steering vector at its own spacing in wavelengths (norm_spacing is the spacing at the carrier,
    rate_over_carrier the sample rate divided by the carrier frequency).  combine: "null_mean" for sources that occupy every
    used bin, "power_sum" for bins that hold different sources.  Not a block of the reference.
    Items: input [n * num_bins, inputs**2] complex64, item i * num_bins + j = bin (first_bin + j) mod fft_len of snapshot i;
    weights (optional) [n, num_bins] float32, a bin with a weight that is not positive and finite is skipped; output
    [n, pspectrum_len] float32 and an optional int32 status per snapshot.  noutput_items counts snapshots."""

    _destroy = staticmethod(lib.doa_wideband_music_destroy)

    def __init__(self, norm_spacing, num_targets, inputs, pspectrum_len, fft_len, first_bin=0, num_bins=None,
                 rate_over_carrier=0.0, combine="null_mean"):
        super().__init__()
        self.norm_spacing, self.num_targets = float(norm_spacing), int(num_targets)
        self.num_ant_ele, self.pspectrum_len = int(inputs), int(pspectrum_len)
        self.fft_len, self.first_bin = int(fft_len), int(first_bin)
        self.num_bins = self.fft_len if num_bins is None else int(num_bins)
        self.rate_over_carrier = float(rate_over_carrier)
        self.combine = _named(combine, _COMBINE, "combine rule", "null_mean or power_sum")
        self._h = check_handle(lib.doa_wideband_music_create(self.norm_spacing, self.num_targets, self.num_ant_ele,
                                                             self.pspectrum_len, self.fft_len, self.first_bin, self.num_bins,
                                                             self.rate_over_carrier, self.combine), "wideband_music")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.pspectrum_len), (_I32, 1)]

    def bin_spacings(self) -> np.ndarray:
        """The element spacing in wavelengths at every selected bin, in item order."""
        return np.array([wideband_bin_spacing(self.norm_spacing, self.rate_over_carrier, self.fft_len, f)
                         for f in _selected_bins(self.fft_len, self.first_bin, self.num_bins)])

    def work(self, noutput_items, input_items, output_items, weights=None) -> int:
        """output_items[0]: the spectra; output_items[1] (optional): the status words."""
        n = int(noutput_items)
        return check(lib.doa_wideband_music_work(self._h, n, self._items_in(input_items[0], _C64, n * self.num_bins, self.num_ant_ele ** 2),
                                                 self._weights(weights, n), self._items_out(output_items[0], _F32, n, self.pspectrum_len),
                                                 self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, d_weights_ptr=None, d_q_ptr=None, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_wideband_music_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _opt_ptr(d_weights_ptr),
                                                     _dev_ptr(d_out_ptr), _opt_ptr(d_q_ptr), _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def work_counts(self, noutput_items, input_items, counts, output_items, weights=None) -> int:
        """work with a source count PER ITEM (int32 [n * num_bins], source_count's output) in place of num_targets: a count of 0
        skips the bin, a count outside 0..inputs-1 gives the snapshot status 2 and a NaN row."""
        n = int(noutput_items)
        return check(lib.doa_wideband_music_work_counts(self._h, n, self._items_in(input_items[0], _C64, n * self.num_bins, self.num_ant_ele ** 2),
                                                        self._items_in(counts, _I32, n * self.num_bins, 1), self._weights(weights, n),
                                                        self._items_out(output_items[0], _F32, n, self.pspectrum_len),
                                                        self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev_counts(self, noutput_items, d_in_ptr, d_counts_ptr, d_out_ptr, d_weights_ptr=None, d_q_ptr=None, d_status_ptr=None,
                        stream=None) -> int:
        return check(lib.doa_wideband_music_work_dev_counts(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _opt_ptr(d_counts_ptr),
                                                            _opt_ptr(d_weights_ptr), _dev_ptr(d_out_ptr), _opt_ptr(d_q_ptr),
                                                            _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def nout_items_total(self) -> int:
        return int(lib.doa_wideband_music_items_total(self._h))


def rss_focusing_matrices(norm_spacing, inputs, fft_len, focus_angles, first_bin=0, num_bins=None, rate_over_carrier=0.0,
                          regularization=1e-3) -> np.ndarray:
    """The [num_bins, inputs, inputs] complex128 focusing table of a uniform linear array for focus_covariance, by
    rotational-signal-subspace focusing: T_j is the unitary polar factor of A_0 A_j^H + regularization * J * I, with A_0 / A_j
    the steering matrices of the J focus angles (degrees) at the carrier's spacing and at the spacing of bin
    (first_bin + j) mod fft_len (doa_rss_focusing_matrices, include/doa_hip.h; host only, no device needed).  [j, a, b] is
    T_j[a, b].  A fan over the field of view serves a first pass; the estimates and a few degrees either side of each a second."""
    ang = np.ascontiguousarray(focus_angles, dtype=np.float64).reshape(-1)
    n, f = int(inputs), int(fft_len)
    nb = f if num_bins is None else int(num_bins)
    out = np.empty((max(nb, 0), max(n, 0), max(n, 0)), dtype=np.complex128)
    check(lib.doa_rss_focusing_matrices(float(norm_spacing), n, f, int(first_bin), nb, float(rate_over_carrier), ang.size, _vp(ang),
                                        float(regularization), _vp(out)))
    return out


class focus_covariance(_ItemBlock):
    """doa.focus_covariance(inputs, num_bins, matrices) — coherent wideband focusing (include/doa_hip.h has the definition):
    one focused covariance item per snapshot, sum_j w_j T_j H(R_j) T_j^H / sum_j w_j over the num_bins covariance items
    channel_covariance writes for it.  matrices: [num_bins, inputs, inputs] complex128, [j, a, b] = T_j[a, b]
    (rss_focusing_matrices builds one for a uniform linear array; for_ula does both); the table belongs to the block, not to a
    snapshot.  The output is an ordinary covariance item for MUSIC_lin_array, capon_lin_array, rootMUSIC_linear_array,
    esprit_linear_array, source_count or spatial_smooth, which all assume white noise: T must be unitary for that.  A source
    and its echo, which no per-bin estimator separates, are two sources in the focused item.  Not a block of the reference.
    Items: input [n * num_bins, inputs**2] complex64, item i * num_bins + j = bin j of snapshot i; weights (optional)
    [n, num_bins] float32, a bin with a weight that is not positive and finite is skipped; output [n, inputs**2] complex64 and
    an optional int32 status per snapshot (0 ok, 1 no bin used, 3 a used item not finite; not 0: a NaN item).
    noutput_items counts snapshots."""

    _destroy = staticmethod(lib.doa_focus_covariance_destroy)

    def __init__(self, inputs, num_bins, matrices):
        super().__init__()
        self.num_ant_ele, self.num_bins = int(inputs), int(num_bins)
        t = None if matrices is None else np.ascontiguousarray(matrices, dtype=np.complex128)
        if t is not None and t.size != max(self.num_bins, 0) * max(self.num_ant_ele, 0) ** 2:
            raise ValueError(f"matrices holds {t.size} entries, not num_bins * inputs**2 = {self.num_bins} * {self.num_ant_ele}**2")
        self.matrices = t
        self._h = check_handle(lib.doa_focus_covariance_create(self.num_ant_ele, self.num_bins,
                                                               C.c_void_p(0) if t is None else _vp(t)), "focus_covariance")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_C64, self.num_ant_ele ** 2), (_I32, 1)]

    @classmethod
    def for_ula(cls, norm_spacing, inputs, fft_len, focus_angles, first_bin=0, num_bins=None, rate_over_carrier=0.0,
                regularization=1e-3):
        """The block for a uniform linear array with the table of rss_focusing_matrices (same arguments)."""
        t = rss_focusing_matrices(norm_spacing, inputs, fft_len, focus_angles, first_bin, num_bins, rate_over_carrier, regularization)
        return cls(inputs, t.shape[0], t)

    def work(self, noutput_items, input_items, output_items, weights=None) -> int:
        """output_items[0]: the focused items; output_items[1] (optional): the status words."""
        n = int(noutput_items)
        return check(lib.doa_focus_covariance_work(self._h, n, self._items_in(input_items[0], _C64, n * self.num_bins, self.num_ant_ele ** 2),
                                                   self._weights(weights, n), self._items_out(output_items[0], _C64, n, self.num_ant_ele ** 2),
                                                   self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, d_weights_ptr=None, d_status_ptr=None, stream=None) -> int:
        """d_out_ptr must not overlap d_in_ptr."""
        return check(lib.doa_focus_covariance_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _opt_ptr(d_weights_ptr),
                                                       _dev_ptr(d_out_ptr), _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def nout_items_total(self) -> int:
        return int(lib.doa_focus_covariance_items_total(self._h))


class find_local_max(_ItemBlock):
    """doa.find_local_max(num_max_vals, vector_len, x_min, x_max) — gr::sync_block with two
    outputs (reference lib/find_local_max_impl.cc:47-71)."""

    _destroy = staticmethod(lib.doa_find_local_max_destroy)

    def __init__(self, num_max_vals, vector_len, x_min, x_max):
        super().__init__()
        self.num_max_vals, self.vector_len = int(num_max_vals), int(vector_len)
        self.x_min, self.x_max = float(x_min), float(x_max)
        self._h = check_handle(lib.doa_find_local_max_create(self.num_max_vals, self.vector_len,
                                                             self.x_min, self.x_max), "find_local_max")
        self.in_sig = [(_F32, self.vector_len)]
        self.out_sig = [(_F32, self.num_max_vals), (_F32, self.num_max_vals)]

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        o0, o1 = output_items
        return check(lib.doa_find_local_max_work(self._h, n, self._items_in(input_items[0], _F32, n, self.vector_len),
                                                 self._items_out(o0, _F32, n, self.num_max_vals),
                                                 self._items_out(o1, _F32, n, self.num_max_vals)))

    def work_dev(self, noutput_items, d_in_ptr, d_out0_ptr, d_out1_ptr, stream=None) -> int:
        return check(lib.doa_find_local_max_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                     _dev_ptr(d_out0_ptr), _dev_ptr(d_out1_ptr),
                                                     _stream_ptr(stream)))

    def work_counts(self, noutput_items, input_items, counts, output_items) -> int:
        """work with a peak count m_i PER ITEM (int32 array): the first m_i slots of both ports are find_local_max(m_i, ...)'s,
        the rest of the num_max_vals-wide items NaN; m_i outside 0..num_max_vals: all NaN (doa_find_local_max_work_counts)."""
        n = int(noutput_items)
        o0, o1 = output_items
        return check(lib.doa_find_local_max_work_counts(self._h, n, self._items_in(input_items[0], _F32, n, self.vector_len),
                                                        self._items_in(counts, _I32, n, 1),
                                                        self._items_out(o0, _F32, n, self.num_max_vals),
                                                        self._items_out(o1, _F32, n, self.num_max_vals)))

    def work_dev_counts(self, noutput_items, d_in_ptr, d_counts_ptr, d_out0_ptr, d_out1_ptr, stream=None) -> int:
        return check(lib.doa_find_local_max_work_dev_counts(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                            _opt_ptr(d_counts_ptr), _dev_ptr(d_out0_ptr),
                                                            _dev_ptr(d_out1_ptr), _stream_ptr(stream)))


class source_count(_ItemBlock):
    """doa.source_count(num_ant_ele, num_snapshots, method="mdl", max_sources=None) — the number of sources per covariance
    item, estimated on the device from its eigenvalues (Wax-Kailath MDL, or AIC; include/doa_hip.h).  Not a block of the
    reference, which takes num_targets as a flowgraph parameter.  Port 0: int32 count (-1: non-finite or non-positive item);
    port 1 (optional): the num_ant_ele eigenvalues, ascending.  max_sources None = num_ant_ele - 1."""

    _destroy = staticmethod(lib.doa_source_count_destroy)

    def __init__(self, num_ant_ele, num_snapshots, method="mdl", max_sources=None):
        super().__init__()
        self.num_ant_ele, self.num_snapshots = int(num_ant_ele), int(num_snapshots)
        self.method = _count_method(method)
        self.max_sources = self.num_ant_ele - 1 if max_sources is None else int(max_sources)
        self._h = check_handle(lib.doa_source_count_create(self.num_ant_ele, self.num_snapshots, self.method,
                                                           self.max_sources), "source_count")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_I32, 1), (_F32, self.num_ant_ele)]

    def work(self, noutput_items, input_items, output_items) -> int:
        """output_items = [counts int32 [n]] or [counts, eigenvalues float32 [n, num_ant_ele]]."""
        n = int(noutput_items)
        return check(lib.doa_source_count_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                               self._items_out(output_items[0], _I32, n, 1),
                                               self._opt_out(output_items, 1, _F32, n, self.num_ant_ele)))

    def work_dev(self, noutput_items, d_in_ptr, d_count_ptr, d_eig_ptr=None, stream=None) -> int:
        return check(lib.doa_source_count_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                   _dev_ptr(d_count_ptr), _opt_ptr(d_eig_ptr), _stream_ptr(stream)))


class spatial_smooth(_ItemBlock):
    """doa.spatial_smooth(num_ant_ele, subarray_size, forward_backward=True) — spatial smoothing of covariance items for
    coherent sources (multipath, emitters on one oscillator): each num_ant_ele x num_ant_ele item is replaced by the
    average of its num_ant_ele - subarray_size + 1 overlapping subarray_size x subarray_size diagonal blocks, with
    forward_backward also of their persymmetric images (definition: include/doa_hip.h).  The output feeds MUSIC_lin_array /
    rootMUSIC_linear_array / source_count created for subarray_size elements.  Not a block of the reference."""

    _destroy = staticmethod(lib.doa_spatial_smooth_destroy)

    def __init__(self, num_ant_ele, subarray_size, forward_backward=True):
        super().__init__()
        self.num_ant_ele, self.subarray_size = int(num_ant_ele), int(subarray_size)
        self.forward_backward = int(forward_backward)
        self._h = check_handle(lib.doa_spatial_smooth_create(self.num_ant_ele, self.subarray_size, self.forward_backward),
                               "spatial_smooth")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_C64, self.subarray_size ** 2)]

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        return check(lib.doa_spatial_smooth_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                 self._items_out(output_items[0], _C64, n, self.subarray_size ** 2)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, stream=None) -> int:
        """d_out_ptr must not overlap d_in_ptr."""
        return check(lib.doa_spatial_smooth_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                     _dev_ptr(d_out_ptr), _stream_ptr(stream)))


# modes of coarray_covariance (DOA_COARRAY_SMOOTHED / DOA_COARRAY_TOEPLITZ, include/doa_hip.h)
_COARRAY_MODES = {"smoothed": 0, "toeplitz": 1}


def _positions(positions) -> np.ndarray:
    """Element positions as the int32 array the C entries take; anything that is not a whole number is refused here."""
    p = np.asarray(positions).reshape(-1)
    q = p.astype(np.int64) if p.size else np.zeros(0, np.int64)
    if p.size and (not np.array_equal(q, p) or np.abs(q).max() >= 2 ** 31):
        raise ValueError(f"positions must be integers (multiples of the element spacing), got {positions!r}")
    return np.ascontiguousarray(q, dtype=_I32)


def coarray_lags(positions):
    """(contiguous_size, counts) of a sparse linear array's difference co-array: the largest L such that every lag 0 .. L-1
    occurs among positions[a] - positions[b], and the number of ordered pairs with each of those lags
    (doa_coarray_lags, include/doa_hip.h; host only, no device needed).  coarray_covariance offers a virtual array of up to
    min(contiguous_size, 16) elements."""
    p = _positions(positions)
    size = C.c_int(0)
    check(lib.doa_coarray_lags(_vp(p), p.size, C.byref(size), C.c_void_p(0)))
    counts = np.zeros(size.value, _I32)
    check(lib.doa_coarray_lags(_vp(p), p.size, C.byref(size), _vp(counts)))
    return size.value, counts.tolist()


class coarray_covariance(_ItemBlock):
    """doa.coarray_covariance(positions, virtual_size=0, mode="smoothed") — the difference co-array of a sparse linear array
    (include/doa_hip.h has the definition): each len(positions) x len(positions) covariance item of elements at the integer
    positions (in units of norm_spacing, counted as MUSIC_lin_array numbers its elements) becomes the covariance item of a
    virtual uniform array of virtual_size elements (0: as many as the layout gives, at most 16; coarray_lags tells), so that
    MUSIC_lin_array, rootMUSIC_linear_array and esprit_linear_array created for self.virtual_size inputs find up to
    virtual_size - 1 sources: more than there are antennas.  mode "smoothed" (positive semidefinite, T T^H / virtual_size; its
    eigenvalues are squared, so source_count is not valid on it) or "toeplitz" (T itself, which may be indefinite).
    Not a block of the reference."""

    _destroy = staticmethod(lib.doa_coarray_covariance_destroy)

    def __init__(self, positions, virtual_size=0, mode="smoothed"):
        super().__init__()
        self.positions = _positions(positions)
        self.num_ant_ele = int(self.positions.size)
        self.mode = _named(mode, _COARRAY_MODES, "co-array mode", "smoothed or toeplitz")
        self._h = check_handle(lib.doa_coarray_covariance_create(_vp(self.positions), self.num_ant_ele, int(virtual_size), self.mode),
                               "coarray_covariance")
        self.virtual_size = int(lib.doa_coarray_covariance_virtual_size(self._h))
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_C64, self.virtual_size ** 2)]

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        return check(lib.doa_coarray_covariance_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                     self._items_out(output_items[0], _C64, n, self.virtual_size ** 2)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, stream=None) -> int:
        """d_out_ptr must not overlap d_in_ptr."""
        return check(lib.doa_coarray_covariance_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                         _dev_ptr(d_out_ptr), _stream_ptr(stream)))


class capon_lin_array(_ItemBlock):
    """doa.capon_lin_array(norm_spacing, inputs, pspectrum_len, diagonal_loading=0.0) — the Capon (minimum-variance, MVDR)
    spectrum 1 / (a^H R^-1 a) of each covariance item on MUSIC_lin_array's angle grid, in its output format (dB against the
    row maximum): no source count, no eigendecomposition, a run time that does not depend on the data (definition:
    include/doa_hip.h).  diagonal_loading is relative to the mean diagonal entry; fewer snapshots than antennas need it > 0.
    Port 0: the spectrum; port 1 (optional): int32 status, 1 = not positive definite enough (that item's row is NaN).
    Not a block of the reference."""

    _destroy = staticmethod(lib.doa_capon_lin_array_destroy)

    def __init__(self, norm_spacing, inputs, pspectrum_len, diagonal_loading=0.0):
        super().__init__()
        self.norm_spacing, self.num_ant_ele = float(norm_spacing), int(inputs)
        self.pspectrum_len, self.diagonal_loading = int(pspectrum_len), float(diagonal_loading)
        self._h = check_handle(lib.doa_capon_lin_array_create(self.norm_spacing, self.num_ant_ele, self.pspectrum_len,
                                                              self.diagonal_loading), "capon_lin_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.pspectrum_len), (_I32, 1)]

    def work(self, noutput_items, input_items, output_items) -> int:
        """output_items = [spectrum float32 [n, P]] or [spectrum, status int32 [n]]."""
        n = int(noutput_items)
        return check(lib.doa_capon_lin_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                  self._items_out(output_items[0], _F32, n, self.pspectrum_len),
                                                  self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_capon_lin_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _dev_ptr(d_out_ptr),
                                                      _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def debug(self, R_items: np.ndarray):
        """(W [n, N*N] complex64 column-major items, Q [n, P] float32) for the tests."""
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, self.num_ant_ele ** 2)
        n = a.shape[0]
        w = np.empty((n, self.num_ant_ele ** 2), dtype=_C64)
        q = np.empty((n, self.pspectrum_len), dtype=_F32)
        check(lib.doa_capon_lin_array_debug(self._h, n, _vp(a), _vp(w), _vp(q)))
        return w, q

    def nout_items_total(self) -> int:
        return int(lib.doa_capon_lin_array_items_total(self._h))


class iaa_lin_array(_ItemBlock):
    """doa.iaa_lin_array(norm_spacing, inputs, pspectrum_len, diagonal_loading=0.0, iterations=10) — the iterative adaptive
    (IAA) power spectrum of each covariance item on MUSIC_lin_array's angle grid: no source count, no eigendecomposition, no
    smoothing; it works on rank-one items (one snapshot) and on coherent sources at the full aperture, and its peak heights
    are source powers (definition: include/doa_hip.h).  A fixed number of iterations (1..32), so the run time does not
    depend on the data.  Port 0: the spectrum in dB against the row maximum; port 1 (optional): the power per direction in
    the units of the item, float32 [n, P]; port 2 (optional): int32 status, 1 = a failed pivot or a non-finite item (both
    rows NaN).  Not a block of the reference."""

    _destroy = staticmethod(lib.doa_iaa_lin_array_destroy)

    def __init__(self, norm_spacing, inputs, pspectrum_len, diagonal_loading=0.0, iterations=10):
        super().__init__()
        self.norm_spacing, self.num_ant_ele = float(norm_spacing), int(inputs)
        self.pspectrum_len, self.diagonal_loading = int(pspectrum_len), float(diagonal_loading)
        self.iterations = int(iterations)
        self._h = check_handle(lib.doa_iaa_lin_array_create(self.norm_spacing, self.num_ant_ele, self.pspectrum_len,
                                                            self.diagonal_loading, self.iterations), "iaa_lin_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.pspectrum_len), (_F32, self.pspectrum_len), (_I32, 1)]

    def work(self, noutput_items, input_items, output_items) -> int:
        """output_items = [spectrum float32 [n, P]], [spectrum, power float32 [n, P]] or [spectrum, power, status int32 [n]];
        power may be None."""
        n = int(noutput_items)
        return check(lib.doa_iaa_lin_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                self._items_out(output_items[0], _F32, n, self.pspectrum_len),
                                                self._opt_out(output_items, 1, _F32, n, self.pspectrum_len),
                                                self._opt_out(output_items, 2, _I32, n, 1)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, d_power_ptr=None, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_iaa_lin_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _dev_ptr(d_out_ptr),
                                                    _opt_ptr(d_power_ptr), _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def debug(self, R_items: np.ndarray):
        """(p [n, P] float64: the final p_k before the scaling by mu, lags [n, N] complex128: r_l of the last iteration's R)
        for the tests."""
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, self.num_ant_ele ** 2)
        n = a.shape[0]
        p = np.empty((n, self.pspectrum_len), dtype=np.float64)
        lags = np.empty((n, self.num_ant_ele), dtype=np.complex128)
        check(lib.doa_iaa_lin_array_debug(self._h, n, _vp(a), _vp(p), _vp(lags)))
        return p, lags

    def nout_items_total(self) -> int:
        return int(lib.doa_iaa_lin_array_items_total(self._h))


def _steering(table) -> np.ndarray:
    """[P, N] complex128, C-contiguous (the layout doa_MUSIC_array_create / doa_capon_array_create read)."""
    a = np.ascontiguousarray(table, dtype=np.complex128)
    if a.ndim != 2:
        raise ValueError("a steering table is a [pspectrum_len, inputs] complex array")
    return a


def uca_positions(num_ant_ele, radius) -> np.ndarray:
    """[N, 2] element positions (x, y, in wavelengths) of a uniform circular array: element n at angle 2 pi n / N."""
    ang = 2.0 * np.pi * np.arange(int(num_ant_ele), dtype=np.float64) / int(num_ant_ele)
    return np.stack([float(radius) * np.cos(ang), float(radius) * np.sin(ang)], axis=1)


def planar_steering_table(positions, pspectrum_len, az_min=0.0, az_max=360.0, elevation=90.0) -> np.ndarray:
    """The [pspectrum_len, N] complex128 steering table of a planar array (positions: [N, 2] in wavelengths) on the azimuth
    grid az_i = az_min + i (az_max - az_min) / pspectrum_len at one elevation (degrees from the array normal; 90 = in the
    array's plane): a_i[n] = exp(+j 2 pi sin(elevation) (x_n cos az_i + y_n sin az_i))  (doa_planar_steering_table; host
    only, no device needed)."""
    xy = np.ascontiguousarray(positions, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("positions is an [inputs, 2] array of (x, y) in wavelengths")
    n, p = xy.shape[0], int(pspectrum_len)
    out = np.empty((max(p, 0), n), dtype=np.complex128)
    check(lib.doa_planar_steering_table(n, _vp(xy), p, float(az_min), float(az_max), float(elevation), _vp(out)))
    return out


def planar_steering_grid(positions, n_az, n_el, az_min=0.0, az_max=360.0, el_min=0.0, el_max=90.0) -> np.ndarray:
    """The [n_az * n_el, N] complex128 steering table of a planar array on an azimuth x elevation grid: row e * n_az + a is row
    a of planar_steering_table(positions, n_az, az_min, az_max, el_e), el_e = el_min + e (el_max - el_min) / n_el, bit for
    bit (doa_planar_steering_grid; host only, no device needed).  The row order find_local_max_2d reads."""
    xy = np.ascontiguousarray(positions, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("positions is an [inputs, 2] array of (x, y) in wavelengths")
    n, na, ne = xy.shape[0], int(n_az), int(n_el)
    out = np.empty((max(na, 0) * max(ne, 0), n), dtype=np.complex128)
    check(lib.doa_planar_steering_grid(n, _vp(xy), na, float(az_min), float(az_max), ne, float(el_min), float(el_max), _vp(out)))
    return out


def array_grid_debug(table, n_az, n_el, records, num_max_vals, fused=True, az_min=0.0, az_max=360.0, el_min=0.0, el_max=90.0,
                     wrap_az=True, spectrum=True):
    """Test hook (doa_hip_array_grid_debug): the steering-table scan that ends in find_local_max_2d's pick, on supplied full
    records [n, inputs^2] float64 (the packing of csrc/kernels.hpp).  fused: the one launch of music_pipeline's grid mode, else the
    two launches it replaces.  Returns (spectrum [n, P] or None, values, azimuths, elevations [n, num_max_vals])."""
    a = _steering(table)
    rec = np.ascontiguousarray(records, np.float64)
    n, M = rec.shape[0], int(num_max_vals)
    assert rec.shape == (n, a.shape[1] ** 2) and a.shape[0] == int(n_az) * int(n_el)
    spec = np.empty((n, a.shape[0]), _F32) if spectrum else None
    val, az, el = (np.empty((n, M), _F32) for _ in range(3))
    check(lib.doa_hip_array_grid_debug(a.shape[1], _vp(a), int(n_az), int(n_el), float(az_min), float(az_max), float(el_min),
                                       float(el_max), int(bool(wrap_az)), M, n, _vp(rec), int(bool(fused)),
                                       _vp(spec) if spectrum else C.c_void_p(0), _vp(val), _vp(az), _vp(el)))
    return spec, val, az, el


class find_local_max_2d(_ItemBlock):
    """doa.find_local_max_2d(num_max_vals, n_az, n_el, az_min, az_max, el_min, el_max, wrap_az) — the num_max_vals largest
    local maxima of an azimuth x elevation grid (items of n_az * n_el floats, cell (e, a) at e * n_az + a) as three paired
    outputs: values (descending), azimuths, elevations; slots beyond the number of peaks are NaN.  wrap_az makes the first and
    the last azimuth neighbours; n_el = 1 with wrap_az is the circular one-dimensional peak pick (the rule:
    include/doa_hip.h).  Not a block of the reference."""

    _destroy = staticmethod(lib.doa_find_local_max_2d_destroy)

    def __init__(self, num_max_vals, n_az, n_el, az_min=0.0, az_max=360.0, el_min=0.0, el_max=90.0, wrap_az=True):
        super().__init__()
        self.num_max_vals, self.n_az, self.n_el = int(num_max_vals), int(n_az), int(n_el)
        self.az_min, self.az_max, self.el_min, self.el_max = float(az_min), float(az_max), float(el_min), float(el_max)
        self.wrap_az = bool(wrap_az)
        self._h = check_handle(lib.doa_find_local_max_2d_create(self.num_max_vals, self.n_az, self.n_el, self.az_min, self.az_max,
                                                                self.el_min, self.el_max, int(self.wrap_az)), "find_local_max_2d")
        self.vector_len = self.n_az * self.n_el
        self.in_sig = [(_F32, self.vector_len)]
        self.out_sig = [(_F32, self.num_max_vals)] * 3

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        o0, o1, o2 = output_items
        return check(lib.doa_find_local_max_2d_work(self._h, n, self._items_in(input_items[0], _F32, n, self.vector_len),
                                                    self._items_out(o0, _F32, n, self.num_max_vals),
                                                    self._items_out(o1, _F32, n, self.num_max_vals),
                                                    self._items_out(o2, _F32, n, self.num_max_vals)))

    def work_dev(self, noutput_items, d_in_ptr, d_out0_ptr, d_out1_ptr, d_out2_ptr, stream=None) -> int:
        return check(lib.doa_find_local_max_2d_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _dev_ptr(d_out0_ptr),
                                                        _dev_ptr(d_out1_ptr), _dev_ptr(d_out2_ptr), _stream_ptr(stream)))

    def nout_items_total(self) -> int:
        return int(lib.doa_find_local_max_2d_items_total(self._h))


class MUSIC_array(_ItemBlock):
    """doa.MUSIC_array(num_targets, steering) — the MUSIC spectrum for an arbitrary array geometry: steering is a
    [pspectrum_len, inputs] complex table (row i = the array response towards direction i; planar_steering_table builds one
    for a planar array, a measured manifold works as well), Q_i = Re(a_i^H P_N a_i) in double, output as MUSIC_lin_array's
    (dB against the row maximum; definition: include/doa_hip.h).  Internal precision 64 only.  Not a block of the reference."""

    _destroy = staticmethod(lib.doa_MUSIC_array_destroy)
    _set_precision = staticmethod(lib.doa_MUSIC_array_set_internal_precision)

    def __init__(self, num_targets, steering):
        super().__init__()
        a = _steering(steering)
        self.num_targets, self.pspectrum_len, self.num_ant_ele = int(num_targets), int(a.shape[0]), int(a.shape[1])
        self._h = check_handle(lib.doa_MUSIC_array_create(self.num_targets, self.num_ant_ele, self.pspectrum_len, _vp(a)),
                               "MUSIC_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.pspectrum_len)]

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        return check(lib.doa_MUSIC_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                              self._items_out(output_items[0], _F32, n, self.pspectrum_len)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, stream=None) -> int:
        return check(lib.doa_MUSIC_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _dev_ptr(d_out_ptr),
                                                  _stream_ptr(stream)))

    def debug(self, R_items: np.ndarray):
        """(P_N [n, N*N] complex128 column-major items, Q [n, P] float32) for the tests."""
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, self.num_ant_ele ** 2)
        n = a.shape[0]
        pn = np.empty((n, self.num_ant_ele ** 2), dtype=np.complex128)
        q = np.empty((n, self.pspectrum_len), dtype=_F32)
        check(lib.doa_MUSIC_array_debug(self._h, n, _vp(a), _vp(pn), _vp(q)))
        return pn, q

    def nout_items_total(self) -> int:
        return int(lib.doa_MUSIC_array_items_total(self._h))


class capon_array(_ItemBlock):
    """doa.capon_array(steering, diagonal_loading=0.0) — the Capon (MVDR) spectrum 1 / (a^H R^-1 a) for an arbitrary array
    geometry: steering as for MUSIC_array, the inverse, its status and diagonal_loading exactly as capon_lin_array's
    (definition: include/doa_hip.h).  Port 0: the spectrum; port 1 (optional): int32 status, 1 = not positive definite enough
    (that item's row is NaN).  Internal precision 64 only.  Not a block of the reference."""

    _destroy = staticmethod(lib.doa_capon_array_destroy)

    def __init__(self, steering, diagonal_loading=0.0):
        super().__init__()
        a = _steering(steering)
        self.pspectrum_len, self.num_ant_ele = int(a.shape[0]), int(a.shape[1])
        self.diagonal_loading = float(diagonal_loading)
        self._h = check_handle(lib.doa_capon_array_create(self.num_ant_ele, self.pspectrum_len, _vp(a), self.diagonal_loading),
                               "capon_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.pspectrum_len), (_I32, 1)]

    def work(self, noutput_items, input_items, output_items) -> int:
        """output_items = [spectrum float32 [n, P]] or [spectrum, status int32 [n]]."""
        n = int(noutput_items)
        return check(lib.doa_capon_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                              self._items_out(output_items[0], _F32, n, self.pspectrum_len),
                                              self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_capon_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _dev_ptr(d_out_ptr),
                                                  _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def debug(self, R_items: np.ndarray):
        """(W [n, N*N] complex128 column-major items, Q [n, P] float32) for the tests."""
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, self.num_ant_ele ** 2)
        n = a.shape[0]
        w = np.empty((n, self.num_ant_ele ** 2), dtype=np.complex128)
        q = np.empty((n, self.pspectrum_len), dtype=_F32)
        check(lib.doa_capon_array_debug(self._h, n, _vp(a), _vp(w), _vp(q)))
        return w, q

    def nout_items_total(self) -> int:
        return int(lib.doa_capon_array_items_total(self._h))


class rootMUSIC_linear_array(_ItemBlock):
    """doa.rootMUSIC_linear_array(norm_spacing, num_targets, inputs) — gr::sync_block
    (reference lib/rootMUSIC_linear_array_impl.cc:46-59)."""

    _destroy = staticmethod(lib.doa_rootMUSIC_linear_array_destroy)
    _set_precision = staticmethod(lib.doa_rootMUSIC_linear_array_set_internal_precision)

    def __init__(self, norm_spacing, num_targets, inputs):
        super().__init__()
        self.norm_spacing, self.num_targets, self.num_ant_ele = float(norm_spacing), int(num_targets), int(inputs)
        self._h = check_handle(lib.doa_rootMUSIC_linear_array_create(self.norm_spacing, self.num_targets,
                                                                     self.num_ant_ele), "rootMUSIC_linear_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.num_targets)]   # io_signature::make(1, num_targets, ...): port 0 only is written

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        return check(lib.doa_rootMUSIC_linear_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                         self._items_out(output_items[0], _F32, n, self.num_targets)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, stream=None) -> int:
        return check(lib.doa_rootMUSIC_linear_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                             _dev_ptr(d_out_ptr), _stream_ptr(stream)))

    def work_counts(self, noutput_items, input_items, counts, output_items) -> int:
        """work with a source count PER ITEM (int32 array) in place of num_targets: items stay num_targets floats wide, the
        first count slots are rootMUSIC_linear_array(norm_spacing, count, inputs)'s and the rest NaN; count 0 gives an all-NaN
        item, and so does a count outside 0..min(num_targets, inputs-1) (source_count's -1 status included).  Raises
        DoaError(DOA_ERR_NUMERIC) only for an item with a usable count and no root inside the unit circle
        (doa_rootMUSIC_linear_array_work_counts)."""
        n = int(noutput_items)
        return check(lib.doa_rootMUSIC_linear_array_work_counts(
            self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2), self._items_in(counts, _I32, n, 1),
            self._items_out(output_items[0], _F32, n, self.num_targets)))

    def work_dev_counts(self, noutput_items, d_in_ptr, d_counts_ptr, d_out_ptr, d_status_ptr=None, stream=None) -> int:
        """The device form; d_status_ptr (optional): one int32 per item, 0 = fine, 1 = no root inside the unit circle,
        2 = no usable count."""
        return check(lib.doa_rootMUSIC_linear_array_work_dev_counts(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                                    _opt_ptr(d_counts_ptr), _dev_ptr(d_out_ptr),
                                                                    _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def debug(self, R_items: np.ndarray):
        """(angles [n, M] float32, roots [n, 2N-2] complex128, status [n] int32) for parity tests."""
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, self.num_ant_ele ** 2)
        n = a.shape[0]
        ang = np.empty((n, self.num_targets), dtype=_F32)
        roots = np.empty((n, 2 * self.num_ant_ele - 2), dtype=np.complex128)
        status = np.empty(n, dtype=np.int32)
        check(lib.doa_rootMUSIC_linear_array_debug(self._h, n, _vp(a), _vp(ang), _vp(roots), _vp(status)))
        return ang, roots, status

    def select_debug(self, roots: np.ndarray):
        """The device's root-selection stage alone (reference lib/rootMUSIC_linear_array_impl.cc:122-145) on the given
        roots [n, 2N-2] complex128 -> (angles [n, M] float32, status [n] int32; 1 = no interior root)."""
        z = np.ascontiguousarray(roots, dtype=np.complex128).reshape(-1, 2 * self.num_ant_ele - 2)
        n = z.shape[0]
        ang = np.empty((n, self.num_targets), dtype=_F32)
        status = np.empty(n, dtype=np.int32)
        check(lib.doa_rootMUSIC_linear_array_select_debug(self._h, n, _vp(z), _vp(ang), _vp(status)))
        return ang, status

    def select_counts_debug(self, roots: np.ndarray, counts):
        """select_debug with a count per item (int32 [n]) -> (angles [n, M] float32, status [n] int32; 1 = no interior root,
        2 = no usable count): the selection stage of work_counts."""
        z = np.ascontiguousarray(roots, dtype=np.complex128).reshape(-1, 2 * self.num_ant_ele - 2)
        n = z.shape[0]
        ang = np.empty((n, self.num_targets), dtype=_F32)
        status = np.empty(n, dtype=np.int32)
        check(lib.doa_rootMUSIC_linear_array_select_counts_debug(self._h, n, _vp(z), self._items_in(counts, _I32, n, 1), _vp(ang),
                                                                 _vp(status)))
        return ang, status


class esprit_linear_array(_ItemBlock):
    """doa.esprit_linear_array(norm_spacing, num_targets, inputs) — least-squares ESPRIT for a uniform linear array: the
    angles from the eigenvalues of the num_targets x num_targets matrix that maps the signal subspace of rows 0..N-2 onto rows
    1..N-1; no polynomial, no search, no unit-circle filter (definition: include/doa_hip.h).  Port 0: num_targets angles in
    degrees, ascending, NaN last; port 1 (optional): int32 status, 0 = ok, 1 = not solvable, 2 = no usable count (counts
    entries), 3 = the eigenvalue iteration reached its cap; a non-zero status gives an all-NaN item.
    Not a block of the reference."""

    _destroy = staticmethod(lib.doa_esprit_linear_array_destroy)

    def __init__(self, norm_spacing, num_targets, inputs):
        super().__init__()
        self.norm_spacing, self.num_targets, self.num_ant_ele = float(norm_spacing), int(num_targets), int(inputs)
        self._h = check_handle(lib.doa_esprit_linear_array_create(self.norm_spacing, self.num_targets, self.num_ant_ele),
                               "esprit_linear_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_F32, self.num_targets), (_I32, 1)]

    def work(self, noutput_items, input_items, output_items) -> int:
        """output_items = [angles float32 [n, num_targets]] or [angles, status int32 [n]]."""
        n = int(noutput_items)
        return check(lib.doa_esprit_linear_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                      self._items_out(output_items[0], _F32, n, self.num_targets),
                                                      self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_esprit_linear_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr), _dev_ptr(d_out_ptr),
                                                          _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def work_counts(self, noutput_items, input_items, counts, output_items) -> int:
        """work with a source count PER ITEM (int32 array) in place of num_targets, with the semantics of
        rootMUSIC_linear_array.work_counts: items stay num_targets floats wide, the first count slots are
        esprit_linear_array(norm_spacing, count, inputs)'s and the rest NaN; count 0: all NaN, status 0; a count outside
        0..min(num_targets, inputs-1) (source_count's -1 included): all NaN, status 2."""
        n = int(noutput_items)
        return check(lib.doa_esprit_linear_array_work_counts(
            self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2), self._items_in(counts, _I32, n, 1),
            self._items_out(output_items[0], _F32, n, self.num_targets), self._opt_out(output_items, 1, _I32, n, 1)))

    def work_dev_counts(self, noutput_items, d_in_ptr, d_counts_ptr, d_out_ptr, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_esprit_linear_array_work_dev_counts(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                                 _opt_ptr(d_counts_ptr), _dev_ptr(d_out_ptr),
                                                                 _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def record_debug(self, R_items: np.ndarray, records: np.ndarray, counts=None):
        """esprit_kernel alone on the given signal-subspace records [n, 2 N^2] float64 (gr-doa_amd/csrc/kernels.hpp) in place
        of the eigen stage's; R_items [n, N*N] complex64 supplies the trace and finiteness test; counts: int32 [n] or None
        -> (angles [n, num_targets] float32, status [n] int32), for the solver tests."""
        N = self.num_ant_ele
        a = np.ascontiguousarray(R_items, dtype=_C64).reshape(-1, N * N)
        n = a.shape[0]
        rec = np.ascontiguousarray(records, dtype=np.float64).reshape(n, 2 * N * N)
        cnt = None if counts is None else np.ascontiguousarray(counts, dtype=_I32).reshape(n)
        ang = np.empty((n, self.num_targets), dtype=_F32)
        status = np.empty(n, dtype=np.int32)
        check(lib.doa_esprit_linear_array_record_debug(self._h, n, _vp(a), _vp(rec), C.c_void_p(0) if cnt is None else _vp(cnt),
                                                       _vp(ang), _vp(status)))
        return ang, status


class calibrate_lin_array(_ItemBlock):
    """doa.calibrate_lin_array(norm_spacing, num_ant_ele, pilot_angle) — gr::sync_block, vlen N^2
    complex in, vlen N complex out (reference lib/calibrate_lin_array_impl.cc:46-75)."""

    _destroy = staticmethod(lib.doa_calibrate_lin_array_destroy)
    _set_precision = staticmethod(lib.doa_calibrate_lin_array_set_internal_precision)

    def __init__(self, norm_spacing, num_ant_ele, pilot_angle):
        super().__init__()
        self.norm_spacing, self.num_ant_ele, self.pilot_angle = float(norm_spacing), int(num_ant_ele), float(pilot_angle)
        self._h = check_handle(lib.doa_calibrate_lin_array_create(self.norm_spacing, self.num_ant_ele, self.pilot_angle),
                               "calibrate_lin_array")
        self.in_sig = [(_C64, self.num_ant_ele ** 2)]
        self.out_sig = [(_C64, self.num_ant_ele)]

    def work(self, noutput_items, input_items, output_items) -> int:
        n = int(noutput_items)
        return check(lib.doa_calibrate_lin_array_work(self._h, n, self._items_in(input_items[0], _C64, n, self.num_ant_ele ** 2),
                                                      self._items_out(output_items[0], _C64, n, self.num_ant_ele)))

    def work_dev(self, noutput_items, d_in_ptr, d_out_ptr, stream=None) -> int:
        return check(lib.doa_calibrate_lin_array_work_dev(self._h, int(noutput_items), _dev_ptr(d_in_ptr),
                                                          _dev_ptr(d_out_ptr), _stream_ptr(stream)))


class _Pipeline(_StreamInput, _Block):
    """Base of the two fused handles (music_pipeline, root_pipeline): the autocorrelate front, the lanes and the test aids,
    which their C entries share word for word (csrc/pipeline_front.hpp).  The C functions are doa_<_prefix>_<name>."""

    _prefix = None

    @classmethod
    def _fn(cls, name):
        return getattr(lib, f"doa_{cls._prefix}_{name}")

    def history(self) -> int:
        return self.overlap_size + 1                          # as doa.autocorrelate (autocorrelate_impl.cc:56-57)

    def forecast(self, noutput_items: int) -> int:
        return (self.snapshot_size - self.overlap_size) * int(noutput_items)

    def input_span(self, noutput_items) -> int:
        n = int(noutput_items)
        return 0 if n <= 0 else (n - 1) * (self.snapshot_size - self.overlap_size) + self.snapshot_size

    def fuse_antenna_correction(self, correction) -> None:
        _fuse(self._fn("fuse_antenna_correction"), self._h, correction, self.inputs)

    def set_spatial_smoothing(self, subarray_size, forward_backward=True) -> None:
        """Spatial smoothing between K1 and the eigen stage (coherent sources), from the next work call on, in every entry:
        the eigen stage and what follows it (scan and peak pick, or the root finder) then run for subarray_size elements
        (num_targets < subarray_size <= inputs; for root_pipeline choose subarray_size >= num_targets + 2); the covariance
        output stays inputs x inputs; work_dev_auto's eigenvalues are subarray_size per item.  0 switches it off
        (doa_music_pipeline_set_spatial_smoothing, doa_root_pipeline_set_spatial_smoothing)."""
        check(self._fn("set_spatial_smoothing")(self._h, int(subarray_size), int(forward_backward)))
        self.subarray_size = int(subarray_size)
        self.forward_backward = int(forward_backward) if self.subarray_size else 0

    def inject_failure(self, chunk_index: int) -> None:
        """Test aid: the next work() / work_dev_batches() call fails in chunk / batch `chunk_index` as if a HIP call had
        (one-shot; -1 disarms)."""
        check(self._fn("inject_failure")(self._h, int(chunk_index)))

    def lanes_idle(self) -> bool:
        """Test aid: True when neither copy/compute lane of the host-buffer entry has work pending."""
        return bool(check(self._fn("lanes_idle")(self._h)))

    def set_lanes(self, n_lanes: int) -> None:
        check(self._fn("set_lanes")(self._h, int(n_lanes)))

    def set_lane_streams(self, streams) -> None:
        """Lanes on streams the caller created (torch.cuda.Stream objects or hipStream_t values); the caller keeps them alive."""
        self._lane_streams = list(streams)
        check(self._fn("set_lane_streams")(self._h, len(self._lane_streams),
                                           ptr_array([_stream_ptr(s).value or 0 for s in self._lane_streams])))

    def synchronize(self) -> None:
        """Host-side join of the lanes (after work_dev_batches(..., stream=doa.DETACHED))."""
        check(self._fn("synchronize")(self._h))

    def _flat_inputs(self, nb, d_input_ptrs):
        """prepare_batches: nb lists of `inputs` device pointers (or one flat list) as one pointer array."""
        flat = [p for b in d_input_ptrs for p in b] if nb and isinstance(d_input_ptrs[0], (list, tuple)) else list(d_input_ptrs)
        assert len(flat) == nb * self.inputs
        return ptr_array(flat)

    @staticmethod
    def _opt_ptrs(ptrs):
        """prepare_batches: an optional list of device pointers (0 / None = not wanted), or None."""
        return None if ptrs is None else ptr_array([int(p or 0) for p in ptrs])


class music_pipeline(_Pipeline):
    """autocorrelate -> MUSIC_lin_array -> find_local_max(num_targets, pspectrum_len, 0, 180) on
    device-resident streams (the wiring of apps/run_MUSIC_lin_array_simulation.grc); the batch
    entry point the benchmark drives.  Not a block of the reference."""

    _prefix = "music_pipeline"
    _destroy = staticmethod(lib.doa_music_pipeline_destroy)
    _set_precision = staticmethod(lib.doa_music_pipeline_set_internal_precision)
    _set_format = staticmethod(lib.doa_music_pipeline_set_input_format)

    def __init__(self, inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets,
                 pspectrum_len, max_batch=4096):
        super().__init__()
        self.inputs, self.snapshot_size, self.overlap_size = int(inputs), int(snapshot_size), int(overlap_size)
        self.avg_method, self.norm_spacing = int(avg_method), float(norm_spacing)
        self.num_targets, self.pspectrum_len, self.max_batch = int(num_targets), int(pspectrum_len), int(max_batch)
        self.subarray_size, self.forward_backward = 0, 0            # set_spatial_smoothing
        self.estimator, self.diagonal_loading = "music", 0.0        # set_estimator
        self.steering_table = None                                  # set_steering_table / set_steering_grid
        self.steering_grid = None                                   # set_steering_grid: (n_az, n_el), argmax is [n, 2 M]
        self._h = check_handle(lib.doa_music_pipeline_create(self.inputs, self.snapshot_size, self.overlap_size,
                                                             self.avg_method, self.norm_spacing, self.num_targets,
                                                             self.pspectrum_len, self.max_batch), "music_pipeline")
        # as a flowgraph block (gr::doa::music_pipeline of the C++ shells, grc/doa_music_pipeline.xml): N complex
        # streams in; out0 = peak locations, out1 = peak values, out2 = spectrum
        self.in_sig = [(_C64, 1)] * self.inputs
        self.out_sig = [(_F32, self.num_targets), (_F32, self.num_targets), (_F32, self.pspectrum_len)]

    def general_work(self, noutput_items, input_items, output_items):
        """output_items = [argmax [>=n, M], max [>=n, M], spectrum [>=n, P]] (trailing ports may be omitted).
        Returns (items produced, items consumed per input)."""
        n, done = int(noutput_items), 0
        S = self.snapshot_size - self.overlap_size
        while done < n:
            k = min(self.max_batch, n - done)
            am = output_items[0][done:done + k]
            mx = output_items[1][done:done + k] if len(output_items) > 1 else np.empty((k, self.num_targets), _F32)
            sp = output_items[2][done:done + k] if len(output_items) > 2 else None
            done += self.work(k, [self._samples(a)[done * S:] for a in input_items], mx, am, spectrum_out=sp)
        return done, self.forecast(done)

    def set_estimator(self, estimator, diagonal_loading=0.0) -> None:
        """ "music" (the default) or "capon": from the next work call on, the eigen launch is replaced by the Capon inverse
        launch (capon_lin_array's; diagonal_loading as there) and num_targets only means "how many peaks"; an item that is
        not positive definite enough gets NaN peaks and a NaN row.  work_dev_auto is not available in Capon mode
        (doa_music_pipeline_set_estimator)."""
        code = _named(estimator, _ESTIMATORS, "estimator", "music or capon", ints=False)
        check(lib.doa_music_pipeline_set_estimator(self._h, code, float(diagonal_loading)))
        self.estimator = estimator.lower()
        self.diagonal_loading = float(diagonal_loading) if self.estimator == "capon" else 0.0

    def set_steering_table(self, table, x_min=0.0, x_max=360.0) -> None:
        """An arbitrary array geometry, from the next work call on: table is a [pspectrum_len, inputs] complex steering table
        (planar_steering_table builds one; MUSIC_array / capon_array define its use), (x_min, x_max) the peak pick's axis for its
        directions.  The outputs are those of autocorrelate -> MUSIC_array | capon_array -> find_local_max, bit for bit.  None
        restores the uniform linear array and the 0..180 axis.  Not available together with spatial smoothing or
        work_dev_auto (doa_music_pipeline_set_steering_table)."""
        if table is None:
            check(lib.doa_music_pipeline_set_steering_table(self._h, C.c_void_p(0), 0.0, 180.0))
            self.steering_table = self.steering_grid = None
            return
        a = _steering(table)
        if a.shape != (self.pspectrum_len, self.inputs):
            raise ValueError(f"the steering table must be [pspectrum_len, inputs] = [{self.pspectrum_len}, {self.inputs}], got {list(a.shape)}")
        check(lib.doa_music_pipeline_set_steering_table(self._h, _vp(a), float(x_min), float(x_max)))
        self.steering_table, self.steering_grid = a, None

    def set_steering_grid(self, table, n_az, n_el, az_min=0.0, az_max=360.0, el_min=0.0, el_max=90.0, wrap_az=True) -> None:
        """Grid mode, from the next work call on: table is a [n_az * n_el, inputs] complex steering table whose row e * n_az + a
        is the direction (azimuth a, elevation e) (planar_steering_grid builds one; n_az * n_el == pspectrum_len), and the peak
        pick is find_local_max_2d(num_targets, n_az, n_el, az_min, az_max, el_min, el_max, wrap_az) on each row while the scan
        still holds it on chip.  max stays [n, M]; argmax becomes [n, 2 M]: argmax[:, :M] the azimuths and argmax[:, M:] the
        elevations, in the order of max, NaN beyond the number of peaks.  The outputs are those of autocorrelate -> MUSIC_array |
        capon_array -> find_local_max_2d, bit for bit.  Limits as for set_steering_table: no spatial smoothing, no work_dev_auto,
        internal precision 64.  set_steering_table(None) leaves grid mode (doa_pipeline_set_steering_grid)."""
        a = _steering(table)
        if a.shape != (self.pspectrum_len, self.inputs):
            raise ValueError(f"the steering table must be [pspectrum_len, inputs] = [{self.pspectrum_len}, {self.inputs}], got {list(a.shape)}")
        check(lib.doa_pipeline_set_steering_grid(self._h, _vp(a), int(n_az), int(n_el), float(az_min), float(az_max), float(el_min),
                                                 float(el_max), int(bool(wrap_az))))
        self.steering_table, self.steering_grid = a, (int(n_az), int(n_el))

    def set_stages(self, cov=True, evd=True, scan=True) -> None:
        """Profiling aid: drop stages from later work_dev calls (their outputs keep the previous call's values)."""
        check(lib.doa_music_pipeline_set_stages(self._h, (1 if cov else 0) | (2 if evd else 0) | (4 if scan else 0)))

    def work_dev(self, noutput_items, d_input_ptrs, d_cov_ptr, d_spec_ptr, d_max_ptr, d_argmax_ptr, stream=None) -> int:
        return check(lib.doa_music_pipeline_work_dev(
            self._h, int(noutput_items), ptr_array(d_input_ptrs), C.c_void_p(int(d_cov_ptr or 0)),
            C.c_void_p(int(d_spec_ptr or 0)), C.c_void_p(int(d_max_ptr)), C.c_void_p(int(d_argmax_ptr)),
            _stream_ptr(stream)))

    def work_dev_auto(self, noutput_items, d_input_ptrs, d_max_ptr, d_argmax_ptr, d_count_ptr, method="mdl", d_cov_ptr=None,
                      d_spec_ptr=None, d_eig_ptr=None, stream=None) -> int:
        """work_dev with the source count estimated per snapshot (K = snapshot_size, at most num_targets sources): max / arg-max
        stay num_targets wide, the first count slots filled and the rest NaN; counts (int32, required) and the eigenvalues
        (optional) come out of the same eigen launch (doa_music_pipeline_work_dev_auto)."""
        return check(lib.doa_music_pipeline_work_dev_auto(
            self._h, int(noutput_items), ptr_array(d_input_ptrs), _count_method(method), _opt_ptr(d_cov_ptr), _opt_ptr(d_spec_ptr),
            _opt_ptr(d_max_ptr), _opt_ptr(d_argmax_ptr), _opt_ptr(d_count_ptr), _opt_ptr(d_eig_ptr), _stream_ptr(stream)))

    def work_dev_batches(self, noutput_items, d_input_ptrs, d_cov_ptrs, d_spec_ptrs, d_max_ptrs, d_argmax_ptrs, stream=None) -> int:
        """n_batches = len(d_max_ptrs) batches in one call, overlapped over the handle's own lanes (doa_hip.h).
        d_input_ptrs: n_batches lists of `inputs` device pointers (or one flat list); d_cov_ptrs / d_spec_ptrs: lists of
        device pointers (0 = not wanted) or None."""
        return self.prepare_batches(noutput_items, d_input_ptrs, d_cov_ptrs, d_spec_ptrs, d_max_ptrs, d_argmax_ptrs, stream)()

    def prepare_batches(self, noutput_items, d_input_ptrs, d_cov_ptrs, d_spec_ptrs, d_max_ptrs, d_argmax_ptrs, stream=None):
        """The argument marshalling of work_dev_batches done once: returns a callable that makes the C call (a C or C++
        caller has its pointer arrays at hand; a Python caller that repeats a call should not rebuild them every time)."""
        nb = len(d_max_ptrs)
        assert len(d_argmax_ptrs) == nb
        args = (self._h, nb, int(noutput_items), self._flat_inputs(nb, d_input_ptrs), self._opt_ptrs(d_cov_ptrs),
                self._opt_ptrs(d_spec_ptrs), ptr_array(d_max_ptrs), ptr_array(d_argmax_ptrs), _stream_ptr(stream))
        fn = lib.doa_music_pipeline_work_dev_batches
        return lambda: check(fn(*args))

    def work(self, noutput_items, input_items, max_out, argmax_out, cov_out=None, spectrum_out=None) -> int:
        """Host buffers in, host buffers out (numpy): input_items[k] = complex64 stream k starting at
        its first history sample; max_out / argmax_out [>=n, M] float32; cov_out [>=n, N*N] complex64
        and spectrum_out [>=n, P] float32 are optional.  In grid mode (set_steering_grid) argmax_out is [n, 2 M]."""
        n = int(noutput_items)
        arrs = self._host_streams(input_items, self.input_span(n))
        if self.steering_grid is not None and (argmax_out.ndim != 2 or argmax_out.shape[0] < n or argmax_out.shape[1] != 2 * self.num_targets):
            raise ValueError(f"grid mode: argmax_out must be [>= {n}, 2 * num_targets = {2 * self.num_targets}], got {list(argmax_out.shape)}")
        am_width = self.num_targets * (2 if self.steering_grid is not None else 1)
        for o, dt, per in ((max_out, _F32, self.num_targets), (argmax_out, _F32, am_width),
                           (cov_out, _C64, self.inputs ** 2), (spectrum_out, _F32, self.pspectrum_len)):
            if o is not None:
                assert o.dtype == dt and o.flags.c_contiguous and o.size >= n * per
        none = C.c_void_p(0)
        return check(lib.doa_music_pipeline_work(
            self._h, n, ptr_array([a.ctypes.data for a in arrs]), none if cov_out is None else _vp(cov_out),
            none if spectrum_out is None else _vp(spectrum_out), _vp(max_out), _vp(argmax_out)))


class music_pipeline_sc16(music_pipeline):
    """music_pipeline on complex int16 streams (sc16 items, widened on the device as float32(q) * float32(scale));
    the host entries take int16 arrays [n, 2] (or flat 2n), the device entries pointers to int16 data.  Outputs are bit
    for bit those of music_pipeline on the widened samples.  Not a block of the reference."""

    def __init__(self, inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets, pspectrum_len,
                 scale=SC16_DEFAULT_SCALE, max_batch=4096):
        super().__init__(inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets, pspectrum_len, max_batch)
        self.set_input_format("sc16", scale)
        self.in_sig = [(_I16, 2)] * self.inputs


class root_pipeline(_Pipeline):
    """autocorrelate -> rootMUSIC_linear_array on device-resident streams (the wiring of
    apps/run_RootMUSIC_lin_array_simulation.grc) as ONE handle: the Root-MUSIC branch of the hot path with the same entry
    points as music_pipeline (work_dev, work_dev_batches over the handle's lanes, detached form, host-buffer work).
    Not a block of the reference."""

    _prefix = "root_pipeline"
    _destroy = staticmethod(lib.doa_root_pipeline_destroy)
    _set_precision = staticmethod(lib.doa_root_pipeline_set_internal_precision)
    _set_format = staticmethod(lib.doa_root_pipeline_set_input_format)

    def __init__(self, inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets, max_batch=4096):
        super().__init__()
        self.inputs, self.snapshot_size, self.overlap_size = int(inputs), int(snapshot_size), int(overlap_size)
        self.avg_method, self.norm_spacing = int(avg_method), float(norm_spacing)
        self.num_targets, self.max_batch = int(num_targets), int(max_batch)
        self._h = check_handle(lib.doa_root_pipeline_create(self.inputs, self.snapshot_size, self.overlap_size, self.avg_method,
                                                            self.norm_spacing, self.num_targets, self.max_batch), "root_pipeline")
        self.subarray_size, self.forward_backward = 0, 0            # set_spatial_smoothing
        self.estimator = "root_music"                               # set_estimator
        # as a flowgraph block (gr::doa::root_music_pipeline of the C++ shells): N complex streams in; out0 = angles
        self.in_sig = [(_C64, 1)] * self.inputs
        self.out_sig = [(_F32, self.num_targets)]

    def general_work(self, noutput_items, input_items, output_items):
        """output_items = [angles [>=n, M]].  Returns (items produced, items consumed per input)."""
        n, done = int(noutput_items), 0
        S = self.snapshot_size - self.overlap_size
        while done < n:
            k = min(self.max_batch, n - done)
            done += self.work(k, [self._samples(a)[done * S:] for a in input_items], output_items[0][done:done + k])
        return done, self.forecast(done)

    def set_estimator(self, estimator) -> None:
        """ "root_music" (the default) or "esprit": from the next work call on, in every entry, the eigen launch writes the
        signal-subspace record and esprit_kernel takes the root finder's place (esprit_linear_array's definition and status
        codes; work() raises DoaError(DOA_ERR_NUMERIC) for any non-zero status).  K1 and the covariance output are unchanged
        (doa_root_pipeline_set_estimator)."""
        check(lib.doa_root_pipeline_set_estimator(self._h, _named(estimator, _GRIDFREE, "estimator", "root_music or esprit", ints=False)))
        self.estimator = estimator.lower()

    def work_dev(self, noutput_items, d_input_ptrs, d_cov_ptr, d_angles_ptr, d_status_ptr=None, stream=None) -> int:
        return check(lib.doa_root_pipeline_work_dev(
            self._h, int(noutput_items), ptr_array(d_input_ptrs), C.c_void_p(int(d_cov_ptr or 0)), C.c_void_p(int(d_angles_ptr)),
            C.c_void_p(int(d_status_ptr or 0)), _stream_ptr(stream)))

    def work_dev_auto(self, noutput_items, d_input_ptrs, d_angles_ptr, d_count_ptr, method="mdl", d_cov_ptr=None, d_eig_ptr=None,
                      d_status_ptr=None, stream=None) -> int:
        """work_dev with the source count estimated per snapshot (K = snapshot_size, at most num_targets sources): the angles
        stay num_targets wide, the first count slots filled and the rest NaN; counts (int32, required) and the eigenvalues
        (optional) come out of the same eigen launch; status 2 marks an item without a usable count
        (doa_root_pipeline_work_dev_auto)."""
        return check(lib.doa_root_pipeline_work_dev_auto(
            self._h, int(noutput_items), ptr_array(d_input_ptrs), _count_method(method), _opt_ptr(d_cov_ptr), _opt_ptr(d_angles_ptr),
            _opt_ptr(d_count_ptr), _opt_ptr(d_eig_ptr), _opt_ptr(d_status_ptr), _stream_ptr(stream)))

    def work_dev_batches(self, noutput_items, d_input_ptrs, d_cov_ptrs, d_angles_ptrs, d_status_ptrs=None, stream=None) -> int:
        return self.prepare_batches(noutput_items, d_input_ptrs, d_cov_ptrs, d_angles_ptrs, d_status_ptrs, stream)()

    def prepare_batches(self, noutput_items, d_input_ptrs, d_cov_ptrs, d_angles_ptrs, d_status_ptrs=None, stream=None):
        """The argument marshalling of work_dev_batches done once: returns a callable that makes the C call."""
        nb = len(d_angles_ptrs)
        args = (self._h, nb, int(noutput_items), self._flat_inputs(nb, d_input_ptrs), self._opt_ptrs(d_cov_ptrs),
                ptr_array(d_angles_ptrs), self._opt_ptrs(d_status_ptrs), _stream_ptr(stream))
        fn = lib.doa_root_pipeline_work_dev_batches
        return lambda: check(fn(*args))

    def work(self, noutput_items, input_items, angles_out, cov_out=None) -> int:
        """Host buffers in, host buffers out (numpy): input_items[k] = complex64 stream k starting at its first history
        sample; angles_out [>=n, M] float32; cov_out [>=n, N*N] complex64 is optional.  Raises DoaError(DOA_ERR_NUMERIC) when
        an item has no root inside the unit circle (the outputs of the other items are valid)."""
        n = int(noutput_items)
        arrs = self._host_streams(input_items, self.input_span(n))
        for o, dt, per in ((angles_out, _F32, self.num_targets), (cov_out, _C64, self.inputs ** 2)):
            if o is not None:
                assert o.dtype == dt and o.flags.c_contiguous and o.size >= n * per
        none = C.c_void_p(0)
        return check(lib.doa_root_pipeline_work(self._h, n, ptr_array([a.ctypes.data for a in arrs]),
                                                none if cov_out is None else _vp(cov_out), _vp(angles_out)))


root_music_pipeline = root_pipeline      # the name of the C++ shell (gr::doa::root_music_pipeline) and of grc/doa_root_music_pipeline.xml


class root_music_pipeline_sc16(root_pipeline):
    """root_music_pipeline on complex int16 streams (as music_pipeline_sc16).  Not a block of the reference."""

    def __init__(self, inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets,
                 scale=SC16_DEFAULT_SCALE, max_batch=4096):
        super().__init__(inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets, max_batch)
        self.set_input_format("sc16", scale)
        self.in_sig = [(_I16, 2)] * self.inputs


class compass_mean(_Block):
    """blocks.vector_to_streams(float, num_streams) + the averaging step of doa.compass
    (reference python/compass.py:134-136: next_angle = numpy.mean(input_items[0]) per work call),
    on the device.  The dial/LCD GUI of the compass is not reproduced."""

    _destroy = staticmethod(lib.doa_compass_mean_destroy)

    def __init__(self, num_streams):
        super().__init__()
        self.num_streams = int(num_streams)
        self._h = check_handle(lib.doa_compass_mean_create(self.num_streams), "compass_mean")
        self.next_angle = np.full(self.num_streams, np.nan, _F32)
        self.in_sig = [(_F32, self.num_streams)]
        self.out_sig = []

    def work(self, ninput_items, input_items, output_items=None) -> int:
        n = int(ninput_items)
        a = np.ascontiguousarray(input_items[0], dtype=_F32)
        assert a.size >= n * self.num_streams
        return check(lib.doa_compass_mean_work(self._h, n, _vp(a), _vp(self.next_angle)))

    def work_dev(self, ninput_items, d_in_ptr, d_next_angle_ptr, stream=None) -> int:
        return check(lib.doa_compass_mean_work_dev(self._h, int(ninput_items), C.c_void_p(int(d_in_ptr or 0)),
                                                   C.c_void_p(int(d_next_angle_ptr)), _stream_ptr(stream)))


class twinrx_phase_offset_est(_StreamInput, _Block):
    """doa.twinrx_phase_offset_est(num_ports=2, n_skip_ahead=8192) -- the reference's hier block
    (python/twinrx_phase_offset_est.py:37-94): skiphead + complex_to_arg on every stream, then arg(x_0) - arg(x_p), unwrapped,
    as num_ports - 1 float streams (`work`, `work_dev`); and the same fused with the reductions of its savers, nothing
    materialised (`estimate`, `estimate_dev`: maximum, mean and circular mean of the first `samples` differences).  The
    block keeps the skiphead state over calls; `reset` starts over."""

    _destroy = staticmethod(lib.doa_phase_offset_est_destroy)
    _set_format = staticmethod(lib.doa_phase_offset_est_set_input_format)

    def __init__(self, num_ports=2, n_skip_ahead=8192):
        super().__init__()
        self.num_ports = self.inputs = int(num_ports)
        self.n_skip_ahead = int(n_skip_ahead)
        self._h = check_handle(lib.doa_phase_offset_est_create(self.num_ports, self.n_skip_ahead), "twinrx_phase_offset_est")
        self.in_sig = [(_C64, 1)] * self.num_ports
        self.out_sig = [(_F32, 1)] * (self.num_ports - 1)

    def reset(self) -> None:
        check(lib.doa_phase_offset_est_reset(self._h))

    def work(self, n_items, input_items, output_items) -> int:
        """input_items: num_ports streams of >= n_items samples; output_items: num_ports - 1 float32 arrays of >= n_items.
        Returns the floats written to each output (n_items less what the skip still took)."""
        n = int(n_items)
        arrs = self._host_streams(input_items, n)
        outs = list(output_items[:self.num_ports - 1])
        for o in outs:
            assert o.dtype == _F32 and o.flags.c_contiguous and o.size >= n
        return check(lib.doa_phase_offset_est_work(self._h, n, ptr_array([a.ctypes.data for a in arrs]),
                                                   ptr_array([o.ctypes.data for o in outs])))

    def work_dev(self, n_items, d_input_ptrs, d_output_ptrs, stream=None) -> int:
        return check(lib.doa_phase_offset_est_work_dev(self._h, int(n_items), ptr_array(d_input_ptrs),
                                                       ptr_array(d_output_ptrs), _stream_ptr(stream)))

    def estimate(self, n_items, input_items, samples, mean=True, max=True, circ=True):
        """The fused form on host streams: (mean, max, circ), float32 arrays of num_ports - 1 (None where not asked for)."""
        n = int(n_items)
        arrs = self._host_streams(input_items, n)
        outs = [np.empty(self.num_ports - 1, _F32) if want else None for want in (mean, max, circ)]
        check(lib.doa_phase_offset_est_estimate(self._h, n, ptr_array([a.ctypes.data for a in arrs]), int(samples),
                                                *[C.c_void_p(0) if o is None else _vp(o) for o in outs]))
        return tuple(outs)

    def estimate_dev(self, n_items, d_input_ptrs, samples, d_mean_ptr, d_max_ptr, d_circ_ptr, stream=None) -> None:
        """The fused form on device pointers; each of the three output pointers may be None / 0."""
        check(lib.doa_phase_offset_est_estimate_dev(
            self._h, int(n_items), ptr_array(d_input_ptrs), int(samples), C.c_void_p(int(d_mean_ptr or 0)),
            C.c_void_p(int(d_max_ptr or 0)), C.c_void_p(int(d_circ_ptr or 0)), _stream_ptr(stream)))


def write_phase_config(filename, values) -> None:
    """The phase file phase_correct_hier reads, one value per line (doa_write_phase_config).  ValueError with the
    reference's text when the file cannot be written."""
    v = np.ascontiguousarray(values, dtype=_F32).reshape(-1)
    if lib.doa_write_phase_config(str(filename).encode(), _vp(v), v.size) < 0:
        raise ValueError(_lib.last_error())


def write_antenna_calib(filename, gains, phases) -> None:
    """The antenna file antenna_correction reads, "gain phase" per line (doa_write_antenna_calib)."""
    g = np.ascontiguousarray(gains, dtype=_F32).reshape(-1)
    p = np.ascontiguousarray(phases, dtype=_F32).reshape(-1)
    if g.size != p.size:
        raise ValueError("gains and phases differ in length")
    if lib.doa_write_antenna_calib(str(filename).encode(), _vp(g), _vp(p), g.size) < 0:
        raise ValueError(_lib.last_error())


def calib_mean(mag_items, phase_items, num_inputs):
    """(gain, phase): the per-component means of two inputs of vlen-num_inputs float items, on the device
    (doa_calib_mean_work; the reduction of save_antenna_calib)."""
    N = int(num_inputs)
    m = np.ascontiguousarray(mag_items, dtype=_F32).reshape(-1, N)
    p = np.ascontiguousarray(phase_items, dtype=_F32).reshape(-1, N)
    if m.shape != p.shape:
        raise ValueError("magnitude and phase inputs differ in length")
    g, ph = np.empty(N, _F32), np.empty(N, _F32)
    check(lib.doa_calib_mean_work(m.shape[0], N, _vp(m), _vp(p), _vp(g), _vp(ph)))
    return g, ph


def calib_mean_complex(c_items, num_inputs):
    """(gain, phase) from calibrate_lin_array's complex output items: |c| and atan2f(im, re) per element
    (complex_to_magphase), then the means, on the device (doa_calib_mean_complex_work)."""
    N = int(num_inputs)
    c = np.ascontiguousarray(c_items, dtype=_C64).reshape(-1, N)
    g, ph = np.empty(N, _F32), np.empty(N, _F32)
    check(lib.doa_calib_mean_complex_work(c.shape[0], N, _vp(c), _vp(g), _vp(ph)))
    return g, ph


def calib_mean_dev(n_items, num_inputs, d_mag_ptr, d_phase_ptr, d_gain_ptr, d_phase_out_ptr, stream=None) -> int:
    return check(lib.doa_calib_mean_work_dev(int(n_items), int(num_inputs), C.c_void_p(int(d_mag_ptr)), C.c_void_p(int(d_phase_ptr)),
                                             C.c_void_p(int(d_gain_ptr)), C.c_void_p(int(d_phase_out_ptr)), _stream_ptr(stream)))


def calib_mean_complex_dev(n_items, num_inputs, d_c_ptr, d_gain_ptr, d_phase_out_ptr, stream=None) -> int:
    return check(lib.doa_calib_mean_complex_work_dev(int(n_items), int(num_inputs), C.c_void_p(int(d_c_ptr)),
                                                     C.c_void_p(int(d_gain_ptr)), C.c_void_p(int(d_phase_out_ptr)),
                                                     _stream_ptr(stream)))


class _PhaseSaver:
    """What findmax_and_save and average_and_save share: a sink of num_inputs float streams that reduces the first
    `samples` of each to one number, writes them to config_filename (one per line) and returns -1, which ends the
    reference's flowgraph.  The constructor truncates the file; where the reference writes "Configuration <name>, not
    writable" and exits, this raises ValueError with that text."""

    _which = None                         # index into twinrx_phase_offset_est.estimate's (mean, max, circ)
    _reduce = None

    def __init__(self, samples, num_inputs, config_filename):
        self.samples, self.num_inputs, self.config_filename = int(samples), int(num_inputs), config_filename
        write_phase_config(config_filename, [])
        self.in_sig = [(_F32, 1)] * self.num_inputs
        self.out_sig = []
        self.values = None                # what the last call wrote

    def output_multiple(self) -> int:
        return self.samples               # set_output_multiple(samples) of the reference

    def work(self, input_items, output_items=None) -> int:
        """input_items: num_inputs host float arrays, as the reference's work takes them (numpy, no device)."""
        vals = [type(self)._reduce(np.asarray(input_items[i], dtype=_F32)[:self.samples]) for i in range(self.num_inputs)]
        return self._save(vals)

    def from_estimator(self, est, n_items, input_items, which=None) -> int:
        """The fused form: `est` (a twinrx_phase_offset_est with num_inputs + 1 ports) reduces its host input streams on
        the device in one pass, no float stream in between; which = "circ" writes the circular mean instead of this
        block's own statistic."""
        if est.num_ports != self.num_inputs + 1:
            raise ValueError(f"estimator has {est.num_ports} ports, this sink {self.num_inputs} inputs")
        idx = 2 if which == "circ" else type(self)._which
        want = [i == idx for i in range(3)]
        return self._save(est.estimate(n_items, input_items, self.samples, *want)[idx])

    def from_estimator_dev(self, est, n_items, d_input_ptrs, which=None, stream=None) -> int:
        """from_estimator on device-resident streams (pointers); the num_inputs results come back through a torch tensor."""
        import torch
        if est.num_ports != self.num_inputs + 1:
            raise ValueError(f"estimator has {est.num_ports} ports, this sink {self.num_inputs} inputs")
        idx = 2 if which == "circ" else type(self)._which
        res = torch.empty(self.num_inputs, dtype=torch.float32, device="cuda")
        ptrs = [res.data_ptr() if i == idx else 0 for i in range(3)]
        stream = torch.cuda.current_stream() if stream is None else stream
        est.estimate_dev(n_items, d_input_ptrs, self.samples, *ptrs, stream=stream)
        if hasattr(stream, "synchronize"):
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        return self._save(res.cpu().numpy())

    def _save(self, vals) -> int:
        self.values = np.asarray(vals, dtype=_F32).reshape(self.num_inputs)
        write_phase_config(self.config_filename, self.values)
        return -1


class findmax_and_save(_PhaseSaver):
    """doa.findmax_and_save(samples_to_findmax, num_inputs, config_filename) -- reference python/findmax_and_save.py:36-78:
    numpy.amax of the first samples_to_findmax floats of each input."""

    _which = 1
    _reduce = staticmethod(np.amax)

    def __init__(self, samples_to_findmax, num_inputs, config_filename):
        super().__init__(samples_to_findmax, num_inputs, config_filename)
        self.samples_to_findmax = self.samples


class average_and_save(_PhaseSaver):
    """doa.average_and_save(samples_to_average, num_inputs, config_filename) -- reference python/average_and_save.py:35-80:
    numpy.mean of the first samples_to_average floats of each input (meaningless when the differences straddle +-pi:
    reproduced, not repaired)."""

    _which = 0
    _reduce = staticmethod(np.mean)

    def __init__(self, samples_to_average, num_inputs, config_filename):
        super().__init__(samples_to_average, num_inputs, config_filename)
        self.samples_to_average = self.samples


class save_antenna_calib:
    """doa.save_antenna_calib(num_inputs, config_filename="", samples_to_average=1024) -- reference
    python/save_antenna_calib.py:30-75: two inputs of vlen-num_inputs float items (magnitude, phase); per component the mean
    over ALL items of the call (samples_to_average only sets the output multiple), written as "gain phase" per line.
    Raises ValueError("Configuration <name>, not valid") where the reference exits."""

    def __init__(self, num_inputs, config_filename="", samples_to_average=1024):
        self.num_inputs, self.config_filename = int(num_inputs), config_filename
        self.samples_to_average = int(samples_to_average)
        write_antenna_calib(config_filename, [], [])
        self.in_sig = [(_F32, self.num_inputs)] * 2
        self.out_sig = []
        self.gains = self.phases = None   # what the last call wrote

    def output_multiple(self) -> int:
        return self.samples_to_average

    def work(self, input_items, output_items=None) -> int:
        """input_items = [magnitude items, phase items], host float arrays [n, num_inputs], as the reference's work takes
        them (numpy.mean per component, no device)."""
        g = np.asarray(input_items[0], dtype=_F32).reshape(-1, self.num_inputs)
        p = np.asarray(input_items[1], dtype=_F32).reshape(-1, self.num_inputs)
        return self._save([np.mean(g[:, i]) for i in range(self.num_inputs)], [np.mean(p[:, i]) for i in range(self.num_inputs)])

    def from_calibration(self, c_items) -> int:
        """The fused form on calibrate_lin_array's complex output items (host array [n, num_inputs]): magnitude, phase and
        the means in one device kernel."""
        return self._save(*calib_mean_complex(c_items, self.num_inputs))

    def from_calibration_dev(self, n_items, d_c_ptr, stream=None) -> int:
        """from_calibration on a device pointer (calibrate_lin_array.work_dev's output); the 2 num_inputs results come back
        through a torch tensor."""
        import torch
        res = torch.empty(2 * self.num_inputs, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream() if stream is None else stream
        calib_mean_complex_dev(n_items, self.num_inputs, d_c_ptr, res.data_ptr(), res.data_ptr() + 4 * self.num_inputs, stream)
        if hasattr(stream, "synchronize"):
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        r = res.cpu().numpy()
        return self._save(r[:self.num_inputs], r[self.num_inputs:])

    def _save(self, gains, phases) -> int:
        self.gains = np.asarray(gains, dtype=_F32).reshape(self.num_inputs)
        self.phases = np.asarray(phases, dtype=_F32).reshape(self.num_inputs)
        write_antenna_calib(self.config_filename, self.gains, self.phases)
        return -1


class sim_source(_Block):
    """The signal front end of apps/run_MUSIC_lin_array_simulation.py (:66-74, :204-210) as one
    device-side generator: tones + per-source Gaussian noise through the array manifold, plus
    optional per-antenna noise.  tone_freq in cycles/sample."""

    _destroy = staticmethod(lib.doa_sim_source_destroy)

    def __init__(self, num_ant_ele, norm_spacing, theta_deg, tone_freq, tone_ampl=None, source_noise_ampl=None,
                 antenna_noise_sigma=0.0, seed=0):
        super().__init__()
        th = np.ascontiguousarray(np.atleast_1d(theta_deg), dtype=_F32)
        fr = np.ascontiguousarray(np.atleast_1d(tone_freq), dtype=np.float64)
        M = th.shape[0]
        if fr.shape[0] != M:
            raise ValueError("tone_freq and theta_deg differ in length")
        opt = []
        for v in (tone_ampl, source_noise_ampl):
            if v is None:
                opt.append(None)
            else:
                v = np.ascontiguousarray(np.atleast_1d(v), dtype=_F32)
                if v.shape[0] != M:
                    raise ValueError("per-source arrays differ in length")
                opt.append(v)
        self.num_ant_ele, self.num_sources = int(num_ant_ele), int(M)
        none = C.c_void_p(0)
        self._h = check_handle(lib.doa_sim_source_create(
            self.num_ant_ele, self.num_sources, float(norm_spacing), _vp(th), _vp(fr),
            none if opt[0] is None else _vp(opt[0]), none if opt[1] is None else _vp(opt[1]),
            float(antenna_noise_sigma), int(seed) & 0xFFFFFFFFFFFFFFFF), "sim_source")

    def seek(self, sample_index) -> None:
        check(lib.doa_sim_source_seek(self._h, int(sample_index)))

    def tell(self) -> int:
        return int(lib.doa_sim_source_tell(self._h))

    def work(self, noutput_items, output_items) -> int:
        n = int(noutput_items)
        for o in output_items[:self.num_ant_ele]:
            assert o.dtype == _C64 and o.flags.c_contiguous and o.size >= n
        return check(lib.doa_sim_source_work(self._h, n, ptr_array([o.ctypes.data for o in output_items[:self.num_ant_ele]])))

    def work_dev(self, noutput_items, d_output_ptrs, stream=None) -> int:
        return check(lib.doa_sim_source_work_dev(self._h, int(noutput_items), ptr_array(d_output_ptrs), _stream_ptr(stream)))


def set_internal_precision(bits: int) -> None:
    check(lib.doa_set_internal_precision(int(bits)))


def get_internal_precision() -> int:
    return int(lib.doa_get_internal_precision())


def device_count() -> int:
    return int(lib.doa_hip_device_count())


def evd_fallback_count(reset: bool = False) -> int:
    """Diagnostics: items whose eigendecomposition left the signal-subspace fast path for the Jacobi fall-back."""
    return int(lib.doa_hip_evd_fallback_count(1 if reset else 0))
