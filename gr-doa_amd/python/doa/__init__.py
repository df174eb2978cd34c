"""`doa` — the hot-path slice of the reference's Python namespace (python/__init__.py:26-41,
swig/doa_swig.i:22-34), backed by hand-written gfx950 HIP kernels behind a C ABI.

    import doa
    blk = doa.autocorrelate(inputs, snapshot_size, overlap_size, avg_method)
    blk = doa.MUSIC_lin_array(norm_spacing, num_targets, inputs, pspectrum_len)
    blk = doa.find_local_max(num_max_vals, vector_len, x_min, x_max)
    blk = doa.rootMUSIC_linear_array(norm_spacing, num_targets, inputs)

plus, beyond the reference, the number of sources estimated per covariance item (MDL / AIC) for the `*_counts` / `*_auto` entries:

    blk = doa.source_count(num_ant_ele, num_snapshots, method="mdl", max_sources=None)

spatial smoothing of the covariance items for coherent sources (also `music_pipeline.set_spatial_smoothing`):

    blk = doa.spatial_smooth(num_ant_ele, subarray_size, forward_backward=True)

the Capon (MVDR) spectrum, which needs no source count and no eigendecomposition (also `music_pipeline.set_estimator("capon")`):

    blk = doa.capon_lin_array(norm_spacing, inputs, pspectrum_len, diagonal_loading=0.0)

the iterative adaptive (IAA) power spectrum, for single snapshots, for coherent sources at the full aperture and for source
powers: a dB row like the others and, on a second port, the power per direction in the units of the covariance item:

    blk = doa.iaa_lin_array(norm_spacing, inputs, pspectrum_len, diagonal_loading=0.0, iterations=10)

one covariance per snapshot and frequency bin, for several narrowband emitters at different frequencies in one band:

    blk = doa.channel_covariance(inputs, snapshot_size, overlap_size, fft_len, window="hann")

one spectrum per snapshot from all those bins, each at its own spacing in wavelengths, for a wideband emitter:

    blk = doa.wideband_music(norm_spacing, num_targets, inputs, pspectrum_len, fft_len, rate_over_carrier=fs / fc)

or one focused covariance per snapshot from all those bins (coherent focusing), for a wideband emitter with echoes and for
Root-MUSIC, ESPRIT, Capon and the source count on wideband data:

    blk = doa.focus_covariance.for_ula(norm_spacing, inputs, fft_len, focus_angles, rate_over_carrier=fs / fc)

the difference co-array of a sparse linear array (minimum-redundancy, nested, coprime), for more sources than antennas: the
covariance item of a virtual uniform array for MUSIC_lin_array, rootMUSIC_linear_array and esprit_linear_array:

    blk = doa.coarray_covariance((0, 1, 4, 6))            # 4 antennas -> blk.virtual_size == 7: up to 6 sources

least-squares ESPRIT, the grid-free estimate without a polynomial or a search (also `root_pipeline.set_estimator("esprit")`):

    blk = doa.esprit_linear_array(norm_spacing, num_targets, inputs)

the two spectra for an arbitrary array geometry (a uniform circular array, a measured manifold), given as a steering table
(also `music_pipeline.set_steering_table`):

    table = doa.planar_steering_table(doa.uca_positions(5, 0.425), 720)      # [720, 5] complex128, azimuth 0..360
    blk = doa.MUSIC_array(num_targets, table)
    blk = doa.capon_array(table, diagonal_loading=0.0)

directions as (azimuth, elevation) pairs: the table of an azimuth x elevation grid and the two-dimensional peak pick, which
can wrap around 360 degrees:

    table = doa.planar_steering_grid(doa.uca_positions(8, 0.6), 72, 18)      # [72 * 18, 8], azimuth 0..360, elevation 0..90
    blk = doa.find_local_max_2d(num_max_vals, 72, 18, 0.0, 360.0, 0.0, 90.0, wrap_az=True)

and the calibration chain that produces the files phase_correct_hier and antenna_correction read
(python/twinrx_phase_offset_est.py, findmax_and_save.py, average_and_save.py, save_antenna_calib.py):

    est = doa.twinrx_phase_offset_est(num_ports, n_skip_ahead)
    snk = doa.findmax_and_save(samples_to_findmax, num_inputs, config_filename)

Importing fails if gr-doa_amd/lib/libdoa_hip.so has not been built; constructing a block fails if
no HIP device is usable.  There is no CPU fallback.
"""
from ._lib import DoaError, LIB_PATH, last_error  # noqa: F401
from .blocks import (autocorrelate, channel_covariance, wideband_music, wideband_bin_spacing, focus_covariance, rss_focusing_matrices, coarray_covariance, coarray_lags, antenna_correction, phase_correct_hier, read_phase_config, calibrate_lin_array, MUSIC_lin_array, find_local_max, source_count, spatial_smooth, capon_lin_array, iaa_lin_array, rootMUSIC_linear_array,  # noqa: F401
                     esprit_linear_array,
                     MUSIC_array, capon_array, planar_steering_table, uca_positions, planar_steering_grid, find_local_max_2d, array_grid_debug,
                     music_pipeline, root_pipeline, root_music_pipeline, autocorrelate_sc16, music_pipeline_sc16,
                     root_music_pipeline_sc16, compass_mean, sim_source, set_internal_precision, get_internal_precision, device_count,
                     evd_fallback_count, DETACHED,
                     twinrx_phase_offset_est, findmax_and_save, average_and_save, save_antenna_calib, write_phase_config,
                     write_antenna_calib, calib_mean, calib_mean_complex, calib_mean_dev, calib_mean_complex_dev)
from . import runtime, sim, sharding, distributed, launch  # noqa: F401
