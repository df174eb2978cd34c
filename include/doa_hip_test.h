/*
 * doa_hip_test.h -- entry points of libdoa_hip.so that exist for the TEST SUITE and for profiling, not for applications:
 * diagnostics of intermediate results (what the parity tests compare against the oracle), a stage mask for timing one
 * kernel of the pipeline on valid intermediates, and fault injection for the error paths.  Same library, same symbols as
 * before round 4; kept out of doa_hip.h so that the drop-in boundary declares only what a gr-doa block shell binds.
 */
#ifndef DOA_HIP_TEST_H
#define DOA_HIP_TEST_H

#include "doa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics used by the parity tests (host buffers, synchronous): the noise-subspace projector
 * U_N U_N^H of each item (column-major num_ant_ele^2 gr_complex, lib/MUSIC_lin_array_impl.cc:133)
 * and the un-normalised null spectrum Q_i = Re(a_i^H P_N a_i) (:139), pspectrum_len floats per
 * item.  Either output pointer may be NULL. */
DOA_HIP_API int doa_MUSIC_lin_array_debug(doa_MUSIC_lin_array_t *h, int noutput_items,
                                          const void *input_items0, void *projector_out,
                                          void *null_spectrum_out);

/* Diagnostics for parity tests (as doa_MUSIC_lin_array_debug): besides the angles, the 2*num_ant_ele-2 polynomial
 * roots the solver found per item (roots_out: interleaved re, im doubles; may be NULL) and the per-item status
 * (status_out: 1 = no root strictly inside the unit circle, the case in which the reference raises inside
 * arma::index_min and doa_..._work returns DOA_ERR_NUMERIC; may be NULL).  Always returns noutput_items on success. */
DOA_HIP_API int doa_rootMUSIC_linear_array_debug(doa_rootMUSIC_linear_array_t *h, int noutput_items,
                                                 const void *input_items0, void *output_items0,
                                                 void *roots_out, int *status_out);
/* Diagnostics, second half: ONLY the root-selection stage of work() (lib/rootMUSIC_linear_array_impl.cc:122-145), run
 * on the device -- the very code the solver kernel ends in -- on CALLER-SUPPLIED roots (roots_in: noutput_items x
 * (2*num_ant_ele-2) interleaved re, im doubles, host memory), so that every branch of the rule can be driven with
 * hand-made root lists: fewer than num_targets roots strictly inside the unit circle (missing slots read 90 degrees,
 * :131-141), roots exactly on the circle (excluded by dist > 0, :125), equal distances (index_min takes the first),
 * no interior root at all (status 1 / NaN angles; the reference raises).  PARITY UNPINNED in two corners, both stated
 * in DESIGN.md section 5: the reference tests a FLOAT dist = 1 - |z| of cgeev's float roots, here dist is formed in double from
 * double roots (a root within 6e-8 of the circle is dropped there and kept here); NaN angles (|arg z| > 2 pi d) sort
 * last here, arma::sort's treatment of NaN depends on the Armadillo version. */
DOA_HIP_API int doa_rootMUSIC_linear_array_select_debug(doa_rootMUSIC_linear_array_t *h, int noutput_items,
                                                        const void *roots_in, void *output_items0,
                                                        int *status_out);

/* The counted selection stage on caller-supplied roots, the counterpart of select_debug for
 * doa_rootMUSIC_linear_array_work_counts: counts = one int32 per item (host memory), output items num_targets floats wide,
 * status_out (may be NULL) 0 / 1 / 2 as that entry defines them.  An item with count m is bit-identical to the select_debug
 * row of a num_targets = m handle on the same roots; the roots of an item with count 0 or no usable count are not read. */
DOA_HIP_API int doa_rootMUSIC_linear_array_select_counts_debug(doa_rootMUSIC_linear_array_t *h, int noutput_items,
                                                               const void *roots_in, const void *counts,
                                                               void *output_items0, int *status_out);

/* Diagnostics of capon_lin_array (host buffers, synchronous): the inverse W of each item (inverse_out: column-major
 * num_ant_ele^2 gr_complex; NaN for a status-1 item) and the un-normalised null spectrum Q_i = a_i^H W a_i
 * (null_spectrum_out: pspectrum_len floats per item).  Either output pointer may be NULL. */
DOA_HIP_API int doa_capon_lin_array_debug(doa_capon_lin_array_t *h, int noutput_items, const void *cov_items,
                                          void *inverse_out, void *null_spectrum_out);

/* Diagnostics of iaa_lin_array (host buffers, synchronous): per item the final p_k in double (power_out: pspectrum_len doubles,
 * before the scaling by mu) and the lags r_l of the last iteration's R (lags_out: num_ant_ele (re, im) pairs of doubles); both
 * NaN for a status-1 item.  Either output pointer may be NULL. */
DOA_HIP_API int doa_iaa_lin_array_debug(doa_iaa_lin_array_t *h, int noutput_items, const void *cov_items, void *power_out,
                                        void *lags_out);

/* Diagnostics of MUSIC_array and capon_array (host buffers, synchronous): per item the matrix X the scan read (projector_out /
 * inverse_out: N x N complex128, column-major, unpacked from the double full record; NaN for a status-1 Capon item) and
 * the un-normalised null spectrum Q_i = Re(a_i^H X a_i) (null_spectrum_out: pspectrum_len floats).  Either output pointer may
 * be NULL. */
DOA_HIP_API int doa_MUSIC_array_debug(doa_MUSIC_array_t *h, int noutput_items, const void *cov_items, void *projector_out,
                                      void *null_spectrum_out);
DOA_HIP_API int doa_capon_array_debug(doa_capon_array_t *h, int noutput_items, const void *cov_items, void *inverse_out,
                                      void *null_spectrum_out);

/* The steering-table scan that ends in the two-dimensional peak pick (what music_pipeline's grid mode launches), on
 * CALLER-SUPPLIED full records: no handle, host buffers, synchronous.  steering: n_az * n_el rows of num_ant_ele complex
 * doubles; the grid, the limits, wrap_az and num_max_vals as doa_find_local_max_2d_create takes them; records: n_items x
 * num_ant_ele^2 doubles, the full-record packing ([r + r N] = X[r][r]; r < c: [r + c N] = Re X[r][c], [c + r N] = Im X[r][c]).
 * fused = 1 runs the one launch, fused = 0 the two launches it replaces (the scan of MUSIC_array / capon_array, then
 * find_local_max_2d's kernel) on the same records: the outputs must agree bit for bit.  spectrum_out (n_items x n_az n_el
 * floats) may be NULL, and the fused launch then stores no row; val_out, az_out, el_out: n_items x num_max_vals floats each.
 * Every argument is validated before the device is touched.  Returns n_items, or DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_hip_array_grid_debug(int num_ant_ele, const double *steering, int n_az, int n_el, float az_min, float az_max,
                                         float el_min, float el_max, int wrap_az, int num_max_vals, int n_items,
                                         const double *records, int fused, float *spectrum_out, float *val_out, float *az_out,
                                         float *el_out);

/* Diagnostics of esprit_linear_array (host buffers, synchronous): ONLY esprit_kernel, the very launch the work entries end
 * in, on CALLER-SUPPLIED signal-subspace records in place of the eigen stage's (records: noutput_items x 2 num_ant_ele^2
 * doubles, [2 (k N + row)] = Re, [.. + 1] = Im of entry `row` of column k; the kernel reads the first m columns of an item
 * with count m and no others), so that the eigenvalue solver can be driven with subspaces no covariance item produces on
 * purpose: non-normal Psi, gamma at its threshold, components outside the visible region.  cov_items supplies only what
 * the kernel takes from the item itself, the trace and finiteness test of status 1.  counts (int32 per item) may be NULL:
 * every item takes num_targets columns.  angles_out: num_targets floats per item; status_out (may be NULL): 0 / 1 / 2 / 3 as
 * doa_esprit_linear_array_work_counts defines them.  Returns noutput_items on success. */
DOA_HIP_API int doa_esprit_linear_array_record_debug(doa_esprit_linear_array_t *h, int noutput_items, const void *cov_items,
                                                     const void *records, const void *counts, void *angles_out,
                                                     int *status_out);

/* Profiling aid: which stages later work_dev calls on this handle launch (bit 0 = K1 covariance, bit 1 = K2+K3
 * EVD, bit 2 = K4+K5 scan + peak pick; default 7).  A dropped stage leaves its outputs as the previous call
 * wrote them, so a profiler can time one kernel on valid intermediates; not for production use. */
DOA_HIP_API int doa_music_pipeline_set_stages(doa_music_pipeline_t *h, int stage_mask);
/* Test aids for the error paths of doa_music_pipeline_work and doa_music_pipeline_work_dev_batches (not for production
 * use).  inject_failure: the NEXT such call on this handle behaves as if a HIP call had failed in chunk `chunk_index` (0 =
 * the first ~32 MiB chunk, or the only one of a scheduler-sized call) after that chunk's uploads were enqueued -- for the
 * batches entry: before batch `chunk_index` is launched, the earlier ones already running on their lanes; one-shot, -1
 * disarms.  Whatever fails inside either call, it returns only after every lane it used has been synchronised (the
 * detached form included), so nothing of a failed call is still running or copying afterwards; lanes_idle reports exactly
 * that (1 = all lanes idle, 0 = work pending, < 0 = error). */
DOA_HIP_API int doa_music_pipeline_inject_failure(doa_music_pipeline_t *h, int chunk_index);
DOA_HIP_API int doa_music_pipeline_lanes_idle(doa_music_pipeline_t *h);

/* The same two test aids for root_pipeline. */
DOA_HIP_API int doa_root_pipeline_inject_failure(doa_root_pipeline_t *h, int chunk_index);
DOA_HIP_API int doa_root_pipeline_lanes_idle(doa_root_pipeline_t *h);

/* The device (HIP ordinal) that holds the fall-back counter a K2+K3 launch made NOW -- with the calling thread's current
 * device -- would add into, or -1 when there is none.  The counters are per device since round 4 (a kernel must never add
 * into another device's memory); the test creates a handle, binds its device and checks that this equals it. */
DOA_HIP_API int doa_hip_evd_fallback_counter_device_debug(void);

/* The lane streams of the pipeline handles are probed when they are created (gr-doa_amd/csrc/lane_streams.hip): how many
 * lanes of the set created LAST in this process were seen to run their kernels side by side (-1: none created yet, or the
 * probing is switched off with DOA_HIP_NO_LANE_PROBE), and how many candidate streams were set aside on the way because they
 * shared a hardware queue with an accepted lane. */
DOA_HIP_API int doa_hip_lane_streams_verified_debug(void);
DOA_HIP_API int doa_hip_lane_streams_set_aside_debug(void);

/* The plan of a doa_*_pipeline_work_dev_batches call (gr-doa_amd/csrc/batch_plan.hpp; doa_hip.h, GROUPS and ORDER) on flat
 * host arrays: no handle, no device.  Per batch b: outputs[4 b .. 4 b + 3] its output pointers (values only, never
 * dereferenced; NULL = absent), flags[b] (bit 0 lean: the batch may share a group's launches, bit 1 store: it wants its
 * spectrum, bit 2 vec2: its K1 takes the pair-load route), caps[b] >= 1 (how many batches a group that starts with b may
 * hold).  n_lanes (1 .. 8) and rotation_in (0 .. n_lanes - 1): the lanes of the call and where their rotation stands.
 * Written per batch: the index of its group, the group's lane, and whether the group joins all lanes on the host before it
 * is launched (sync_first_out, 0 / 1); *rotation_out: where the rotation stands afterwards.  Returns the number of groups,
 * or DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_hip_batch_plan_debug(int n_batches, const void *const *outputs, const unsigned char *flags, const int *caps,
                                         int n_lanes, int rotation_in, int *group_out, int *lane_out, int *sync_first_out,
                                         int *rotation_out);

/* The records a spectrum estimator keeps between its stage in front (eigen stage or Capon inverse) and its scan
 * (gr-doa_amd/csrc/spectrum_chain.hpp: spectrum_plan), as the four spectrum blocks and music_pipeline size them: no handle, no
 * device.  estimator: DOA_ESTIMATOR_MUSIC / _CAPON; steering_table: 0 = uniform linear array, 1 = a steering table; bits: the
 * internal precision; counted: 1 = a source count per item.  bytes_out[0..4], bytes per item, 0 = the record does not exist:
 * coefficient record, Chebyshev record, full record, status word, and the coefficient SLOT (sized as doubles whatever bits
 * is).  Returns DOA_OK, DOA_ERR_UNSUPPORTED for a combination no entry runs (bytes_out all 0), or DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_hip_spectrum_plan_debug(int estimator, int steering_table, int num_ant_ele, int bits, int counted,
                                            long long *bytes_out);

/* The records a grid-free estimator keeps between its eigen launch and its solver kernel (gr-doa_amd/csrc/gridfree_chain.hpp:
 * gridfree_plan), as rootMUSIC_linear_array, esprit_linear_array and root_pipeline size them: no handle, no device.
 * estimator: DOA_GRIDFREE_ROOT_MUSIC / _ESPRIT; bits: the internal precision; counted: 1 = a source count per item.
 * bytes_out[0..2], bytes per item, 0 = the record does not exist: coefficient record (doubles whatever bits is),
 * signal-subspace record, status word.  Returns DOA_OK, DOA_ERR_UNSUPPORTED for a combination no entry runs (bytes_out all
 * 0), or DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_hip_gridfree_plan_debug(int estimator, int num_ant_ele, int bits, int counted, long long bytes_out[3]);

/* Which kernels a shape launches, and with which grids (gr-doa_amd/csrc/launch_routes.hpp: cov_route, evd_route, scan_route): no
 * handle, no device; cu_count is the device's compute-unit count as the launchers would pass it.  stage 0 = K1 (covariance), 1 =
 * K2+K3 (eigen stage), 2 = K4 (scan of a uniform linear array).  shape, n_shape values, 0 / 1 where a flag:
 *   stage 0 (9):  inputs, snapshot_size, overlap_size, avg_method, noutput_items, sample format, every stream aligned to two
 *                 samples, a piece-sum workspace was supplied, a group of batches (noutput_items = the group's total)
 *   stage 1 (8):  num_ant_ele, num_targets, internal precision, items, mode (0 fixed source count, 1 a count per item, 2 the
 *                 signal-subspace record only, 3 the full record, 4 calibrate, 5 a group of batches), projector wanted (mode
 *                 0), Chebyshev record wanted (mode 1), signal-subspace record wanted (mode 1)
 *   stage 2 (11): num_ant_ele, internal precision, pspectrum_len, items, spectrum pointer 16-byte aligned, null spectrum wanted,
 *                 fused peak pick wanted, its num_max_vals, spectrum stored, Chebyshev record supplied, a group of batches
 * text_out (text_cap bytes): one line per launch in launch order, "kernel<template,arguments> grid block lanes work strides":
 * the kernel's name without namespace or blanks, workgroups, threads per workgroup, lanes per work item, work items of the
 * launch, 1 if the kernel strides over them by its grid; then one "key value" line per further fact of the route
 * (workspace_bytes; counts_fallbacks; reads_cheb, picked).  Returns the number of launches; a shape the route refuses returns
 * the launcher's status with its error text set; DOA_ERR_INVALID_ARG for bad arguments of this entry. */
DOA_HIP_API int doa_hip_launch_route_debug(int stage, const int *shape, int n_shape, int cu_count, char *text_out, int text_cap);

/* One primitive of gr-doa_amd/csrc/wave_ops.hpp (the moves and reductions between the lanes of a wave) applied by ONE workgroup
 * of 256 threads -- four waves -- to host data: thread t starts from in[t] and out[t] is what it holds afterwards (256 elements
 * of the op's type; wave_argbest's element is a (float value, int32 index) pair).  n = the number of input elements: 256, and 512
 * for the DPP move, whose `old` operand of thread t is in[256 + t].  op:
 *   0           wave_index() (int32; the input is not read)
 *   10 + g      group_sum<G, double>, G = 4, 8, 16 for g = 0, 1, 2;  20 + g the same in float;  30 + g group_max<G, double>;
 *               40 + g group_or<G> (int32)
 *   51, 52, 53  quad_rot<1>, <2>, <3>;  54 quad_sum;  55 row_sum16 (double)
 *   60 .. 65    wave_allreduce_sum (float), wave_allreduce_sum (int32), wave_allreduce_max, wave_allreduce_min,
 *               wave_allreduce_min_int, wave_argbest
 *   70, 71      wave_butterfly_sum_fetch in float and double;  72 wave_butterfly_sum_xor (double);  73 wave_butterfly_nan_max
 *   1000 + 100 t + c   dpp<control, row mask, bank mask>(old, v) on int32, float, double for t = 0, 1, 2; full masks for c = 0 .. 3:
 *               the two quad swaps (i ^ 1, i ^ 2), row_shl:2, row_shr:2; c = 4: row_shr:2 with bank mask 0x1; c = 5: row_bcast:15
 *               with row mask 0xA; c = 6: row_bcast:31 with row mask 0xC; c = 7: the first quad swap with row mask 0x5 and bank
 *               mask 0x6; c = 10 + k: row_ror:k, k = 1 .. 15
 * Returns 256, or DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_hip_wave_ops_debug(int op, int n, const void *in, void *out);

#ifdef __cplusplus
}
#endif
#endif /* DOA_HIP_TEST_H */
