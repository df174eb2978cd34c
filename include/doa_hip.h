/*
 * doa_hip.h — C ABI of libdoa_hip.so, the MI355X (gfx950) implementation of gr-doa's hot path
 *
 *     autocorrelate -> MUSIC_lin_array (+ find_local_max)  /  rootMUSIC_linear_array
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Every block of the
 * reference that sits on the path gets one opaque handle type with
 *
 *     doa_X_create(<the reference's make() arguments>)   -> handle, or NULL + doa_last_error()
 *     doa_X_work(h, noutput_items, <host pointers laid out like the GNU Radio item buffers>)
 *     doa_X_work_dev(h, noutput_items, <device pointers, same layouts>, hipStream_t as void*)
 *     doa_X_destroy(h)
 *
 * `work` returns the number of items produced (what the reference's work()/general_work()
 * returns) or a negative doa_status on failure; it never falls back to a CPU path: if no HIP
 * device / kernel is usable the call fails and doa_last_error() says why.
 *
 * Reference interfaces replaced (paths relative to the gr-doa tree):
 *   doa_autocorrelate_*          include/doa/autocorrelate.h:56, lib/autocorrelate_impl.cc:47-118
 *   doa_MUSIC_lin_array_*        include/doa/MUSIC_lin_array.h:56, lib/MUSIC_lin_array_impl.cc:47-150
 *   doa_find_local_max_*         include/doa/find_local_max.h:56, lib/find_local_max_impl.cc:47-194
 *   doa_rootMUSIC_linear_array_* include/doa/rootMUSIC_linear_array.h:54,
 *                                lib/rootMUSIC_linear_array_impl.cc:46-152
 *   doa_music_pipeline_*         the three blocks as wired by apps/run_MUSIC_lin_array_simulation.grc
 *                                (autocorrelate -> MUSIC_lin_array -> find_local_max(M, P, 0, 180))
 *   doa_root_pipeline_*          the two blocks as wired by apps/run_RootMUSIC_lin_array_simulation.grc
 *                                (autocorrelate -> rootMUSIC_linear_array)
 *   doa_phase_offset_est_*       python/twinrx_phase_offset_est.py:37-94, fused with the reductions of
 *                                python/findmax_and_save.py:66-78 and python/average_and_save.py:68-80
 *   doa_calib_mean_*, doa_write_*  python/save_antenna_calib.py:30-75 and the two calibration file formats
 *
 * Threading: like GNU Radio's thread-per-block scheduler assumes, different handles may be used
 * from different threads concurrently; one handle must not be used from two threads at once.
 * Ownership: the caller owns every buffer it passes; the library owns its device tables, staging
 * buffers and (for the host-pointer entry points) one HIP stream per handle.
 * What the library does to the HOST PROCESS besides that: the first handle created on a device makes it create four
 * throw-away non-blocking HIP streams and run one 64-byte memset on each; they (and 64 bytes of device memory) stay alive for
 * the life of the process.  The HIP runtime maps streams onto its hardware queues lazily, and streams that caused a queue to be
 * created overlap kernels measurably worse than later ones (26 against 33 us per pipeline step); priming
 * the pool once makes every stream created afterwards -- the library's and the application's -- one of the good kind.
 * Set DOA_HIP_NO_QUEUE_PRIMING=1 in the environment to switch this off.
 * The pipeline handles also PROBE the lane streams they create (first doa_*_pipeline_work_dev_batches / chunked host call on
 * a handle): the runtime may put two streams on one hardware queue, where their kernels run one after the other (measured: a
 * 4-lane step at 44 instead of 37.5 us with one foreign stream alive), and nothing in the HIP API tells; so every new lane
 * and the lanes accepted before it run a one-wave kernel that sleeps 150 us and time-stamps itself, and a lane whose interval
 * does not overlap the others' is replaced (csrc/lane_streams.hip).  About a millisecond per handle, once;
 * DOA_HIP_NO_LANE_PROBE=1 switches it off.  Streams handed in with doa_*_pipeline_set_lane_streams are the caller's and
 * are taken as they are.
 * Diagnostics, profiling and fault-injection entry points used by the test suite are exported by the same library but
 * declared in doa_hip_test.h, not here: this header is the drop-in boundary only.
 */
#ifndef DOA_HIP_H
#define DOA_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define DOA_HIP_API __attribute__((visibility("default")))
#else
#define DOA_HIP_API
#endif

typedef enum doa_status {
    DOA_OK = 0,
    DOA_ERR_INVALID_ARG = -1, /* a constructor/work argument violates the block's contract        */
    DOA_ERR_NO_DEVICE = -2,   /* no HIP device (or the HIP runtime failed to initialise)         */
    DOA_ERR_HIP = -3,         /* a HIP runtime call or kernel launch failed                      */
    DOA_ERR_UNSUPPORTED = -4, /* valid for the reference, not built into this library (size caps) */
    DOA_ERR_NUMERIC = -5      /* the reference would raise here (e.g. no root inside the circle)  */
} doa_status;

/* Largest array the HIP kernels are instantiated for (the reference's flowgraphs use 4, its QA
 * tests 4/8/16). */
#define DOA_MAX_ANT_ELE 16
/* Largest num_max_vals / num_targets handled by the peak-pick kernel. */
#define DOA_MAX_PEAKS 16

/* Thread-local description of the last failure on the calling thread ("" if none). */
DOA_HIP_API const char *doa_last_error(void);
/* Library/ABI version, bumped when a signature changes. */
DOA_HIP_API int doa_hip_abi_version(void);
/* Number of visible HIP devices (0 if none / runtime unusable). Does not create a context. */
DOA_HIP_API int doa_hip_device_count(void);

/* Layout advice for the N input streams of autocorrelate / music_pipeline on the device (the N stream pointers of
 * gr::doa::autocorrelate's general_work, lib/autocorrelate_impl.cc:83-100, when they are device memory): the
 * recommended distance in bytes between the first samples of consecutive streams that hold `stream_bytes` bytes each.
 * Every wave of the covariance kernel reads the same sample range of all N streams at the same time; streams whose
 * addresses agree modulo 8 KiB meet in the same HBM channels (measured on MI355X: 5.86 TB/s for N = 4 streams
 * 32 MiB apart against 6.25 TB/s with the distance returned here, 5.0 against 5.8 TB/s at N = 8).  The value is a
 * multiple of 16 (streams stay 16-byte aligned) and at least stream_bytes; any layout is accepted by the kernels, this
 * one is what the library's own staging buffers use. */
DOA_HIP_API size_t doa_stream_stride_bytes(size_t stream_bytes);

/* Internal precision of the batched Hermitian eigendecomposition and of the null-spectrum
 * evaluation used by MUSIC / Root-MUSIC / pipeline handles created *after* the call:
 * 64 (default) = double Jacobi + double Horner scan, 32 = float for both.  Item formats stay
 * complex64 in / float32 out either way; Root-MUSIC always finds its roots in double.
 * 64 is the parity configuration: it is what the tests pin to the fp64 evaluation of the
 * reference's formulas.  32 is an opt-in, NON-parity mode: it shares the reference's single
 * precision but not its LAPACK rounding sequence, so at spectrum nulls (where float Q is
 * cancellation-dominated) it differs from the reference by as much as two correct fp32
 * implementations differ from each other; it is tested to a loose bound only.
 * Returns DOA_OK or DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_set_internal_precision(int bits);
DOA_HIP_API int doa_get_internal_precision(void);
/* The call above only sets the process-wide DEFAULT a handle copies when it is created (two threads that want handles of
 * different precisions would race on it); the precision is a property of the HANDLE and can be set on it directly, at
 * any time between two work calls: doa_X_set_internal_precision(h, 32 | 64) for the four handle types that run the
 * eigendecomposition (declared with their blocks below). */

/* ---------------------------------------------------------------------------------------------
 * autocorrelate — gr::doa::autocorrelate::make(inputs, snapshot_size, overlap_size, avg_method)
 *   (include/doa/autocorrelate.h:56).  gr::block with history overlap_size+1
 *   (lib/autocorrelate_impl.cc:57) and forecast nonoverlap*noutput (:75-80).
 * Item layouts: input_items[k] = stream k, gr_complex (float re, im), pointing at the first
 *   history sample exactly like general_work's input_items[k]; window i is the snapshot_size
 *   samples starting at input_items[k] + i*(snapshot_size-overlap_size) (:95-100).
 *   output = noutput_items column-major inputs x inputs gr_complex matrices (:103).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_autocorrelate doa_autocorrelate_t;

DOA_HIP_API doa_autocorrelate_t *doa_autocorrelate_create(int inputs, int snapshot_size,
                                                          int overlap_size, int avg_method);
DOA_HIP_API void doa_autocorrelate_destroy(doa_autocorrelate_t *h);
/* set_history() value the shell must apply: overlap_size + 1. */
DOA_HIP_API int doa_autocorrelate_history(const doa_autocorrelate_t *h);
/* forecast(): new input items required per stream for noutput_items outputs. */
DOA_HIP_API int doa_autocorrelate_forecast(const doa_autocorrelate_t *h, int noutput_items);
/* Samples per stream that must be readable behind input_items[k]:
 * (noutput_items-1)*(snapshot-overlap) + snapshot. */
DOA_HIP_API long long doa_autocorrelate_input_span(const doa_autocorrelate_t *h, int noutput_items);
/* general_work on host buffers; the shell then calls consume_each(forecast(noutput_items)). */
DOA_HIP_API int doa_autocorrelate_work(doa_autocorrelate_t *h, int noutput_items,
                                       const void *const *input_items, void *output_items0);
/* Same on device buffers: d_input_items is a HOST array of `inputs` DEVICE pointers. Asynchronous
 * on `hip_stream` (a hipStream_t, NULL = the default stream). */
DOA_HIP_API int doa_autocorrelate_work_dev(doa_autocorrelate_t *h, int noutput_items,
                                           const void *const *d_input_items, void *d_output_items0,
                                           void *hip_stream);

/* Input sample format of the streams (autocorrelate and the two pipelines; every entry of the handle: work, work_dev,
 * work_dev_batches).  The default is the reference's gr_complex; the setter takes effect from the next work call (work
 * already enqueued keeps what it was launched with) and may be called between any two calls.
 *   DOA_SAMPLE_FC32  gr_complex, two float32 (real first), 8 B per sample; scale must be 1.0f (fc32 is never rescaled).
 *                    Device streams must be 8-byte aligned; 16-byte aligned streams with an even snapshot-overlap take the
 *                    pair-load kernels (and, with overlap, the read-once path).
 *   DOA_SAMPLE_SC16  complex int16, two little-endian int16 (real first) -- std::complex<int16_t>, UHD's sc16, GRC's sc16
 *                    port type -- 4 B per sample, read by the covariance kernel as it is and widened in registers:
 *                        re = __fmul_rn((float)q_re, scale),  im = __fmul_rn((float)q_im, scale)
 *                    (one rounding per component, never contracted).  scale: finite, > 0; 1.0f/32768 maps full scale to
 *                    [-1, 1) exactly, a radio driver's own factor reproduces that driver's fc32 values.  Device streams
 *                    must be 4-byte aligned; 8-byte aligned streams with an even snapshot-overlap take the same routes as
 *                    16-byte aligned fc32 streams.  No fc32 copy of the streams is made anywhere.
 * Parity: on int16 streams q, every output (covariance, spectrum, peaks, angles, status) is BIT-IDENTICAL to the fc32
 * path's on the streams np.float32(q) * np.float32(scale): the kernels sum the same floats in the same order.
 * Returns DOA_OK, or DOA_ERR_INVALID_ARG (doa_last_error() says why) for an unknown format, a scale that is not finite or
 * not > 0, or DOA_SAMPLE_FC32 with a scale other than 1.0f; the handle keeps its previous format then. */
#define DOA_SAMPLE_FC32 0   /* gr_complex, 8 B/sample: the default and the reference's format */
#define DOA_SAMPLE_SC16 1   /* complex int16, 4 B/sample (real first) */
DOA_HIP_API int doa_autocorrelate_set_input_format(doa_autocorrelate_t *h, int format, float scale);

/* ---------------------------------------------------------------------------------------------
 * MUSIC_lin_array — gr::doa::MUSIC_lin_array::make(norm_spacing, num_targets, num_ant_ele,
 *   pspectrum_len) (include/doa/MUSIC_lin_array.h:56).  gr::sync_block.
 * Item layouts: input = column-major num_ant_ele^2 gr_complex (only the upper triangle is
 *   significant, as with LAPACK uplo='U'); output = pspectrum_len floats, dB normalised to the
 *   item's maximum (lib/MUSIC_lin_array_impl.cc:49-50,124-142).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_MUSIC_lin_array doa_MUSIC_lin_array_t;

DOA_HIP_API doa_MUSIC_lin_array_t *doa_MUSIC_lin_array_create(float norm_spacing, int num_targets,
                                                              int num_ant_ele, int pspectrum_len);
DOA_HIP_API void doa_MUSIC_lin_array_destroy(doa_MUSIC_lin_array_t *h);
DOA_HIP_API int doa_MUSIC_lin_array_work(doa_MUSIC_lin_array_t *h, int noutput_items,
                                         const void *input_items0, void *output_items0);
DOA_HIP_API int doa_MUSIC_lin_array_work_dev(doa_MUSIC_lin_array_t *h, int noutput_items,
                                             const void *d_input_items0, void *d_output_items0,
                                             void *hip_stream);
/* Diagnostics for tests: for 4 < num_ant_ele <= 16 and num_targets <= 4 (2 num_targets <= num_ant_ele), internal
 * precision 64, the noise projector of MUSIC / Root-MUSIC / music_pipeline handles is computed from the SIGNAL subspace
 * (shifted orthogonal iteration, every result checked by its residual and by a certificate that the subspace found is the
 * one of the num_targets largest eigenvalues), and an item that fails any check takes the full Jacobi
 * eigendecomposition instead.  This returns how many items took that fall-back since the last reset (process-wide, all
 * handles and all devices: one 64-bit device counter per device, each kernel adds into the counter of the device it runs on;
 * synchronises the devices), or -1 without a device. */
DOA_HIP_API long long doa_hip_evd_fallback_count(int reset);
/* Items processed so far — the counter the reference prints from its destructor
 * (lib/MUSIC_lin_array_impl.cc:92-95,146). */
DOA_HIP_API long long doa_MUSIC_lin_array_items_total(const doa_MUSIC_lin_array_t *h);
DOA_HIP_API int doa_MUSIC_lin_array_set_internal_precision(doa_MUSIC_lin_array_t *h, int bits);

/* ---------------------------------------------------------------------------------------------
 * find_local_max — gr::doa::find_local_max::make(num_max_vals, vector_len, x_min, x_max)
 *   (include/doa/find_local_max.h:56).  gr::sync_block with two outputs.
 * Item layouts: input = vector_len floats; output 0 = num_max_vals floats (peak values, descending
 *   value order); output 1 = num_max_vals floats (x-axis locations of those peaks, sorted
 *   descending on their own) (lib/find_local_max_impl.cc:49-50,186-188).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_find_local_max doa_find_local_max_t;

DOA_HIP_API doa_find_local_max_t *doa_find_local_max_create(int num_max_vals, int vector_len,
                                                            float x_min, float x_max);
DOA_HIP_API void doa_find_local_max_destroy(doa_find_local_max_t *h);
DOA_HIP_API int doa_find_local_max_work(doa_find_local_max_t *h, int noutput_items,
                                        const void *input_items0, void *output_items0,
                                        void *output_items1);
DOA_HIP_API int doa_find_local_max_work_dev(doa_find_local_max_t *h, int noutput_items,
                                            const void *d_input_items0, void *d_output_items0,
                                            void *d_output_items1, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * rootMUSIC_linear_array — gr::doa::rootMUSIC_linear_array::make(norm_spacing, num_targets,
 *   num_ant_ele) (include/doa/rootMUSIC_linear_array.h:54).  gr::sync_block.
 * Item layouts: input as MUSIC_lin_array; output 0 = num_targets floats, angles in degrees,
 *   ascending (lib/rootMUSIC_linear_array_impl.cc:48-49,144-145).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_rootMUSIC_linear_array doa_rootMUSIC_linear_array_t;

DOA_HIP_API doa_rootMUSIC_linear_array_t *doa_rootMUSIC_linear_array_create(float norm_spacing,
                                                                            int num_targets,
                                                                            int num_ant_ele);
DOA_HIP_API void doa_rootMUSIC_linear_array_destroy(doa_rootMUSIC_linear_array_t *h);
DOA_HIP_API int doa_rootMUSIC_linear_array_work(doa_rootMUSIC_linear_array_t *h, int noutput_items,
                                                const void *input_items0, void *output_items0);
DOA_HIP_API int doa_rootMUSIC_linear_array_work_dev(doa_rootMUSIC_linear_array_t *h,
                                                    int noutput_items, const void *d_input_items0,
                                                    void *d_output_items0, void *hip_stream);
DOA_HIP_API int doa_rootMUSIC_linear_array_set_internal_precision(doa_rootMUSIC_linear_array_t *h, int bits);

/* ---------------------------------------------------------------------------------------------
 * antenna_correction — gr::doa::antenna_correction::make(num_ant_ele, config_filename)
 *   (include/doa/antenna_correction.h:55, lib/antenna_correction_impl.cc:47-99).  gr::sync_block,
 *   num_ant_ele gr_complex streams in and out: out_k[i] = g_k * in_k[i] with
 *   g_k = (1/gain_k) * exp(-j phase_k) read from a text file with one "gain phase" pair per line.
 *   create fails (message = the reference's std::invalid_argument text) when the file is missing
 *   or has too many / too few lines.
 * The block sits directly in front of autocorrelate; doa_autocorrelate_fuse_antenna_correction folds
 * it into K1 (R[a,b] *= g_a conj(g_b) before the forward-backward step) so the corrected streams are
 * never materialised.  (a "next" row beyond the north-star path.)
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_antenna_correction doa_antenna_correction_t;

DOA_HIP_API doa_antenna_correction_t *doa_antenna_correction_create(int num_ant_ele, const char *config_filename);
/* The same block from explicit per-stream complex gains (re, im interleaved) instead of a file: what
 * python/phase_correct_hier.py:90-97 builds out of multiply_const_vcc blocks (stream 0 untouched, stream p+1 times
 * exp(j phase_p)); the Python mirror doa.phase_correct_hier parses the phase file as the reference does and calls this. */
DOA_HIP_API doa_antenna_correction_t *doa_antenna_correction_create_gains(int num_ant_ele, const float *gains_re_im);
DOA_HIP_API void doa_antenna_correction_destroy(doa_antenna_correction_t *h);
/* Copies the num_ant_ele complex gains (re, im interleaved) out; returns num_ant_ele. */
DOA_HIP_API int doa_antenna_correction_gains(const doa_antenna_correction_t *h, float *gains_re_im);
DOA_HIP_API int doa_antenna_correction_work(doa_antenna_correction_t *h, int noutput_items,
                                            const void *const *input_items, void *const *output_items);
DOA_HIP_API int doa_antenna_correction_work_dev(doa_antenna_correction_t *h, int noutput_items,
                                                const void *const *d_input_items, void *const *d_output_items,
                                                void *hip_stream);
/* Fold a per-stream complex gain into this autocorrelate handle (gains_re_im: inputs pairs, or NULL
 * to remove it).  Equivalent to an antenna_correction block feeding the autocorrelate block. */
DOA_HIP_API int doa_autocorrelate_fuse_antenna_correction(doa_autocorrelate_t *h, const float *gains_re_im);

/* ---------------------------------------------------------------------------------------------
 * calibrate_lin_array — gr::doa::calibrate_lin_array::make(norm_spacing, num_ant_ele, pilot_angle)
 *   (include/doa/calibrate_lin_array.h, lib/calibrate_lin_array_impl.cc:36-134).  gr::sync_block:
 *   input = column-major num_ant_ele^2 gr_complex covariance items measured with one pilot source at
 *   pilot_angle degrees; output = num_ant_ele gr_complex per item, the estimated per-antenna complex
 *   responses (unit-norm vector).  The reference's output carries an arbitrary unit-modulus factor
 *   (LAPACK eigenvector phase); here element 0 is real and non-negative.  
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_calibrate_lin_array doa_calibrate_lin_array_t;

DOA_HIP_API doa_calibrate_lin_array_t *doa_calibrate_lin_array_create(float norm_spacing, int num_ant_ele,
                                                                      float pilot_angle);
DOA_HIP_API void doa_calibrate_lin_array_destroy(doa_calibrate_lin_array_t *h);
DOA_HIP_API int doa_calibrate_lin_array_work(doa_calibrate_lin_array_t *h, int noutput_items,
                                             const void *input_items0, void *output_items0);
DOA_HIP_API int doa_calibrate_lin_array_work_dev(doa_calibrate_lin_array_t *h, int noutput_items,
                                                 const void *d_input_items0, void *d_output_items0,
                                                 void *hip_stream);
DOA_HIP_API int doa_calibrate_lin_array_set_internal_precision(doa_calibrate_lin_array_t *h, int bits);

/* ---------------------------------------------------------------------------------------------
 * music_pipeline — autocorrelate -> MUSIC_lin_array -> find_local_max(num_targets, pspectrum_len,
 *   0, 180) on device-resident streams, the batch entry point the benchmark drives
 *   (apps/run_MUSIC_lin_array_simulation.grc wiring).  All pointers are DEVICE pointers except
 *   d_input_items itself (host array of device pointers).  d_cov_out and d_spectrum_out may be
 *   NULL when the caller does not want that intermediate materialised in its own buffer.  A NULL spectrum pointer is
 *   the ANGLES-ONLY mode: for the benchmark-shaped spectra (pspectrum_len 256 / 512 / 1024, polynomial size = array size)
 *   the scan kernel then neither converts the row to dB nor writes it (the maximum of a normalised row is 0 dB by
 *   construction and its position follows from the null spectrum itself); peaks and angles are bit-identical to a call
 *   that asks for the spectrum (21.1 against 25.3 us per 4096-snapshot step on MI355X, 500-step runs of round 3).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_music_pipeline doa_music_pipeline_t;

DOA_HIP_API doa_music_pipeline_t *doa_music_pipeline_create(int inputs, int snapshot_size,
                                                            int overlap_size, int avg_method,
                                                            float norm_spacing, int num_targets,
                                                            int pspectrum_len, int max_batch);
DOA_HIP_API void doa_music_pipeline_destroy(doa_music_pipeline_t *h);
/* Same fusion as doa_autocorrelate_fuse_antenna_correction, for the pipeline's K1. */
DOA_HIP_API int doa_music_pipeline_fuse_antenna_correction(doa_music_pipeline_t *h, const float *gains_re_im);
DOA_HIP_API int doa_music_pipeline_work_dev(doa_music_pipeline_t *h, int noutput_items,
                                            const void *const *d_input_items, void *d_cov_out,
                                            void *d_spectrum_out, void *d_max_out,
                                            void *d_argmax_out, void *hip_stream);
/* n_batches independent batches of noutput_items snapshots each (<= max_batch) in ONE call, overlapped by the library:
 * the batches run their K1 -> EVD -> scan chains on the handle's own LANES (a HIP stream plus a private workspace; 4
 * by default, rotating from call to call), so that the HBM-bound covariance kernel of one batch runs beside the
 * issue-bound EVD / scan kernels of its neighbours -- the overlap a caller otherwise has to build from several handles on
 * several streams of its own (reference work being chained: lib/autocorrelate_impl.cc:83-118 ->
 * lib/MUSIC_lin_array_impl.cc:121-142 -> lib/find_local_max_impl.cc:167-194, wiring
 * apps/run_MUSIC_lin_array_simulation.grc:1099-1370).  Results are bit-identical to n_batches work_dev calls.
 *   GROUPS: on the lean route (no overlap, inputs <= 4, double inside, pspectrum_len 256 / 512 / 1024, and not inputs = 4
 *   with two targets) consecutive batches are launched together -- ONE covariance, ONE eigen and ONE scan launch cover a
 *   group of up to 8 batches on one lane, up to 4 when the groups alternate over two lanes; a group
 *   ends early where the next batch differs in wanting a spectrum, in the alignment of its streams or of its spectrum
 *   pointer, or writes a buffer a batch of the group writes.  Every other shape runs one chain of launches per batch.
 *   ORDER: groups (batches) on one lane run in order, lanes run side by side.  Two batches of a call that share an OUTPUT
 *   buffer (covariance, spectrum, maxima or arg-max pointer) run in the order of the call: the later one follows the
 *   earlier one on its lane (if its outputs were last written on two different lanes, the call waits on the host for the
 *   lanes first), so the later batch's results are the ones that stay.  Batches that share no output buffer are not
 *   ordered, and nothing orders a batch's INPUTS against another batch's outputs.  Between calls the attached form orders
 *   everything through the caller's stream; in the detached form the caller joins with doa_music_pipeline_synchronize.
 *   d_input_items   HOST array of n_batches * inputs DEVICE pointers (batch b: entries b*inputs .. b*inputs+inputs-1)
 *   d_cov_out, d_spectrum_out  HOST arrays of n_batches DEVICE pointers; the array or single entries may be NULL (no
 *                   covariance copy wanted / angles-only mode for that batch, as in work_dev)
 *   d_max_out, d_argmax_out    HOST arrays of n_batches DEVICE pointers (required)
 *   hip_stream      a hipStream_t: the call is asynchronous like work_dev and ordered on that stream AS A WHOLE -- every lane
 *                   it uses starts behind the work the stream held at the call (one event) and the stream continues behind
 *                   the last batch of every lane (one event per lane): one fork and one join per call whatever n_batches
 *                   is.  Or DOA_STREAM_DETACHED: no ordering against any caller stream (the inputs must be complete when
 *                   the call is made); the caller joins with doa_music_pipeline_synchronize before it touches the
 *                   outputs.  Cross-stream events cost tens of microseconds on this runtime: callers
 *                   that submit many short calls want the detached form.
 * Returns n_batches * noutput_items or a negative doa_status; after an error the join has still been enqueued. */
#define DOA_STREAM_DETACHED ((void *)(size_t)-1)
DOA_HIP_API int doa_music_pipeline_work_dev_batches(doa_music_pipeline_t *h, int n_batches, int noutput_items,
                                                    const void *const *d_input_items, void *const *d_cov_out,
                                                    void *const *d_spectrum_out, void *const *d_max_out,
                                                    void *const *d_argmax_out, void *hip_stream);
/* Host-side join: returns when every lane of the handle has finished what work_dev_batches gave it. */
DOA_HIP_API int doa_music_pipeline_synchronize(doa_music_pipeline_t *h);
/* Upper bound of the lanes work_dev_batches spreads its batches over (1..8, default 4; 1 = everything on hip_stream
 * itself); grouped launches (above) use at most two of them. */
DOA_HIP_API int doa_music_pipeline_set_lanes(doa_music_pipeline_t *h, int n_lanes);
/* Lanes on streams the CALLER created (n_lanes hipStream_t; they stay the caller's, the handle only uses them).  For a
 * host program that draws its streams from a pool of its own (PyTorch, a GNU Radio buffer manager): HIP maps streams
 * onto a few hardware queues in creation order, and which streams share a queue with which decides how well kernels of
 * different lanes overlap (measured: 26 against 33 us per 4096-snapshot step for four lanes on one set of streams or
 * another) -- the program that owns the process's streams is the one that can choose. */
DOA_HIP_API int doa_music_pipeline_set_lane_streams(doa_music_pipeline_t *h, int n_lanes, void *const *hip_streams);
DOA_HIP_API int doa_music_pipeline_set_internal_precision(doa_music_pipeline_t *h, int bits);
/* Input sample format of the streams, as doa_autocorrelate_set_input_format (all entries of the handle; the host entry
 * stages 4 B per sample for sc16, so half the bytes cross PCIe). */
DOA_HIP_API int doa_music_pipeline_set_input_format(doa_music_pipeline_t *h, int format, float scale);
/* The same three blocks on HOST buffers (the layouts the GNU Radio scheduler hands to the blocks'
 * work(): input_items[k] = stream k, doa_autocorrelate_input_span(noutput_items) samples; outputs
 * noutput_items items each).  cov_out and spectrum_out may be NULL: only the 2*num_targets floats
 * per snapshot then cross PCIe on the way back.  Samples are moved in ~32 MiB chunks alternating over
 * two streams owned by the handle (transfers of neighbouring chunks overlap when the caller's
 * buffers are page-locked); returns when every output has landed.  This path is PCIe-bound
 * (N*(snapshot-overlap)*8 B per snapshot in), see DESIGN.md §6. */
DOA_HIP_API int doa_music_pipeline_work(doa_music_pipeline_t *h, int noutput_items,
                                        const void *const *input_items, void *cov_out,
                                        void *spectrum_out, void *max_out, void *argmax_out);

/* ---------------------------------------------------------------------------------------------
 * source_count — the number of sources per covariance item, estimated on the device from the item's eigenvalues
 *   (Wax-Kailath MDL, or AIC), and the entries that take a count PER ITEM instead of the num_targets fixed at create.
 *   Not a block of the reference: gr-doa takes num_targets as a flowgraph parameter; MUSIC is only right when that number
 *   is (too small: a source's eigenvector lands in the noise subspace; too large: spurious peaks), and a receiver in the
 *   field does not know it.
 * The criterion, one definition for every entry: for one item (column-major num_ant_ele^2 gr_complex, upper triangle only,
 *   as MUSIC_lin_array) let l_0 <= ... <= l_{N-1} be its eigenvalues in double at the item's true scale.
 *     status : a non-finite entry, or l_{N-1} <= 0  ->  count -1 (a non-finite item's eigenvalue outputs are NaN)
 *     floor  : l_i <- max(l_i, l_{N-1} * 2^-40)
 *     L_k    = sum log l_i - m log((sum l_i) / m) over the m = N - k smallest, summed in ascending index order
 *     MDL_k  = -K L_k + 0.5 k (2N - k) log K        AIC_k = -2K L_k + 2 k (2N - k)        K = num_snapshots
 *     count  = the smallest k in 0 .. max_sources that attains the minimum
 *   (scale-invariant, so forward-backward averaging's factor does not matter; forward-backward-specific parameter counts
 *   are not applied).  Eigenvalues come from the double Jacobi kernels of MUSIC_lin_array (never the subspace iteration,
 *   which does not form the noise eigenvalues); internal precision 32 is not supported: DOA_ERR_UNSUPPORTED.
 * Item layouts: input as MUSIC_lin_array; count_out = one int32 per item; eig_out (optional, NULL = not wanted) =
 *   num_ant_ele floats per item, the eigenvalues ascending.
 * create validates before the device is touched: 2 <= num_ant_ele (> DOA_MAX_ANT_ELE: rejected), num_snapshots >= 2,
 *   method DOA_SOURCE_COUNT_MDL or _AIC, 1 <= max_sources <= num_ant_ele - 1.
 * --------------------------------------------------------------------------------------------- */
#define DOA_SOURCE_COUNT_MDL 0
#define DOA_SOURCE_COUNT_AIC 1
typedef struct doa_source_count doa_source_count_t;

DOA_HIP_API doa_source_count_t *doa_source_count_create(int num_ant_ele, int num_snapshots, int method, int max_sources);
DOA_HIP_API void doa_source_count_destroy(doa_source_count_t *h);
DOA_HIP_API int doa_source_count_work(doa_source_count_t *h, int noutput_items, const void *cov_items, void *count_out,
                                      void *eig_out);
DOA_HIP_API int doa_source_count_work_dev(doa_source_count_t *h, int noutput_items, const void *d_cov_items,
                                          void *d_count_out, void *d_eig_out, void *hip_stream);

/* MUSIC_lin_array with a count per item: counts = one int32 per item, used in place of the handle's num_targets (noise set =
 * the num_ant_ele - count smallest eigenvalues).  Count 0 is legal: P_N = I exactly, the row is all 0.0 dB.  A count outside
 * 0 .. num_ant_ele-1 (the -1 status of source_count included) gives a NaN row; other items are not affected.  Always the
 * double Jacobi route (a uniform count therefore agrees with doa_MUSIC_lin_array_work to the parity bounds, not bit for
 * bit); a handle at internal precision 32: DOA_ERR_UNSUPPORTED.  NULL counts: DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_MUSIC_lin_array_work_counts(doa_MUSIC_lin_array_t *h, int noutput_items, const void *cov_items,
                                                const void *counts, void *spectrum_out);
DOA_HIP_API int doa_MUSIC_lin_array_work_dev_counts(doa_MUSIC_lin_array_t *h, int noutput_items, const void *d_cov_items,
                                                    const void *d_counts, void *d_spectrum_out, void *hip_stream);
/* find_local_max with a count per item: counts = one int32 m_i per item.  The first m_i slots of both outputs are what
 * find_local_max(m_i, vector_len, x_min, x_max) writes for that vector (fill rule and the m_i == 1 global arg-max rule
 * included); items stay num_max_vals floats wide and the remaining slots are NaN; m_i outside 0 .. num_max_vals: all NaN. */
DOA_HIP_API int doa_find_local_max_work_counts(doa_find_local_max_t *h, int noutput_items, const void *input_items0,
                                               const void *counts, void *output_items0, void *output_items1);
DOA_HIP_API int doa_find_local_max_work_dev_counts(doa_find_local_max_t *h, int noutput_items, const void *d_input_items0,
                                                   const void *d_counts, void *d_output_items0, void *d_output_items1,
                                                   void *hip_stream);
/* music_pipeline with the count estimated per snapshot: K1 exactly as doa_music_pipeline_work_dev runs it (fused gains,
 * sc16 input and overlap honoured; the covariance is bit-identical), then ONE eigen launch that also estimates the count
 * (K = snapshot_size, max_sources = the handle's num_targets, `method` as above) and forms each item's noise set from it,
 * the scan, and the counted peak pick: four launches (a fifth, which only turns the rows of count -1 items into NaN, when
 * d_spectrum_out is given), asynchronous on hip_stream.  d_count_out (int32 per item) is
 * required; d_eig_out (num_ant_ele floats per item), d_cov_out and d_spectrum_out may be NULL.  d_max_out / d_argmax_out
 * stay num_targets floats per item: the first count slots are find_local_max(count, ...)'s, the rest NaN; count -1: the
 * spectrum row and all slots are NaN; count 0: the row is 0.0 dB and all slots are NaN.  The outputs are bit-identical to
 * the chain source_count -> MUSIC_lin_array_work_dev_counts -> find_local_max_work_dev_counts on the covariance written.
 * One batch of at most max_batch items; internal precision 32: DOA_ERR_UNSUPPORTED. */
DOA_HIP_API int doa_music_pipeline_work_dev_auto(doa_music_pipeline_t *h, int noutput_items,
                                                 const void *const *d_input_items, int method, void *d_cov_out,
                                                 void *d_spectrum_out, void *d_max_out, void *d_argmax_out,
                                                 void *d_count_out, void *d_eig_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * spatial_smooth — spatial smoothing of covariance items for COHERENT sources (a source and its multipath echo, emitters
 *   locked to one oscillator): the signal part of their covariance has rank one, and MUSIC, Root-MUSIC and source_count
 *   all fail quietly on it.  For a uniform linear array the N x N covariance (N = num_ant_ele) is replaced by the average
 *   of its L = N - S + 1 overlapping S x S diagonal blocks (S = subarray_size; Shan-Wax-Kailath), with forward_backward
 *   = 1 also of their persymmetric images (Pillai-Kwon); the smoothed items are covariances of an S-element array with
 *   the same spacing and go to MUSIC_lin_array / rootMUSIC_linear_array / source_count created for S elements.  Up to
 *   S - 1 sources can be resolved; forward smoothing restores the rank for up to L mutually coherent sources, the
 *   forward-backward form for more.  Not a block of the reference.
 * The definition, one for every entry (tests/spatial_smooth_ref.py restates it in numpy):
 *   input item   column-major N x N gr_complex, as MUSIC_lin_array takes it; ONLY THE UPPER TRIANGLE IS READ, and of the
 *                diagonal the real part (its imaginary part is taken as 0): H = the Hermitian matrix these define
 *   output item  column-major S x S gr_complex, the full Hermitian matrix
 *   for 0 <= i <= j < S:
 *     f[i,j]   = sum_{l=0}^{L-1} (double) H[i+l, j+l]        l ascending, re and im separately
 *     fb == 0 : s = f[i,j]
 *     fb == 1 : s = 0.5 * (f[i,j] + f[S-1-j, S-1-i])         (= 0.5 (F + J conj(F) J); no conjugate appears)
 *     out[i,j] = (float)(s * (1.0 / L))                      1.0 / L formed in double; one rounding per component
 *     out[j,i] = conj(out[i,j]);  Im out[i,i] = +0.0
 *   No product feeds an addition, so an implementation that does these operations in this order is bit-identical to the
 *   numpy statement; the device kernel is, for either pointer alignment and any batch size.  Non-finite entries propagate
 *   by IEEE rules to the outputs whose sums touch them; there is no status output.  S == N with fb == 0 is the Hermitian
 *   completion of the upper triangle.  (MUSIC and the source count are scale-invariant; the 1 / L keeps the items
 *   covariances.)
 * create validates before the device is touched: 2 <= subarray_size <= num_ant_ele <= DOA_MAX_ANT_ELE, forward_backward
 *   0 or 1.  smoothed_items must NOT overlap cov_items (not checked).  The device entry takes 16-byte loads and stores when
 *   both pointers are 16-byte aligned and 8-byte ones otherwise (gr_complex alignment is the minimum).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_spatial_smooth doa_spatial_smooth_t;

DOA_HIP_API doa_spatial_smooth_t *doa_spatial_smooth_create(int num_ant_ele, int subarray_size, int forward_backward);
DOA_HIP_API void doa_spatial_smooth_destroy(doa_spatial_smooth_t *h);
DOA_HIP_API int doa_spatial_smooth_work(doa_spatial_smooth_t *h, int noutput_items, const void *cov_items,
                                        void *smoothed_items);
DOA_HIP_API int doa_spatial_smooth_work_dev(doa_spatial_smooth_t *h, int noutput_items, const void *d_cov_items,
                                            void *d_smoothed_items, void *hip_stream);
/* music_pipeline with the smoothing between K1 and the eigen stage: a per-handle setting, taking effect from the next
 * work call, honoured by every entry (work_dev, work_dev_batches, work, work_dev_auto).  subarray_size == 0 switches it
 * off (the default).  Otherwise 2 <= subarray_size <= inputs, num_targets < subarray_size, forward_backward 0 or 1; a
 * bad call returns DOA_ERR_INVALID_ARG and leaves the handle as it was.  When it is on:
 *   K1 runs exactly as before (fused gains, sc16 and overlap honoured) and d_cov_out stays the inputs x inputs
 *   covariance, bit-identical to an unsmoothed handle's; ONE more launch writes the smoothed items to a workspace of the
 *   handle, and eigen stage, scan and peak pick run for subarray_size elements: the outputs are those of the chain
 *   spatial_smooth -> MUSIC_lin_array(norm_spacing, num_targets, subarray_size, pspectrum_len) -> find_local_max on the
 *   covariance written.  The smoothing arithmetic is the definition above at either internal precision.
 *   work_dev_batches runs one chain of launches per batch (no grouped launches for a smoothed handle).
 *   work_dev_auto: K in the criterion stays snapshot_size, and d_eig_out is subarray_size floats per item. */
DOA_HIP_API int doa_music_pipeline_set_spatial_smoothing(doa_music_pipeline_t *h, int subarray_size, int forward_backward);

/* ---------------------------------------------------------------------------------------------
 * capon_lin_array — the Capon (minimum-variance, MVDR) spectrum of a uniform linear array,
 *       P(theta) = 1 / (a(theta)^H R^-1 a(theta)),
 *   on the angle grid and in the output format of MUSIC_lin_array (pspectrum_len floats, dB against the row maximum).  It
 *   needs no source count and no eigendecomposition: one Cholesky factorisation and one triangular inverse per item, no
 *   iteration, so its time does not depend on the data.  The companion to MUSIC when the number of sources is uncertain.
 *   Not a block of the reference.
 * The definition, one for every entry (tests/capon_ref.py restates it in numpy):
 *   input item   column-major N x N gr_complex (N = num_ant_ele), as MUSIC_lin_array and spatial_smooth take it; ONLY THE
 *                UPPER TRIANGLE IS READ, and of the diagonal the real part: H = the Hermitian matrix these define.  All
 *                arithmetic is in double.
 *     mu  = (sum_i H[i,i]) / N
 *     A   = H / mu + delta I              delta = (double) diagonal_loading  (float argument, >= 0)
 *     W   = A^-1                          via Cholesky A = L L^H, W = L^-H L^-1
 *     u_l = sum_r W[r+l, r]               l = 0 .. N-1: the coefficient record of the scan kernels (csrc/kernels.hpp)
 *     Q_i = u_0 + 2 Re sum_l u_l z_i^l = a_i^H W a_i;  out = 1 / Q;  spectrum = 10 log10(out / max out)
 *   (the kernel multiplies by 1 / mu formed once, within one double rounding of the quotient; the normalisation by the row
 *   maximum cancels the scale of W, and an item multiplied by a power of two gives the same bits.)
 *   status per item (int32): 0 ok; 1 = "not positive definite enough":
 *     mu > 0 does not hold (a zero item; a negative trace, for which H / mu would change sign), or
 *     some Cholesky pivot s_j = A[j,j] - sum_{k<j} |L[j,k]|^2 fails s_j > DOA_CAPON_PIVOT_MIN * A[j,j], or
 *     any quantity is not finite (NaN / Inf entries).
 *   At the threshold 2^-44 the double result no longer carries float accuracy.  A status-1 item gets an all-NaN spectrum
 *   row (and all-NaN peaks where peaks are produced); the other items of the call are not affected.
 *   diagonal_loading: with fewer snapshots than antennas the sample covariance is singular and delta > 0 is required;
 *   delta is relative to the mean diagonal entry.
 * Internal precision 64 only: a handle created while the process default is 32 returns DOA_ERR_UNSUPPORTED from its work
 * entries.  create validates before the device is touched: 2 <= num_ant_ele <= DOA_MAX_ANT_ELE, 0 < norm_spacing <= 0.5,
 * pspectrum_len > 0, diagonal_loading finite and >= 0.  status_out / d_status_out (one int32 per item) may be NULL.
 * --------------------------------------------------------------------------------------------- */
#define DOA_CAPON_PIVOT_MIN (1.0 / 17592186044416.0)   /* 2^-44, exact */
typedef struct doa_capon_lin_array doa_capon_lin_array_t;

DOA_HIP_API doa_capon_lin_array_t *doa_capon_lin_array_create(float norm_spacing, int num_ant_ele, int pspectrum_len,
                                                              float diagonal_loading);
DOA_HIP_API void doa_capon_lin_array_destroy(doa_capon_lin_array_t *h);
DOA_HIP_API int doa_capon_lin_array_work(doa_capon_lin_array_t *h, int noutput_items, const void *cov_items,
                                         void *spectrum_out, void *status_out);
DOA_HIP_API int doa_capon_lin_array_work_dev(doa_capon_lin_array_t *h, int noutput_items, const void *d_cov_items,
                                             void *d_spectrum_out, void *d_status_out, void *hip_stream);
DOA_HIP_API long long doa_capon_lin_array_items_total(const doa_capon_lin_array_t *h);
/* music_pipeline with the Capon spectrum in place of the MUSIC one: a per-handle setting, taking effect from the next work
 * call.  DOA_ESTIMATOR_MUSIC (the default) is the path described above, unchanged.  DOA_ESTIMATOR_CAPON: the eigen launch
 * is replaced by the inverse launch above (diagonal_loading as in doa_capon_lin_array_create; ignored for MUSIC), on the
 * subarray_size x subarray_size items when spatial smoothing is on; scan and peak pick run as before, so num_targets only
 * means "how many peaks", and one small launch after them turns the spectrum row and the peaks of status-1 items into NaN.
 * The outputs are bit-identical to the chain autocorrelate -> capon_lin_array -> find_local_max.  In Capon mode
 * work_dev_batches runs one chain of launches per batch (no grouped launches), work_dev_auto returns DOA_ERR_UNSUPPORTED
 * (it needs eigenvalues), and so does every work entry of a handle at internal precision 32.  A bad call returns
 * DOA_ERR_INVALID_ARG and leaves the handle as it was. */
#define DOA_ESTIMATOR_MUSIC 0
#define DOA_ESTIMATOR_CAPON 1
DOA_HIP_API int doa_music_pipeline_set_estimator(doa_music_pipeline_t *h, int estimator, float diagonal_loading);

/* ---------------------------------------------------------------------------------------------
 * iaa_lin_array — the iterative adaptive (IAA: Yardibi, Li, Stoica et al., 2010) power spectrum of a uniform linear array:
 *   a power per direction, in the units of the covariance item, on the angle grid of MUSIC_lin_array.  It needs no source
 *   count, no eigendecomposition and no smoothing; it works on rank-one items (one snapshot), separates coherent sources at
 *   the full aperture, and its peak heights ARE the source powers.  A fixed number of iterations, so its time does not depend
 *   on the data.  Not a block of the reference.
 * The definition, one for every entry (tests/iaa_ref.py restates it in numpy):
 *   input item   as capon_lin_array reads it: column-major N x N gr_complex, ONLY THE UPPER TRIANGLE, of the diagonal the
 *                real part; H = the Hermitian matrix these define.  All arithmetic is in double.  a_k = the steering vector
 *                of direction k of MUSIC_lin_array's grid (its float-accumulated theta included), k = 0 .. pspectrum_len - 1.
 *     mu   = (sum_i H[i,i]) / N ;  Hn = H / mu
 *     p_k  = Re(a_k^H Hn a_k) / N^2                                    the start: the Bartlett spectrum
 *     repeat L = iterations times (never data dependent):
 *       R   = sum_k p_k a_k a_k^H + delta I                            delta = (double) diagonal_loading, relative as in Capon
 *       W   = R^-1                                                     via Cholesky R = L L^H, W = L^-H L^-1
 *       B   = W Hn W
 *       g_k = Re(a_k^H W a_k) ;  n_k = max(Re(a_k^H B a_k), 0)
 *       p_k = n_k / g_k^2
 *     spectrum row = 10 log10(p / max p), formed as MUSIC_lin_array forms its row from out = p: out rounded to float, a
 *                    float quotient, 0 dB exactly at the largest rounded value; p_k = 0 gives -inf
 *     power row    = (float)(mu p_k)                                   the optional second port
 *   (the kernel multiplies by 1 / mu formed once; an item multiplied by a power of two gives the same spectrum bits and
 *   a power row multiplied by exactly that factor.  For a uniform linear array R is Hermitian Toeplitz, fixed by the N lags
 *   r_l = sum_k p_k w_k^l, w_k = a_k[n+1] / a_k[n], and the kernel builds it from them.)
 *   status per item (int32): 0 ok; 1: mu > 0 does not hold, a Cholesky pivot of any iteration fails
 *     s_j > DOA_CAPON_PIVOT_MIN * R[j,j], or any quantity is not finite.  A status-1 item gets all-NaN rows on both ports; the
 *     other items of the call are not affected.
 * Internal precision 64 only: a handle created while the process default is 32 returns DOA_ERR_UNSUPPORTED from its work
 * entries.  create validates before the device is touched: 2 <= num_ant_ele <= DOA_MAX_ANT_ELE, 0 < norm_spacing <= 0.5,
 * 1 <= pspectrum_len <= DOA_IAA_MAX_PSPECTRUM_LEN, diagonal_loading finite and >= 0, 1 <= iterations <=
 * DOA_IAA_MAX_ITERATIONS (DOA_IAA_DEFAULT_ITERATIONS is what the Python block and the GRC descriptor default to).
 * power_out / d_power_out (pspectrum_len floats per item) and status_out / d_status_out (one int32 per item) may be NULL.
 * --------------------------------------------------------------------------------------------- */
#define DOA_IAA_MAX_PSPECTRUM_LEN 4096
#define DOA_IAA_MAX_ITERATIONS 32
#define DOA_IAA_DEFAULT_ITERATIONS 10
typedef struct doa_iaa_lin_array doa_iaa_lin_array_t;

DOA_HIP_API doa_iaa_lin_array_t *doa_iaa_lin_array_create(float norm_spacing, int num_ant_ele, int pspectrum_len,
                                                          float diagonal_loading, int iterations);
DOA_HIP_API void doa_iaa_lin_array_destroy(doa_iaa_lin_array_t *h);
DOA_HIP_API int doa_iaa_lin_array_work(doa_iaa_lin_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out,
                                       void *power_out, void *status_out);
DOA_HIP_API int doa_iaa_lin_array_work_dev(doa_iaa_lin_array_t *h, int noutput_items, const void *d_cov_items,
                                           void *d_spectrum_out, void *d_power_out, void *d_status_out, void *hip_stream);
DOA_HIP_API long long doa_iaa_lin_array_items_total(const doa_iaa_lin_array_t *h);

/* ---------------------------------------------------------------------------------------------
 * Arbitrary array geometry: MUSIC_array and capon_array — the two spectra for an array given by a STEERING TABLE instead of
 *   a uniform linear array: a uniform circular array, any planar layout, or a measured (calibrated) manifold of a linear one.
 *   Every other estimator of this library assumes a_n = z^n and hands its scan the 2N-1 diagonal sums of the projector, which
 *   summarise a^H X a for that manifold only.  Not blocks of the reference.
 * The definition, one for every entry (tests/array_ref.py restates it in numpy):
 *   steering table  P rows of N complex doubles (N = num_ant_ele, P = pspectrum_len), a_i[n] at [i*N + n] (re, im); a HOST
 *                   pointer at create, copied to the device once.  Rows need not have unit modulus (a calibrated manifold
 *                   carries gains); every value must be finite.  Row i is direction i of the output; what the directions are
 *                   is the caller's business (doa_planar_steering_table below builds an azimuth grid).
 *   input item      column-major N x N gr_complex, upper triangle read, as MUSIC_lin_array / capon_lin_array take it.
 *   X               MUSIC_array: the noise projector P_N = U_N U_N^H of the item (U_N = the eigenvectors of the N - num_targets
 *                   smallest eigenvalues), as MUSIC_lin_array forms it; capon_array: W = (H / mu + delta I)^-1 EXACTLY as
 *                   capon_lin_array defines it above (status, pivot rule DOA_CAPON_PIVOT_MIN and the all-NaN row included).
 *   All arithmetic in double:
 *       Q_i = Re(a_i^H X a_i)        out_i = 1 / Q_i        spectrum_i = 10 log10(out_i / max out)
 *   with the dB normalisation of the ULA scans: Q is rounded to float, the row maximum is exactly 0.0 dB, and where several
 *   directions tie the first one is the maximum find_local_max reports.
 * Internal precision 64 only: a handle whose process default (at create) or handle precision is 32 returns
 * DOA_ERR_UNSUPPORTED from its work entries.  create validates before the device is touched: 2 <= num_ant_ele <=
 * DOA_MAX_ANT_ELE, 1 <= num_targets < num_ant_ele, pspectrum_len >= 1, a non-NULL finite table, diagonal_loading finite and
 * >= 0.  An item's result depends on the item and the table alone (not on the batch size or its position in the batch).
 * Peaks: find_local_max(num_max_vals, pspectrum_len, x_min, x_max) on the output, with the axis of the table's directions;
 * it does not wrap around: for a full circle, or an azimuth x elevation grid, use find_local_max_2d below (wrap_az), which
 * treats the first and the last azimuth as neighbours.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_MUSIC_array doa_MUSIC_array_t;
typedef struct doa_capon_array doa_capon_array_t;

/* Host helper, no device needed: the steering table of a planar array for an azimuth grid at one elevation.
 *   xy            2 * num_ant_ele doubles: element positions in wavelengths, x_n at [2n], y_n at [2n + 1]
 *   az_i        = az_min_deg + i (az_max_deg - az_min_deg) / pspectrum_len,  i = 0 .. pspectrum_len - 1  (double; the end point
 *                 is excluded, as in the grids of MUSIC_lin_array and find_local_max)
 *   elevation     theta, measured from the array normal: 90 degrees is in the array's plane
 *   a_i[n]      = exp(+j 2 pi sin(theta) (x_n cos(az_i) + y_n sin(az_i)))      -> table_out[i * num_ant_ele + n] (re, im)
 * With x_n = d (n - (N-1)/2), y_n = 0 this is the ULA manifold of doa.sim.  DOA_OK, or DOA_ERR_INVALID_ARG unless
 * 2 <= num_ant_ele <= DOA_MAX_ANT_ELE, pspectrum_len >= 1, everything finite, az_max_deg > az_min_deg, pointers non-NULL. */
DOA_HIP_API int doa_planar_steering_table(int num_ant_ele, const double *xy, int pspectrum_len, double az_min_deg,
                                          double az_max_deg, double elevation_deg, double *table_out);

/* MUSIC_array: work / work_dev as doa_MUSIC_lin_array_work / _work_dev (items in, pspectrum_len floats per item out). */
DOA_HIP_API doa_MUSIC_array_t *doa_MUSIC_array_create(int num_targets, int num_ant_ele, int pspectrum_len,
                                                      const double *steering);
DOA_HIP_API void doa_MUSIC_array_destroy(doa_MUSIC_array_t *h);
DOA_HIP_API int doa_MUSIC_array_work(doa_MUSIC_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out);
DOA_HIP_API int doa_MUSIC_array_work_dev(doa_MUSIC_array_t *h, int noutput_items, const void *d_cov_items,
                                         void *d_spectrum_out, void *hip_stream);
DOA_HIP_API long long doa_MUSIC_array_items_total(const doa_MUSIC_array_t *h);
/* bits = 32 or 64; a handle at 32 returns DOA_ERR_UNSUPPORTED from its work entries (there is no float form of this scan) */
DOA_HIP_API int doa_MUSIC_array_set_internal_precision(doa_MUSIC_array_t *h, int bits);

/* capon_array: work / work_dev as doa_capon_lin_array_work / _work_dev, the status output included (one int32 per item,
 * may be NULL; a status-1 item gets an all-NaN row and does not disturb its neighbours). */
DOA_HIP_API doa_capon_array_t *doa_capon_array_create(int num_ant_ele, int pspectrum_len, const double *steering,
                                                      float diagonal_loading);
DOA_HIP_API void doa_capon_array_destroy(doa_capon_array_t *h);
DOA_HIP_API int doa_capon_array_work(doa_capon_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out,
                                     void *status_out);
DOA_HIP_API int doa_capon_array_work_dev(doa_capon_array_t *h, int noutput_items, const void *d_cov_items,
                                         void *d_spectrum_out, void *d_status_out, void *hip_stream);
DOA_HIP_API long long doa_capon_array_items_total(const doa_capon_array_t *h);
/* music_pipeline for an arbitrary array geometry: a per-handle setting, taking effect from the next work call.  steering is a
 * HOST pointer to pspectrum_len rows of `inputs` complex doubles (the table defined above; copied to the device once);
 * (x_min, x_max) is the axis of find_local_max for the table's directions (float, x_max > x_min, both finite).  With a table
 * the stage in front (the eigen launch, or the Capon inverse when the estimator is DOA_ESTIMATOR_CAPON) writes full records
 * into a workspace of the handle (one per lane in work_dev_batches), the steering-table scan replaces the ULA scan, and the
 * peak pick runs as its own launch on the axis rebuilt for (x_min, x_max):  the outputs are bit-identical to the chain
 * autocorrelate -> MUSIC_array | capon_array -> find_local_max(num_targets, pspectrum_len, x_min, x_max).  steering == NULL
 * restores the uniform linear array of create and the 0 .. 180 axis (outputs bit-identical to a fresh handle's).
 * On a table handle: work_dev_batches runs one chain of launches per batch (no grouped launches); work_dev_auto returns
 * DOA_ERR_UNSUPPORTED (no count per item); switching spatial smoothing on -- or setting a table while it is on -- returns
 * DOA_ERR_UNSUPPORTED (smoothing assumes a translation-invariant array); every work entry of a handle at internal precision
 * 32 returns DOA_ERR_UNSUPPORTED.  A bad table or axis returns DOA_ERR_INVALID_ARG.  A refused call leaves the handle as it
 * was.  Call it, like every setter, when no work of the handle is in flight. */
DOA_HIP_API int doa_music_pipeline_set_steering_table(doa_music_pipeline_t *h, const double *steering, float x_min,
                                                      float x_max);

/* ---------------------------------------------------------------------------------------------
 * find_local_max_2d — the top num_max_vals local maxima of an azimuth x elevation grid, each reported as a PAIR
 *   (azimuth, elevation); with n_el = 1 and wrap_az the circular one-dimensional peak pick.  Not a block of the reference.
 * The rule, one for every entry (tests/peaks2d_ref.py restates it in numpy):
 *   grid        an item is n_az * n_el floats; the cell at elevation index e, azimuth index a has flat index i = e n_az + a.
 *   neighbours  the up-to-eight cells (e + de, a + da), de, da in {-1, 0, 1}, not both zero.  A neighbour outside
 *               0 <= e + de < n_el does not exist.  With wrap_az the azimuth index is taken modulo n_az; without it a
 *               neighbour outside 0 <= a + da < n_az does not exist.  A neighbour that is the cell itself (a wrap with
 *               n_az = 1) is skipped, and so is a NaN neighbour.
 *   peak        a cell with value c is a peak if c is not NaN and, for every existing neighbour j with value w,
 *               c > w || (c == w && i < j).  Edge cells can be peaks; a plateau yields its first cell; an all-NaN item has
 *               no peak.
 *   outputs     three per item, each num_max_vals floats: the num_max_vals peaks with the largest value in descending value
 *               order (equal values: lowest flat index first): output 0 the values (the cell's own bits), output 1 their
 *               azimuths, output 2 their elevations IN THE SAME ORDER (paired, unlike the two independently sorted ports of
 *               find_local_max).  Slots beyond the number of peaks are NaN in all three.
 *   axes        az_a = (float)(az_min + a (az_max - az_min) / n_az),  el_e = (float)(el_min + e (el_max - el_min) / n_el),
 *               formed in double from the float limits of create, the end point excluded: the formulas of
 *               doa_planar_steering_grid below, whose limits are doubles -- limits that are not exact in float (0.1) give
 *               axes that differ from the table's directions by that rounding.
 * Compare and integer logic only: the result is bit-exact and depends on the item alone.  create validates before the device
 * is touched: 1 <= num_max_vals <= DOA_MAX_PEAKS, n_az, n_el >= 1, n_az * n_el <= 2^24, finite limits with az_max > az_min
 * and el_max > el_min.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_find_local_max_2d doa_find_local_max_2d_t;

DOA_HIP_API doa_find_local_max_2d_t *doa_find_local_max_2d_create(int num_max_vals, int n_az, int n_el, float az_min,
                                                                  float az_max, float el_min, float el_max, int wrap_az);
DOA_HIP_API void doa_find_local_max_2d_destroy(doa_find_local_max_2d_t *h);
DOA_HIP_API int doa_find_local_max_2d_work(doa_find_local_max_2d_t *h, int noutput_items, const void *input_items0,
                                           void *output_items0, void *output_items1, void *output_items2);
DOA_HIP_API int doa_find_local_max_2d_work_dev(doa_find_local_max_2d_t *h, int noutput_items, const void *d_input_items0,
                                               void *d_output_items0, void *d_output_items1, void *d_output_items2,
                                               void *hip_stream);
DOA_HIP_API long long doa_find_local_max_2d_items_total(const doa_find_local_max_2d_t *h);

/* Host helper, no device needed: the steering table of a planar array for an azimuth x elevation grid.  Row e * n_az + a of
 * table_out is, bit for bit, row a of doa_planar_steering_table(num_ant_ele, xy, n_az, az_min_deg, az_max_deg, el_e, ...)
 * with el_e = el_min_deg + e (el_max_deg - el_min_deg) / n_el in double (elevation from the array normal, as there).
 * table_out: n_az * n_el rows of num_ant_ele complex doubles.  DOA_OK, or DOA_ERR_INVALID_ARG unless 2 <= num_ant_ele <=
 * DOA_MAX_ANT_ELE, n_az, n_el >= 1, n_az * n_el <= 2^24, everything finite, az_max_deg > az_min_deg, el_max_deg >
 * el_min_deg, pointers non-NULL. */
DOA_HIP_API int doa_planar_steering_grid(int num_ant_ele, const double *xy, int n_az, double az_min_deg, double az_max_deg,
                                         int n_el, double el_min_deg, double el_max_deg, double *table_out);

/* music_pipeline in GRID MODE: a steering table whose rows are an azimuth x elevation grid, and directions reported as pairs.
 * A per-handle setting like doa_music_pipeline_set_steering_table, taking effect from the next work call.  (The name does
 * not begin with doa_music_pipeline_ on purpose: the suite pins the number of entries with that prefix, and this one has a
 * test of its own.)
 *   steering    HOST pointer: n_az * n_el rows of `inputs` complex doubles, row e * n_az + a, as doa_planar_steering_grid
 *               writes them; n_az * n_el must equal the handle's pspectrum_len; every value finite.
 *   grid, axes  checked as doa_find_local_max_2d_create checks them, with num_max_vals = num_targets.
 * The chain of a work call is then K1 -> the eigen launch | the Capon inverse (full records) -> ONE launch that scans the
 * table and runs find_local_max_2d's rule on each item's row while it is in LDS (grids above 16384 cells: the scan and the
 * pick as two launches).  Outputs of work_dev, work_dev_batches and work, whose signatures do not change:
 *   spectrum    [n][pspectrum_len], as with a table; optional: without it no row is written to memory at all
 *   max         [n][num_targets]: the peak values
 *   argmax      [n][2 num_targets]: argmax[i][0 .. M-1] the azimuths, argmax[i][M .. 2M-1] the elevations, both in the order
 *               of max (the one order of find_local_max_2d; NaN beyond the number of peaks).  TWICE as wide as in every
 *               other mode: size the buffer for it; the host entry moves 2 num_targets floats per item.
 * All of it bit-identical to autocorrelate -> MUSIC_array | capon_array -> find_local_max_2d(num_targets, n_az, n_el, ...)
 * chained on the device.  A Capon status-1 item ends with a NaN row and 3 num_targets NaN and does not disturb its
 * neighbours.  Limits as for a table handle: work_dev_auto and switching spatial smoothing on (or setting a grid while it is
 * on) return DOA_ERR_UNSUPPORTED, so does every work entry at internal precision 32; work_dev_batches runs one chain per
 * batch.  DOA_ERR_INVALID_ARG for a NULL handle or table, a grid that does not match pspectrum_len, bad limits or a value
 * that is not finite.  A refused call leaves the handle exactly as it was.  doa_music_pipeline_set_steering_table(h, NULL,
 * ...) clears the grid with the table; setting a plain table replaces the grid by the table mode (argmax M wide again). */
DOA_HIP_API int doa_pipeline_set_steering_grid(doa_music_pipeline_t *h, const double *steering, int n_az, int n_el,
                                               float az_min, float az_max, float el_min, float el_max, int wrap_az);

/* rootMUSIC_linear_array with a count per item: counts = one int32 m_i per item, used in place of the handle's num_targets
 * W.  Items stay W floats wide.  With top = min(W, num_ant_ele - 1):
 *   1 <= m_i <= top   the first m_i slots are what rootMUSIC_linear_array(norm_spacing, m_i, num_ant_ele) writes for the
 *                     item's record (selection rule, 90 degrees once the interior roots run out, ascending, NaN last), the
 *                     slots m_i .. W-1 are NaN; status 0, or 1 (all W slots NaN) when no root lies strictly inside the circle
 *   m_i == 0          all W slots NaN, status 0 (the root finder does not run on the item)
 *   any other value   (the -1 of source_count included) all W slots NaN, status 2 = "no usable count"; other items are not
 *                     affected
 * The eigen stage is the forced-count launch of doa_MUSIC_lin_array_work_dev_counts (always the double Jacobi route, so a
 * uniform count agrees with doa_rootMUSIC_linear_array_work to the parity bounds, not bit for bit).  d_status_out (one int
 * per item) may be NULL.  The host entry returns DOA_ERR_NUMERIC only when some item has status 1 (the angles of the other
 * items are valid); status 2 items are the caller's own counts and no error.  A handle at internal precision 32:
 * DOA_ERR_UNSUPPORTED.  NULL counts: DOA_ERR_INVALID_ARG. */
DOA_HIP_API int doa_rootMUSIC_linear_array_work_counts(doa_rootMUSIC_linear_array_t *h, int noutput_items,
                                                       const void *cov_items, const void *counts, void *angles_out);
DOA_HIP_API int doa_rootMUSIC_linear_array_work_dev_counts(doa_rootMUSIC_linear_array_t *h, int noutput_items,
                                                           const void *d_cov_items, const void *d_counts,
                                                           void *d_angles_out, int *d_status_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * root_pipeline — autocorrelate -> rootMUSIC_linear_array on device-resident streams: the Root-MUSIC branch of the hot
 *   path as one handle (the chain apps/run_RootMUSIC_lin_array_simulation.grc wires; reference work being chained:
 *   lib/autocorrelate_impl.cc:83-118 -> lib/rootMUSIC_linear_array_impl.cc:90-152).  Same conventions as music_pipeline:
 *   all pointers are DEVICE pointers except the pointer arrays themselves; d_cov_out may be NULL.  Output: num_targets
 *   floats per snapshot, angles in degrees, ascending (rootMUSIC_linear_array's output 0).
 *   d_status_out (optional): one int per snapshot, 1 = the polynomial has no root strictly inside the unit circle -- the
 *   case in which the reference raises inside arma::index_min and the host entry returns DOA_ERR_NUMERIC; the device entries
 *   are asynchronous and leave the check to the caller.  Results are bit-identical to the two block handles chained by hand
 *   (doa_autocorrelate_work_dev -> doa_rootMUSIC_linear_array_work_dev).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_root_pipeline doa_root_pipeline_t;

DOA_HIP_API doa_root_pipeline_t *doa_root_pipeline_create(int inputs, int snapshot_size, int overlap_size,
                                                          int avg_method, float norm_spacing, int num_targets,
                                                          int max_batch);
DOA_HIP_API void doa_root_pipeline_destroy(doa_root_pipeline_t *h);
/* Same fusion as doa_autocorrelate_fuse_antenna_correction, for the pipeline's K1. */
DOA_HIP_API int doa_root_pipeline_fuse_antenna_correction(doa_root_pipeline_t *h, const float *gains_re_im);
DOA_HIP_API int doa_root_pipeline_work_dev(doa_root_pipeline_t *h, int noutput_items,
                                           const void *const *d_input_items, void *d_cov_out,
                                           void *d_angles_out, int *d_status_out, void *hip_stream);
/* n_batches independent batches in ONE call, overlapped over the handle's lanes; arguments, stream semantics
 * (DOA_STREAM_DETACHED included), error contract and return value as doa_music_pipeline_work_dev_batches.  Every batch is a
 * group of its own, and ORDER (above) holds with the covariance, angle and status pointers as the output buffers.
 *   d_cov_out, d_status_out   HOST arrays of n_batches DEVICE pointers; the array or single entries may be NULL
 *   d_angles_out              HOST array of n_batches DEVICE pointers (required) */
DOA_HIP_API int doa_root_pipeline_work_dev_batches(doa_root_pipeline_t *h, int n_batches, int noutput_items,
                                                   const void *const *d_input_items, void *const *d_cov_out,
                                                   void *const *d_angles_out, int *const *d_status_out,
                                                   void *hip_stream);
DOA_HIP_API int doa_root_pipeline_synchronize(doa_root_pipeline_t *h);
DOA_HIP_API int doa_root_pipeline_set_lanes(doa_root_pipeline_t *h, int n_lanes);
DOA_HIP_API int doa_root_pipeline_set_lane_streams(doa_root_pipeline_t *h, int n_lanes, void *const *hip_streams);
DOA_HIP_API int doa_root_pipeline_set_internal_precision(doa_root_pipeline_t *h, int bits);
/* Input sample format of the streams, as doa_autocorrelate_set_input_format. */
DOA_HIP_API int doa_root_pipeline_set_input_format(doa_root_pipeline_t *h, int format, float scale);
/* The same chain on HOST buffers (the layouts the GNU Radio scheduler hands to the blocks' work()); cov_out may be NULL.
 * Scheduler-sized calls take one staged copy each way, large ones ~32 MiB chunks alternating over two streams; returns when
 * every output has landed: noutput_items, or DOA_ERR_NUMERIC if some item had no root inside the unit circle (the angles of
 * the other items are valid, that item's are NaN). */
DOA_HIP_API int doa_root_pipeline_work(doa_root_pipeline_t *h, int noutput_items,
                                       const void *const *input_items, void *cov_out, void *angles_out);
/* root_pipeline with the count estimated per snapshot: K1 exactly as doa_root_pipeline_work_dev runs it (fused gains, sc16
 * input and overlap honoured; the covariance is bit-identical), then ONE eigen launch that also estimates the count (K =
 * snapshot_size, max_sources = the handle's num_targets, `method` DOA_SOURCE_COUNT_MDL or _AIC) and writes each item's
 * record for the noise set that count gives, then the counted root kernel: three launches (four on a smoothed handle),
 * asynchronous on hip_stream.  d_count_out (int32 per item) is required; d_cov_out, d_eig_out (num_ant_ele floats per item)
 * and d_status_out may be NULL.  d_angles_out stays num_targets floats per item, filled as
 * doa_rootMUSIC_linear_array_work_dev_counts fills it: count 0: all NaN, status 0; count -1: all NaN, status 2.  The outputs
 * are bit-identical to the chain source_count -> rootMUSIC_linear_array_work_dev_counts on the covariance written.  One
 * batch of at most max_batch items; internal precision 32: DOA_ERR_UNSUPPORTED. */
DOA_HIP_API int doa_root_pipeline_work_dev_auto(doa_root_pipeline_t *h, int noutput_items,
                                                const void *const *d_input_items, int method, void *d_cov_out,
                                                void *d_angles_out, void *d_count_out, void *d_eig_out,
                                                int *d_status_out, void *hip_stream);
/* root_pipeline with spatial smoothing between K1 and the eigen stage; the contract of
 * doa_music_pipeline_set_spatial_smoothing: a per-handle setting, taking effect from the next work call, honoured by
 * work_dev, work_dev_batches, work and work_dev_auto.  subarray_size == 0 switches it off (the default).  Otherwise
 * 2 <= subarray_size <= inputs, num_targets < subarray_size, forward_backward 0 or 1; a bad call returns
 * DOA_ERR_INVALID_ARG and leaves the handle as it was.  When it is on, K1 runs exactly as before and d_cov_out stays the
 * inputs x inputs covariance, bit-identical to an unsmoothed handle's; ONE more launch writes the smoothed items to a
 * workspace (one per lane), and eigen stage and root finder run for subarray_size elements: the outputs are those of the
 * chain autocorrelate -> spatial_smooth(inputs, subarray_size, forward_backward) -> rootMUSIC_linear_array(norm_spacing,
 * num_targets, subarray_size), bit for bit.  work_dev_auto: K in the criterion stays snapshot_size, and d_eig_out is
 * subarray_size floats per item.  Choose subarray_size >= num_targets + 2 (with one noise vector the
 * smoothed polynomial's roots lie ON the unit circle). */
DOA_HIP_API int doa_root_pipeline_set_spatial_smoothing(doa_root_pipeline_t *h, int subarray_size, int forward_backward);

/* ---------------------------------------------------------------------------------------------
 * esprit_linear_array — least-squares ESPRIT for a uniform linear array: the grid-free estimate
 *   from the rotational invariance of the signal subspace; no polynomial, no search.  Not a block of the reference.
 *
 * The definition, one for every entry (tests/esprit_ref.py restates it in numpy):
 *   input item      column-major N x N gr_complex; only the upper triangle is read, of the diagonal only the real part, as
 *                   capon_lin_array reads it.  H = the Hermitian matrix these define.  All arithmetic in double;
 *                   d = (double)(float)norm_spacing.
 *   (w, V) = eigh(H), ascending, ranked by the eig_sym rule of the Jacobi kernels (ties: lower index first)
 *   Es     = the eigenvectors of the M largest eigenvalues                            (N x M, orthonormal)
 *   Es1    = rows 0 .. N-2 of Es,   Es2 = rows 1 .. N-1
 *   gamma  = 1 - sum_k |Es[N-1, k]|^2                (the smallest eigenvalue of Es1^H Es1 = I - e e^H, e = Es[N-1, :]^H)
 *   Psi    = (Es1^H Es1)^-1 Es1^H Es2                (M x M; evaluated as F + e (e^H F) / gamma, F = Es1^H Es2)
 *   lambda_k = the eigenvalues of Psi                (M = 1: Psi itself; M = 2: the stable quadratic; M >= 3: Householder
 *                                                     reduction to Hessenberg form, Wilkinson-shifted QR with deflation)
 *   c_k    = atan2(Im lambda_k, Re lambda_k) / (2 pi d)
 *   angle_k = (float)(180 / pi * acos(c_k)),  NaN when |c_k| > 1
 *   output item     M floats, ascending, NaN last.  There is no unit-circle filter (ESPRIT's eigenvalues straddle the circle).
 *                   With the steering a_n = exp(j 2 pi d cos(theta) (n - (N-1)/2)), a_{n+1} / a_n = exp(j 2 pi d cos(theta)):
 *                   the angle map of rootMUSIC_linear_array.
 *   status          int32 per item.  0 ok.  1 not solvable: trace(H) > 0 does not hold, an entry is not finite, or
 *                   gamma > DOA_ESPRIT_GAMMA_MIN does not hold (the relative error of Psi grows like eps / gamma: at 2^-30 a
 *                   double is left with float accuracy).  2 (counts entries): no usable count.  3: the eigenvalue iteration
 *                   reached its cap of 30 M QR steps.  A non-zero status gives an all-NaN item; other items are not affected.
 *   An item multiplied by a power of two gives the same bits (the Jacobi prescale is exact).  The result does not depend on
 *   the basis of the signal subspace, so the device and numpy agree to rounding, not bit for bit.
 *
 * Two launches: the double Jacobi eigen stage (4 lanes per item for N <= 4, 8 for N <= 8, one wave for N <= 16) writes the
 * SIGNAL-SUBSPACE RECORD -- all N eigenvectors as columns by descending eigenvalue, 2 N^2 doubles per item,
 * [2 (k N + row)] = Re, [.. + 1] = Im of component `row` of the k-th vector -- and esprit_kernel reads its first M columns.
 * Internal precision 64 only: a handle created while the process default is 32 returns DOA_ERR_UNSUPPORTED from its work
 * entries.  create validates before the device is touched: 2 <= num_ant_ele <= DOA_MAX_ANT_ELE, 1 <= num_targets <
 * num_ant_ele, 0 < norm_spacing <= 0.5.  status_out / d_status_out may be NULL.
 * The _counts entries take one int32 m_i per item in place of num_targets W; items stay W floats wide, with the semantics
 * of doa_rootMUSIC_linear_array_work_counts: 1 <= m_i <= min(W, num_ant_ele - 1): the first m_i slots are what
 * esprit_linear_array(norm_spacing, m_i, num_ant_ele) writes, bit for bit, the others NaN; m_i == 0: all NaN, status 0; any
 * other value (the -1 of source_count included): all NaN, status 2.  NULL counts: DOA_ERR_INVALID_ARG.
 * --------------------------------------------------------------------------------------------- */
#define DOA_ESPRIT_GAMMA_MIN (1.0 / 1073741824.0)   /* 2^-30, exact */
typedef struct doa_esprit_linear_array doa_esprit_linear_array_t;

DOA_HIP_API doa_esprit_linear_array_t *doa_esprit_linear_array_create(float norm_spacing, int num_targets, int num_ant_ele);
DOA_HIP_API void doa_esprit_linear_array_destroy(doa_esprit_linear_array_t *h);
DOA_HIP_API int doa_esprit_linear_array_work(doa_esprit_linear_array_t *h, int noutput_items, const void *cov_items,
                                             void *angles_out, void *status_out);
DOA_HIP_API int doa_esprit_linear_array_work_dev(doa_esprit_linear_array_t *h, int noutput_items, const void *d_cov_items,
                                                 void *d_angles_out, void *d_status_out, void *hip_stream);
DOA_HIP_API int doa_esprit_linear_array_work_counts(doa_esprit_linear_array_t *h, int noutput_items, const void *cov_items,
                                                    const void *counts, void *angles_out, void *status_out);
DOA_HIP_API int doa_esprit_linear_array_work_dev_counts(doa_esprit_linear_array_t *h, int noutput_items,
                                                        const void *d_cov_items, const void *d_counts, void *d_angles_out,
                                                        void *d_status_out, void *hip_stream);
/* root_pipeline with ESPRIT in place of Root-MUSIC: a per-handle setting, taking effect from the next work call, honoured by
 * work_dev, work_dev_batches, work, work_dev_auto and set_spatial_smoothing.  DOA_GRIDFREE_ROOT_MUSIC (the default) is the
 * path described above, unchanged.  DOA_GRIDFREE_ESPRIT: K1 runs exactly as before (d_cov_out is bit-identical), then the
 * eigen launch that writes the signal-subspace record (into the handle's workspace, one per lane), then esprit_kernel;
 * d_status_out carries the statuses of esprit_linear_array, and the host entry returns DOA_ERR_NUMERIC if any item has a
 * non-zero status.  work_dev_auto: K1, ONE estimating eigen launch that writes counts, eigenvalues and the record, the
 * counted ESPRIT kernel.  With smoothing on, eigen stage and ESPRIT run on subarray_size x subarray_size items.  The
 * outputs are bit-identical to the blocks chained by hand: autocorrelate -> [spatial_smooth ->] [source_count ->]
 * esprit_linear_array[_counts] -- with one limit: for num_ant_ele (or subarray_size) <= 4 work_dev_auto's estimating launch is
 * the 4-lanes-per-item Jacobi form while source_count runs one lane per item, a different sweep order, so d_eig_out agrees
 * with source_count's eigenvalues to one float rounding, not guaranteed bit for bit (the tested shape is bit-identical), and
 * -- an untested possibility -- a count could differ where the criterion is tied to that rounding; given the counts, angles
 * and status are bit-identical.  Above 4 elements both are the same launch.
 * Internal precision 32: DOA_ERR_UNSUPPORTED from the work entries while the mode is ESPRIT.
 * A bad value returns DOA_ERR_INVALID_ARG and leaves the handle as it was. */
#define DOA_GRIDFREE_ROOT_MUSIC 0
#define DOA_GRIDFREE_ESPRIT 1
DOA_HIP_API int doa_root_pipeline_set_estimator(doa_root_pipeline_t *h, int estimator);

/* ---------------------------------------------------------------------------------------------
 * compass_mean — blocks.vector_to_streams(float, num_streams) + the averaging of doa.compass
 *   (reference python/compass.py:134-136: next_angle = numpy.mean(input_items[0]) over the items of
 *   one work call; wiring apps/run_MUSIC_lin_array_simulation.py:199,236-239).
 *   input item = num_streams floats (port 1 of find_local_max); output = num_streams floats, the
 *   mean of each de-interleaved stream over the ninput_items items (NaN for 0 items, as numpy).
 *   Returns the number of items consumed (= ninput_items).  The compass GUI is out of scope.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_compass_mean doa_compass_mean_t;

DOA_HIP_API doa_compass_mean_t *doa_compass_mean_create(int num_streams);
DOA_HIP_API void doa_compass_mean_destroy(doa_compass_mean_t *h);
DOA_HIP_API int doa_compass_mean_work(doa_compass_mean_t *h, int ninput_items,
                                      const void *input_items0, float *next_angle);
DOA_HIP_API int doa_compass_mean_work_dev(doa_compass_mean_t *h, int ninput_items,
                                          const void *d_input_items0, float *d_next_angle,
                                          void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * phase_offset_est — doa.twinrx_phase_offset_est(num_ports, n_skip_ahead), the reference's hier block
 *   (python/twinrx_phase_offset_est.py:37-94): blocks.skiphead(n_skip_ahead) and blocks.complex_to_arg on each of the
 *   num_ports streams, then blocks.sub_ff(stream 0, stream p): num_ports - 1 float streams
 *       out_{p-1}[i] = atan2f(im x_0[i], re x_0[i]) - atan2f(im x_p[i], re x_p[i]),   p = 1 .. num_ports-1,
 *   one float subtraction, NOT wrapped into any interval: the values lie in (-2 pi, 2 pi) and take the two branches phi and
 *   phi -+ 2 pi of the offset phi, which is what the reference's savers are fed.  atan2f(0, 0) = 0; a sample with a NaN or
 *   Inf component gives NaN for that sample's outputs alone (not the limit atan2f defines for an infinite operand).  2 <= num_ports <= DOA_MAX_ANT_ELE, n_skip_ahead >= 0.
 *   The handle carries the skiphead state: the first n_skip_ahead samples it is ever given, over any number of calls to
 *   any of its entries, are dropped on every stream; doa_phase_offset_est_reset starts over.
 *   What is NOT parity: GNU Radio 3.7's complex_to_arg evaluates a table-driven fast arctangent of its own (not part of the
 *   gr-doa tree, not reproduced); this is the formula, each output within 4 * 2^-21 rad of its float64 evaluation.
 * Streaming form (the block as the flowgraph wires it): work consumes n_items samples per stream and writes
 *   n_items - (skip still owed) floats to each output, from index 0; returns that count (0 while the skip is being paid).
 *   input_items: num_ports streams (host array of pointers), output_items: num_ports - 1 float streams.
 * Fused form (the block and its saver in one pass; nothing is materialised): of the n_items samples given, drop what the
 *   skip still owes, take the first `samples` of the rest -- DOA_ERR_INVALID_ARG if fewer remain (the reference's savers
 *   get them through set_output_multiple) -- and write num_ports - 1 floats to each output that is not NULL:
 *     max_out[p-1]   the maximum of the streaming form's floats, bit for bit (numpy.amax: a NaN sticks).  What
 *                    findmax_and_save writes (python/findmax_and_save.py:66-78): of the two branches the maximum is the
 *                    one in [0, 2 pi).
 *     mean_out[p-1]  their mean, summed in double in a fixed order, rounded once.  What average_and_save writes
 *                    (python/average_and_save.py:68-80), its flaw included: when the difference crosses +-pi the two
 *                    branches are averaged and the number means nothing.
 *     circ_out[p-1]  arg(sum_i x_0[i] conj(x_p[i])), products and sum in double, rounded to float: in [-pi, pi].  Not in
 *                    the reference: the estimate that does not depend on the branch and that noise does not bias.
 *   Results are bit-identical from run to run, between the host and the device entry and for any stream alignment: the
 *   samples are summed in a partition that depends on `samples` alone.  Returns DOA_OK.
 * Device entries: device pointers (the pointer arrays themselves are host arrays), asynchronous on hip_stream; fc32 streams
 *   8-byte aligned (16-byte aligned streams take 16-byte loads when the skip leaves them so), sc16 4 / 8.  The layout
 *   advice of doa_stream_stride_bytes applies: every wave reads the same sample range of all streams.  The host estimate
 *   entry stages ~32 MiB of samples per copy.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_phase_offset_est doa_phase_offset_est_t;

DOA_HIP_API doa_phase_offset_est_t *doa_phase_offset_est_create(int num_ports, int n_skip_ahead);
DOA_HIP_API void doa_phase_offset_est_destroy(doa_phase_offset_est_t *h);
/* Forget the samples skipped so far: the next n_skip_ahead samples are dropped again. */
DOA_HIP_API int doa_phase_offset_est_reset(doa_phase_offset_est_t *h);
/* Input sample format of the streams: exactly the contract of doa_autocorrelate_set_input_format (sc16 widened in
 * registers, no fc32 copy made, every output of both forms bit-identical to the fc32 path's on float(q) * scale). */
DOA_HIP_API int doa_phase_offset_est_set_input_format(doa_phase_offset_est_t *h, int format, float scale);
DOA_HIP_API int doa_phase_offset_est_work(doa_phase_offset_est_t *h, int n_items, const void *const *input_items,
                                          void *const *output_items);
DOA_HIP_API int doa_phase_offset_est_work_dev(doa_phase_offset_est_t *h, int n_items, const void *const *d_input_items,
                                              void *const *d_output_items, void *hip_stream);
DOA_HIP_API int doa_phase_offset_est_estimate(doa_phase_offset_est_t *h, long long n_items,
                                              const void *const *input_items, long long samples, float *mean_out,
                                              float *max_out, float *circ_out);
DOA_HIP_API int doa_phase_offset_est_estimate_dev(doa_phase_offset_est_t *h, long long n_items,
                                                  const void *const *d_input_items, long long samples,
                                                  float *d_mean_out, float *d_max_out, float *d_circ_out,
                                                  void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * calib_mean — the reduction of doa.save_antenna_calib (python/save_antenna_calib.py:61-69): two inputs of n_items items
 *   of num_inputs floats each (magnitude and phase of the estimated antenna responses; wiring
 *   apps/run_calib_lin_array_simulation.grc: autocorrelate -> calibrate_lin_array -> complex_to_magphase -> here);
 *   gain_out[m] / phase_out[m] = mean over ALL n_items items of component m (the reference's numpy.mean(G[m::num_inputs])),
 *   summed in double in a fixed order and rounded once (numpy's float32 pairwise mean differs by a few ulp); NaN for 0 items.
 *   The complex form takes calibrate_lin_array's output items (num_inputs gr_complex each) and forms |c| and
 *   atan2f(im, re) itself, so the chain stays on the device.  No handle: the host entries stage through buffers of their
 *   own.  Return n_items or a negative doa_status.
 * --------------------------------------------------------------------------------------------- */
DOA_HIP_API int doa_calib_mean_work(int n_items, int num_inputs, const float *mag_in, const float *phase_in,
                                    float *gain_out, float *phase_out);
DOA_HIP_API int doa_calib_mean_work_dev(int n_items, int num_inputs, const float *d_mag_in, const float *d_phase_in,
                                        float *d_gain_out, float *d_phase_out, void *hip_stream);
DOA_HIP_API int doa_calib_mean_complex_work(int n_items, int num_inputs, const void *c_in, float *gain_out,
                                            float *phase_out);
DOA_HIP_API int doa_calib_mean_complex_work_dev(int n_items, int num_inputs, const void *d_c_in, float *d_gain_out,
                                                float *d_phase_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * The calibration files, written.  No device needed.
 *   doa_write_phase_config   the file doa.phase_correct_hier reads (python/phase_correct_hier.py:33-45) and
 *                            findmax_and_save / average_and_save write (python/findmax_and_save.py:66-78): n lines, one
 *                            value each.
 *   doa_write_antenna_calib  the file doa_antenna_correction_create reads (lib/antenna_correction_impl.cc:56-73) and
 *                            save_antenna_calib writes (python/save_antenna_calib.py:61-72): n lines "gain phase".
 * The file is truncated; every float is printed with nine significant digits, so it parses back to the same float32
 * (the reference prints Python's str() of a numpy float).  A value of 0 is written like any other, although the reference's
 * phase-file reader drops such a line.  Returns DOA_OK, or DOA_ERR_INVALID_ARG with the reference's message in
 * doa_last_error(): "Configuration <name>, not writable" (phase file) / "Configuration <name>, not valid" (antenna file).
 * --------------------------------------------------------------------------------------------- */
DOA_HIP_API int doa_write_phase_config(const char *filename, const float *values, int n);
DOA_HIP_API int doa_write_antenna_calib(const char *filename, const float *gains, const float *phases, int n);

/* ---------------------------------------------------------------------------------------------
 * Snapshots of bins — what channel_covariance writes and wideband_music, focus_covariance and doa_rss_focusing_matrices
 *   read.  The four sections below refer to this paragraph (the library states it once, in csrc/bin_plan.hpp).
 *   Item order: a snapshot is nb covariance items, one per selected frequency bin; a call of n snapshots is n * nb
 *   column-major N x N gr_complex items, item i nb + j = bin j of snapshot i.  Per-bin weights and counts are n x nb in the
 *   same order.
 *   Selection: fft_len F, first_bin and num_bins nb with 0 <= first_bin < F and 1 <= nb <= F; item j is FFT bin
 *   f_j = (first_bin + j) mod F, so a selection may wrap past F - 1.  Bins are in natural FFT order: bin f is f / F cycles
 *   per sample, bins >= F / 2 are negative frequencies.
 *   Allowed fft_len: 16, 32, 64, 128 or 256.
 *   Used bins: with weights w_ij (optional, NULL = all ones) bin j of snapshot i is USED when 0 < w_ij < +inf.  The item of
 *   a bin that is not used is not read: it may hold anything, NaN included, and does not change a bit of the output.
 *   Call size: n * nb must not exceed INT_MAX; a larger call is refused with DOA_ERR_INVALID_ARG.
 * --------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * channel_covariance — one covariance per snapshot AND frequency bin (the Welch / Bartlett cross-spectral matrix): the
 *   front end for several narrowband emitters at different frequencies inside one captured band, which the whole-band
 *   covariance of autocorrelate mixes (an N-element array separates at most N - 1 of them).  Every (snapshot, bin) matrix
 *   is an ordinary covariance item: MUSIC_lin_array, capon_*, rootMUSIC_linear_array, esprit_linear_array, source_count,
 *   spatial_smooth and the array blocks take the noutput_items * num_bins items as they are.  Not a block of the reference.
 * The definition, one for every entry (tests/channel_covariance_ref.py restates it in numpy).  inputs N, snapshot_size K,
 *   fft_len F, window w (F floats, NULL = all ones), B = K / F blocks per snapshot; snapshot i starts at sample
 *   s_i = i (K - overlap_size) exactly as in autocorrelate, block b covers samples [bF, bF + F) of it:
 *       X[a,b,f]   = sum_t w[t] x_a[s_i + bF + t] exp(-2 pi i f t / F)
 *       R_i,f[p,q] = 1 / (B W2) sum_b X[p,b,f] conj(X[q,b,f]),      W2 = sum_t w[t]^2  (double, from the float32 w)
 *   so white noise of variance s^2 gives a diagonal of s^2 in every bin for any window, and with the rectangular window
 *   the mean of R_i,f over the F bins is the autocorrelate covariance (avg_method 0).  A bin's matrix has rank <= B.
 *   Arithmetic is float: widened sample x window, float radix-2 FFT with twiddles rounded from double, float accumulation
 *   over the blocks in block order, ONE final multiply by (float)(1 / (B W2)).  The result is exactly Hermitian (the lower
 *   triangle is the bitwise conjugate of the upper one, diagonal imaginary parts are +0), has no atomics in it and does
 *   not depend on noutput_items or on the item's position in the call.
 * Layouts: input_items as autocorrelate (and its set_input_format contract, sc16 bit-identical to fc32 on the widened
 *   samples).  out_cov = noutput_items snapshots of num_bins bins ("Snapshots of bins" above: item order and selection).
 *   out_power (optional, may be NULL) = noutput_items x F floats, ALWAYS all F bins in natural
 *   order whatever the selection: power[i,f] = the float sum over p = 0..N-1, in that order, of the real diagonal of R_i,f
 *   -- 4 F bytes per snapshot to find the occupied bins with.
 * create validates before the device is looked for: 1 <= inputs <= 8 (9..16: not built into this library), an allowed
 *   fft_len, snapshot_size a positive multiple of fft_len, 0 <= overlap_size < snapshot_size, a finite window with W2 > 0.
 *   set_bins takes a selection; the default is all F bins; a refused call returns DOA_ERR_INVALID_ARG and leaves the handle
 *   as it was.  Downstream cost scales with num_bins.
 * work_dev queues on the caller's stream and does nothing else.  Device streams aligned to two samples with an even
 *   snapshot_size - overlap_size take 16-byte (sc16: 8-byte) loads, any other stream aligned to one sample the scalar-load
 *   route; both do the same arithmetic in the same order.  The host work returns with its stream synchronised whether it
 *   worked or not.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_channel_covariance doa_channel_covariance_t;

DOA_HIP_API doa_channel_covariance_t *doa_channel_covariance_create(int inputs, int snapshot_size, int overlap_size,
                                                                    int fft_len, const float *window);
DOA_HIP_API void doa_channel_covariance_destroy(doa_channel_covariance_t *h);
/* history, forecast and input_span: the formulas of autocorrelate */
DOA_HIP_API int doa_channel_covariance_history(const doa_channel_covariance_t *h);
DOA_HIP_API int doa_channel_covariance_forecast(const doa_channel_covariance_t *h, int noutput_items);
DOA_HIP_API long long doa_channel_covariance_input_span(const doa_channel_covariance_t *h, int noutput_items);
DOA_HIP_API int doa_channel_covariance_set_input_format(doa_channel_covariance_t *h, int format, float scale);
DOA_HIP_API int doa_channel_covariance_set_bins(doa_channel_covariance_t *h, int first_bin, int num_bins);
DOA_HIP_API int doa_channel_covariance_num_bins(const doa_channel_covariance_t *h);
/* noutput_items counts snapshots */
DOA_HIP_API int doa_channel_covariance_work(doa_channel_covariance_t *h, int noutput_items,
                                            const void *const *input_items, void *out_cov, float *out_power);
DOA_HIP_API int doa_channel_covariance_work_dev(doa_channel_covariance_t *h, int noutput_items,
                                                const void *const *d_input_items, void *d_out_cov, void *d_out_power,
                                                void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * wideband_music — incoherent wideband MUSIC on a uniform linear array (Wax, Shan and Kailath 1984): ONE spectrum per
 *   snapshot from the covariance items of all its frequency bins, for an emitter that fills many bins (a modem, a radar,
 *   a noise source).  Every bin gets its own noise subspace and a steering vector at that bin's own element spacing in
 *   wavelengths, and the null spectra are combined over the bins.  The chain is channel_covariance -> [source_count ->]
 *   wideband_music -> find_local_max.  Not a block of the reference.
 * The definition, one for every entry (tests/wideband_ref.py restates it in numpy).
 *   Parameters: norm_spacing d (the spacing in wavelengths AT THE CARRIER, held as float32 as in MUSIC_lin_array),
 *   num_targets M, num_ant_ele N, pspectrum_len P; fft_len F, first_bin, num_bins nb: the selection the items were made
 *   with ("Snapshots of bins" above; f_j is the bin of item j);
 *   rate_over_carrier rho = sample rate / carrier frequency (0: every bin at the carrier's spacing); combine.
 *       nu_f     = f / F for f < F/2, else f / F - 1          (numpy.fft.fftfreq, channel_covariance's bin frequencies)
 *       d_f      = double(float(d)) (1 + nu_f rho)            the element spacing in wavelengths at bin f
 *       psi_j,p  = -2 pi cos(theta_p) d_fj                    theta: the float-accumulated grid of MUSIC_lin_array
 *       Q_ij(p)  = Re(a^H P_N a),  a_n = exp(i psi_j,p (N - 1 - 2n) / 2),  P_N = the noise projector of item (i, j) for M
 *                  sources (the *_counts entries: for the item's own count c_ij); everything but theta in double.
 *   A bin is USED by the rule of "Snapshots of bins" and, in the *_counts entries, when also 1 <= c_ij <= N - 1.  A bin
 *   whose weight is not usable is skipped whatever its count; with a usable weight a count of 0 skips the bin and any other
 *   count outside 1..N-1 gives the snapshot status 2.  Combined in double over the used bins in item order:
 *       DOA_WIDEBAND_NULL_MEAN   Q_i(p) = sum_j w_ij Q_ij(p) / sum_j w_ij          for sources that occupy every used bin
 *       DOA_WIDEBAND_POWER_SUM   Q_i(p) = sum_j w_ij / sum_j (w_ij / Q_ij(p))      for bins that hold different sources
 *   (the mean of the null spectra is tilted by bins that hold only some of the sources; the sum of the pseudo-spectra
 *   1 / Q_ij is ruled by its luckiest bin when all bins hold the same sources.)
 *   Output: q = (float) Q_i(p); the row is 10 log10(out / max out), out = 1 / q, with MUSIC_lin_array's normalisation and
 *   tie rule, so the maximum is exactly 0 dB and find_local_max follows unchanged.
 *   Status (optional port, one int32 per snapshot): 0 ok; 1 no bin used; 2 a count outside 0..N-1; 3 the coefficient record
 *   of a used bin is not finite (2 wins over 3).  A status other than 0 gives an all-NaN row (and q row) and leaves the
 *   other snapshots as they are.  A row does not depend on noutput_items, on the snapshot's position in the call or on its
 *   neighbours.
 * create validates before the device is looked for: 0 < M < N <= DOA_MAX_ANT_ELE, 0 < d <= 0.5, 1 <= P <= 16384, an allowed
 *   fft_len, a selection inside it, rho finite and >= 0, every selected bin's d_f in (0, 0.5] (the message names the
 *   bin), combine 0 or 1.  doa_wideband_bin_spacing is d_f itself (pure, no device; NaN for a bin outside
 *   0..F-1).
 * noutput_items counts snapshots (the call-size limit applies).  cov_items: noutput_items snapshots of nb bins; counts:
 *   noutput_items * nb int32.  work_dev is two launches on the caller's stream, the eigen stage of MUSIC_lin_array over all items and one
 *   scan that evaluates all bins of a snapshot in registers; d_q_out (optional): q, P floats per snapshot.  Internal
 *   precision 64 only: a handle created while the process default is 32 returns DOA_ERR_UNSUPPORTED from its work entries.
 *   The host work returns with its stream synchronised whether it worked or not.
 * --------------------------------------------------------------------------------------------- */
#define DOA_WIDEBAND_NULL_MEAN 0
#define DOA_WIDEBAND_POWER_SUM 1
typedef struct doa_wideband_music doa_wideband_music_t;

DOA_HIP_API doa_wideband_music_t *doa_wideband_music_create(float norm_spacing, int num_targets, int num_ant_ele,
                                                            int pspectrum_len, int fft_len, int first_bin, int num_bins,
                                                            double rate_over_carrier, int combine);
DOA_HIP_API void doa_wideband_music_destroy(doa_wideband_music_t *h);
DOA_HIP_API long long doa_wideband_music_items_total(const doa_wideband_music_t *h);
DOA_HIP_API int doa_wideband_music_work(doa_wideband_music_t *h, int noutput_items, const void *cov_items,
                                        const float *weights, void *spectrum_out, void *status_out);
DOA_HIP_API int doa_wideband_music_work_dev(doa_wideband_music_t *h, int noutput_items, const void *d_cov_items,
                                            const void *d_weights, void *d_spectrum_out, void *d_q_out,
                                            void *d_status_out, void *hip_stream);
DOA_HIP_API int doa_wideband_music_work_counts(doa_wideband_music_t *h, int noutput_items, const void *cov_items,
                                               const void *counts, const float *weights, void *spectrum_out,
                                               void *status_out);
DOA_HIP_API int doa_wideband_music_work_dev_counts(doa_wideband_music_t *h, int noutput_items, const void *d_cov_items,
                                                   const void *d_counts, const void *d_weights, void *d_spectrum_out,
                                                   void *d_q_out, void *d_status_out, void *hip_stream);
DOA_HIP_API double doa_wideband_bin_spacing(float norm_spacing, double rate_over_carrier, int fft_len, int bin);

/* ---------------------------------------------------------------------------------------------
 * focus_covariance — coherent wideband focusing (the coherent signal-subspace method, CSSM: Wang and Kaveh 1985): ONE
 *   focused covariance item per snapshot from the covariance items of all its frequency bins.  Where wideband_music keeps
 *   one subspace per bin, a focusing matrix T_j per bin maps the bin's steering vectors onto the carrier's, and the
 *   transformed items are averaged.  A source and its echo are rank one in every bin (no per-bin estimator can separate
 *   them), but the echo's phase turns across the band, so the average has rank two.  The output is an ordinary covariance
 *   item: MUSIC_lin_array, capon_lin_array, rootMUSIC_linear_array, esprit_linear_array, source_count, spatial_smooth and
 *   find_local_max follow unchanged, over n items instead of n * nb.  The chain is channel_covariance -> focus_covariance ->
 *   any of them.  Not a block of the reference.
 * The definition, one for every entry (tests/focus_ref.py restates it in numpy).  Snapshot i, bins j < nb, items R_ij and
 *   optional weights w_ij in the item order of "Snapshots of bins" above, its used-bin rule, the handle's table of nb
 *   matrices T_j (N x N complex double):
 *       R_i     = sum_{j used} w_ij T_j H(R_ij) T_j^H / sum_{j used} w_ij
 *   H(R) is R's upper triangle with the real part of its diagonal, completed Hermitian: what the eigen stage and
 *   spatial_smooth read; the lower triangle and the diagonal's imaginary parts may hold anything.  The arithmetic is in
 *   double and the result is rounded once to gr_complex.  The output is exactly Hermitian: the imaginary parts on the
 *   diagonal are +0.0 and out[b,a] is bit for bit the conjugate of out[a,b].
 *   Status (optional port, one int32 per snapshot, wideband_music's numbers): 0 ok; 1 no bin used; 3 a used bin's item (the
 *   part H reads) is not finite.  A status other than 0 gives an all-NaN item and leaves the other snapshots as they are; a
 *   NaN item is never an error return.  A snapshot's output bits do not depend on noutput_items, on its position in the
 *   call or on the stream.
 * TABLE LAYOUT: matrices[(j N + a) N + b] = T_j[a][b], ROW-MAJOR per matrix, re then im (numpy: a C-ordered [nb, N, N]
 *   complex128 array).  The table belongs to the handle, not to a snapshot: it is uploaded once at create.
 * create validates before the device is looked for: 2 <= N <= DOA_MAX_ANT_ELE, 1 <= nb <= 256 (channel_covariance's
 *   largest fft_len), matrices not NULL and every entry finite.  A table need NOT be unitary (a measured or otherwise
 *   non-unitary focusing table is the caller's business), but MUSIC, Root-MUSIC, ESPRIT and MDL behind the block assume
 *   white noise, which only a unitary T keeps white.
 * noutput_items counts snapshots (the call-size limit applies): the input is noutput_items * nb items, the output
 *   noutput_items items.  work_dev is one
 *   launch on the caller's stream.  d_out must not overlap d_cov_items (not checked).  Internal precision 64 only: a handle
 *   created while the process default is 32 returns DOA_ERR_UNSUPPORTED from its work entries.  The host work returns with
 *   its stream synchronised whether it worked or not.
 *
 * doa_rss_focusing_matrices (pure, no device) builds the table for a uniform linear array by rotational-signal-subspace
 *   focusing (Hung and Kaveh 1988), regularised so that it is unique.  With J = n_focus focus angles theta_k (degrees),
 *   A_d[n][k] = exp(i psi_k (N - 1 - 2n) / 2), psi_k = -2 pi cos(theta_k) d (wideband_music's steering vector),
 *   d_0 = double(float(norm_spacing)) and d_j = doa_wideband_bin_spacing of bin f_j of the selection:
 *       B_j = A_{d_0} A_{d_j}^H + regularization J I
 *       T_j = the unitary polar factor of B_j (U V^H of its singular value decomposition)
 *   which is the unitary T that minimises |A_{d_0} - T A_{d_j}|^2 + regularization J |I - T|^2 (Frobenius norms).  Without
 *   the second term fewer angles than elements leave T arbitrary on the complement of the steering vectors; with it the
 *   carrier's bin gives the identity.  The polar factor is found by the scaled Newton iteration X <- (g X + (g X)^-H) / 2.
 *   Refused (DOA_ERR_INVALID_ARG, doa_last_error says why): N outside 2..DOA_MAX_ANT_ELE, norm_spacing outside (0, 0.5],
 *   an fft_len that is not allowed, a selection outside it, rate_over_carrier not finite or < 0, n_focus < 1, an angle that
 *   is not finite, a selected bin whose d_j is outside (0, 0.5] (the message names the bin), regularization not positive
 *   and finite, NULL pointers.  matrices_out: nb N N complex doubles in the table layout above.
 *   Choosing the angles: a fan over the field of view (as many as elements) for a first pass; then the first pass's
 *   estimates and a few degrees either side of each.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_focus_covariance doa_focus_covariance_t;

DOA_HIP_API int doa_rss_focusing_matrices(float norm_spacing, int num_ant_ele, int fft_len, int first_bin, int num_bins,
                                          double rate_over_carrier, int n_focus, const double *focus_angles_deg,
                                          double regularization, double *matrices_out);
DOA_HIP_API doa_focus_covariance_t *doa_focus_covariance_create(int num_ant_ele, int num_bins, const double *matrices);
DOA_HIP_API void doa_focus_covariance_destroy(doa_focus_covariance_t *h);
DOA_HIP_API long long doa_focus_covariance_items_total(const doa_focus_covariance_t *h);
DOA_HIP_API int doa_focus_covariance_work(doa_focus_covariance_t *h, int noutput_items, const void *cov_items,
                                          const float *weights, void *focused_items, void *status_out);
DOA_HIP_API int doa_focus_covariance_work_dev(doa_focus_covariance_t *h, int noutput_items, const void *d_cov_items,
                                              const void *d_weights, void *d_focused_items, void *d_status_out,
                                              void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * coarray_covariance — the difference co-array of a SPARSE linear array (minimum-redundancy, nested, coprime): more
 *   sources than antennas.  Every estimator here needs num_targets < num_ant_ele.  With the N elements at integer
 *   positions p_n (in units of norm_spacing) the covariance of uncorrelated sources depends on the lag p_a - p_b alone,
 *   and a sparse array holds many more lags than elements: 0, 1, 4, 6 holds every lag 0..6.  Averaging the entries of
 *   equal lag into a Hermitian Toeplitz matrix T of size Lv and squaring it gives the spatially smoothed co-array matrix
 *   (Pal and Vaidyanathan 2010; = T^2 / Lv: Liu and Vaidyanathan 2015), which is the covariance item of a VIRTUAL
 *   Lv-element uniform array: MUSIC_lin_array(d, M, Lv, P), rootMUSIC_linear_array, esprit_linear_array and
 *   find_local_max follow unchanged, with M up to Lv - 1.  The chain is autocorrelate -> coarray_covariance -> any of them.
 *   Not a block of the reference.
 * positions: N distinct integers in any order, 2 <= N <= DOA_MAX_ANT_ELE, max - min <= 255.  positions[n] is the
 *   position of stream n, counted as MUSIC_lin_array numbers its elements (element n of its uniform array is position n).
 *   lag(a, b) = positions[a] - positions[b];  c_l = the number of ordered pairs with lag l;  Lc (the contiguous size) = the
 *   largest L such that every lag 0..L-1 occurs.  virtual_size Lv: 0 means min(Lc, DOA_MAX_ANT_ELE), otherwise
 *   2 <= Lv <= that value.  Lags beyond the first hole are not used.
 * The definition, one for every entry (tests/coarray_ref.py restates it in numpy):
 *   input item   column-major N x N gr_complex, as spatial_smooth takes it; ONLY THE UPPER TRIANGLE IS READ, and of the
 *                diagonal the real part: H = the Hermitian matrix these define
 *   output item  column-major Lv x Lv gr_complex, full and EXACTLY Hermitian: out[j,i] is bit for bit conj(out[i,j]) and
 *                the diagonal's imaginary part is +0.0
 *   for l = 0 .. Lv-1:
 *     s[l] = sum (double) H[a,b] over the pairs with lag(a,b) = l,
 *            ascending column b, then ascending row a; re and im separately; l = 0: real parts only
 *     r[l] = s[l] * (1.0 / c_l)                      1.0 / c_l formed in double; r stays in double
 *   T[i,j] = r[i-j] for i >= j, conj(r[j-i]) for i < j                    (row i, column j)
 *   DOA_COARRAY_TOEPLITZ:  out[i,j] = (float) T[i,j]
 *   DOA_COARRAY_SMOOTHED:  out[i,j] = (float)( (sum_k T[i,k] conj(T[j,k])) * (1.0 / Lv) ),  i <= j, in double; the
 *                          mirror conjugated
 *   In TOEPLITZ mode no product feeds an addition, so an implementation that does these operations in this order is
 *   bit-identical to the numpy statement; the device kernel is, for either pointer alignment and any batch size.  In
 *   SMOOTHED mode the order of the sum over k is free; every component is within 2^-23 of the item's largest component
 *   of the double result.  With positions 0..N-1 and an exactly Toeplitz input TOEPLITZ mode returns the input.
 *   Non-finite entries propagate by IEEE rules within their item; there is no status output.
 * WHICH MODE.  SMOOTHED (the default) is positive semidefinite and is what MUSIC, Root-MUSIC and ESPRIT should read.
 *   Its eigenvalues are the SQUARES of T's: source_count's MDL / AIC are not valid on it, and its float storage has half
 *   the dynamic range in dB.  TOEPLITZ keeps the eigenvalues unsquared but can be indefinite at finite snapshot counts;
 *   it is for callers that know that.  An order estimator for co-array items is not provided.
 * create validates before the device is looked for and says what is wrong (doa_last_error).  output_items must NOT overlap
 *   cov_items (not checked).  work_dev is one launch on the caller's stream; it takes 16-byte loads and stores when both
 *   pointers are 16-byte aligned and 8-byte ones otherwise (gr_complex alignment is the minimum): the same bits either way.
 * doa_coarray_lags (pure, no device): *contiguous_size = Lc of a layout, and counts[l] = c_l for l < Lc if counts is not
 *   NULL (the caller provides Lc entries: call once with NULL to learn Lc; Lc <= 256).  Array designers check a layout
 *   with it.  DOA_ERR_INVALID_ARG for NULL positions or contiguous_size, n < 1, n > DOA_MAX_ANT_ELE, duplicates or a span
 *   above 255.
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_coarray_covariance doa_coarray_covariance_t;
#define DOA_COARRAY_SMOOTHED 0
#define DOA_COARRAY_TOEPLITZ 1

DOA_HIP_API int doa_coarray_lags(const int *positions, int n, int *contiguous_size, int *counts);
DOA_HIP_API doa_coarray_covariance_t *doa_coarray_covariance_create(const int *positions, int num_ant_ele, int virtual_size,
                                                                    int mode);
DOA_HIP_API void doa_coarray_covariance_destroy(doa_coarray_covariance_t *h);
DOA_HIP_API int doa_coarray_covariance_virtual_size(const doa_coarray_covariance_t *h);
DOA_HIP_API int doa_coarray_covariance_work(doa_coarray_covariance_t *h, int noutput_items, const void *cov_items,
                                            void *output_items);
DOA_HIP_API int doa_coarray_covariance_work_dev(doa_coarray_covariance_t *h, int noutput_items, const void *d_cov_items,
                                                void *d_output_items, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * sim_source — the signal front end of the simulation flowgraphs as one generator
 *   (reference apps/run_MUSIC_lin_array_simulation.py:66-74 array manifold, :204-210 sig_source_c +
 *   noise_source_c per source -> add -> multiply_matrix_cc):
 *     x_n[t] = sum_m A[n][m] (tone_ampl[m] e^{j 2 pi tone_freq[m] t} + source_noise_ampl[m] (g + j g'))
 *              + antenna_noise_sigma (g + j g') / sqrt(2)
 *   tone_freq in cycles per sample; tone_ampl / source_noise_ampl may be NULL (1 / 0).  Noise is
 *   Philox4x32-10 keyed by `seed` (counter = sample-pair index and noise stream), so sample ranges
 *   are reproducible independently of call boundaries; it is not GNU Radio's generator.
 *   work produces the next noutput_items samples of the num_ant_ele output streams (complex64 each);
 *   every call except the last of a run must ask for an even number (seek positions are even).
 * --------------------------------------------------------------------------------------------- */
typedef struct doa_sim_source doa_sim_source_t;

DOA_HIP_API doa_sim_source_t *doa_sim_source_create(int num_ant_ele, int num_sources,
                                                    float norm_spacing, const float *theta_deg,
                                                    const double *tone_freq, const float *tone_ampl,
                                                    const float *source_noise_ampl,
                                                    float antenna_noise_sigma,
                                                    unsigned long long seed);
DOA_HIP_API void doa_sim_source_destroy(doa_sim_source_t *h);
DOA_HIP_API int doa_sim_source_seek(doa_sim_source_t *h, long long sample_index);
DOA_HIP_API long long doa_sim_source_tell(const doa_sim_source_t *h);
DOA_HIP_API int doa_sim_source_work(doa_sim_source_t *h, int noutput_items,
                                    void *const *output_items);
DOA_HIP_API int doa_sim_source_work_dev(doa_sim_source_t *h, int noutput_items,
                                        void *const *d_output_items, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DOA_HIP_H */
