/*
 * slm_hip.h — C-ABI of libslm_hip.so, the MI355X (gfx950) hot path of the
 * Gerchberg–Saxton / gradient-descent hologram loops.
 *
 * Reference interfaces replaced (pranislav/Spatial_Light_Modulator_Module,
 * snapshot 2024-10-08; the reference is pure Python and has no FFI, so these
 * are the entry points a ctypes binding of that path binds — see
 * INTEGRATION.md):
 *   slm_gs / slm_plan_* with SLM_ALGO_GS  -> gerchberg_saxton(demanded_output, args)
 *                                            src/algorithms.py:10-49
 *   slm_gd / slm_plan_* with SLM_ALGO_GD  -> gradient_descent(demanded_output, args)
 *                                            src/algorithms.py:60-112 (+ error_f :161,
 *                                            dEdX_complex :179, make_initial_guess
 *                                            "fourier" :153-156)
 *   slm_fft2                              -> scipy.fft.fft2 / ifft2 as called at
 *                                            src/algorithms.py:27,31,34,84,88 (unscaled)
 *   slm_gsw / slm_plan_* with SLM_ALGO_GSW -> no reference counterpart: GS with Di Leonardo's
 *                                            per-pixel weight feedback, an addition next to
 *                                            the drop-in (see "weighted GS" below).
 *   slm_plan_* with SLM_ALGO_MRAF         -> no reference counterpart: GS with a signal region
 *                                            (mixed-region amplitude freedom) for extended,
 *                                            flat shapes (see "MRAF" below).
 *   slm_spots_*                           -> no reference counterpart: weighted GS on a list
 *                                            of traps (fractional positions, defocus, any
 *                                            panel shape; see "trap lists" below).
 *   slm_farfield_zoom                     -> no reference counterpart: the far field of any
 *                                            hologram or SLM frame on a fractional grid (see
 *                                            "zoomed far field" below).
 *   slm_comm_* / slm_plan_gather_phase    -> no reference counterpart: the batch
 *                                            loop of src/generate_hologram_sequence.py:19-31
 *                                            sharded over GPUs, phases gathered over RCCL.
 *
 * Conventions: plain pointers and sizes, C-contiguous row-major host arrays,
 * complex values interleaved (re, im) float32. The caller owns host buffers;
 * the library owns device buffers. Every function returns 0 on success or a
 * negative code; slm_last_error() describes the last failure of the calling
 * thread. Nothing here falls back to the CPU: without a usable gfx950 device
 * every compute entry point fails.
 */
#ifndef SLM_HIP_H
#define SLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLM_ALGO_GS 0
#define SLM_ALGO_GD 1
/* weighted Gerchberg-Saxton (uniform trap intensities); no reference counterpart, see below */
#define SLM_ALGO_GSW 2
/* mixed-region amplitude freedom (smooth extended shapes); no reference counterpart, see below */
#define SLM_ALGO_MRAF 3

#define SLM_TGT_U8 0  /* uint8 target; amplitude = float16(sqrt(T)) as numpy does */
#define SLM_TGT_F32 1 /* float32 target; amplitude = sqrtf(T) */

/* arithmetic precision of the transforms (state is complex64 in HBM either way) */
#define SLM_PRECISION_F32 0 /* float32 butterflies and twiddles (default; $SLM_PRECISION=f64 overrides) */
#define SLM_PRECISION_F64 1 /* float64 butterflies and twiddles */

/* kernel classes for timing / roofline queries */
#define SLM_KERNEL_COL_MAIN 0 /* GS / weighted-GS column pass, or GD column pass (fused statistics + gradient, or the gradient launch) */
#define SLM_KERNEL_ROW_MAIN 1 /* GS / GD fused row pass */
#define SLM_KERNEL_GD_STATS 2 /* GD statistics column pass */
#define SLM_KERNEL_OTHER 3    /* setup, phase extraction, reductions */
#define SLM_NUM_KERNEL_CLASSES 4

#define SLM_ERR_ARG (-1)
#define SLM_ERR_HIP (-2)
#define SLM_ERR_UNSUPPORTED (-3)
#define SLM_ERR_STATE (-4)
#define SLM_ERR_COMM (-5)

typedef struct slm_plan slm_plan;

/* ---- library ---------------------------------------------------------- */
int slm_init(int device);            /* select the GPU of this process */
int slm_device_count(void);
const char* slm_last_error(void);
const char* slm_version(void);
int slm_supported_length(int n);    /* 1 if n is a supported row/column length */
/* PCI bus id ("0000:05:00.0") of a HIP device: which GPU a rank ran on */
int slm_device_pci_bus_id(int device, char* buf, int len);
/* Measured streaming-copy rate (read + write bytes / s, in GB/s) of two
 * `bytes`-sized device buffers on the current device, `reps` timed copies
 * (16 B per lane, grid-stride): the practical peak next to the 8 TB/s spec
 * (SURVEY.md 8d asks for a measured copy-kernel peak). */
int slm_copy_bandwidth(long long bytes, int reps, double* gbs);

/* ---- plans: device-resident batches ------------------------------------
 * A plan holds `batch` holograms of height x width on the current device.
 * Upload once, run many times (bench), read results.
 * GD plans run their column side as one launch that waits for the hologram's
 * max |F|^2 across workgroups when the whole column grid is resident at once
 * (float32, unchecked runs), else as two launches; $SLM_GD_MODE=auto|fused|
 * two|lin at plan creation picks one ($SLM_GD_FUSE=0 = two). If the one-launch
 * wait ever gives up (other work on the device broke co-residency),
 * slm_plan_sync / slm_plan_read / slm_plan_run_timed redo that run in-process
 * on the two-launch path and the plan keeps that path: the caller sees
 * results, never the fault (slm_plan_gd_recoveries counts such reruns).    */
int slm_plan_create(int algo, int batch, int height, int width, int tgt_type, int has_ain, int max_loops,
                    slm_plan** out);
int slm_plan_destroy(slm_plan* plan);
/* targets [batch][height][width] of tgt_type; norm = max(T) and sum(T^2) are
 * reduced on the device */
int slm_plan_set_target(slm_plan* plan, const void* tgt);
int slm_plan_set_precision(slm_plan* plan, int precision);       /* SLM_PRECISION_* */
int slm_plan_get_precision(slm_plan* plan);
int slm_plan_set_ain(slm_plan* plan, const float* ain);           /* [height][width] sqrt(incoming intensity) */
int slm_plan_set_phase(slm_plan* plan, const float* phase);       /* GS warm start [batch][h][w]; NULL = cold */
int slm_plan_set_field(slm_plan* plan, const float* field_re_im); /* GD initial x [batch][h][w][2]; NULL = fourier */
int slm_plan_set_lr(slm_plan* plan, const float* lr);             /* GD learning rate per iteration [max_loops] */
/* ---- weighted GS (SLM_ALGO_GSW): no reference counterpart ----------------
 * Per hologram, with the support sup = T > 0, weights g (ones, or the caller's)
 * and the feedback exponent p >= 0, every GS iteration additionally does
 *     on sup where |C| > 0:  g *= (a_T / |C|)^p;   D = a_T g C/|C|
 * (a_T, the start, E, the statistics and the stop test as GS defines them; p = 0
 * is GS bit for bit, statistics included; with p > 0 the sums behind the error
 * are taken in float64 against the exact target, because the error of a trap
 * target made uniform is a ~1e-4 remainder of those sums). Only angle(A) and E leave the loop, so g is defined up to a
 * positive factor per hologram: the device keeps it near mean 1 over the support
 * with the previous iteration's sum and clamps it to [2^-40, 2^40] of that scale.
 * On trap targets the iteration is contracting for the exponents tested up to
 * p = 1.5 (a small change of the start shrinks) and is not at p = 2, where it
 * grows: runs with p >= 2 stay finite but are not reproducible to rounding.
 * Plans of the fused engine only: both sides one of 64 ... 4096 (powers of two)
 * or 768; other shapes and $SLM_ENGINE=float64 get SLM_ERR_UNSUPPORTED from
 * slm_plan_create. slm_plan_set_phase warm-starts such a plan as a GS plan.
 *
 * slm_plan_set_feedback: the exponent p (default 1); negative or non-finite
 *   values give SLM_ERR_ARG.
 * slm_plan_set_weights: initial weights [batch][h][w], NULL = ones. Call after
 *   slm_plan_set_target (a new target returns the plan to ones); an entry on the
 *   support that is not positive and finite gives SLM_ERR_ARG. The plan keeps
 *   them in a buffer of their own: every run starts from them again.
 * slm_plan_read_weights: g after the last run (of a stopped hologram: at its
 *   stop iteration), or the weights set since; scaled to mean 1 over the
 *   support, exactly 1 off it.
 * All three give SLM_ERR_STATE on a plan of another algorithm.             */
int slm_plan_set_feedback(slm_plan* plan, float feedback);
int slm_plan_set_weights(slm_plan* plan, const float* weights);
int slm_plan_read_weights(slm_plan* plan, float* weights);
/* ---- MRAF (SLM_ALGO_MRAF): no reference counterpart -----------------------
 * Mixed-region amplitude freedom (Pasienski and DeMarco 2008) for extended,
 * flat targets, on which GS ends in speckle. Per hologram of S = h w pixels,
 * with the signal region sr = R > 0, the mixing parameter 0 < m <= 1,
 * P = S sum a_in^2 (= sum |fft2(B)|^2; S^2 for uniform light) and
 * kappa = sqrt(P / sum_sr a_T^2) (float64, once per change of target, region
 * or a_in: the target carries the whole power), every iteration does
 *     B = a_in exp(i angle A);  C = fft2(B);  E = |C|^2
 *     D = m kappa a_T C/|C| on sr (angle(0) = 0, as GS has it),  (1 - m) C off sr
 *     A = ifft2(D)
 * and starts exactly as GS does (ifft2(a_T) of the target as uploaded, or
 * slm_plan_set_phase). T outside the region is ignored by the projection and
 * by the statistics, which run over sr only:
 *     error      = sum_sr (E max_sr(T) / max_sr(E) - T)^2 / N_sr
 *     efficiency = sum_sr E / P
 * stats rows hold max_sr E, sum_sr E^2, sum_sr E T and that error; tol stops on
 * it. m = 1 with R all ones is GS, up to rounding. Plans of the fused engine
 * only: other shapes and $SLM_ENGINE=float64 get SLM_ERR_UNSUPPORTED from
 * slm_plan_create. There is no one-call or multi-GPU entry.
 *
 * slm_plan_set_region: R [batch][h][w] uint8, nonzero = signal. The plan keeps
 *   it in a buffer of its own that runs read and never write. A hologram whose
 *   region holds no pixel with T > 0 gives SLM_ERR_ARG (checked here against
 *   the target set before, and again when a run is asked for). Running an MRAF
 *   plan without a region gives SLM_ERR_STATE.
 * slm_plan_set_mixing: m (default 0.4); values outside (0, 1] or non-finite
 *   give SLM_ERR_ARG.
 * slm_plan_read_efficiency: eff [batch][max_loops] of the last run; the rows of
 *   a stopped hologram past its stop are left as the statistics rows are.
 * All three give SLM_ERR_STATE on a plan of another algorithm.             */
int slm_plan_set_region(slm_plan* plan, const uint8_t* region);
int slm_plan_set_mixing(slm_plan* plan, float m);
int slm_plan_read_efficiency(slm_plan* plan, double* eff);
/* Enqueue one full run (setup + loops iterations + outputs) on the plan's
 * stream. tol as in `while error > tolerance`; checked != 0 evaluates that
 * test on the device after every iteration (required when tol > 0). */
int slm_plan_run(slm_plan* plan, int loops, double tol, int checked, float white_attention);
/* As slm_plan_run, additionally timing every launch with HIP events on the
 * plan's stream; accumulates microseconds and launch counts per kernel class. */
int slm_plan_run_timed(slm_plan* plan, int loops, double tol, int checked, float white_attention,
                       double* us_per_class, int* launches_per_class);
int slm_plan_sync(slm_plan* plan);
/* Device-side stopwatch on the plan stream: slm_plan_mark(plan, 0) and
 * (plan, 1) record the plan's two HIP events; slm_plan_marked_ms waits for
 * mark 1 and returns the device time between them (what bench.py's timed
 * region took on the GPU, graph replays and gathers included). */
int slm_plan_mark(slm_plan* plan, int which);
int slm_plan_marked_ms(slm_plan* plan, double* ms);
int slm_plan_gd_recoveries(slm_plan* plan); /* GD runs redone after a one-launch wait gave up */
/* phase [batch][h][w] float32 (radians, angle convention of np.angle);
 * expected [batch][h][w] float32 = |C|^2 of the last iteration (scale by
 * norm / stats[..][0] for expected_outcome); stats [batch][max_loops][4] =
 * (max E, sum E^2, sum E T, error); iters [batch] iterations executed.
 * Any pointer may be NULL. */
int slm_plan_read(slm_plan* plan, float* phase, float* expected, double* stats, int* iters);
/* norm [batch] and sum T^2 [batch] as reduced on the device */
int slm_plan_read_target_stats(slm_plan* plan, double* norm, double* sum_t2);
/* Override norm = max(T) and sum T^2 per hologram with values the caller
 * computed in float64 from its own target (np.amax(demanded_output),
 * src/algorithms.py:23, and the constant term of error_f :161-162): a
 * float64 target keeps them exact although the device copy of T is float32.
 * Call after slm_plan_set_target. */
int slm_plan_set_target_stats(slm_plan* plan, const double* norm, const double* sum_t2);
/* GD state x [batch][h][w] complex64 (interleaved re, im) after the last run:
 * the field a chunked run continues from with slm_plan_set_field (GIF frames,
 * src/algorithms.py:94-101). */
int slm_plan_read_field(slm_plan* plan, float* field);
/* Image sequences: F frames of targets (moving traps drawn as pictures) as one
 * chain enqueued on the plan's stream, on GS, weighted-GS and MRAF plans of any
 * engine the algorithm runs on. The chain is, bit for bit, this host loop:
 *     for f = 0 .. F-1:
 *         slm_plan_set_target(targets[f])      (MRAF with regions: and
 *                                               slm_plan_set_region(regions[f]))
 *         f > 0: slm_plan_set_phase(the float32 phase frame f-1 ended with)
 *         f = 0: the start the plan has (slm_plan_set_phase, or the cold start)
 *         slm_plan_run(f = 0 ? loops_first : loops, tol, tol > 0, 0)
 *         outputs of frame f: phase, E, the statistics rows, iters, the
 *         efficiency rows (MRAF), and frame = the SLM_QUANT_* `rule` of
 *         slm_quantize applied to ((double)phase, mask, ct2pi)
 * without the host in it: the frames are uploaded once, each is landed from
 * device memory by the kernels slm_plan_set_target runs, the phase passes from
 * frame to frame on the device, and one epilogue kernel per frame writes the
 * uint8 frame, the next start and the kept phase. Nothing synchronises with the
 * host between frames. Weighted-GS weights return to ones at every frame, as
 * slm_plan_set_target has it.
 * slm_plan_sequence: targets [n_frames][batch][h][w] of the plan's target type;
 *   regions [n_frames][batch][h][w] uint8 (MRAF plans only) or NULL = the region
 *   in force serves every frame; mask [h][w] float64 or NULL, ct2pi and rule as
 *   slm_quantize; want_frames / want_phases / want_expected != 0 keep the uint8
 *   frames / the float32 phases / E of every frame on the device for
 *   slm_plan_sequence_read. With resume != 0, frame 0 of the call is treated as
 *   a frame f > 0 of the previous sequence on this plan (starts from its last
 *   phase, runs `loops`): a sequence cut in two is the uncut one. Everything is
 *   checked on the host before anything is enqueued. SLM_ERR_ARG: n_frames < 1,
 *   loops_first or loops outside 1 .. max_loops, tol negative or not finite, an
 *   unknown rule, ct2pi not positive and finite, an MRAF frame whose region
 *   holds no pixel with T > 0 (the message names frame and hologram; checked on
 *   the host over all frames, so the chain's refresh needs no copy back).
 *   SLM_ERR_STATE: a GD plan, has_ain without slm_plan_set_ain, regions on a
 *   plan that is not MRAF, MRAF with neither regions nor a region in force,
 *   resume without a previous sequence or after any slm_plan_set_* or
 *   slm_plan_run since. SLM_ERR_HIP when a sequence buffer cannot be allocated
 *   (they are sized at the call, only grow and go with the plan; the plan stays
 *   usable). After a sequence the plan is as after slm_plan_set_target (and
 *   slm_plan_set_region) with the last frame: a start phase the caller set
 *   before is still in force, a captured run stays valid, and slm_plan_read
 *   gives SLM_ERR_STATE until the next slm_plan_run.
 * slm_plan_sequence_read: waits for the chain, then copies what is asked for
 *   (any pointer NULL): frames [n_frames][batch][h][w] uint8, phases and
 *   expected [n_frames][batch][h][w] float32, stats [n_frames][batch][rows][4]
 *   and efficiency [n_frames][batch][rows] (MRAF) with rows = max(loops_first,
 *   loops), iters [n_frames][batch] as slm_plan_read has them. Rows a frame did
 *   not reach are as slm_plan_read would leave them. SLM_ERR_STATE before a
 *   sequence, for an output the sequence was not asked to keep, and for the
 *   efficiency of a plan that is not MRAF.                                    */
int slm_plan_sequence(slm_plan* plan, int n_frames, const void* targets, const uint8_t* regions, int loops_first,
                      int loops, double tol, int resume, const double* mask, double ct2pi, int rule, int want_frames,
                      int want_phases, int want_expected);
int slm_plan_sequence_read(slm_plan* plan, unsigned char* frames, float* phases, float* expected, double* stats,
                           double* efficiency, int* iters);
/* algorithmic HBM bytes moved by one launch of a kernel class */
long long slm_plan_kernel_bytes(slm_plan* plan, int kernel_class);
/* info[0] = column tile width, info[1] = column workgroups per hologram,
 * info[2] = column threads, info[3] = row threads, info[4] = rows per workgroup,
 * info[5] / info[6] = radix plan keys of rows / columns, info[7] = precision
 * (info must hold 8 ints) */
int slm_plan_info(slm_plan* plan, int* info);
/* The geometry an any-size plan (engines 2 .. 5 of slm_plan_engine) runs, as
 * chosen at its creation from the shape, the batch, the device and the
 * $SLM_GENERIC_ENGINE / $SLM_RZ_* / $SLM_MR_* overrides (info must hold 8 ints):
 * info[0] = engine (slm_plan_engine's code), info[1] = precision,
 * info[2] / info[3] = radix plan keys of rows / columns (-1 off the radix-plan
 * engines 4 and 5), info[4] = rows per row tile, info[5] = columns per column
 * tile, info[6] = state layout between the passes (0 = row-major, 1 = two-
 * column panels; always 0 off engines 4 and 5), info[7] = column workgroups
 * per hologram. Engine 2 (line transforms) has no tiles: info[4] = info[5] = 1,
 * info[7] = 0. A plan of the fused float32 engine is refused with
 * SLM_ERR_STATE and info is left untouched: slm_plan_info describes those
 * (and keeps reporting 0 / 1 / -1 for any-size plans). */
int slm_plan_generic_info(slm_plan* plan, int* info);
/* panel widths (log2) of the plan's two blocked device layouts: X (row-pass
 * output, column-pass input, target) and Y (column-pass output, GD field) */
int slm_plan_layout(slm_plan* plan, int* x_log2, int* y_log2);
/* transform engine of the GS iteration kernels: 0 = Stockham pair (LDS
 * exchange before every pass), 1 = wave-shuffle pair (fft_shuffle.hpp: 1024-
 * point lines, float32; v_permlane swaps for four of the six exchanges; the
 * GS and GD iteration kernels), 2 = line transforms (float64 1-D transforms
 * along rows and transposed columns, Bluestein's chirp-z for a side with a
 * prime factor above 13), 3 = mixed radix (float64 in-place radix-2..13
 * kernels: other sides without a float32 radix plan), 4 = complex128 radix
 * plans (float64 Stockham kernels with complex128 state: 2^k / 768 sides
 * under $SLM_ENGINE=float64), 5 = complex64 radix plans (the same kernels at
 * float32: GS on 13-smooth SLM panel sides such as 1080 x 1920, float32
 * precision; slm_plan_set_precision(F64) moves such a plan to engine 4) */
int slm_plan_engine(slm_plan* plan, int* col_engine, int* row_engine);
/* HIP device the plan lives on */
int slm_plan_device(slm_plan* plan);

/* Diagnostics: per-workgroup phase timestamps (s_memrealtime, 100 MHz: tile
 * start, loads complete, transforms done, stores complete, kernel entry) plus
 * the wave's HW_ID and XCC_ID, of the last launch of a kernel class,
 * [batch][workgroups][8]. Needs a library built with
 * -DSLM_TRACE=1 and SLM_TRACE_BUF=1 in the environment at plan creation. */
int slm_plan_read_trace(slm_plan* plan, int kernel_class, unsigned long long* out);

/* ---- one-shot helpers (upload, run, read) ------------------------------ */
int slm_gs(const void* tgt, int tgt_type, const float* ain, int batch, int height, int width, int max_loops,
           double tol, const float* init_phase, float* out_phase, float* out_expected, double* out_stats,
           int* out_iters);
int slm_gd(const void* tgt, int tgt_type, const float* ain, int batch, int height, int width, int max_loops,
           double tol, const float* init_field, const float* lr, float white_attention, float* out_phase,
           float* out_expected, double* out_stats, int* out_iters);
/* weighted GS (no reference counterpart): slm_gs's arguments, then the feedback
 * exponent, the initial weights (NULL = ones) and the weights out (may be NULL) */
int slm_gsw(const void* tgt, int tgt_type, const float* ain, int batch, int height, int width, int max_loops,
            double tol, const float* init_phase, float* out_phase, float* out_expected, double* out_stats,
            int* out_iters, float feedback, const float* init_weights, float* out_weights);

/* One process, several GPUs (SURVEY.md 8b's slm_gs_multi): the batch is cut
 * into n_gpus contiguous shards (the first batch % n_gpus one hologram larger,
 * as parallel.shard_counts), shard r runs on devices[r] (NULL = 0..n_gpus-1;
 * a device may repeat) from its own host thread with its own plan and stream,
 * and lands in its slice of the caller's arrays, each GPU copying over its own
 * link concurrently. Arguments otherwise as slm_gs; results are bitwise those
 * of slm_gs on each shard. The reference counterpart is the frame loop of
 * src/generate_hologram_sequence.py:19-31 run as one batch. */
int slm_gs_multi(int n_gpus, const int* devices, const void* tgt, int tgt_type, const float* ain, int batch,
                 int height, int width, int max_loops, double tol, const float* init_phase, float* out_phase,
                 float* out_expected, double* out_stats, int* out_iters);
/* The same for weighted GS (no reference counterpart): every shard starts from
 * weights of one; the weights themselves stay on the shards. */
int slm_gsw_multi(int n_gpus, const int* devices, const void* tgt, int tgt_type, const float* ain, int batch,
                  int height, int width, int max_loops, double tol, const float* init_phase, float* out_phase,
                  float* out_expected, double* out_stats, int* out_iters, float feedback);
/* Per-shard timing of the calling process's last slm_gs_multi / slm_gsw_multi: wall_ms[r] =
 * shard r's whole thread (plan, upload, run, read back), run_ms[r] = its run
 * alone (enqueue to stream drained); up to max_shards values each (either
 * pointer may be NULL). Returns the number of shards of that call (0 if none). */
int slm_gs_multi_timing(int max_shards, double* wall_ms, double* run_ms);

/* unscaled 2-D C2C transform of [batch][h][w] complex64 (test entry) */
int slm_fft2(const float* in_re_im, float* out_re_im, int batch, int height, int width, int inverse);
/* unscaled 2-D C2C transform of [batch][h][w] complex128 in float64 arithmetic
 * (any shape with sides up to 4096, or up to 8192 without a prime factor
 * above 13: mixed-radix kernels where both sides factor into 2..13, else
 * chirp-z line transforms; the engines are cached per (device, batch, h, w)
 * and the $SLM_ENGINE / $SLM_GENERIC_ENGINE / $SLM_RZ_* / $SLM_MR_* overrides
 * in force) -> the float64 scipy.fft.ifft2 of move_traps.update_hologram,
 * src/move_traps.py:66 (times h w) */
int slm_fft2_c128(const double* in_re_im, double* out_re_im, int batch, int height, int width, int inverse);
/* frees the float64 engines slm_fft2_c128 keeps per (device, batch, h, w)
 * (a few shapes; the drop-in's clear_plans calls it) */
int slm_release_caches(void);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ------------------- */
int slm_comm_unique_id(unsigned char* id128);
int slm_comm_init(int nranks, int rank, const unsigned char* id128);
int slm_comm_destroy(void);
/* Gather every rank's phase output to `root`: rank r contributes its plan's
 * batch (counts[r] holograms, same h x w everywhere); on root, host_out
 * receives sum(counts) x h x w float32 in rank order (may be NULL to leave
 * the gathered array on the device). Collective; enqueued on the plan stream,
 * which is synchronised before returning only when host_out is given (a
 * device-side gather stays stream-ordered with the plan's later work). */
int slm_plan_gather_phase(slm_plan* plan, const int* counts, int root, float* host_out);
/* The same collective for the per-iteration statistics that become each
 * hologram's error_evolution (src/generate_hologram_sequence.py:19-31 keeps one
 * per frame): on root, stats_out receives sum(counts) x
 * max_loops x 4 doubles (max E, sum E^2, sum E T, error) and iters_out
 * sum(counts) ints (iterations executed, -1 = all), rank order; either may be
 * NULL. */
int slm_plan_gather_stats(slm_plan* plan, const int* counts, int root, double* stats_out, int* iters_out);
/* Diagnostics of the phase gather (collective, every rank calls it): drains
 * the plan stream, then times `reps` device-side slm_plan_gather_phase calls
 * with HIP events on the plan stream; *ms = average per gather on this rank,
 * *bytes_out = bytes this rank sends to root per gather (0 on root, whose own
 * slab is a device-local copy). */
int slm_plan_time_gather(slm_plan* plan, const int* counts, int root, int reps, double* ms, long long* bytes_out);
/* Element offsets of a rank-order gather: offsets[r] = per_item x sum(counts[:r]),
 * offsets[nranks] = the total (offsets holds nranks + 1 values). The arithmetic
 * every gather above uses; host-only, needs no device. */
int slm_gather_layout(int nranks, const int* counts, long long per_item, long long* offsets);

/* ---- SLM frames: trap holograms and 8-bit quantisation ------------------
 * (element-wise, one launch per call, host buffers in/out)
 * slm_trap_frames      -> update_hologram(black_image, coords, which)
 *                         src/move_traps.py:64-68 (phase_out, float64, the
 *                         angle of ifft2 of a single 255 pixel at (ys[b], xs[b]))
 *                         fused with display_hologram's quantisation
 *                         src/move_traps.py:135-139 (frame_out, rule ASTYPE)
 * slm_quantize         -> mask_hologram(path, mask_arr, ct2pi)
 *                         src/display_holograms.py:253-266 (.npy branch: SRC_F64 +
 *                         rule PIL; image branch: SRC_I16) and display_hologram
 *                         (SRC_F64 + rule ASTYPE)
 * mask is [height][width] float64 (broadcast over the batch) or NULL; any
 * output pointer may be NULL.                                              */
#define SLM_QUANT_ASTYPE 0 /* ((h + mask) % 2pi * ct2pi / 2pi).astype(uint8) */
#define SLM_QUANT_PIL 1    /* PIL 'F'->'L' (clip, truncate) of ((h + mask) % 2pi) / 2pi * ct2pi */
#define SLM_SRC_F64 0      /* phase hologram, float64 */
#define SLM_SRC_I16 1      /* 8-bit hologram image widened to int16 (PIL 'L' -> np.int16) */
int slm_trap_frames(int batch, int height, int width, const int* ys, const int* xs, const double* mask,
                    double ct2pi, int rule, double* phase_out, unsigned char* frame_out);
int slm_quantize(const void* src, int src_type, const double* mask, int batch, int height, int width, double ct2pi,
                 int rule, unsigned char* out);

/* ---- trap lists: no reference counterpart --------------------------------
 * Weighted GS in its spot form (Di Leonardo et al. 2007): the field is
 * evaluated at the M traps only, with no transform, so every panel shape runs
 * (sides 2 ... 4096, 1 <= M <= 1024). Per hologram of H x W pixels (row k,
 * column l), with a = a_in or ones, traps at (y_m, x_m) in far-field pixel
 * units (real numbers, any sign), a defocus z_m in radians per pixel^2, target
 * intensities I_m > 0, a_T,m = sqrt(I_m) and the feedback exponent p >= 0:
 *     D_m(k,l) = 2 pi (k y_m / H + l x_m / W) + z_m ((k - H/2)^2 + (l - W/2)^2)
 *     start:   w = 1 (or the caller's); phi = the caller's phase, or
 *              angle(sum_m a_T,m exp(i (D_m + theta_m))), theta_m = 2 pi frac(m 0.6180339887498949)
 *     each iteration:
 *         V_m = sum_kl a(k,l) exp(i (phi(k,l) - D_m(k,l)))
 *         where |V_m| > 0:  w_m *= (a_T,m / |V_m|)^p, the factor clamped to [2^-64, 2^64];
 *         w /= mean(w)   (over all M traps, current each iteration)
 *         phi = angle(sum_m a_T,m w_m (V_m / |V_m|) exp(i D_m))          (angle(0) = 0)
 *         statistics from V, before the update, with r_m = (|V_m|^2 / I_m) / mean_m(|V_m|^2 / I_m):
 *             (efficiency sum_m |V_m|^2 / (H W sum a^2), uniformity std(r), min r, max r)
 * For integer (y, x) and z = 0, V_m is fft2(a exp(i phi))[y][x]; for M = 1 the
 * hologram is slm_trap_frames' (update_hologram); p = 0 is unweighted spot GS.
 * The state is the unit field exp(i phi), complex64; both sums run as float32
 * matrix products on the matrix cores (v_mfma_f32_32x32x2_f32), the fold over
 * rows, the statistics and the weights in float64. Results are bitwise
 * reproducible and do not depend on the batch a hologram sits in.
 *
 * slm_spots_create: `batch` holograms of height x width with up to max_traps
 *   traps each; has_ain != 0 requires slm_spots_set_ain before a run.
 * slm_spots_set_traps: ys, xs, zs (NULL = 0), intensity (NULL = 1), each
 *   [batch][n_traps]; builds the phase tables on the device (float64, rounded to
 *   complex64) and returns the weights to ones. A non-finite coordinate, or an
 *   intensity that is not positive and finite, gives SLM_ERR_ARG.
 * slm_spots_set_ain: [height][width] sqrt(incoming intensity), as slm_plan_set_ain.
 * slm_spots_set_phase: start phase [batch][h][w] float32, NULL = the start above.
 * slm_spots_set_weights: start weights [batch][n_traps], NULL = ones; call after
 *   slm_spots_set_traps; an entry that is not positive and finite gives SLM_ERR_ARG.
 * slm_spots_set_feedback: p (default 1); negative or non-finite gives SLM_ERR_ARG.
 * The start phase and weights live in buffers that runs read and never write:
 * every run starts from them again.
 * slm_spots_run: `loops` (1 ... max_loops) iterations, enqueued on the handle's stream.
 * slm_spots_run_timed: the same, every launch timed with HIP events;
 *   us_per_class[SLM_SPOTS_NUM_KERNEL_CLASSES] receives microseconds per class.
 * slm_spots_read: phase [batch][h][w] float32; fields [batch][n_traps][2] = V of
 *   the last iteration; stats [batch][loops][4] (loops of the last run);
 *   weights [batch][n_traps] (mean 1). Any pointer may be NULL; SLM_ERR_STATE
 *   before a run.
 * slm_spots_info: info[0] = Mp (the trap count padded to the matrix-core tile, 32),
 *   info[1] = partial sums per hologram and trap the fields kernel writes,
 *   info[2] = columns per such partial (each covers 128 rows), info[3] = waves
 *   per workgroup of the two product kernels (info holds 4 ints).
 * slm_spots_fields / slm_spots_superpose: one-shot test entries for the two
 *   products alone: V [batch][n_traps][2] of exp(i phase) (times a_in), and
 *   angle(sum_m c_m exp(i D_m)) for complex c [batch][n_traps][2].
 *
 * Trap trajectories: F frames of a moving list of the same M traps (trap m of
 * frame f is trap m of frame f-1, moved) as one chain enqueued on the handle's
 * stream, with everything above unchanged per iteration:
 *     frame 0:   start phase = the handle's (slm_spots_set_phase) or the default
 *                start for list 0; weights = weights0 or ones; at most
 *                loops_first iterations on list 0
 *     frame f>0: tables and a_T of list f; start = the unit field U and the
 *                weights w that frame f-1 ended with (U as it is on the device,
 *                complex64, no float32 phase in between); at most `loops` iterations
 *     stop:      tol > 0: the first iteration of a frame whose uniformity std(r)
 *                (of the field entering that iteration) is <= tol still completes
 *                and is the frame's last; iters[f] = its index + 1. Holograms of a
 *                batch stop on their own. tol = 0: every frame runs its full count.
 *     outputs of frame f, from its last executed iteration: phase float32, V, w
 *                (mean 1), statistics rows 0 .. iters[f]-1 (later rows are 0),
 *                iters[f], and frame = the SLM_QUANT_* `rule` of slm_quantize
 *                applied to ((double)phase, mask, ct2pi), written by the
 *                superposition kernel itself.
 * So F frames of one list at n iterations each with tol = 0 are one
 * slm_spots_run of F n iterations, and a sequence cut in two with `resume` is
 * the uncut one, both bit for bit.
 * slm_spots_sequence: ys, xs, zs (NULL = 0), intensity (NULL = 1) are
 *   [n_frames][batch][n_traps]; weights0 [batch][n_traps] (NULL = ones; must be
 *   NULL with resume). mask [height][width] float64 or NULL, ct2pi and rule as
 *   slm_quantize. want_frames / want_phases != 0 keep the uint8 frames / the
 *   float32 phases of every frame on the device for slm_spots_sequence_read.
 *   Everything is checked on the host before anything is enqueued. SLM_ERR_ARG:
 *   a non-finite coordinate, an intensity or weight that is not positive and
 *   finite, n_traps outside 1 .. max_traps, n_frames < 1, loops_first or loops
 *   outside 1 .. max_loops, tol negative or not finite, an unknown rule, ct2pi
 *   not positive and finite (both checked whether or not frames are wanted),
 *   weights0 with resume. SLM_ERR_STATE: has_ain without slm_spots_set_ain;
 *   resume != 0 without a previous sequence of the same n_traps on this handle
 *   or after any slm_spots_set_* or slm_spots_run since. SLM_ERR_HIP when a
 *   sequence buffer cannot be allocated (they are sized at the call, only grow,
 *   and are freed with the handle). The call uploads the coordinates of all
 *   frames once, enqueues the chain (per frame: one launch that builds the four
 *   tables from the device-resident coordinates, then the iterations; no host
 *   synchronisation between frames) and returns.
 *   With resume, frame 0 of the call is treated as a frame f > 0: it starts from
 *   the U and w the previous sequence ended with and runs `loops` iterations.
 *   The feedback exponent and a_in are the handle's. After a sequence the
 *   handle is as after slm_spots_set_traps with the last frame's list: weights
 *   back to ones, a caller's start phase still in force, slm_spots_read refuses
 *   until the next slm_spots_run.
 * slm_spots_sequence_read: waits for the chain, then copies what is asked for
 *   (any pointer NULL): frames [n_frames][batch][h][w] uint8, phases
 *   [n_frames][batch][h][w] float32, fields [n_frames][batch][n_traps][2], stats
 *   [n_frames][batch][max(loops_first, loops)][4], weights
 *   [n_frames][batch][n_traps], iters [n_frames][batch]. SLM_ERR_STATE before a
 *   sequence, and for frames or phases the sequence was not asked to keep.    */
#define SLM_SPOTS_KERNEL_FIELDS 0    /* spot_fields_kernel: V partials */
#define SLM_SPOTS_KERNEL_UPDATE 1    /* spot_update_kernel: fold, statistics, weights */
#define SLM_SPOTS_KERNEL_SUPERPOSE 2 /* spot_superpose_kernel: the next unit field (and the phase) */
#define SLM_SPOTS_NUM_KERNEL_CLASSES 3
typedef struct slm_spots slm_spots;
int slm_spots_create(int batch, int height, int width, int max_traps, int has_ain, int max_loops, slm_spots** out);
int slm_spots_destroy(slm_spots* sp);
int slm_spots_set_traps(slm_spots* sp, int n_traps, const double* ys, const double* xs, const double* zs,
                        const float* intensity);
int slm_spots_set_ain(slm_spots* sp, const float* ain);
int slm_spots_set_phase(slm_spots* sp, const float* phase);
int slm_spots_set_weights(slm_spots* sp, const float* weights);
int slm_spots_set_feedback(slm_spots* sp, float feedback);
int slm_spots_run(slm_spots* sp, int loops);
int slm_spots_run_timed(slm_spots* sp, int loops, double* us_per_class);
int slm_spots_read(slm_spots* sp, float* phase, double* fields, double* stats, float* weights);
int slm_spots_info(slm_spots* sp, int* info);
int slm_spots_sequence(slm_spots* sp, int n_frames, int n_traps, const double* ys, const double* xs, const double* zs,
                       const float* intensity, const float* weights0, int loops_first, int loops, double tol,
                       int resume, const double* mask, double ct2pi, int rule, int want_frames, int want_phases);
int slm_spots_sequence_read(slm_spots* sp, unsigned char* frames, float* phases, double* fields, double* stats,
                            float* weights, int* iters);
int slm_spots_fields(int batch, int height, int width, int n_traps, const double* ys, const double* xs,
                     const double* zs, const float* ain, const float* phase, double* fields_out);
int slm_spots_superpose(int batch, int height, int width, int n_traps, const double* ys, const double* xs,
                        const double* zs, const double* c_re_im, float* phase_out);

/* ---- zoomed far field: no reference counterpart ---------------------------
 * The far field of a hologram on a regular fractional grid, in the trap-list
 * conventions above, so that a sample is what slm_spots_fields gives for a trap
 * at its position. Per hologram of H x W pixels (row k, column l), a = a_in or
 * ones, u = exp(i phi), a window of ny x nx samples y_j = y0 + j dy,
 * x_i = x0 + i dx (far-field pixels = FFT bins, fractional, any sign; formed in
 * float64) and one defocus z in radians per pixel^2 for the whole window:
 *     fy_j(k) = 2 pi frac(k y_j / H) + z (k - H/2)^2      fx_i(l) likewise with x_i, W
 *     R[k][i] = sum_l a(k,l) u(k,l) exp(-i fx_i(l))
 *     V[j][i] = sum_k exp(-i fy_j(k)) R[k][i]
 *     I[j][i] = |V[j][i]|^2
 * For integer y0, x0, dy = dx = 1 and z = 0, V is fft2(a u)[y_j mod H][x_i mod W].
 * `hologram` is [batch][h][w]: SLM_ZOOM_PHASE_F32, a float32 phase in radians
 * (u = its float64 sine and cosine rounded to complex64, as slm_spots_set_phase
 * forms it), or SLM_ZOOM_LEVELS_U8, a uint8 SLM frame as it is displayed
 * (u = exp(i 2 pi level / ct2pi), evaluated in float64 per level and rounded to
 * complex64; no correction mask is applied). ct2pi is read for levels only.
 * Both sums are float32 matrix products on the matrix cores
 * (v_mfma_f32_32x32x2_f32) with tables built as the trap lists' are; no float32
 * chain is longer than 256 summed pixels, the chunks (pixels 256 c .. 256 c + 255)
 * are added in float64 in their order (in registers, or from a partial buffer
 * when the sum is split over workgroups: the same additions), R is rounded to
 * complex64 once. No atomics: results are bitwise reproducible, do not depend
 * on the batch, and a sample's value depends on its position alone, not on the
 * window around it.
 * slm_farfield_zoom: one-shot, host pointers in and out: a resident zoom (below)
 *   of one hologram, created and destroyed by the call. The batch shares the
 *   window and ain [h][w] (NULL = ones) and runs hologram by hologram;
 *   intensity [batch][ny][nx] float32; field [batch][ny][nx][2] = V from the
 *   float64 fold, or NULL. It synchronises and frees its buffers before it
 *   returns; while it runs it holds one hologram's whole window on the device
 *   (at 4096 x 4096 samples 64 MB of intensity and, with the field, 256 MB
 *   more). Its caps on the partial buffers are the built-in ones: it does not
 *   read $SLM_ZOOM_PARTIAL_BYTES. Every argument is checked before anything is
 *   created on the device. SLM_ERR_ARG: a null hologram or intensity, an unknown kind,
 *   batch < 1, a side outside 2 .. 4096, ny or nx outside 1 .. 4096, y0, x0, dy,
 *   dx or z not finite, dy or dx <= 0, ct2pi not finite or <= 0 with levels, a
 *   non-finite a_in entry, a_in zero everywhere.
 * slm_farfield_zoom_timed: the same; kernel_us[SLM_ZOOM_NUM_KERNEL_CLASSES]
 *   (NULL = untimed) receives the microseconds HIP events measured around the
 *   kernels of each class, summed over the holograms (the two table launches
 *   once per call); copies are excluded.                                      */
#define SLM_ZOOM_PHASE_F32 0
#define SLM_ZOOM_LEVELS_U8 1
#define SLM_ZOOM_KERNEL_TABLES 0 /* zoom_table_kernel: Px and Py, once per call */
#define SLM_ZOOM_KERNEL_FIELD 1  /* zoom_field_kernel: a u as complex64 */
#define SLM_ZOOM_KERNEL_ROWS 2   /* zoom_rows_kernel (and its fold when the columns are split): R */
#define SLM_ZOOM_KERNEL_COLS 3   /* zoom_cols_kernel and zoom_fold_kernel: V and I */
#define SLM_ZOOM_NUM_KERNEL_CLASSES 4
int slm_farfield_zoom(const void* hologram, int kind, int batch, int height, int width, const float* ain, double ct2pi,
                      double y0, double x0, double dy, double dx, int ny, int nx, double z, float* intensity,
                      double* field);
int slm_farfield_zoom_timed(const void* hologram, int kind, int batch, int height, int width, const float* ain,
                            double ct2pi, double y0, double x0, double dy, double dx, int ny, int nx, double z,
                            float* intensity, double* field, double* kernel_us);

/* ---- resident zoom: the zoomed far field with stream, buffers and tables kept --
 * The same far field on a handle, the one host path of the kernels (the one-shot
 * above creates such a handle for one hologram and destroys it again). It keeps
 * stream, buffers and tables, runs all holograms of a call in the same launches (in groups that
 * bound the work buffers), gives each hologram a window of its own if asked,
 * takes a correction mask off, and reads the uint8 frames of the last trap or
 * image sequence where they already are, on the device. Without a mask a
 * sample is the one-shot's, bit for bit: the kernels, the tables and the
 * accumulation (chunks of 256 pixels, added in float64 in their order) are the
 * same, and a sample's value depends on its own position, the pixel indices,
 * the hologram, a_in, the mask and z; never on the number of holograms in the
 * run, the group a hologram falls in, the band, whether the first product split
 * its columns, or whether the windows are shared.
 * With a mask, per pixel: arg = t - mask[k][l] (one rounded float64
 * subtraction), t = 2 pi level / ct2pi as the one-shot's level table evaluates
 * it, or (double)phase for SLM_ZOOM_PHASE_F32; u = the float64 sine and cosine
 * of arg rounded to complex64, times a_in as before.
 * slm_zoom_create: `batch` (1 .. 1024) holograms per run at most, sides as the
 *   one-shot, windows of up to max_ny x max_nx (1 .. 4096) samples. Creates the
 *   stream; buffers are sized at need (the level tables at the first run on
 *   levels), only grow, and go with the handle.
 *   $SLM_ZOOM_PARTIAL_BYTES (a positive whole number, read here) replaces the two
 *   caps of the partial buffers (64 MB for the second product, 128 MB for the
 *   split first product); anything else in it gives SLM_ERR_ARG.
 * slm_zoom_set_ain: [h][w], NULL = ones; checked as the one-shot's.
 * slm_zoom_set_mask: [h][w] float64 radians, NULL = none; a non-finite entry
 *   gives SLM_ERR_ARG.
 * slm_zoom_set_window: per_hologram == 0: y0, x0, z hold one entry each and the
 *   tables are shared; otherwise `batch` entries each, and hologram i of a run
 *   gets origin (y0[i], x0[i]) and defocus z[i]. Pitch and size are shared.
 *   Builds the tables; no run rebuilds them. Checks and messages are the
 *   one-shot's; ny > max_ny or nx > max_nx gives SLM_ERR_ARG.
 * slm_zoom_set_timed: timed != 0: later runs time their kernels with HIP events.
 * slm_zoom_run: `count` (1 .. batch) holograms [count][h][w] of `kind` from the
 *   host: one upload, everything enqueued on the handle's stream, no host
 *   synchronisation. `hologram` must stay valid until slm_zoom_read (or the
 *   next call on the handle that waits). SLM_ERR_STATE before
 *   slm_zoom_set_window. (A run with another ct2pi than the last one's uploads
 *   the 256 level values again.)
 * slm_zoom_run_spots / slm_zoom_run_plan: the holograms are the uint8 frames
 *   with flat index f B + b in [first, first + count) of the source's last
 *   sequence, read from the source's device buffer (kind = levels). The
 *   handle's stream waits for an event recorded on the source's stream (the
 *   chain that writes the frames), and the source's stream waits for an event
 *   recorded after the run (so a later sequence overwrites the frames only
 *   after they have been read); no host synchronisation. SLM_ERR_STATE: no
 *   sequence, or one that did not keep its frames; SLM_ERR_ARG: another shape
 *   than the handle's, a range outside the sequence.
 * slm_zoom_read: waits for the run; intensity [count][ny][nx] float32, field
 *   [count][ny][nx][2] float64 (SLM_ERR_STATE if the run had want_field == 0),
 *   kernel_us[SLM_ZOOM_NUM_KERNEL_CLASSES] (SLM_ERR_STATE unless the run was
 *   timed; the tables are no part of a run: class 0 is 0). Any pointer may be
 *   NULL. SLM_ERR_STATE before the first run.
 * slm_zoom_info: of the last run, info[0] = groups, info[1] = bands per group,
 *   info[2] = launches of the first product that split their columns (info
 *   holds 3 ints). SLM_ERR_STATE before the first run.
 * slm_release_caches does not touch handles: they belong to the caller.       */
typedef struct slm_zoom slm_zoom;
int slm_zoom_create(int batch, int height, int width, int max_ny, int max_nx, slm_zoom** out);
int slm_zoom_destroy(slm_zoom* zm);
int slm_zoom_set_ain(slm_zoom* zm, const float* ain);
int slm_zoom_set_mask(slm_zoom* zm, const double* mask);
int slm_zoom_set_window(slm_zoom* zm, int per_hologram, const double* y0, const double* x0, const double* z,
                        double dy, double dx, int ny, int nx);
int slm_zoom_set_timed(slm_zoom* zm, int timed);
int slm_zoom_run(slm_zoom* zm, const void* hologram, int kind, int count, double ct2pi, int want_field);
int slm_zoom_run_spots(slm_zoom* zm, slm_spots* sp, int first, int count, double ct2pi, int want_field);
int slm_zoom_run_plan(slm_zoom* zm, slm_plan* plan, int first, int count, double ct2pi, int want_field);
int slm_zoom_read(slm_zoom* zm, float* intensity, double* field, double* kernel_us);
int slm_zoom_info(slm_zoom* zm, int* info);

/* ---- CLI post-processing ------------------------------
 * slm_transform_hologram -> transform_hologram(hologram, args)
 *                           src/generate_hologram.py:82-87: deflect_hologram
 *                           (:178-181 with wavefront_correction.deflect_2pi,
 *                           src/wavefront_correction.py:440-449) and add_lens
 *                           (:184-203, lens() stored as uint8). float64,
 *                           reference operation order, bit for bit.
 * holo_in [height][width] float64 or NULL (zeros); params = {sin(y_angle u),
 * sin(x_angle u), 2 pi px_distance / wavelength, 2 pi focal / wavelength,
 * focal, px_distance} as the reference computes them on the host.
 * slm_fft2_intensity     -> show_expected_outcome's |fft2(exp(1j h))|^2
 *                           (src/generate_hologram.py:24-34) on the plan
 *                           kernels (complex64), row-major float32 out.   */
#define SLM_TRANSFORM_DEFLECT 1
#define SLM_TRANSFORM_LENS 2
int slm_transform_hologram(const double* holo_in, int height, int width, int flags, const double* params,
                           double* holo_out);
int slm_fft2_intensity(const float* phase, int batch, int height, int width, float* intensity_out);

#ifdef __cplusplus
}
#endif
#endif /* SLM_HIP_H */
