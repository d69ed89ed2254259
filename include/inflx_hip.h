/*
 * inflx_hip.h -- C ABI of libinflx_hip.so, the MI355X-native replacement for the grid-sweep
 * entry points of the reference's native module `libinflx_rs`.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the reference
 * repository).  Signatures use plain pointers and sizes only; the caller owns every host buffer
 * (`p`, `out`, `start_stop`, `x`), the library owns the device memory, stream and code object
 * held by an `inflx_model`.  All functions return an `inflx_status`; on failure
 * `inflx_last_error()` returns a thread-local message.  The mapping to the Python exception
 * classes the reference raises (src/err.rs:63-74) is given with each status.
 *
 * Threads: calls on different handles may run concurrently; calls on the SAME handle are serialised
 * by the library (a per-handle lock held for the call) -- the reference gets the same effect from
 * the GIL, which it holds for a whole sweep (src/anguelova.rs:458-465) and which a ctypes / cgo /
 * FFI binding of this library does not.  Closing a handle that another thread still uses remains
 * the caller's error.
 *
 * A "model artefact" is the per-model gfx950 code object written by inflatox_amd.Compiler -- the
 * counterpart of the per-model dylib the reference compiles with zig cc
 * (python/inflatox/compiler.py:568-598) and opens with libloading (src/dylib.rs:67-161).
 */
#ifndef INFLX_HIP_H
#define INFLX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct inflx_model inflx_model;

typedef enum inflx_status {
  INFLX_OK = 0,
  INFLX_ERR_IO = 1,      /* artefact cannot be opened              -> IOError      (err.rs:65)    */
  INFLX_ERR_SYMBOL = 2,  /* artefact lacks a required symbol       -> SystemError  (err.rs:66-69) */
  INFLX_ERR_VERSION = 3, /* artefact built for another ABI version -> SystemError  (err.rs:70)    */
  INFLX_ERR_SHAPE = 4,   /* array shape / parameter count mismatch -> Exception    (err.rs:71)    */
  INFLX_ERR_DEVICE = 5,  /* HIP runtime failure (no counterpart)   -> SystemError                 */
  INFLX_ERR_ARG = 6,     /* invalid argument (NULL, bad enum)      -> ValueError; the reference
                            panics on the analogous conditions (anguelova.rs:473,501)             */
  INFLX_ERR_BASIS = 7,   /* basis not orthonormal (BasisNorm/BasisOth) -> Exception (err.rs:36-37,72) */
  INFLX_ERR_GSL = 8      /* a special function was called outside its domain (see inflx_sf_policy): the reference's GSL error
                            handler prints the reason and panics (err.rs:86-103) -> ArithmeticError       */
} inflx_status;

/* bits of a model's special-function status (csrc/inflx_sf.h) */
typedef enum inflx_sf_bits {
  INFLX_SF_EDOM = 1,      /* an argument outside the function's domain: GSL_EDOM (1) in the reference's GSL */
  INFLX_SF_EDECLINED = 2  /* inside the domain, but the device function could not deliver 1e-13 and returned NaN
                             rather than a plausible number (GSL's counterparts: GSL_ELOSS, GSL_EMAXITER, GSL_EUNIMPL) */
} inflx_sf_bits;

typedef enum inflx_sf_policy_t {
  INFLX_SF_QUIET = 0, /* NaN at the point, nothing else */
  INFLX_SF_FAIL = 1   /* the call that finds a bit set returns INFLX_ERR_GSL -- after its result is complete */
} inflx_sf_policy_t;

/* per-point operation selector; numbering shared with the kernels (csrc/inflx_kernel_abi.h) */
typedef enum inflx_op {
  INFLX_SWEEP_COMPLETE = 0,    /* ops::complete_analysis          anguelova.rs:103-135, 6 f64/point */
  INFLX_SWEEP_CONSISTENCY = 1, /* ops::consistency_only           anguelova.rs:157-163, 1 f64/point */
  INFLX_SWEEP_RAPIDTURN = 2,   /* ops::consistency_rapidturn_only anguelova.rs:143-154, 1 f64/point */
  INFLX_SWEEP_EPSILON_V = 3,   /* ops::epsilon_v_only             anguelova.rs:138-140, 1 f64/point */
  INFLX_SWEEP_RAW = 4,         /* V,v00,v10,v11,|dV|^2 (diagnostic, 5 f64/point; what Potential /
                                  Hesse2D return, hesse_bindings.rs:52-57,106-110,213-231)          */
  INFLX_SWEEP_HESSE = 6        /* v00,v01,v10,v11 (4 f64/point): the projected Hesse matrix row-major, what `hesse` /
                                  `hesse_array` return (src/lib.rs:384-462) -- v01 is the reference's own v01 expression
                                  (hesse_bindings.rs:202-210), evaluated on its own wherever it is not the very expression
                                  of v10                                                             */
} inflx_op;

typedef enum inflx_layout {
  INFLX_AOS = 0, /* [P][rows][N1][K] -- the reference's (N0,N1,6) array (consistency_conditions.py:290) */
  INFLX_SOA = 1  /* [P][K][rows][N1] -- K contiguous planes */
} inflx_layout;

/* thread-local description of the last failure on the calling thread */
const char* inflx_last_error(void);

/* number of visible HIP devices */
int inflx_device_count(int* count);

/*
 * Open a model artefact on `device` -- replaces InflatoxDylib::open (src/dylib.rs:67-161) as
 * reached from open_inflx_dylib (src/lib.rs:108-115): loads the code object, checks VERSION
 * (major.minor against 5.0, src/inflatox_version.rs:48-53, src/lib.rs:50), reads DIM,
 * N_PARAMETERS, MODEL_NAME and resolves the sweep kernels.
 */
int inflx_open(const char* artefact_path, int device, inflx_model** out);
void inflx_close(inflx_model* model);

/*
 * Kernel groups.  Every kernel that evaluates the model inlines the whole model, and a complete artefact holds ~45 of them: building
 * all of it costs a heavy model several seconds of hipcc where the reference's one `zig cc` step takes about one
 * (python/inflatox/compiler.py:568-598).  The artefact inflx_open takes is therefore the model's CORE object -- everything
 * complete_analysis, the on-trajectory complete_analysis and the basis validation need -- or a complete one
 * (Compiler(kernel_groups="all")); the kernels of the other operations live in one small code object per group:
 *   "stats" (the fused summary), "consistency", "rapidturn", "epsilon_v", "raw", "qdif", "hesse", "values" (inflx_ops_on_values).
 * An entry point that needs a group the handle lacks loads the file `<artefact>.<group>` if it exists (inflatox_amd builds the group
 * and puts it there on first use) and fails with INFLX_ERR_SYMBOL otherwise.  inflx_attach loads a group object from any path; it must
 * come from the same generated model and options as the core object (its MODEL_TAG global), else INFLX_ERR_VERSION.
 * inflx_groups: bit mask of the groups loaded so far (bit k = the k-th name of: core, stats, values, consistency, rapidturn,
 * epsilon_v, raw, qdif, hesse).
 */
int inflx_attach(inflx_model* model, const char* group_object_path);
uint32_t inflx_groups(const inflx_model* model);

/* InflatoxDylib::{n_fields,n_pars,name} (src/dylib.rs:285-301) */
uint32_t inflx_n_fields(const inflx_model* model);
uint32_t inflx_n_parameters(const inflx_model* model);
const char* inflx_model_name(const inflx_model* model);
int inflx_device_of(const inflx_model* model);
/* staging facts of the loaded kernels: exported uniform/row/column values and the axis mask of the
 * five model values (bit0 = x[0], bit1 = x[1]) */
int inflx_stage_info(const inflx_model* model, uint32_t* n_uniform, uint32_t* n_row, uint32_t* n_col, uint32_t* out_mask);

/*
 * Drop-ins for the #[pyfunction]s of src/anguelova.rs.  Host buffers, C-contiguous f64:
 *   p           (n_p,)           model parameters
 *   start_stop  (2,2) row-major  [[x0_start,x0_stop],[x1_start,x1_stop]]  (src/lib.rs:117-139)
 *   out         (N0,N1,6) for complete_analysis, (N0,N1) for the single-quantity sweeps
 * `progress` != 0 prints the reference's start/finish lines to stderr and, while a call with a result of 1 GiB or more
 * has been running for longer than 0.5 s, a progress line twice a second (time to completion, grid points/s,
 * percentage: the figures of the reference's progress bar, src/anguelova.rs:42-50); `threads` is accepted for
 * signature compatibility and ignored by these single-device entry points (the *_multi entry points below give it the
 * reference's meaning, with GPUs as the workers).
 */
int inflx_complete_analysis(inflx_model* model, const double* p, size_t n_p, double* out, const double* start_stop,
                            size_t N0, size_t N1, int progress, size_t threads); /* anguelova.rs:458-550 */
int inflx_consistency_only(inflx_model* model, const double* p, size_t n_p, double* out, const double* start_stop,
                           size_t N0, size_t N1, int progress, size_t threads); /* anguelova.rs:176-264 */
int inflx_consistency_rapidturn_only(inflx_model* model, const double* p, size_t n_p, double* out,
                                     const double* start_stop, size_t N0, size_t N1, int progress,
                                     size_t threads); /* anguelova.rs:267-356 */
int inflx_epsilon_v_only(inflx_model* model, const double* p, size_t n_p, double* out, const double* start_stop,
                         size_t N0, size_t N1, int progress, size_t threads); /* anguelova.rs:359-447 */

/* flag_quantum_dif_py (src/anguelova.rs:574-626): out is a (N0,N1) array of bytes (numpy bool), 1 where
 * every component of the normalised potential gradient (basis vector `v`) is <= accuracy */
int inflx_flag_quantum_dif(inflx_model* model, const double* p, size_t n_p, uint8_t* out, const double* start_stop,
                           size_t N0, size_t N1, int progress, double accuracy);

/* on-trajectory variants (src/anguelova.rs:633-977): x is (n,2), out is (n,K) */
int inflx_sweep_on_trajectory(inflx_model* model, int op, const double* p, size_t n_p, const double* x, size_t n,
                              double* out, int progress, size_t threads);

/*
 * Basis validation (src/lib.rs:141-300).  The reference calls the artefact's C functions `v`, `w1` and
 * `inner_prod` (compiler.py:417-472) point by point; here one launch evaluates them at n explicit points.
 *   inflx_basis_on_points: x is (n,2); out is (n,7): v.v, v.w1, w1.w1, v[0], v[1], w1[0], w1[1]
 *   inflx_validate_basis_at_random (lib.rs:142-199, run by open_inflx_dylib(check_basis=true), lib.rs:109-114):
 *     one random parameter vector in [-10,10), 100 random points in [-1,1)^2, accuracy 1e-3;
 *     seed 0 = seed from the OS (the reference's rand::random), any other value = reproducible
 *   inflx_validate_basis_on_domain (lib.rs:207-300): num_points is (n_axes,), start_stop (n_axes,2) row-major
 * Both return INFLX_ERR_BASIS with the reference's message when a norm or overlap misses its target by
 * >= accuracy, and print the reference's warnings for inner products that are not normal numbers.
 */
int inflx_basis_on_points(inflx_model* model, const double* p, size_t n_p, const double* x, size_t n, double* out);
int inflx_validate_basis_at_random(inflx_model* model, uint64_t seed);
int inflx_validate_basis_on_domain(inflx_model* model, const uint32_t* num_points, size_t n_axes, const double* p,
                                   size_t n_p, const double* start_stop, double accuracy);

/*
 * The per-point operations of src/anguelova.rs:99-171 (`mod ops`) applied to GIVEN model values instead of values the
 * kernels evaluate from a model: `values` is (n,5) -- V, v00, v10, v11, grad_norm_squared, what Potential / Hesse2D
 * return (hesse_bindings.rs:52-57,106-110,213-231) --, `out` is (n,9): [0..5] ops::complete_analysis (:103-135),
 * [6] ops::consistency_only (:157-163), [7] ops::consistency_rapidturn_only (:143-154), [8] ops::epsilon_v_only
 * (:138-140).  The model's own functions are not called.  `ieee_only` = 0 evaluates complete_analysis the way the
 * sweep kernels do (divisions without special-case handling where every operand is in mid range, csrc/inflx_ops.h),
 * != 0 with the compiler's IEEE divisions throughout; the two must agree bit for bit on every input, and both are
 * what the parity tests compare with the oracle on arbitrary tuples (specials, zeros, denormals, random bit patterns).
 */
int inflx_ops_on_values(inflx_model* model, const double* values, size_t n, double* out, int ieee_only);

/*
 * Generalised sweep, host result.  P parameter rows (p is (P,n_p)), grid rows
 * [row_begin,row_begin+row_count) of the N0 x N1 grid, result written to the host buffer `out`
 * of P*row_count*N1*K doubles in `layout`.  Rows are processed in device-sized chunks and copied
 * back while the next chunk computes.
 */
int inflx_sweep_host(inflx_model* model, int op, const double* p, size_t P, size_t n_p, double* out,
                     const double* start_stop, size_t N0, size_t N1, size_t row_begin, size_t row_count, int layout);

/*
 * As inflx_sweep_host with the planes layout, but only planes [first_plane, first_plane + n_planes) of every parameter row cross
 * PCIe: `out` holds P*n_planes*row_count*N1 doubles, (P, n_planes, row_count, N1).  The device evaluates all K values of the
 * operation in one pass; a caller that wants one of them (calc_V_array: plane 0 of the five raw values, reference
 * consistency_conditions.py:67-101; calc_H_array: planes 1-3, :119-156) does not pay the copy of the others.
 */
int inflx_sweep_host_planes(inflx_model* model, int op, const double* p, size_t P, size_t n_p, double* out,
                            const double* start_stop, size_t N0, size_t N1, size_t row_begin, size_t row_count,
                            size_t first_plane, size_t n_planes);

/*
 * Generalised sweep, device-resident result: `d_out` is device memory of at least
 * P*row_count*N1*K*8 bytes on the model's device (`d_out_bytes` is checked); the kernel is
 * enqueued on `stream` (a hipStream_t; NULL = the model's own stream) and the call returns without
 * synchronising.  This is what the multi-GPU sharding and the benchmark use.
 * `p` is copied into pinned memory owned by the model before the call returns: the caller may free or
 * change it immediately, and consecutive calls with different parameters need no synchronisation.
 */
int inflx_sweep_device(inflx_model* model, int op, const double* p, size_t P, size_t n_p, void* d_out,
                       size_t d_out_bytes, const double* start_stop, size_t N0, size_t N1, size_t row_begin,
                       size_t row_count, int layout, void* stream);

/*
 * Which kernels a sweep of this shape takes (introspection for tests and profiles; no launch):
 *   plan[0] inflx_path; for INFLX_PATH_ROW_STREAM also plan[1] = parameter rows per row-table batch,
 *   plan[2] = number of batches the call is cut into, plan[3] = replicas of a row's table entry; for INFLX_PATH_COL_STREAM
 *   plan[1] = parameter rows per column-table batch, plan[2] = number of batches;
 *   for INFLX_PATH_TILE plan[1] = parameter rows per launch, plan[2] = number of launches, plan[3] = grid rows per workgroup
 *   tile of the first launch (the full height for large launches, lower for launches of fewer than ~4096 tiles).
 */
typedef enum inflx_path {
  INFLX_PATH_TILE = 0,       /* inflx_sweep_tile_*: some model value depends on x[1]                    */
  INFLX_PATH_ROW_STREAM = 1, /* inflx_sweep_rowvals_* + inflx_sweep_rowstream6/_planes (row-only model) */
  INFLX_PATH_ROWS = 2,       /* inflx_sweep_rows_*: row-only model, result shape the streams do not cover */
  INFLX_PATH_COL_STREAM = 3  /* inflx_sweep_colvals_* + inflx_sweep_colstream (no value depends on x[0])      */
} inflx_path;
int inflx_sweep_plan(const inflx_model* model, int op, size_t P, size_t N1, size_t row_count, int layout, uint32_t plan[4]);

/*
 * Per-call options of the device-result sweeps (the *_ex entry points; the plain ones pass INFLX_SWEEP_DEFAULT).
 *   INFLX_SWEEP_FORCE_TILE  evaluate EVERY grid point in the tile kernels (one lane per grid point, inflx_sweep_tile_*), also for a
 *                           model whose values ignore a grid axis and would otherwise take a broadcast path (one evaluated line
 *                           + store stream).  That is what the reference does for every model -- its loop calls the five model
 *                           functions at every point whatever they depend on (src/anguelova.rs:526-539) -- and the results are
 *                           the broadcast path's bit for bit; the flag exists so that the per-lane rate of such a workload can be
 *                           measured and the two paths compared (bench.py `c1_tile_path_*`, tests/test_parity_gpu.py).
 */
typedef enum inflx_sweep_flags {
  INFLX_SWEEP_DEFAULT = 0,
  INFLX_SWEEP_FORCE_TILE = 1
} inflx_sweep_flags;
int inflx_sweep_device_ex(inflx_model* model, int op, const double* p, size_t P, size_t n_p, void* d_out,
                          size_t d_out_bytes, const double* start_stop, size_t N0, size_t N1, size_t row_begin,
                          size_t row_count, int layout, void* stream, unsigned flags);
int inflx_sweep_plan_ex(const inflx_model* model, int op, size_t P, size_t N1, size_t row_count, int layout, unsigned flags,
                        uint32_t plan[4]);

/*
 * Host helper threads (no launch, no device needed).  The host-result paths start helper threads -- page residency ahead of the
 * device-to-host copy, the streaming-store fill of results that are constant along a grid axis.  Their number comes from ONE
 * budget per process, read once: the CPUs of the scheduler affinity mask, cut down to the smallest cgroup CPU quota between the
 * process's cgroup and the root (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us); INFLX_HOST_THREADS overrides it.  The
 * reference sizes its rayon pool the same way (`threads` = 0 -> every core the process has, src/anguelova.rs:467,524-525).  A
 * multi-device call divides the budget among the devices at work.  out = {budget, residency helpers, fill helpers} of one device
 * pipeline when `devices_at_work` pipelines run at once (0 is read as 1).
 */
int inflx_host_threads(unsigned devices_at_work, unsigned out[3]);

/* As inflx_sweep_device, `repeats` times back to back between two HIP events recorded on the
 * launch stream; returns the mean duration of one sweep in milliseconds (synchronises).  A sweep of a
 * model whose values do not depend on x[1] is two launches (per-row evaluation, then the store stream);
 * with `dominant_only` == 1 only the dominant one -- the store stream -- is repeated and timed; with
 * `dominant_only` == 2 the full sweeps are enqueued as in mode 0 and the value returned is the time spent
 * between event pairs recorded around every launch of the dominant kernel, per sweep: its duration inside
 * the pipeline (side-stream evaluation overlapping, cross-stream waits in place). */
int inflx_sweep_device_timed(inflx_model* model, int op, const double* p, size_t P, size_t n_p, void* d_out,
                             size_t d_out_bytes, const double* start_stop, size_t N0, size_t N1, size_t row_begin,
                             size_t row_count, int layout, void* stream, int repeats, int dominant_only,
                             float* ms_per_launch);
/*
 * The same with the timing mode by name and the inflx_sweep_flags of inflx_sweep_device_ex:
 *   INFLX_TIME_BACK_TO_BACK   mode 0 above: `repeats` sweeps enqueued back to back between two events -- the THROUGHPUT of a scan:
 *                             the tables (per-row values) of sweep n+1 are evaluated on a side stream under the kernels of sweep n;
 *   INFLX_TIME_DOMINANT_ONLY  mode 1;   INFLX_TIME_IN_PIPELINE  mode 2;
 *   INFLX_TIME_SINGLE_CALL    what ONE call costs a caller whose handle is idle (one call = one sweep, reference
 *                             python/inflatox/consistency_conditions.py:290-300): before every repetition the call waits until
 *                             nothing of this handle is left on the device, then brackets one whole inflx_sweep_device_ex call --
 *                             stage tables / per-row evaluation AND the sweep kernel -- with two events on the launch stream;
 *                             returns the mean over `repeats` calls.
 */
typedef enum inflx_timing {
  INFLX_TIME_BACK_TO_BACK = 0,
  INFLX_TIME_DOMINANT_ONLY = 1,
  INFLX_TIME_IN_PIPELINE = 2,
  INFLX_TIME_SINGLE_CALL = 3
} inflx_timing;
int inflx_sweep_device_timed_ex(inflx_model* model, int op, const double* p, size_t P, size_t n_p, void* d_out,
                                size_t d_out_bytes, const double* start_stop, size_t N0, size_t N1, size_t row_begin,
                                size_t row_count, int layout, void* stream, int repeats, int mode, unsigned flags,
                                float* ms_per_launch);

/*
 * Running summary of the six complete_analysis outputs over a sweep (no counterpart in the reference's
 * native module; its users compute such statistics afterwards with numpy, e.g. np.nanmax in
 * tests/test_doc.py:58).  NaN values are ignored, +-Inf count as values; min/max are +Inf/-Inf for a
 * quantity that is NaN everywhere.
 */
typedef struct inflx_summary {
  double min[6];     /* per quantity k: consistency, epsilon_V, epsilon_H, eta, delta, omega */
  double max[6];
  uint64_t count[6]; /* number of non-NaN values */
} inflx_summary;

/*
 * complete_analysis sweep (AoS layout) with the summary reduced on the device inside the sweep kernels
 * (wave-wide butterfly reduction + one set of f64 atomics per wavefront).  `d_out` may be NULL: the sweep
 * then only evaluates and reduces and writes no result array.  Synchronous: returns when the summary is
 * in `*summary`.
 */
int inflx_sweep_device_stats(inflx_model* model, const double* p, size_t P, size_t n_p, void* d_out, size_t d_out_bytes,
                             const double* start_stop, size_t N0, size_t N1, size_t row_begin, size_t row_count,
                             void* stream, inflx_summary* summary);

/* wait for everything enqueued on the model's own stream (under INFLX_SF_FAIL this is where the asynchronous device-resident
 * sweeps report a special-function error) */
int inflx_synchronize(inflx_model* model);

/*
 * Special functions outside their domain.  The reference links GSL for sympy's Bessel and hypergeometric functions
 * (python/inflatox/compiler.py:123-212) and, when the artefact says USE_GSL = 1, installs an error handler that prints the reason
 * and panics (compiler.py:145-149 `err_setup`, src/dylib.rs:141-148, src/err.rs:86-103): a sweep that evaluates, say, K_nu at
 * x <= 0 anywhere on its grid does not return.  The device counterparts (csrc/inflx_sf.h) return NaN for the point and set a bit in
 * the code object's status word; what the host makes of it is the handle's policy:
 *   INFLX_SF_FAIL  (default when USE_GSL = 1) -- every call that hands results to the host (the inflx_sweep_host* family, the named
 *                  sweeps, inflx_sweep_on_trajectory, inflx_sweep_device_stats, the *_multi forms, and inflx_synchronize for
 *                  the asynchronous device-resident sweeps) returns INFLX_ERR_GSL, with the reference handler's first line in
 *                  inflx_last_error(), AFTER the result has been written: the caller's array is complete, NaN at the points;
 *                  a call that integrates trajectories (inflx_solve_eom and every entry point that follows its error policy) returns
 *                  INFLX_ERR_GSL if and only if a bit is set AND a lane of the call stopped INFLX_EOM_NONFINITE -- the adaptive step
 *                  control retries a trial step that left a function's domain with a shorter one, which sets the bit in a lane that
 *                  goes on inside the domain -- and clears the bits otherwise.  (A retried trial in one lane together with an
 *                  unrelated INFLX_EOM_NONFINITE in another still fails the call.)  inflx_kinematics and inflx_masses evaluate
 *                  given states and fail on any bit;
 *   INFLX_SF_QUIET (default otherwise)        -- NaN at the points, INFLX_OK.
 * inflx_sf_status: OR of the bits (inflx_sf_bits) set since they were last cleared, after waiting for the handle's streams;
 * `clear` != 0 resets them.  Reported conditions: the argument domains GSL documents (nu >= 0; Y, K, y_l for x > 0; J_nu, I_nu, j_l
 * for x >= 0; 0F1 / 1F1 / 2F1 with the lower parameter a non-positive integer; 2F1 outside -1 <= x < 1; 2F0 for x > 0) and this
 * implementation's own refusals.  A NaN argument is not an error (it propagates, as through GSL's comparisons).  NOT reported:
 * overflow and underflow (+-inf / 0 here; GSL_EOVRFLW / GSL_EUNDRFLW reach the reference's handler too).  GSL itself is not part of the
 * reference's sources or of this image: which arguments it rejects is taken from its manual, not from a run.
 */
int inflx_sf_status(inflx_model* model, unsigned* bits, int clear);
int inflx_sf_policy(inflx_model* model, int policy);
/* the artefact's USE_GSL global (0 / 1): Compiler(link_gsl=True), compiler.py:558, dylib.rs:135-141 */
int inflx_uses_gsl(const inflx_model* model);
/* 1 when the row pass of a row-only model (`<artefact>.rowpass`, CompilationArtifact.ensure_rowpass) was found beside the artefact
 * and its broadcast sweeps evaluate their rows with it; 0 when they use the per-row kernels of the core object (slower by some
 * microseconds per sweep, same results) or the model is not row-only */
int inflx_has_row_pass(const inflx_model* model);

/*
 * One call, several GPUs.  The reference's knob for "use the whole machine" is the `threads` argument of its sweeps:
 * threads = None -> 0 -> a rayon pool over all cores (python/inflatox/consistency_conditions.py:297,
 * src/anguelova.rs:185,236,524-540).  Here the workers are the node's GPUs: an `inflx_multi` is the model artefact opened
 * on several devices (`devices` NULL or n_dev <= 0: every visible device; the same device may be listed more than once),
 * and one call splits the outermost axis of the sweep into one contiguous balanced block per device --
 *   the parameter axis when P >= devices, else the grid's row axis (inflx_shard_plan: plan = {axis (0 parameter rows,
 *   1 grid rows), p_begin, p_count, row_begin, row_count}, the first n % world parts get one item more) --
 * runs every device's pipeline (launch, device-to-host copy, page residency) on a host thread of its own and lets each
 * device copy its slab straight into its place in the caller's array.  No exchange between devices is needed: every grid
 * point and every parameter row is independent (the reference's threads do not communicate either).
 *   inflx_sweep_host_multi:        as inflx_sweep_host for the whole grid; `out` is the whole (P, N0, N1, K) [AOS] or
 *                                  (P, K, N0, N1) [SOA] array; `max_devices` = 0 uses every device of the handle, k > 0 the
 *                                  first k; `progress` != 0 prints the start / finish lines and, for calls longer than
 *                                  0.5 s, progress lines (time to completion, grid points/s, percentage: the figures of the
 *                                  reference's progress bar, src/anguelova.rs:42-50) to stderr
 *   inflx_complete_analysis_multi: the drop-in shape of libinflx_rs.complete_analysis (anguelova.rs:458-465) with
 *                                  `threads` = 0: every device of the handle, k: at most k
 *   inflx_sweep_stats_multi:       the summary of inflx_sweep_device_stats over the whole grid, every device reducing its
 *                                  block inside its sweep kernels (no array is written), combined on the host
 * Results are bit-identical to the single-device calls whatever the split: a grid point's value depends on its index
 * and parameter row only.
 */
typedef struct inflx_multi inflx_multi;
int inflx_shard_plan(size_t P, size_t N0, int world, int rank, size_t plan[5]);
int inflx_open_multi(const char* artefact_path, const int* devices, int n_dev, inflx_multi** out);
void inflx_close_multi(inflx_multi* multi);
int inflx_multi_device_count(const inflx_multi* multi);
inflx_model* inflx_multi_handle(const inflx_multi* multi, int index); /* the handle of device `index` (owned by `multi`) */
int inflx_sweep_host_multi(inflx_multi* multi, int op, const double* p, size_t P, size_t n_p, double* out,
                           const double* start_stop, size_t N0, size_t N1, int layout, int progress, size_t max_devices);
int inflx_complete_analysis_multi(inflx_multi* multi, const double* p, size_t n_p, double* out, const double* start_stop,
                                  size_t N0, size_t N1, int progress, size_t threads);
int inflx_sweep_stats_multi(inflx_multi* multi, const double* p, size_t P, size_t n_p, const double* start_stop, size_t N0,
                            size_t N1, size_t max_devices, inflx_summary* summary);
/*
 * Device-resident results on several GPUs (no counterpart in the reference; the exchange step SURVEY section 8e allows
 * "when the result must be device-resident on every GPU").
 *   inflx_sweep_device_multi:    device k sweeps its block (inflx_shard_plan with world = the handle's device count, rank = k)
 *                                into d_out[k], device memory ON device k laid out as the block; asynchronous, enqueued on
 *                                streams[k] (NULL array / entry: the handle's own stream).  No data crosses a link.
 *   inflx_sweep_allgather_multi: every d_full[k] (device memory on device k, the whole (P, N0, N1, K) AOS array) holds the
 *                                whole result on return.  Each device sweeps its block in place into its slice of its own
 *                                buffer and pushes the slice to every peer with hipMemcpyPeerAsync on a stream per peer:
 *                                xGMI is point to point, the n - 1 pushes of a device use n - 1 links at once (a direct
 *                                all-to-all broadcast, slab / link-rate instead of a ring's (n - 1) steps).  Synchronous.
 */
int inflx_sweep_device_multi(inflx_multi* multi, int op, const double* p, size_t P, size_t n_p, void* const* d_out,
                             const size_t* d_out_bytes, const double* start_stop, size_t N0, size_t N1, int layout,
                             void* const* streams);
int inflx_sweep_allgather_multi(inflx_multi* multi, int op, const double* p, size_t P, size_t n_p, void* const* d_full,
                                size_t d_full_bytes, const double* start_stop, size_t N0, size_t N1);
/*
 *   inflx_sweep_allgather_multi_ex: the same call with the exchange step chosen by the caller --
 *     INFLX_GATHER_PEER_PUSH  the direct pushes described above (what inflx_sweep_allgather_multi does; any split, also
 *                             several handles on one device);
 *     INFLX_GATHER_RCCL       ONE in-place ncclAllGather over xGMI per contiguous image (the whole array when the parameter
 *                             axis is split, one per parameter row when grid rows are), all of them fused in one RCCL group
 *                             and enqueued on every device's sweep stream behind its sweep: the collective BASELINE.json's
 *                             north_star names ("one RCCL ncclAllGather (equal slabs ...)").  Needs equal
 *                             blocks (the split axis divides by the device count), one device per handle and a buffer per
 *                             device; INFLX_ERR_SHAPE / INFLX_ERR_ARG otherwise.  RCCL is bound at run time (the copy already
 *                             mapped into the process if there is one, e.g. PyTorch's, else librccl.so.1): libinflx_hip.so
 *                             does not link it, and a caller that never asks for it never loads it.
 *                             EXPERIMENTAL until a run on two or more GPUs has passed: no node with more than one GPU has been
 *                             available to this build, so the collective has executed with one rank only; the (send, recv, count) of
 *                             every rank are checked against inflx_shard_plan on the host (tests/host_units.cpp).  On an error the
 *                             call waits for every device's streams before it returns.
 */
typedef enum inflx_gather {
  INFLX_GATHER_PEER_PUSH = 0,
  INFLX_GATHER_RCCL = 1
} inflx_gather;
int inflx_sweep_allgather_multi_ex(inflx_multi* multi, int op, const double* p, size_t P, size_t n_p, void* const* d_full,
                                   size_t d_full_bytes, const double* start_stop, size_t N0, size_t N1, int gather);

/*
 * Background trajectories (the reference's inflatox.background.solve_eom, src/background_solver.rs): B trajectories of the model's
 * equations of motion, one GPU lane each (csrc/inflx_background.h).  State (phi^0, phi^1, chi^0, chi^1, H, N); H starts from the
 * Friedmann constraint H0 = sqrt((V + G_ab chi^a chi^b / 2) / 3), N and t from 0.
 *   p          (P, n_p) parameter rows, P = 1 (shared) or B (one per trajectory)
 *   init       (B, 4): phi^0, phi^1, chi^0, chi^1
 *   rows       rows per trajectory: row 0 is the initial state, row k the state after k*substeps accepted steps
 *   method     INFLX_EOM_RK4 (step doubling) or INFLX_EOM_RKF (Fehlberg 4(5))
 *   max_err    error bound of the adaptive step (absolute Euclidean norm over phi, chi, H); dt > 0: fixed step, no error control
 *   flags      INFLX_EOM_STOP_AT_END: a trajectory stops at the first accepted step with epsilon_H >= 1 (the row it stops in holds
 *              that state); INFLX_EOM_FINAL_ONLY: no rows are kept -- `states` is (B, 6) and `t` (B,): where each trajectory stopped
 *   states     (B, rows, 6) phi^0, phi^1, chi^0, chi^1, H, N;  t (B, rows);  efolds (B,): N at epsilon_H = 1 (linear in epsilon_H
 *              across the step), NaN unless the trajectory ended;  status (B,) inflx_eom_status;  last_row (B,): the last row that
 *              holds a state (the rows after it are NaN)
 * Every output except `status` may be NULL.  The object `<artefact>.background` (CompilationArtifact.ensure_background()) is loaded on
 * first use and must carry the artefact's MODEL_TAG; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs to
 * another model.  Runs on the handle's stream; returns when the outputs are complete.
 * The kernels write rows trajectory fastest; a transpose kernel (inflx_bg_rows_transpose) puts every pass of at most
 * min(2^20, 2 GiB / (rows x 56 B)) trajectories into the layout above on the device, and two contiguous copies take it to `states`
 * and `t`.  INFLX_EOM_HOST_SCATTER: the rows are copied out as the kernels wrote them and rearranged by the calling thread instead
 * -- the same values, much slower; a call with rows >= 2341 (fewer than 2^14 trajectories per pass) always runs that way.
 */
typedef enum inflx_eom_method {
  INFLX_EOM_RK4 = 0,
  INFLX_EOM_RKF = 1
} inflx_eom_method;
typedef enum inflx_eom_flags {
  INFLX_EOM_STOP_AT_END = 1,
  INFLX_EOM_FINAL_ONLY = 2,
  INFLX_EOM_SAMPLE_T = 4,   /* inflx_solve_eom_sampled: the samples are times, not e-fold counts */
  INFLX_EOM_HOST_SCATTER = 8 /* inflx_solve_eom: rearrange the rows on the host, not with the transpose kernel */
} inflx_eom_flags;
typedef enum inflx_modes_flags {
  INFLX_MODES_TENSOR = 8 /* inflx_mode_spectra: the lanes carry one tensor mode instead of the scalar perturbations, `out` is (8, n) */
} inflx_modes_flags;
typedef enum inflx_eom_status {
  INFLX_EOM_COMPLETE = 0,   /* every requested step was taken */
  INFLX_EOM_ENDED = 1,      /* epsilon_H reached 1 (INFLX_EOM_STOP_AT_END) */
  INFLX_EOM_NONFINITE = 2,  /* the state or the equations of motion at it are not finite */
  INFLX_EOM_REJECTED = 3,   /* 50 consecutive rejected steps */
  INFLX_EOM_UNDERFLOW = 4,  /* the step no longer moves t */
  INFLX_EOM_TARGET = 5      /* N reached its target (inflx_solve_eom_to_efolds); every sample was emitted (inflx_solve_eom_sampled) */
} inflx_eom_status;
int inflx_solve_eom(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, size_t rows, size_t substeps,
                    int method, double max_err, double dt, unsigned flags, double* states, double* t, double* efolds, int8_t* status,
                    int64_t* last_row);

/*
 * inflx_solve_eom with a device-resident result: `d_states` (B, rows, 6) and `d_t` (B, rows) are device pointers of
 * `d_states_bytes` and `d_t_bytes` bytes (INFLX_ERR_SHAPE when one is too small for B x rows; either pointer may be NULL).  Every
 * window of rows is transposed straight into them on the device: no row crosses to the host.  `efolds`, `status` and `last_row` are
 * host arrays as for inflx_solve_eom.  INFLX_EOM_STOP_AT_END is the only flag (INFLX_EOM_FINAL_ONLY is INFLX_ERR_ARG: that mode
 * keeps no rows).  Everything runs on `stream` (a hipStream_t; NULL: the handle's stream), and the call returns after it has
 * synchronised that stream: the device arrays are complete on return, and work enqueued on `stream` afterwards sees them.
 */
int inflx_solve_eom_device(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, size_t rows,
                           size_t substeps, int method, double max_err, double dt, unsigned flags, double* d_states, size_t d_states_bytes,
                           double* d_t, size_t d_t_bytes, double* efolds, int8_t* status, int64_t* last_row, void* stream);

/*
 * The state of B trajectories where each has made `target[l]` e-folds: inflx_solve_eom's final-only run with one more way for a lane
 * to stop.  A lane stops at the first accepted step whose new state has N >= its target, with INFLX_EOM_TARGET and the state where
 * N equals the target inside that step: the cubic Hermite interpolant over the step (fourth order, as the steppers), N set to the
 * target exactly.  A target <= 0 is reached by the initial state.  With INFLX_EOM_STOP_AT_END (the only flag) a lane whose
 * epsilon_H reaches 1 before its target stops with INFLX_EOM_ENDED as in inflx_solve_eom.
 *   p, P, n_p, init, B, method, max_err, dt    as for inflx_solve_eom
 *   target     (B,): the target on N of every trajectory; a NaN is INFLX_ERR_ARG
 *   max_steps  accepted steps a trajectory may take (INFLX_EOM_COMPLETE when they run out before the target)
 *   states     (B, 6), t (B,), eps_h (B,): where each trajectory stopped -- for INFLX_EOM_TARGET the located state, its time and
 *              epsilon_H at it (eps_h is NaN for every other status);  efolds (B,): N at epsilon_H = 1, meaningful for
 *              INFLX_EOM_ENDED;  status (B,) inflx_eom_status
 * Every output except `status` may be NULL.  Memory on the device is O(B); launches stop once no trajectory runs any more.
 */
int inflx_solve_eom_to_efolds(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, const double* target,
                              size_t max_steps, int method, double max_err, double dt, unsigned flags, double* states, double* t,
                              double* eps_h, double* efolds, int8_t* status);

/*
 * The state of B trajectories at every point of one list of samples shared by all of them: e-fold counts, or times with
 * INFLX_EOM_SAMPLE_T.  The steps are inflx_solve_eom's; after every accepted step a lane emits the samples that step passed
 * (sample <= N, or <= t, at the step's end), each located inside the step with the cubic Hermite interpolant of
 * inflx_solve_eom_to_efolds: for N the sample's e-fold count exactly and t interpolated -- bit for bit what
 * inflx_solve_eom_to_efolds returns for that target --, for t the sample's time exactly and N interpolated.  A sample equal to 0 is
 * the initial state.  With INFLX_EOM_STOP_AT_END, in the step that ends inflation only the samples up to epsilon_H = 1 are emitted
 * (N_s <= N_end; t_s <= t0 + f h with N_end's fraction f of the step), and a trajectory that is past the end at the start emits
 * only a sample at 0.
 *   p, P, n_p, init, B, method, max_err, dt    as for inflx_solve_eom
 *   samples    (S,): finite, >= 0, strictly increasing; 1 <= S < 2^32
 *   max_steps  accepted steps a trajectory may take
 *   flags      INFLX_EOM_STOP_AT_END, INFLX_EOM_SAMPLE_T
 *   out        (S, 8, B), trajectory fastest: phi^0, phi^1, chi^0, chi^1, H, N, t, epsilon_H at every sample; NaN for a sample that
 *              the trajectory did not reach
 *   efolds     (B,): N at epsilon_H = 1, meaningful for INFLX_EOM_ENDED;  n_stored (B,): the samples emitted (the first n_stored)
 *   status     (B,): INFLX_EOM_TARGET once all S samples are emitted, INFLX_EOM_COMPLETE when max_steps ran out first, the other
 *              codes as for inflx_solve_eom (INFLX_EOM_NONFINITE also when a located state is not finite)
 * `efolds` and `n_stored` may be NULL.  Memory on the device is O(B S) for at most 2^28 bytes of samples per pass of lanes; every pass
 * is copied into `out` as it is, with one strided copy.  Launches stop once no trajectory runs any more.
 */
int inflx_solve_eom_sampled(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, const double* samples,
                            size_t S, size_t max_steps, int method, double max_err, double dt, unsigned flags, double* out, double* efolds,
                            int8_t* status, uint32_t* n_stored);

/*
 * Trajectory kinematics at n states (csrc/inflx_kinematics.h): a post-pass over states of the background solver -- rows of
 * inflx_solve_eom, states of inflx_solve_eom_to_efolds or inflx_solve_eom_sampled -- or over any other states.  With kin =
 * G_ab chi^a chi^b, vchi = d_a V chi^a and cross = (d_0 V chi_1 - d_1 V chi_0) / sqrt(det G), chi_a = G_ab chi^b:
 *   plane 0  eps_H     = kin / 2 / H^2, bit for bit the solver's own epsilon_H at that state
 *   plane 1  eta_par   = 3 + vchi / (H kin) = -sigma_ddot / (H sigma_dot)
 *   plane 2  omega     = cross / (kin H): the turn rate per e-fold Omega / H, SIGNED (> 0: the trajectory turns counter-clockwise in the
 *                        (phi^0, phi^1) chart); the sweeps' omega >= 0 corresponds to its absolute value
 *   plane 3  sigma_dot = sqrt(kin)
 *   plane 4  V_sigma   = vchi / sigma_dot, the gradient along the velocity
 *   plane 5  V_N       = cross / sigma_dot, the gradient normal to it; V_sigma^2 + V_N^2 = |dV|^2
 * IEEE arithmetic throughout.  A component of a state that is not finite (NaN, +-inf) gives six NaNs there, whether or not the model
 * depends on that component (0 * y[c], summed over the five, is added to every plane); a state at rest (kin = 0) gives eps_H = 0, sigma_dot = 0
 * and NaN in the other four.
 *   p          (P, n_p) parameter rows, P = 1 (shared) or n / traj_len: one per run of traj_len consecutive states
 *   states     state i is states[i * ld + c], c = 0..4 = phi^0, phi^1, chi^0, chi^1, H; ld >= 5 (6 for the rows of inflx_solve_eom, whose
 *              sixth column is not read).  The array holds (n - 1) * ld + 5 doubles at least.
 *   traj_len   >= 1 and a divisor of n
 *   out        (6, n): the planes above
 * The object `<artefact>.kinematics` (CompilationArtifact.ensure_kinematics()) is loaded on first use and must carry the artefact's
 * MODEL_TAG and this library's layout word INFLX_KIN_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs
 * to another model or layout.  It is independent of `<artefact>.background`.  Arguments are checked before anything touches the
 * device; n = 0 succeeds and launches nothing.  Runs on the handle's stream in chunks of at most 2^20 states -- each copied in,
 * evaluated and its six plane segments copied out -- and returns when `out` is complete.  A USE_GSL artefact follows the error
 * policy of inflx_solve_eom (inflx_sf_policy).
 */
int inflx_kinematics(inflx_model* model, const double* p, size_t P, size_t n_p, const double* states, size_t n, size_t ld, size_t traj_len,
                     double* out);

/*
 * inflx_kinematics on device arrays: `d_states` (d_states_bytes >= ((n - 1) * ld + 5) * 8) and `d_out` (d_out_bytes >= 6 * n * 8) are
 * device pointers, INFLX_ERR_SHAPE when a buffer is too small; `p` is a host array.  One launch on `stream` (a hipStream_t; NULL: the
 * handle's stream); like inflx_solve_eom_device the call returns after it has synchronised that stream: `d_out` is complete on
 * return, and work enqueued on `stream` afterwards sees it.  No state and no result crosses to the host.
 */
int inflx_kinematics_device(inflx_model* model, const double* p, size_t P, size_t n_p, const void* d_states, size_t d_states_bytes, size_t n,
                            size_t ld, size_t traj_len, void* d_out, size_t d_out_bytes, void* stream);

/*
 * Entropic masses at n states (csrc/inflx_masses.h): like inflx_kinematics a post-pass over states, with the same arguments and the
 * same T, N and sign of omega.  With V_;ab = d_a d_b V - Gamma^c_ab d_c V, kin = G_ab chi^a chi^b and n^b = eps^be chi_e /
 * sqrt(det G), chi_e = G_ed chi^d (the unit normal times sigma_dot):
 *   plane 0  V_TT   = V_;ab chi^a chi^b / kin, the covariant Hesse matrix along the velocity
 *   plane 1  V_TN   = V_;ab chi^a n^b / kin
 *   plane 2  V_NN   = V_;ab n^a n^b / kin, ... and across it
 *   plane 3  ricci  = the Ricci scalar R = 2 K of the field-space metric: 2 / r^2 on a sphere, -2 / L^2 on diag(1, L^2 sinh^2(phi / L))
 *   plane 4  eps_H  = kin / 2 / H^2, bit for bit inflx_kinematics' plane 0
 *   plane 5  omega  = the signed turn rate per e-fold, bit for bit inflx_kinematics' plane 2
 *   plane 6  M_eff2 = V_NN / H^2 + eps_H R - omega^2, the entropic mass of the sub-horizon Q_s equation in units of H^2
 *   plane 7  mu_s2  = V_NN / H^2 + eps_H R + 3 omega^2, the super-horizon effective entropic mass in units of H^2
 * IEEE arithmetic throughout.  A component of a state that is not finite (NaN, +-inf) gives eight NaNs there, whether or not the
 * model depends on that component; a state at rest (kin = 0) gives eps_H = 0, a finite ricci and NaN in the other six.
 *   p, states, traj_len   as for inflx_kinematics
 *   out                   (8, n): the planes above
 * The object `<artefact>.masses` (CompilationArtifact.ensure_masses()) is loaded on first use and must carry the artefact's MODEL_TAG
 * and this library's layout word INFLX_MASS_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs to
 * another model or layout.  It is independent of `<artefact>.background` and `<artefact>.kinematics`.  Arguments are checked before
 * anything touches the device; n = 0 succeeds and launches nothing.  Runs on the handle's stream in chunks of at most 2^20 states --
 * each copied in, evaluated and its eight plane segments copied out with one strided copy -- and returns when `out` is complete.  A
 * USE_GSL artefact follows the error policy of inflx_solve_eom (inflx_sf_policy).
 */
int inflx_masses(inflx_model* model, const double* p, size_t P, size_t n_p, const double* states, size_t n, size_t ld, size_t traj_len, double* out);

/*
 * inflx_masses on device arrays: `d_states` (d_states_bytes >= ((n - 1) * ld + 5) * 8) and `d_out` (d_out_bytes >= 8 * n * 8) are
 * device pointers, INFLX_ERR_SHAPE when a buffer is too small; `p` is a host array.  One launch on `stream` (a hipStream_t; NULL: the
 * handle's stream); like inflx_kinematics_device the call returns after it has synchronised that stream.  No state and no result
 * crosses to the host.
 */
int inflx_masses_device(inflx_model* model, const double* p, size_t P, size_t n_p, const void* d_states, size_t d_states_bytes, size_t n, size_t ld,
                        size_t traj_len, void* d_out, size_t d_out_bytes, void* stream);

/*
 * Super-horizon transfer functions of B trajectories (csrc/inflx_transfer.h): the background of inflx_solve_eom_sampled and, carried
 * along it from the initial state (horizon exit), the entropic perturbation q = Q_s / Q_s(0) and the curvature perturbation it
 * sources.  With kin, cross and m[.] as for inflx_kinematics and inflx_masses, Omega = cross / kin = omega H, eps = kin / (2 H^2):
 *   dq/dt = u      du/dt = -3 H u - H^2 mu_s2 q      dr/dt = 2 Omega q sqrt(eps_star / eps)      (q, u, r)(0) = (1, H0 dq_dN, 0)
 * T_SS = q sqrt(eps_star / eps) = S / S_star with S = Q_s / sqrt(2 eps), and T_RS = r: R(N) = R_star + T_RS S_star.  Q_s is measured
 * along T turned COUNTER-CLOCKWISE in the chart -- minus the N of inflx_kinematics, the side the trajectory turns towards when
 * omega > 0 --, so that dR/dN = +2 omega S with the signed omega of inflx_kinematics.
 *   p, P, n_p, init, B, method, dt    as for inflx_solve_eom
 *   dq_dn      (B,) finite: dq/dN at the start -- or NULL: the slowly decaying root of lambda^2 + (3 - eps_star) lambda + mu_s2_star
 *              = 0 (its real part when the discriminant is negative), from the model at every lane's initial state
 *   samples    (S,): e-fold counts since the start; finite, >= 0, strictly increasing; 1 <= S < 2^32
 *   max_steps  accepted steps a trajectory may take
 *   max_err    error bound of the adaptive step: the absolute Euclidean norm over phi, chi, H, q, u and r (eight components), so an
 *              adaptive run takes other steps than inflx_solve_eom_sampled; with dt > 0 the background is that call's bit for bit
 *   flags      INFLX_EOM_STOP_AT_END
 *   out        (S, 10, B), trajectory fastest: phi^0, phi^1, chi^0, chi^1, H, N, t, epsilon_H, T_SS, T_RS at every sample, located
 *              as inflx_solve_eom_sampled locates them (q and r by the same cubic Hermite interpolant); NaN for a sample that the
 *              trajectory did not reach.  A sample at 0 has T_SS = 1 and T_RS = 0 exactly
 *   ends       (B, 2): T_SS and T_RS at epsilon_H = 1, linear across the step that ends inflation at N_end's own fraction of it;
 *              meaningful for INFLX_EOM_ENDED (NaN otherwise)
 *   efolds, status, n_stored    as for inflx_solve_eom_sampled, except that a sample emitted by the initial state (N = 0) never
 *              stops a lane: INFLX_EOM_TARGET comes from the step that emits the last sample, and samples = {0} runs on to the
 *              end of inflation or max_steps.  A lane whose initial state has kin = 0, or whose eps_star,
 *              omega_star or mu_s2_star is not finite, is INFLX_EOM_NONFINITE at once and all its outputs are NaN
 * `ends`, `efolds` and `n_stored` may be NULL.  The object `<artefact>.transfer` (CompilationArtifact.ensure_transfer()) is loaded on
 * first use and must carry the artefact's MODEL_TAG and this library's layout word INFLX_TR_ABI; INFLX_ERR_SYMBOL when it does not
 * exist, INFLX_ERR_VERSION when it belongs to another model or layout.  Arguments are checked before anything touches the device.
 * Runs on the handle's stream in passes of at most 2^20 lanes and 2^28 bytes of samples, launches of at most 256 accepted steps,
 * and stops launching once no trajectory runs any more.  A USE_GSL artefact follows the error policy of inflx_solve_eom.
 */
int inflx_transfer_functions(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, const double* dq_dn,
                             const double* samples, size_t S, size_t max_steps, int method, double max_err, double dt, unsigned flags, double* out,
                             double* ends, double* efolds, int8_t* status, uint32_t* n_stored);

/*
 * Mode functions and power spectra of n lanes, one per (trajectory, wavenumber) (csrc/inflx_modes.h): the background of
 * inflx_solve_eom and, carried along it from the Bunch-Davies vacuum at the lane's start, the two independent complex solutions
 * I = sigma, s of the full linear perturbation equations in the adiabatic-entropic frame (e_s = T turned counter-clockwise, the
 * direction of inflx_transfer_functions), in the scaled variables Qt = a_in sqrt(2 k) Q, Pt = a_in sqrt(2 k) D_t Q, with
 * Qt^I_J = delta_IJ and Pt^I_J = (-i kappa - H_in) delta_IJ at the start and k / a = kappa e^-N, N the lane's own e-fold count.
 *   p, P, n_p, method, dt    as for inflx_solve_eom; P is 1 or n
 *   init       (n, 4): phi^0, phi^1, chi^0, chi^1 at the lane's start; H from the Friedmann constraint
 *   kappa      (n,): k / a at the lane's start
 *   n_target   (n,): the e-fold count since the lane's start at which the lane is evaluated; NaN: no target
 *   max_steps  accepted steps a lane may take
 *   max_err    error bound of the adaptive step: the absolute Euclidean norm over phi, chi, H, the eight Qt and the eight Pt / kappa
 *   flags      INFLX_EOM_STOP_AT_END, INFLX_MODES_TENSOR (below)
 *   out        (22, n), lane fastest: P_R, P_S, C_RS = kappa^2 sum_I (|Qt^I_sigma|^2, |Qt^I_s|^2, Re Qt^I_sigma conj Qt^I_s) /
 *              (8 pi^2 eps); the 16 mode components Qt^I_J then Pt^I_J at index 4 I + 2 J + (0: real, 1: imaginary); N; t; eps_H --
 *              where the lane stopped with INFLX_EOM_TARGET (the state located at its target, cubic Hermite in all components) or
 *              INFLX_EOM_ENDED (linear across the step that ends inflation at N_end's own fraction, eps_H = 1); NaN for a lane that
 *              stopped otherwise
 *   efolds     (n,): N at epsilon_H = 1, meaningful for INFLX_EOM_ENDED
 *   status     (n,): inflx_eom_status; INFLX_EOM_NONFINITE at once for a lane at rest at the start (no direction), with coefficients
 *              that are not finite there, or with a kappa that is not a positive finite number
 * `efolds` may be NULL.  The object `<artefact>.modes` (CompilationArtifact.ensure_modes()) is loaded on first use and must carry the
 * artefact's MODEL_TAG and this library's layout word INFLX_MD_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it
 * belongs to another model or layout.  Arguments are checked before anything touches the device.  Runs on the handle's stream in
 * passes of at most 2^20 lanes, launches of at most 256 accepted steps, and stops launching once no lane runs any more.  A USE_GSL
 * artefact follows the error policy of inflx_solve_eom.
 *
 * With INFLX_MODES_TENSOR in `flags` the lanes carry one tensor mode instead (csrc/inflx_tensor.h): the same arguments, checks, passes
 * and statuses, and along the same background one complex amplitude ht = a_in sqrt(2 k) u, pt = d ht/dt, with u = h / 2 the
 * canonically normalised amplitude of one polarisation in reduced Planck units:
 *     d ht/dt = pt,   d pt/dt = -3 H pt - kappa^2 e^-2N ht,   ht = 1 and pt = -i kappa - H_in at the start.
 *   max_err    the absolute Euclidean norm over phi, chi, H, the two components of ht and the two of pt / kappa
 *   out        (8, n), lane fastest: P_T = 2 kappa^2 |ht|^2 / pi^2 (both polarisations: 2 H^2 / pi^2 in de Sitter, and P_T / P_R = 16 eps
 *              in single-field slow roll); Re ht, Im ht, Re pt, Im pt; N; t; eps_H -- located and interpolated as above
 *   status     a lane at rest at the start is NOT an error here (a tensor mode needs no direction in field space): it runs like any
 *              other; INFLX_EOM_NONFINITE for a state or right-hand side that is not finite or a kappa that is not a positive
 *              finite number
 * The object is `<artefact>.tensor` (CompilationArtifact.ensure_tensor()) with the layout word INFLX_TN_ABI, loaded on first use and
 * refused in the same two ways; the modes object is not needed.  A call without the flag is not affected by one with it.
 */
int inflx_mode_spectra(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t n, const double* kappa,
                       const double* n_target, size_t max_steps, int method, double max_err, double dt, unsigned flags, double* out, double* efolds,
                       int8_t* status);

#ifdef __cplusplus
}
#endif

/* the delta-N expansion (derivatives of N with respect to the initial fields, local f_NL): its entry point is declared in a header of its own */
#include "inflx_hip_deltan.h"
/* the spectra of a mode sampled along its evolution (inflx_mode_spectra with samples): likewise */
#include "inflx_hip_evolution.h"
/* stochastic e-folds (Langevin noise on every trajectory, moments of N over the realisations): likewise */
#include "inflx_hip_stochastic.h"
/* first-passage histograms (the distribution of N over realisations on lanes that are used again): likewise */
#include "inflx_hip_distribution.h"
/* horizon crossings (the state where ln(a H) reaches given values, the located end of inflation): likewise */
#include "inflx_hip_crossing.h"
/* reheating (trajectories whose fields decay into radiation, to the point where the radiation dominates): likewise */
#include "inflx_hip_reheating.h"

#endif /* INFLX_HIP_H */
