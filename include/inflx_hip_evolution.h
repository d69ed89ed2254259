/* Part of include/inflx_hip.h, which includes it: the mode-evolution entry point of libinflx_hip.so.  Include inflx_hip.h, not this file. */
#ifndef INFLX_HIP_EVOLUTION_H
#define INFLX_HIP_EVOLUTION_H

#ifndef INFLX_HIP_H
#error "include inflx_hip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The spectra of a mode sampled along its evolution: inflx_mode_spectra's scalar lanes (include/inflx_hip.h, csrc/inflx_modes.h --
 * the same state, equations, vacuum, steppers, step control, stop rules and statuses), each of which returns, besides its 22 values
 * where it stops, P_R, P_S, C_RS, N, t and eps_H at every point of one list of e-fold counts shared by all lanes, the way
 * inflx_solve_eom_sampled returns a trajectory's states (csrc/inflx_evolution.h).  Every lane is integrated once.
 *   p, P, n_p, init, n, kappa, n_target, max_steps, method, max_err, dt, out, efolds, status    as for inflx_mode_spectra
 *   flags      INFLX_EOM_STOP_AT_END (INFLX_MODES_TENSOR is refused)
 *   shift      (n,): finite; the local e-fold count of sample k of lane l is samples[k] - shift[l], formed by that one subtraction
 *   samples    (S,): finite and strictly increasing, S in [1, 2^32); a negative one is allowed
 *   sampled    (S, 6, n), lane fastest: P_R, P_S, C_RS, the lane's local N (samples[k] - shift[l]), its local t and eps_H at sample k
 * A sample before the lane's start (local count < 0) stays NaN; one at its start is the vacuum, P_R = P_S = kappa^2 / (8 pi^2 eps_0),
 * C_RS = 0.  Every other sample is emitted from the accepted step that passes it, located and interpolated exactly as
 * inflx_mode_spectra's target: what that call returns with n_target = samples[k] - shift[l], bit for bit, since the lane goes on from
 * the step's end state and its steps are those of the run without samples.  The step that ends inflation emits the samples up to
 * N_end only, the step that reaches the target those up to the target; a sample whose values are not finite stops the lane with
 * INFLX_EOM_NONFINITE.  A lane keeps the samples it passed whatever its status, and NaN for the others.  `out`, `efolds` and `status`
 * are inflx_mode_spectra's for the same lanes, bit for bit, with one addition: a lane without a target (NaN) in a call without
 * INFLX_EOM_STOP_AT_END stops with INFLX_EOM_TARGET once its last sample is passed, and its 22 final values stay NaN.
 * `efolds` may be NULL.  The object `<artefact>.evolution` (CompilationArtifact.ensure_evolution()) is loaded on first use and must
 * carry the artefact's MODEL_TAG and this library's layout word INFLX_EV_ABI; INFLX_ERR_SYMBOL when it does not exist,
 * INFLX_ERR_VERSION when it belongs to another model or layout; the modes object is not needed.  Arguments are checked before
 * anything touches the device.  Runs on the handle's stream in passes whose lanes' results, (22 + 6 S) doubles each, fit a device
 * buffer of 256 MiB (whole workgroups of 256 lanes where more than one fits, at least one lane), launches of at most 256 accepted
 * steps, and stops launching once no lane runs any more.  A USE_GSL artefact follows the error policy of inflx_solve_eom.
 */
int inflx_mode_evolution(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t n, const double* kappa,
                         const double* n_target, const double* shift, const double* samples, size_t S, size_t max_steps, int method, double max_err,
                         double dt, unsigned flags, double* out, double* sampled, double* efolds, int8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* INFLX_HIP_EVOLUTION_H */
