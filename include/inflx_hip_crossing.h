/* Part of include/inflx_hip.h, which includes it: the horizon-crossing entry points of libinflx_hip.so.  Include inflx_hip.h, not this file. */
#ifndef INFLX_HIP_CROSSING_H
#define INFLX_HIP_CROSSING_H

#ifndef INFLX_HIP_H
#error "include inflx_hip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The state of B trajectories where the comoving Hubble scale L = ln(a H) = N + ln H (a = 1 at the start, so L_0 = ln H_0) reaches
 * given values: inflx_solve_eom_sampled's lanes (the same state, equations, steppers, step control and statuses) with the event on L
 * instead of N (csrc/inflx_crossing.h).
 *   p, P, n_p, init, B, max_steps, method, max_err, dt, efolds, status    as for inflx_solve_eom_sampled
 *   flags      INFLX_EOM_STOP_AT_END
 *   offset     (B,): finite; the targets of trajectory l are offset[l] + samples[j] -- or NULL: all zero
 *   samples    (S,): finite and strictly increasing, S in [1, 2^32); a negative one is allowed
 *   out        (S, 8, B), trajectory fastest: y[0..5], t and eps_H at crossing j; NaN where it was not emitted
 *   n_stored   (B,): the crossings emitted;  n_before (B,): the targets below L_0, which belong to modes outside the horizon before
 *              the start and are not emitted.  The emitted ones are j = n_before .. n_before + n_stored - 1.  Either may be NULL.
 * Crossing j is emitted from the first accepted step whose end state has L >= its target, at the theta in (0, 1] where the step's cubic
 * Hermite interpolants have N(theta) + ln H(theta) = target: Newton's iteration in a bracket, bisection for an iterate that leaves it or
 * is not finite, at most 64 iterations, stopping at 1e-15 in theta.  All six components come from the interpolant at theta, t = t0 +
 * theta h, eps_H from the model there; neither N nor H is overwritten.  A target equal to L_0 is the initial state.  With
 * INFLX_EOM_STOP_AT_END the step that ends inflation emits the crossings whose located N is <= N_end only.  INFLX_EOM_TARGET once no
 * target is left, INFLX_EOM_NONFINITE for a located state that is not finite.  A trajectory goes on from the step's end state: its
 * steps are those of inflx_solve_eom.  The object `<artefact>.crossing` (CompilationArtifact.ensure_crossing()) is loaded on first use
 * and must carry the artefact's MODEL_TAG and this library's layout word INFLX_HX_ABI; INFLX_ERR_SYMBOL when it does not exist,
 * INFLX_ERR_VERSION when it belongs to another model or layout; no other companion object is needed.  Arguments are checked before
 * anything touches the device.  Passes, launches and the error policy of a USE_GSL artefact are inflx_solve_eom_sampled's.
 */
int inflx_solve_eom_crossings(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, const double* offset,
                              const double* samples, size_t S, size_t max_steps, int method, double max_err, double dt, unsigned flags, double* out,
                              double* efolds, int8_t* status, uint32_t* n_stored, uint32_t* n_before);

/*
 * The end of inflation of B trajectories, located on the dense output: a trajectory stops in the first accepted step whose end state
 * has eps_H >= 1, and the state where eps_H = 1 on the step's cubic Hermite interpolant is found by the Illinois iteration that the
 * delta-N centres use (csrc/inflx_deltan.h), eps_H evaluated through the model.
 *   states (B, 6): y[0..5] there -- N_end is states[., 5], H_end states[., 4];  t (B,);  eps_h (B,): eps_H there, 1 up to the iteration's
 *   bracket;  status (B,): INFLX_EOM_ENDED where it was found, INFLX_EOM_RUNNING (0) when max_steps ran out first.  states, t, eps_h
 *   hold the state the trajectory stopped at for every other status.  Any of states, t, eps_h may be NULL.
 * A trajectory that starts at or past the end ends at its initial state, N_end = 0.  This N_end differs from inflx_solve_eom's, which
 * is linear in eps_H across the step, at second order in the step.  The object is `<artefact>.crossing`, as above.
 */
int inflx_inflation_end(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, size_t max_steps, int method,
                        double max_err, double dt, double* states, double* t, double* eps_h, int8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* INFLX_HIP_CROSSING_H */
