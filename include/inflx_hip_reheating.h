/* Part of include/inflx_hip.h, which includes it: the reheating entry point of libinflx_hip.so.  Include inflx_hip.h, not this file. */
#ifndef INFLX_HIP_REHEATING_H
#define INFLX_HIP_REHEATING_H

#ifndef INFLX_HIP_H
#error "include inflx_hip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* the status of a reheating trajectory beyond inflx_eom_status (0..5), the delta-N statuses (7, 8) and the two Python-only codes (6, 9) */
typedef enum inflx_rh_status {
  INFLX_RH_STATUS_REHEATED = 10 /* rho_r / (3 H^2) reached omega_r; the trajectory's state is the one located there */
} inflx_rh_status;

/*
 * B trajectories whose fields decay into a radiation bath, each followed until the bath dominates (csrc/inflx_reheating.h).  The state
 * is y = (phi^0, phi^1, chi^0, chi^1, H, N, rho_r) with one constant decay rate per trajectory:
 *     dchi^a/dt = -eom^a - (3 H + Gamma) chi^a,  dH/dt = V - 3 H^2 + rho_r / 3,  dN/dt = H,  drho_r/dt = -4 H rho_r + Gamma G_ab chi^a chi^b,
 * H_0 from the constraint 3 H^2 = V + G_ab chi^a chi^b / 2 + rho_r, N = 0 and t = 0 at the start.  Steppers, step control, first dt and
 * the bounds on rejections and dt are inflx_solve_eom's; the error norm is the absolute Euclidean norm over phi, chi, H and rho_r.
 *   p, P, n_p, init, B, max_steps, method, max_err, dt    as for inflx_inflation_end
 *   gamma      (B,): finite, >= 0
 *   rho_r0     (B,): finite, >= 0 -- or NULL: all zero
 *   omega_r    in (0, 1)
 *   states     (B, 7): y[0..6] where each trajectory stopped;  t (B,);  h_start (B,): H_0.  Any of the three may be NULL.
 *   status     (B,): INFLX_RH_STATUS_REHEATED, INFLX_EOM_RUNNING (0) when max_steps ran out first, or INFLX_EOM_NONFINITE /
 *              _REJECTED / _UNDERFLOW
 * A trajectory stops at the first accepted step whose end state has rho_r - 3 omega_r H^2 >= 0, and `states` / `t` are then the
 * point of the step's cubic Hermite interpolant where rho_r(theta) - 3 omega_r H(theta)^2 = 0: the Illinois iteration inside a
 * bracket, at most 64 iterations, stopping at a zero or a bracket of 1e-15 in theta; no model evaluation.  A trajectory that starts
 * with rho_r0 >= omega_r 3 H_0^2 is REHEATED at its initial state.  For every other status the last state the trajectory held is
 * returned.  Gamma = 0 with rho_r0 = 0 never reheats: INFLX_EOM_RUNNING after max_steps, not an error.  Every oscillation of the
 * fields is resolved, so the cost grows with the oscillation frequency over Gamma.  The object `<artefact>.reheating`
 * (CompilationArtifact.ensure_reheating()) is loaded on first use and must carry the artefact's MODEL_TAG and this library's layout
 * word INFLX_RH_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs to another model or layout; no other
 * companion object is needed.  Arguments are checked before anything touches the device.  Passes, launches and the error policy of a
 * USE_GSL artefact are inflx_inflation_end's.
 */
int inflx_reheating(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, const double* gamma, const double* rho_r0, size_t B,
                    double omega_r, size_t max_steps, int method, double max_err, double dt, double* states, double* t, double* h_start, int8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* INFLX_HIP_REHEATING_H */
