/* Part of include/inflx_hip.h, which includes it: the delta-N entry point of libinflx_hip.so.  Include inflx_hip.h, not this file. */
#ifndef INFLX_HIP_DELTAN_H
#define INFLX_HIP_DELTAN_H

#ifndef INFLX_HIP_H
#error "include inflx_hip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The delta-N expansion zeta = N_,I dphi^I + 1/2 N_,IJ dphi^I dphi^J on B stencils of 9 trajectories each (csrc/inflx_deltan.h): first
 * and second derivatives of the e-fold count N with respect to the initial fields, to a surface of uniform density shared by the
 * stencil, and the local non-Gaussianity f_NL built from them.  Member m = 3 i + j of a stencil, i, j in {0, 1, 2}, starts at the
 * centre's fields plus ((i - 1) h0, (j - 1) h1); m = 4 is the centre.  Every member is one lane of inflx_solve_eom's stepper with its
 * own adaptive step control.
 *   phase A    (skipped when `h_end` is given) every centre runs to the first accepted step with epsilon_H >= 1; the point with
 *              epsilon_H = 1 is located on the step's cubic Hermite dense output, epsilon_H evaluated through the model there; H_c and
 *              N_c are H and N of the dense output at that point
 *   phase B    all nine members run until H falls to H_c; the crossing is located on the dense output of H, and the member's result is
 *              N of the dense output there
 *   p, P, n_p, method, max_err, dt    as for inflx_solve_eom; P is 1 or B: stencil b uses row b for all nine members
 *   centre     (B, 4): phi^0, phi^1, chi^0, chi^1 of the centres (chi is not read under INFLX_DN_VELOCITY_SLOW_ROLL)
 *   vel, rule  inflx_dn_velocity, how a member's initial velocity follows: FIXED -- the centre's chi for every member; SLOW_ROLL --
 *              chi^a = -G^ab d_b V / (3 H) with H^2 = V / 3 at the member's own fields, the centre included; EXPLICIT -- `vel` (B, 9, 2).
 *              `vel` is NULL under the other two rules.  H starts from the Friedmann constraint.
 *   h0, h1     the stencil's steps, positive, in field-coordinate units
 *   h_end      (B,) H on the surface of every stencil, positive -- or NULL: phase A finds it
 *   max_steps  accepted steps a lane may take in each phase
 *   out        (21, B), stencil fastest: N of the nine members; N_,0 N_,1 (central differences); N_,00 N_,11 N_,01 (three-point, and the
 *              four corners); the covariant N_;00 N_;11 N_;01 = N_,IJ - Gamma^K_IJ N_,K; |grad N|^2 = G^IJ N_,I N_,J;
 *              f_NL = (5/6) N^;I N^;J N_;IJ / |grad N|^4; P_zeta = (H / 2 pi)^2 |grad N|^2 with the centre's initial H; the status as a
 *              double.  Metric and connection are those at the centre.
 *   surface    (2, B): H_c, and N_c of phase A (NaN when `h_end` was given) -- or NULL
 *   status     (B,): INFLX_DN_LOCATED when all nine members met the surface.  Otherwise every derived output of the stencil is NaN (the
 *              nine N are kept: NaN for a member that has none) and status = s + 16 m, with m the lowest member that failed and s its
 *              inflx_eom_status -- INFLX_EOM_COMPLETE: max_steps ran out -- or INFLX_DN_PAST_SURFACE; a centre that fails in phase A
 *              gives its status there with m = 4.
 * The object `<artefact>.deltan` (CompilationArtifact.ensure_deltan()) is loaded on first use and must carry the artefact's MODEL_TAG
 * and this library's layout word INFLX_DN_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs to another
 * model or layout.  Arguments are checked before anything touches the device.  Runs on the handle's stream in passes of whole stencils,
 * at most 2^20 lanes, launches of at most 256 accepted steps, and stops launching once no lane runs any more.  A USE_GSL artefact
 * follows the error policy of inflx_solve_eom.
 */
typedef enum inflx_dn_velocity {
  INFLX_DN_VELOCITY_FIXED = 0,
  INFLX_DN_VELOCITY_SLOW_ROLL = 1,
  INFLX_DN_VELOCITY_EXPLICIT = 2
} inflx_dn_velocity;
typedef enum inflx_dn_status {
  INFLX_DN_STATUS_LOCATED = 7,      /* the lane met its surface */
  INFLX_DN_STATUS_PAST_SURFACE = 8  /* the lane's initial H is already at or below H_c */
} inflx_dn_status;
int inflx_delta_n(inflx_model* model, const double* p, size_t P, size_t n_p, const double* centre, size_t B, const double* vel, int rule,
                  double h0, double h1, const double* h_end, size_t max_steps, int method, double max_err, double dt, double* out,
                  double* surface, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* INFLX_HIP_DELTAN_H */
