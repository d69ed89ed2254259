/* Part of include/inflx_hip.h, which includes it: the stochastic e-fold entry point of libinflx_hip.so.  Include inflx_hip.h, not this file. */
#ifndef INFLX_HIP_STOCHASTIC_H
#define INFLX_HIP_STOCHASTIC_H

#ifndef INFLX_HIP_H
#error "include inflx_hip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The separate-universe Langevin equation on B points x R realisations, one lane each (csrc/inflx_stochastic.h): every lane is a
 * trajectory of inflx_solve_eom's stepper that stops at the end of inflation, and after every accepted step from N_0 to N_1 its fields
 * take an Ito-Euler kick
 *     phi^a <- phi^a + s (H / 2 pi) sqrt(N_1 - N_0) e^a_alpha xi^alpha - 1/2 s^2 (H / 2 pi)^2 (N_1 - N_0) G^bc Gamma^a_bc
 * with e e^T = G^-1 (lower triangular) and xi two independent standard normals; H follows the change of the energy density at the same
 * velocities, which are not kicked.  The e-fold count N_end at epsilon_H = 1 is a random variable; the call returns its moments over
 * the realisations of every point, and every lane's result on request.
 *   p, P, n_p, method, max_err, dt    as for inflx_solve_eom; P is 1 or B: point b uses row b for all its realisations
 *   init         (B, 4): phi^0, phi^1, chi^0, chi^1; H starts from the Friedmann constraint
 *   R            realisations per point, in [1, 2^20]; lane b R + r is realisation r of point b
 *   streams      (B,) a 32-bit id per point -- or NULL: the point's index
 *   seed         the random numbers are Philox4x32-10 (csrc/inflx_philox.h) with the key `seed` and the counter (step low, step high, r,
 *                stream), `step` the lane's accepted-step index: a realisation depends on (seed, stream, r) alone, not on B, R, the
 *                pass or the launch it runs in
 *   noise_scale  s, finite and >= 0; 0 gives the classical trajectory bit for bit
 *   dN_max       > 0 (may be infinite): an adaptive run tries no step longer than dN_max / H, so that no kick covers more e-folds
 *   N_stop       > 0, or NaN: none.  The step that passes N_stop is located as inflx_solve_eom_to_efolds locates it; the lane takes a
 *                kick over the e-folds up to N_stop and stops there with INFLX_EOM_TARGET
 *   max_steps    accepted steps a lane may take
 *   moments      (12, B), point fastest: mean, m2, m3, m4 (central moments sum (N - mean)^k / n), minimum and maximum of N_end over the
 *                lanes that ended inflation (NaN when none did), then the number of lanes with inflx_eom_status 0 .. 5
 *   samples      (7, B R), lane fastest: N (N_end of a lane that ended inflation, the e-fold count where it stopped otherwise),
 *                phi^0, phi^1, chi^0, chi^1, H there and the status as a double -- or NULL
 * A lane's status: INFLX_EOM_ENDED (epsilon_H reached 1: in a step, N_end interpolated as inflx_solve_eom does and no kick follows, or
 * after a kick, N_end = N there), INFLX_EOM_TARGET, INFLX_EOM_NONFINITE (the state, the equations of motion or the radicand of H are
 * not finite after a step or a kick), INFLX_EOM_REJECTED, INFLX_EOM_UNDERFLOW, or INFLX_EOM_COMPLETE: max_steps ran out.
 * The object `<artefact>.stochastic` (CompilationArtifact.ensure_stochastic()) is loaded on first use and must carry the artefact's
 * MODEL_TAG and this library's layout word INFLX_ST_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs to
 * another model or layout.  Arguments are checked before anything touches the device.  Runs on the handle's stream in passes of whole
 * points, at most 2^20 lanes, launches of at most 256 accepted steps, and stops launching once no lane runs any more.  A USE_GSL
 * artefact follows the error policy of inflx_solve_eom.
 */
int inflx_stochastic_efolds(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, size_t R, const uint32_t* streams,
                            uint64_t seed, double noise_scale, double dN_max, double N_stop, size_t max_steps, int method, double max_err, double dt,
                            double* moments, double* samples);

#ifdef __cplusplus
}
#endif
#endif /* INFLX_HIP_STOCHASTIC_H */
