/* Part of include/inflx_hip.h, which includes it: the first-passage histogram entry point of libinflx_hip.so.  Include inflx_hip.h, not this file. */
#ifndef INFLX_HIP_DISTRIBUTION_H
#define INFLX_HIP_DISTRIBUTION_H

#ifndef INFLX_HIP_H
#error "include inflx_hip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The distribution of the e-fold count N_end of inflx_stochastic_efolds' realisations, as a histogram per point, over R realisations
 * that need not fit the device at once (csrc/inflx_distribution.h).  Every point has L lanes.  A lane runs a realisation to its stop,
 * adds it to the point's counts, draws the point's next ticket t and starts realisation first_realisation + t afresh from the point's
 * initial state, until the R tickets have run out.  A realisation is the one inflx_stochastic_efolds runs for the same (seed, stream,
 * r): the Philox counter is (its own accepted-step index, r, stream), so neither the lane nor the launch it runs in can change it,
 * and the counts are integers: the result does not depend on scheduling, bit for bit.
 *   p, P, n_p, init, B, streams, seed, noise_scale, dN_max, max_steps, method, max_err, dt    as for inflx_stochastic_efolds (there is
 *                no N_stop: every N would be the same)
 *   R            realisations per point, in [1, 2^32 - 1]
 *   first_realisation   the realisations are first_realisation .. first_realisation + R - 1; first_realisation + R <= 2^32.  Calls over
 *                adjoining ranges add up to the call over their union
 *   lanes_per_point     L, a multiple of 64 and at most 2^20 -- or 0: the smallest multiple of 64 that is >= R, but no more than an equal
 *                share of the 2^20 lanes of a pass, floor(2^20 / B) in whole wavefronts, and no less than 64.  The result does not
 *                depend on it; the time does (few lanes leave the device idle, R lanes leave nothing to use again)
 *   bins         bins per point, in [1, 2^20]
 *   ranges, n_ranges    (n_ranges, 2): lo and hi of every point, n_ranges = B -- or of all points, n_ranges = 1; finite, hi > lo
 *   hist         (B, bins + 2) uint32: below, bin 0 .. bins - 1, above, over the realisations that ended inflation.  With
 *                scale = bins / (hi - lo) in binary64, k = floor((N - lo) * scale): N < lo (or k < 0) is below, k >= bins is above
 *                (so N = hi is above), else bin k.  This rule is the definition; the edges lo + k (hi - lo) / bins are nominal
 *   counts       (B, 6) uint32: the realisations per inflx_eom_status 0 .. 5 (0, INFLX_EOM_COMPLETE: max_steps ran out)
 * The object `<artefact>.distribution` (CompilationArtifact.ensure_distribution()) is loaded on first use and must carry the artefact's
 * MODEL_TAG and this library's layout word INFLX_PD_ABI; INFLX_ERR_SYMBOL when it does not exist, INFLX_ERR_VERSION when it belongs to
 * another model or layout.  The stochastic object is not involved.  Arguments are checked before anything touches the device.  Runs
 * on the handle's stream in passes of whole points, at most 2^20 lanes and 256 MiB of counts, launches of at most 256 accepted steps
 * per lane, until every lane has retired; memory is O(B L + B bins), not O(R).  The number of launches is bounded by what the
 * arguments imply, (ceil(R / min(L, R)) + 1) (ceil(max_steps / 256) + 1) + 2; past that the call fails with INFLX_ERR_DEVICE and a message that begins
 * "internal:", it never spins.  A USE_GSL artefact
 * follows the error policy of inflx_solve_eom.
 */
int inflx_stochastic_distribution(inflx_model* model, const double* p, size_t P, size_t n_p, const double* init, size_t B, size_t R, const uint32_t* streams,
                                  uint64_t seed, uint64_t first_realisation, size_t lanes_per_point, double noise_scale, double dN_max, size_t max_steps,
                                  int method, double max_err, double dt, size_t bins, const double* ranges, size_t n_ranges, uint32_t* hist,
                                  uint32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* INFLX_HIP_DISTRIBUTION_H */
