// Trajectory kinematics: epsilon_H, eta_parallel and the turn rate of a two-field model at one state (inflatox_amd.background.kinematics).
//
// A state is y = (phi^0, phi^1, chi^0, chi^1, H), the background solver's (csrc/inflx_background.h).  With sigma_dot^2 = kin =
// G_ab chi^a chi^b, T^a = chi^a / sigma_dot the unit tangent and N_a the unit normal of (T, N) in the orientation of the
// coordinates, N_a = sqrt(det G) eps_ab T^b:
//     V_sigma = T^a d_a V = vchi / sigma_dot            vchi  = d_a V chi^a                              (inflx_kin_point o[0])
//     V_N     = N^a d_a V = cross / sigma_dot           cross = (d_0 V chi_1 - d_1 V chi_0) / sqrt(det G) (inflx_kin_point o[1])
// and, from the equations of motion D_t chi^a = -3 H chi^a - G^ab d_b V:
//     sigma_ddot = -3 H sigma_dot - V_sigma             eta_par = -sigma_ddot / (H sigma_dot) = 3 + vchi / (H kin)
//     D_t T^a    = -(V_N / sigma_dot) N^a               omega   = Omega / H = cross / (kin H)
// omega is the turn rate per e-fold and SIGNED.  N is T turned clockwise in the (x0, x1) chart (flat space: T = (1, 0) gives
// N = (0, -1)); omega > 0 where the gradient has a component along +N, so that the force -dV turns the trajectory towards -N:
// counter-clockwise in the chart.  The sweeps' omega >= 0 (GeneralisedAL.complete_analysis) corresponds to its absolute value.
//
// Edge values, by plain IEEE arithmetic (IEEE divisions and square roots, no quick reciprocal, no branch):
//   - a component of the state that is not finite (NaN or +-inf) gives six NaNs, whether or not the model reads that component: a
//     model with a cyclic coordinate never looks at it, and sigma_dot, V_sigma and V_N do not divide by H, so the sum of 0 * y[c]
//     over the five components -- 0 when all are finite, NaN otherwise -- is added to every output.  Adding that zero changes no
//     value (at most the sign of a zero result; eps_H is never -0): eps_H stays the integrator's bit for bit.  A parameter that makes the model NaN at the state gives NaN where it enters;
//   - a state at rest (kin = 0) gives eps_H = 0, sigma_dot = 0 and NaN in the other four (0/0: a point has no direction).
//
// INFLX_FN code over one lane's registers, so that tests/kinematics_twin.cpp compiles the very same text for the host.  The model
// enters through the generated inflx_eom_point (staging.emit_eom_header) and inflx_kin_point (staging.emit_kinematics_header).
#pragma once

enum InflxKinQuantity {
  INFLX_KIN_EPS_H = 0,
  INFLX_KIN_ETA_PAR = 1,
  INFLX_KIN_OMEGA = 2,
  INFLX_KIN_SIGMA_DOT = 3,
  INFLX_KIN_V_SIGMA = 4,
  INFLX_KIN_V_N = 5,
  INFLX_KIN_QUANTITIES = 6,
};

// y: phi^0, phi^1, chi^0, chi^1, H;  out: the six quantities in InflxKinQuantity's order
INFLX_FN void inflx_kin_eval(const double* y, const double* __restrict__ p, double* out) {
  double e[4], k[2];
  inflx_eom_point(y[0], y[1], y[2], y[3], p, e);
  inflx_kin_point(y[0], y[1], y[2], y[3], p, k);
  const double H = y[4], kin = e[3], vchi = k[0], cross = k[1];
  const double taint = 0.0 * y[0] + 0.0 * y[1] + 0.0 * y[2] + 0.0 * y[3] + 0.0 * y[4];  // 0, or NaN when a component is not finite
  const double sigma_dot = sqrt(kin);
  out[INFLX_KIN_EPS_H] = 0.5 * kin / (H * H) + taint;  // the integrator's inflx_bg_epsilon, literally
  out[INFLX_KIN_ETA_PAR] = 3.0 + vchi / (H * kin) + taint;
  out[INFLX_KIN_OMEGA] = cross / (kin * H) + taint;
  out[INFLX_KIN_SIGMA_DOT] = sigma_dot + taint;
  out[INFLX_KIN_V_SIGMA] = vchi / sigma_dot + taint;
  out[INFLX_KIN_V_N] = cross / sigma_dot + taint;
}
