// Entropic masses: the covariant Hesse matrix of the potential on a trajectory's own tangent and normal, the curvature of field
// space and the two entropic masses of a two-field model at one state (inflatox_amd.background.masses).
//
// A state is y = (phi^0, phi^1, chi^0, chi^1, H), the background solver's (csrc/inflx_background.h).  T, N, their orientation and
// the sign of omega are the kinematics' (csrc/inflx_kinematics.h): sigma_dot^2 = kin = G_ab chi^a chi^b, T^a = chi^a / sigma_dot,
// N_a = sqrt(det G) eps_ab T^b, so that N^b = eps^be T_e / sqrt(det G) with T_e = G_ed T^d -- no inverse metric.  With V_;ab =
// d_a d_b V - Gamma^c_ab d_c V and n^b = eps^be chi_e / sqrt(det G) = sigma_dot N^b (|n|^2 = kin), the generated inflx_mass_point
// (staging.emit_masses_header) gives m[0] = V_;ab chi^a chi^b, m[1] = V_;ab chi^a n^b, m[2] = V_;ab n^a n^b and m[3] = R:
//     V_TT = m[0] / kin      V_TN = m[1] / kin      V_NN = m[2] / kin
//     ricci  = R, the Ricci scalar (twice the Gaussian curvature): 2 / r^2 on a sphere, -2 / L^2 on diag(1, L^2 sinh^2(phi / L))
//     eps_H  = kin / 2 / H^2 and omega = cross / (kin H): the kinematics' expressions, literally, on the same inflx_eom_point and
//              inflx_kin_point, so that they are the kinematics' values bit for bit
//     M_eff2 = V_NN / H^2 + eps_H R - omega^2      the entropic mass in the sub-horizon equation of Q_s, in units of H^2
//                                                  (sigma_dot^2 R / 2 = eps_H H^2 R)
//     mu_s2  = V_NN / H^2 + eps_H R + 3 omega^2    the super-horizon effective entropic mass, in units of H^2
//
// Edge values follow the kinematics' rules, by plain IEEE arithmetic (IEEE divisions, no quick reciprocal, no branch):
//   - the taint term, the sum of 0 * y[c] over the five components -- 0 when all are finite, NaN otherwise -- is added to all eight
//     outputs: a component that is not finite (NaN or +-inf) gives eight NaNs, also on a cyclic coordinate and also in ricci, which
//     reads neither the velocity nor H.  Adding that zero changes no value: eps_H and omega stay the kinematics';
//   - a state at rest (kin = 0) gives eps_H = 0, a finite ricci and NaN in the other six (0/0: a point has no direction).
//
// INFLX_FN code over one lane's registers, so that tests/masses_twin.cpp compiles the very same text for the host.  The model
// enters through the generated inflx_eom_point, inflx_kin_point and inflx_mass_point.
#pragma once

enum InflxMassQuantity {
  INFLX_MASS_V_TT = 0,
  INFLX_MASS_V_TN = 1,
  INFLX_MASS_V_NN = 2,
  INFLX_MASS_RICCI = 3,
  INFLX_MASS_EPS_H = 4,
  INFLX_MASS_OMEGA = 5,
  INFLX_MASS_M_EFF2 = 6,
  INFLX_MASS_MU_S2 = 7,
  INFLX_MASS_QUANTITIES = 8,
};

// y: phi^0, phi^1, chi^0, chi^1, H;  out: the eight quantities in InflxMassQuantity's order
INFLX_FN void inflx_mass_eval(const double* y, const double* __restrict__ p, double* out) {
  double e[4], k[2], m[4];
  inflx_eom_point(y[0], y[1], y[2], y[3], p, e);
  inflx_kin_point(y[0], y[1], y[2], y[3], p, k);
  inflx_mass_point(y[0], y[1], y[2], y[3], p, m);
  const double H = y[4], kin = e[3], cross = k[1];
  const double taint = 0.0 * y[0] + 0.0 * y[1] + 0.0 * y[2] + 0.0 * y[3] + 0.0 * y[4];  // 0, or NaN when a component is not finite
  const double eps_H = 0.5 * kin / (H * H) + taint;  // inflx_kin_eval's, literally
  const double omega = cross / (kin * H) + taint;    // inflx_kin_eval's, literally
  const double v_nn = m[2] / kin + taint;
  const double ricci = m[3] + taint;
  const double base = v_nn / (H * H) + eps_H * ricci;
  out[INFLX_MASS_V_TT] = m[0] / kin + taint;
  out[INFLX_MASS_V_TN] = m[1] / kin + taint;
  out[INFLX_MASS_V_NN] = v_nn;
  out[INFLX_MASS_RICCI] = ricci;
  out[INFLX_MASS_EPS_H] = eps_H;
  out[INFLX_MASS_OMEGA] = omega;
  out[INFLX_MASS_M_EFF2] = base - omega * omega;
  out[INFLX_MASS_MU_S2] = base + 3.0 * (omega * omega);
}
