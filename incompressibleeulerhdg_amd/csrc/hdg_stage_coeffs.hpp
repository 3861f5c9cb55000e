// Stage residuals of the IMEX scheme as linear combinations of the stage velocities Q_j and the forcing slots b_j
// (timesteppers/hdg_imex.py:367-413 of the reference): functions of the tableau in hdg_config alone.  Plain C++.
//   r_i = sum cq[j] Q_j + sum cb[j] b_j   (mass matrix = identity in the orthonormal modal basis)
#pragma once
#include <vector>

#include "../../include/hdg_mi355x.h"

namespace hdg {

inline void residual_coeffs(const hdg_config& cfg, int i, std::vector<double>& cq, std::vector<double>& cb) {
  const int s = cfg.nstages;
  cq.assign(s, 0.0); cb.assign(s, 0.0);
  cq[0] = 1.0;
  for (int j = 1; j < i; j++) {  // column 0 is never read (hdg_imex.py:377)
    double aij = cfg.a_impl[i * s + j];
    if (aij != 0.0) {
      double f = aij / cfg.a_impl[j * s + j];
      std::vector<double> q2, b2;
      residual_coeffs(cfg, j, q2, b2);
      cq[j] += f;
      for (int l = 0; l < s; l++) { cq[l] -= f * q2[l]; cb[l] -= f * b2[l]; }
    }
  }
  for (int j = 0; j < i; j++) {
    double ae = cfg.a_expl[i * s + j];
    if (ae != 0.0) cb[j] += cfg.dt * ae;
  }
}
inline void final_residual_coeffs(const hdg_config& cfg, std::vector<double>& cq, std::vector<double>& cb) {
  const int s = cfg.nstages;
  cq.assign(s, 0.0); cb.assign(s, 0.0);
  cq[0] = 1.0;
  for (int i = 1; i < s; i++) {
    double bi = cfg.b_impl[i];
    if (bi != 0.0) {
      double f = bi / cfg.a_impl[i * s + i];
      std::vector<double> q2, b2;
      residual_coeffs(cfg, i, q2, b2);
      cq[i] += f;
      for (int l = 0; l < s; l++) { cq[l] -= f * q2[l]; cb[l] -= f * b2[l]; }
    }
  }
  for (int i = 0; i < s; i++)
    if (cfg.b_expl[i] != 0.0) cb[i] += cfg.dt * cfg.b_expl[i];
}

}  // namespace hdg
