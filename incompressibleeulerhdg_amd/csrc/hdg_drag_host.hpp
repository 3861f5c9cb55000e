// Host packing of the linear drag term, plain C++ without HIP: stand-alone g++ programs reach it as they
// reach hdg_tables.hpp (tests/host/drag_check.cpp).
//
//   - sigma (x) (u - u_s),   sigma >= 0 given by its three vertex values per cell (P1 on the cell, broken across cells).
//
// In the orthonormal modal basis a cell's block of M^-1 D is  (sigma_0 I + (sigma_1 - sigma_0) L_1 + (sigma_2 - sigma_0) L_2) (x) I_2
// with the reference tables of CoriolisTables (hdg_tables.hpp); vertex order: the cell's entry in `cells` on a general mesh,
// (x0,y0), (x1,y0), (x0,y1) for the lower and (x1,y1), (x0,y1), (x1,y0) for the upper triangle of a square.  The block is a
// sigma-weighted mass matrix, so its spectrum lies between the smallest and the largest vertex value: rho(M^-1 D) <= S, the
// largest value given.
#pragma once
#include <cmath>
#include <string>
#include <vector>

namespace hdg {

constexpr int DRAG_REGIONS = 4;  // HDG_DRAG_REGIONS of include/hdg_drag.h

// the first fault of the three arrays of a setting, or the empty string; target (n_target doubles) and region may be null
inline std::string drag_validate(const double* sigma, long nc, const double* target, long n_target, const int* region) {
  if (sigma)
    for (long n = 0; n < 3 * nc; n++)
      if (!(sigma[n] >= 0.0) || !std::isfinite(sigma[n]))
        return "sigma[" + std::to_string(n / 3) + "][" + std::to_string(n % 3) + "] = " + std::to_string(sigma[n]) + " is not a finite value >= 0";
  if (target)
    for (long n = 0; n < n_target; n++)
      if (!std::isfinite(target[n])) return "target[" + std::to_string(n) + "] is not finite";
  if (region)
    for (long c = 0; c < nc; c++)
      if (region[c] < 0 || region[c] >= DRAG_REGIONS)
        return "region[" + std::to_string(c) + "] = " + std::to_string(region[c]) + " is outside 0 .. " + std::to_string(DRAG_REGIONS - 1);
  return std::string();
}

// S = the largest vertex value: the derived bound of rho(M^-1 D); 0 for null
inline double drag_bound(const double* sigma, long nc) {
  double S = 0.0;
  if (sigma)
    for (long n = 0; n < 3 * nc; n++) S = std::fmax(S, sigma[n]);
  return S;
}

// Structured meshes: public cell 2 (j nx + i) + s of a rank's own ny rows  ->  the cell index of the kernels,
// (s R + j + gh) nx + i, R rows per shape plane with gh ghost rows below the owned ones.  The arrays are a rank's own (like its
// fields), so the strip's offset in the global mesh does not enter.
inline long drag_device_cell(int nx, int R, int gh, long pub) {
  const int s = (int)(pub & 1);
  const long sq = pub >> 1;
  const int j = (int)(sq / nx), i = (int)(sq - (long)j * nx);
  return ((long)s * R + (j + gh)) * nx + i;
}

// the three coefficient planes sigma_0, sigma_1 - sigma_0, sigma_2 - sigma_0 in the kernels' cell order, plane stride
// Nc = 2 nx R; ghost and padding rows hold zeros
inline std::vector<double> drag_pack_planes(const double* sigma, int nx, int ny, int R, int gh) {
  const long Nc = 2L * nx * R;
  std::vector<double> out((size_t)(3 * Nc), 0.0);
  for (long pub = 0; pub < 2L * nx * ny; pub++) {
    const long c = drag_device_cell(nx, R, gh, pub);
    out[(size_t)c] = sigma[3 * pub];
    out[(size_t)(Nc + c)] = sigma[3 * pub + 1] - sigma[3 * pub];
    out[(size_t)(2 * Nc + c)] = sigma[3 * pub + 2] - sigma[3 * pub];
  }
  return out;
}

// the region tags in the kernels' cell order (null: all 0)
inline std::vector<int> drag_pack_regions(const int* region, int nx, int ny, int R, int gh) {
  std::vector<int> out((size_t)(2L * nx * R), 0);
  if (region)
    for (long pub = 0; pub < 2L * nx * ny; pub++) out[(size_t)drag_device_cell(nx, R, gh, pub)] = region[pub];
  return out;
}

// general meshes: (sigma_0, sigma_1 - sigma_0, sigma_2 - sigma_0) per cell, nc x 3 in the cells' own order
inline std::vector<double> drag_pack_general(const double* sigma, long nc) {
  std::vector<double> out((size_t)(3 * nc));
  for (long c = 0; c < nc; c++) {
    out[(size_t)(3 * c)] = sigma[3 * c];
    out[(size_t)(3 * c + 1)] = sigma[3 * c + 1] - sigma[3 * c];
    out[(size_t)(3 * c + 2)] = sigma[3 * c + 2] - sigma[3 * c];
  }
  return out;
}

}  // namespace hdg
