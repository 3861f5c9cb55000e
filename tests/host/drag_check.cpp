// Host check of the drag term's tables and packing (g++, no HIP): csrc/hdg_tables.hpp and csrc/hdg_drag_host.hpp.
//   drag_check block k s0 s1 s2 out.bin   forms a cell's block of M^-1 D as the kernels do, s0 I + (s1 - s0) L_1 + (s2 - s0) L_2
//                                         in the orthonormal modal basis, maps it to the nodal one (V B V^-1) and writes it
//                                         (nu, then nu x nu row-major) for tests/test_drag_cpu.py to compare with the numpy
//                                         reference entry by entry
//   drag_check pack                       its own checks: L_1, L_2 symmetric; the public -> device cell permutation a bijection
//                                         onto the owned rows for nx = 3, 12, 130 and for the two strips of a two-rank run, the
//                                         three planes and the tags where the kernels read them; S; the validation
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_drag_host.hpp"
#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"

using namespace hdg;

static int fails = 0;
static void check(bool ok, const char* what) {
  if (!ok) { fails++; std::printf("FAIL %s\n", what); }
}

static int block(int argc, char** argv) {
  if (argc != 7) { std::printf("usage: block k s0 s1 s2 out\n"); return 2; }
  const int k = std::atoi(argv[2]);
  const double s0 = std::atof(argv[3]), s1 = std::atof(argv[4]), s2 = std::atof(argv[5]);
  if (k < 1 || k > 4) { std::printf("k out of range\n"); return 2; }
  const CoriolisTables D(k);
  const Tables T(k, 1.0, 1.0, 1.0, 0);
  const int nu = D.nu;
  const dvec tab = D.general();  // what the kernels read: L_1 then L_2
  std::vector<double> B((size_t)nu * nu), tmp((size_t)nu * nu), Bn((size_t)nu * nu);
  for (int r = 0; r < nu; r++)
    for (int m = 0; m < nu; m++)
      B[(size_t)r * nu + m] = (r == m ? s0 : 0.0) + (s1 - s0) * tab[(size_t)m * nu + r] + (s2 - s0) * tab[(size_t)nu * nu + (size_t)m * nu + r];
  for (int r = 0; r < nu; r++)
    for (int m = 0; m < nu; m++) {
      long double acc = 0;
      for (int l = 0; l < nu; l++) acc += (long double)T.Vu[(size_t)r * nu + l] * B[(size_t)l * nu + m];
      tmp[(size_t)r * nu + m] = (double)acc;
    }
  for (int r = 0; r < nu; r++)
    for (int m = 0; m < nu; m++) {
      long double acc = 0;
      for (int l = 0; l < nu; l++) acc += (long double)tmp[(size_t)r * nu + l] * T.Vuinv[(size_t)l * nu + m];
      Bn[(size_t)r * nu + m] = (double)acc;
    }
  FILE* f = std::fopen(argv[6], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[6]); return 2; }
  const double head[1] = {(double)nu};
  const bool ok = std::fwrite(head, sizeof(double), 1, f) == 1 && std::fwrite(Bn.data(), sizeof(double), Bn.size(), f) == Bn.size();
  std::fclose(f);
  if (!ok) { std::printf("short write\n"); return 2; }
  std::printf("ok\n");
  return 0;
}

// one rank's strip of ny rows of an nx-wide mesh, R rows per shape plane with gh ghost rows below
static void permutation(int nx, int ny, int R, int gh) {
  const long nc = 2L * nx * ny, Nc = 2L * nx * R;
  std::vector<double> sigma((size_t)(3 * nc));
  std::vector<int> region((size_t)nc);
  for (long c = 0; c < nc; c++) {
    for (int v = 0; v < 3; v++) sigma[(size_t)(3 * c + v)] = (double)(4 * c + v + 1);
    region[(size_t)c] = (int)(c % DRAG_REGIONS);
  }
  const std::vector<double> P = drag_pack_planes(sigma.data(), nx, ny, R, gh);
  const std::vector<int> G = drag_pack_regions(region.data(), nx, ny, R, gh);
  check((long)P.size() == 3 * Nc && (long)G.size() == Nc, "sizes of the packed arrays");
  std::set<long> seen;
  bool owned = true, planes = true, tags = true, formula = true;
  for (int j = 0; j < ny; j++)
    for (int i = 0; i < nx; i++)
      for (int s = 0; s < 2; s++) {
        const long pub = 2 * ((long)j * nx + i) + s;
        const long c = drag_device_cell(nx, R, gh, pub);
        formula = formula && c == ((long)s * R + (j + gh)) * nx + i;  // rowbase(g, s, j) + i of the kernels
        const long row = (c / nx) % R;
        owned = owned && c >= 0 && c < Nc && row >= gh && row < gh + ny;
        seen.insert(c);
        planes = planes && P[(size_t)c] == sigma[(size_t)(3 * pub)] && P[(size_t)(Nc + c)] == sigma[(size_t)(3 * pub + 1)] - sigma[(size_t)(3 * pub)] &&
                 P[(size_t)(2 * Nc + c)] == sigma[(size_t)(3 * pub + 2)] - sigma[(size_t)(3 * pub)];
        tags = tags && G[(size_t)c] == region[(size_t)pub];
      }
  check(formula, "the device cell is (s R + j + gh) nx + i");
  check(owned, "every public cell lands in an owned row");
  check((long)seen.size() == nc, "the permutation is one to one");
  check(planes, "the three planes hold sigma_0, sigma_1 - sigma_0, sigma_2 - sigma_0 of the right cell");
  check(tags, "the tags of the right cell");
  long nonzero = 0;
  for (long c = 0; c < Nc; c++) nonzero += P[(size_t)c] != 0.0;
  check(nonzero == nc, "ghost and padding rows hold zeros");
  const std::vector<int> G0 = drag_pack_regions(nullptr, nx, ny, R, gh);
  bool zero = (long)G0.size() == Nc;
  for (int t : G0) zero = zero && t == 0;
  check(zero, "no tags: all 0");
  check(drag_bound(sigma.data(), nc) == (double)(4 * (nc - 1) + 3), "S is the largest vertex value");
  std::printf("nx %d ny %d R %d: %ld cells\n", nx, ny, R, nc);
}

static int pack() {
  for (int k = 1; k <= 4; k++) {
    const CoriolisTables D(k);
    double a = 0.0;
    for (int v = 0; v < 2; v++)
      for (int r = 0; r < D.nu; r++)
        for (int m = 0; m < D.nu; m++) a = std::fmax(a, std::fabs(D.L[v][(size_t)r * D.nu + m] - D.L[v][(size_t)m * D.nu + r]));
    check(a <= 1e-15, "L_1, L_2 symmetric");
    check(D.general().size() == 2 * (size_t)D.nu * D.nu, "size of the table");
  }
  const int gh = 6;
  for (int nx : {3, 12, 130}) permutation(nx, nx, nx + 2 * gh + 3, gh);
  for (int rank = 0; rank < 2; rank++) permutation(8, 4, 4 + 2 * gh + 1, gh);  // two strips of an 8 x 8 mesh: the arrays are a rank's own
  // validation and the bound
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double sg[6] = {0.0, 1.5, 0.25, 2.5, 0.0, 0.5}, tg[4] = {1.0, -2.0, 0.0, 3.0};
  int rg[2] = {0, 3};
  check(drag_validate(sg, 2, tg, 4, rg).empty() && drag_validate(sg, 2, nullptr, 0, nullptr).empty() &&
        drag_validate(nullptr, 2, nullptr, 0, nullptr).empty(), "a good setting passes");
  check(drag_bound(sg, 2) == 2.5 && drag_bound(nullptr, 2) == 0.0, "S");
  for (double bad : {-1e-300, nan, inf, -inf}) {
    double b[6];
    std::memcpy(b, sg, sizeof(b));
    b[4] = bad;
    check(!drag_validate(b, 2, tg, 4, rg).empty(), "a negative or non-finite sigma is refused");
  }
  for (double bad : {nan, inf}) {
    double b[4];
    std::memcpy(b, tg, sizeof(b));
    b[2] = bad;
    check(!drag_validate(sg, 2, b, 4, rg).empty(), "a non-finite target is refused");
  }
  for (int bad : {-1, DRAG_REGIONS}) {
    int b[2] = {0, bad};
    check(!drag_validate(sg, 2, tg, 4, b).empty(), "a tag out of range is refused");
  }
  const std::vector<double> gen = drag_pack_general(sg, 2);
  check(gen.size() == 6 && gen[0] == 0.0 && gen[1] == 1.5 && gen[2] == 0.25 && gen[3] == 2.5 && gen[4] == -2.5 && gen[5] == -2.0,
        "the general-mesh coefficients");
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "block") == 0) return block(argc, argv);
  if (argc == 2 && std::strcmp(argv[1], "pack") == 0) return pack();
  std::printf("usage: drag_check block k s0 s1 s2 out | drag_check pack\n");
  return 2;
}
