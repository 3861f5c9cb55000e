// Host check of csrc/hdg_transfer.hpp (g++, no HIP), for r in {1, 2, 3, 16} and every pair of polynomial degrees 1 .. 5:
//   children     a coarse triangle has r^2 children, r (r+1) / 2 of its own shape, no two of one class, their areas sum to the
//                parent's, and the map of a child's class is the child's own geometry: the vertices of fine cell (a, b, s),
//                written in the parent's reference coordinates from the shapes of hdg_tables.hpp, are the images of the
//                reference vertices under class_map, and lie in the reference triangle
//   reflection   child (a, b, s) of an upper parent has the class of child (r-1-a, r-1-b, 1-s) of a lower parent
//   Parseval     (1 / r^2) sum_children C C^T = I whenever the fine degree >= the coarse degree
//   constants    C[class][0][n] = delta_0n, and sum_children C[class][m][0] = r^2 delta_m0
//   hierarchy    the table of degrees (dc - 1, df - 1) is the leading block of the table of (dc, df)
//   r = 1        the quadrature gives the identity, which child_tables stores exactly
// Tolerance 1e-15 absolute (entries of size <= 1: long double tables rounded to double).
#include <cmath>
#include <cstdio>
#include <set>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_transfer.hpp"

using namespace hdg;
using namespace hdg::transfer;

static int fails = 0;
static double worst = 0.0;
static void expect(bool ok, const char* what, int r, int dc, int df) {
  if (!ok) { fails++; std::printf("FAIL %s: r = %d, degrees %d %d\n", what, r, dc, df); }
}
static bool close(long double a, long double b) {
  const double d = (double)std::fabs(a - b);
  if (d > worst) worst = d;
  return d <= 1e-15;
}

static void check_children(int r) {
  for (int S = 0; S < 2; S++) {
    const std::vector<Child> ch = children(r, S);
    expect((int)ch.size() == r * r, "child count", r, S, 0);
    int own = 0;
    double area = 0.0;
    std::set<int> classes;
    for (const Child& c : ch) {
      own += c.s == S;
      const int cls = child_class(r, S, c.a, c.b, c.s);
      expect(cls >= 0 && cls < r * r, "class range", r, S, 0);
      classes.insert(cls);
      int sigma, ox, oy;
      class_map(r, cls, sigma, ox, oy);
      area += 0.5 * sigma * sigma / ((double)r * r);
      // the fine cell's vertices in units of h relative to the coarse square's corner; reference vertices (0,0), (1,0), (0,1)
      const int ref[3][2] = {{0, 0}, {1, 0}, {0, 1}};
      for (int v = 0; v < 3; v++) {
        const int fx = c.s == 0 ? c.a + ref[v][0] : c.a + 1 - ref[v][0];
        const int fy = c.s == 0 ? c.b + ref[v][1] : c.b + 1 - ref[v][1];
        // parent reference coordinates times r: lower x = X + H xi, upper x = X + H - H xi
        const int px = S == 0 ? fx : r - fx, py = S == 0 ? fy : r - fy;
        expect(px == ox + sigma * ref[v][0] && py == oy + sigma * ref[v][1], "class map is the child's geometry", r, S, cls);
        expect(px >= 0 && py >= 0 && px + py <= r, "child inside its parent", r, S, cls);
      }
      if (S == 1)
        expect(cls == child_class(r, 0, r - 1 - c.a, r - 1 - c.b, 1 - c.s), "upper parent = reflected lower parent", r, S, cls);
    }
    expect(own == r * (r + 1) / 2, "children of the parent's shape", r, S, 0);
    expect((int)classes.size() == r * r, "classes distinct", r, S, 0);
    expect(std::fabs(area - 0.5) < 1e-15, "areas sum to the parent's", r, S, 0);
  }
  // every fine cell of a coarse square has exactly one parent
  for (int b = 0; b < r; b++)
    for (int a = 0; a < r; a++) {
      expect(parent_shape(r, a, b, 0) == (a + b <= r - 1 ? 0 : 1), "parent of a lower child", r, a, b);
      expect(parent_shape(r, a, b, 1) == (a + b <= r - 2 ? 0 : 1), "parent of an upper child", r, a, b);
    }
}

// every table of a ratio is built once: tab[dc][df], degrees 0 .. 5
typedef std::vector<std::vector<dvec>> TableSet;
static TableSet build_all(int r) {
  TableSet t(6, std::vector<dvec>(6));
  for (int dc = 0; dc <= 5; dc++)
    for (int df = 0; df <= 5; df++) t[dc][df] = child_tables(dc, df, r);
  return t;
}

static void check_tables(const TableSet& tab, int r, int dc, int df) {
  const dvec& C = tab[dc][df];
  const int nc = n_scalar(dc), nf = n_scalar(df);
  expect(C.size() == (size_t)r * r * nc * nf, "table size", r, dc, df);
  // |C| <= r (Cauchy-Schwarz: the coarse mode has norm r over the child in the child's coordinates), so (1 / r) C <= 1
  for (double x : C) expect(std::fabs(x) <= r * (1.0 + 1e-15), "entries of (1 / r) C of size <= 1", r, dc, df);
  // constants
  for (int cls = 0; cls < r * r; cls++)
    for (int n = 0; n < nf; n++) expect(close(C[((size_t)cls * nc) * nf + n], n == 0 ? 1.0L : 0.0L), "constant prolongs to the constant", r, dc, df);
  for (int m = 0; m < nc; m++) {
    long double sum = 0;
    for (int cls = 0; cls < r * r; cls++) sum += C[((size_t)cls * nc + m) * nf];
    expect(close(sum / ((long double)r * r), m == 0 ? 1.0L : 0.0L), "only the constant restricts to the constant", r, dc, df);
  }
  // Parseval: the fine space holds the coarse one
  if (df >= dc)
    for (int m = 0; m < nc; m++)
      for (int m2 = 0; m2 < nc; m2++) {
        long double sum = 0;
        for (int cls = 0; cls < r * r; cls++)
          for (int n = 0; n < nf; n++) sum += (long double)C[((size_t)cls * nc + m) * nf + n] * C[((size_t)cls * nc + m2) * nf + n];
        expect(close(sum / ((long double)r * r), m == m2 ? 1.0L : 0.0L), "Parseval", r, dc, df);
      }
  // the scalar table (degrees one lower) is the leading block of the velocity table
  {
    const dvec& Cs = tab[dc - 1][df - 1];
    const int ncs = n_scalar(dc - 1), nfs = n_scalar(df - 1);
    for (int cls = 0; cls < r * r; cls++)
      for (int m = 0; m < ncs; m++)
        for (int n = 0; n < nfs; n++)
          expect(close(Cs[((size_t)cls * ncs + m) * nfs + n], C[((size_t)cls * nc + m) * nf + n]), "leading block", r, dc, df);
  }
  if (r == 1) {
    const std::vector<real> Q = child_tables_quadrature(dc, df, 1);
    for (int m = 0; m < nc; m++)
      for (int n = 0; n < nf; n++) {
        expect(close(Q[(size_t)m * nf + n], m == n ? 1.0L : 0.0L), "r = 1 is the identity", r, dc, df);
        expect(C[(size_t)m * nf + n] == (m == n ? 1.0 : 0.0), "r = 1 is stored exactly", r, dc, df);
      }
  }
}

int main() {
  const int ratios[4] = {1, 2, 3, 16};
  for (int r : ratios) {
    check_children(r);
    const TableSet tab = build_all(r);
    for (int dc = 1; dc <= 5; dc++)
      for (int df = 1; df <= 5; df++) check_tables(tab, r, dc, df);
  }
  // out-of-range requests are refused, not computed
  int refused = 0;
  try { child_tables(1, 1, 17); } catch (const std::string&) { refused++; }
  try { child_tables(6, 1, 2); } catch (const std::string&) { refused++; }
  try { child_tables(1, 1, 0); } catch (const std::string&) { refused++; }
  expect(refused == 3, "range checks", 0, 0, 0);
  std::printf("worst deviation %.3e\n", worst);
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
