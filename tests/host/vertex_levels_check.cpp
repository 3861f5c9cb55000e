// CPU check of csrc/hdg_vertex_levels.hpp (compiled by tests/test_host.py with g++): the level plan of the vertex-grid V-cycle
// for a dozen meshes and the non-default switches, stated as literal values.  The expected plans were derived by hand from
// the rules the engine followed before the plan existed (hierarchy loop, the two V-cycles, the two builders of the dense
// tail), not from the function under test.
// A level prints as its size and the letter of its form: L legs, P per-level kernels, T one-workgroup tail kernel, D dense
// tail, C coarsest-level sweeps; then the level the dense tail is built at and the number of levels a tail covers.
#include <cmath>
#include <cstdio>
#include <string>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_vertex_levels.hpp"

using namespace hdg;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("error line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static std::string show(const VertexPlan& p) {
  std::string s;
  for (const VLevel& v : p.lev) {
    char c = '?';
    switch (v.form) {
      case VForm::Legs: c = 'L'; break;
      case VForm::PerLevel: c = 'P'; break;
      case VForm::TailKernel: c = 'T'; break;
      case VForm::DenseTail: c = 'D'; break;
      case VForm::Coarsest: c = 'C'; break;
    }
    s += std::to_string(v.n) + c + " ";
  }
  return s + "dense=" + std::to_string(p.dense_lev) + " tail=" + std::to_string(p.tail_nlev);
}
static void expect(int line, int nx, bool periodic, const Options& o, const char* want) {
  const VertexPlan p = vertex_plan(nx, periodic, o);
  const std::string got = show(p);
  if (got != want) { std::printf("error line %d: %s %d: got  %s\n                      want %s\n", line, periodic ? "periodic" : "unit", nx, got.c_str(), want); failures++; }
  for (const VLevel& v : p.lev) {  // vertex count and row pitch of each grid
    if (v.pitch != (periodic ? v.n : v.n + 1) || v.nv != (long)v.pitch * v.pitch) { std::printf("error line %d: pitch / vertices of n = %d\n", line, v.n); failures++; }
  }
  if (p.periodic != periodic) { std::printf("error line %d: periodic flag\n", line); failures++; }
}
#define EXPECT(nx, periodic, o, want) expect(__LINE__, nx, periodic, o, want)

// the switches as options_from_env resolves them: no tail -> no dense tail; the periodic dense tail needs the fused legs
static Options resolved(Options o) {
  o.mg_dense_tail = o.mg_dense_tail && o.mg_tail;
  o.mg_dense_tail_periodic = o.mg_dense_tail && o.mg_fuse;
  return o;
}

int main() {
  const Options def = resolved(Options{});
  // ---- defaults, unit square
  EXPECT(1024, false, def, "1024L 512L 256L 128L 64L 32D 16D 8D 4D 2D dense=5 tail=5");
  EXPECT(96, false, def, "96L 48L 24D 12D 6D 3D dense=2 tail=4");
  EXPECT(66, false, def, "66L 33C dense=-1 tail=0");
  EXPECT(65, false, def, "65C dense=-1 tail=0");
  EXPECT(24, false, def, "24D 12D 6D 3D dense=0 tail=4");
  EXPECT(2, false, def, "2T dense=-1 tail=1");
  // ---- defaults, periodic square
  EXPECT(256, true, def, "256L 128L 64L 32D 16D 8D 4D 2D dense=3 tail=5");
  EXPECT(80, true, def, "80L 40L 20D 10D dense=2 tail=2");
  EXPECT(48, true, def, "48L 24D 12D 6D dense=1 tail=3");
  EXPECT(16, true, def, "16P 8P 4P 2C dense=-1 tail=0");  // the dense tail would sit at level 0
  EXPECT(18, true, def, "18C dense=-1 tail=0");
  CHECK(vertex_plan(256, true, def).lev[3].nv == 1024);  // the dense matrix of the periodic tail: N = 1024
  CHECK(vertex_plan(1024, false, def).tail_vertices() == 1089 + 289 + 81 + 25 + 9);  // the census of the unit square's tail counts these
  CHECK(vertex_plan(96, false, def).tail_vertices() == 625 + 169 + 49 + 16);
  // ---- switches
  {
    Options o; o.mg_fuse = false; o = resolved(o);
    EXPECT(1024, false, o, "1024P 512P 256P 128P 64P 32D 16D 8D 4D 2D dense=5 tail=5");
    EXPECT(256, true, o, "256P 128P 64P 32P 16P 8P 4P 2C dense=-1 tail=0");
    EXPECT(80, true, o, "80P 40P 20P 10C dense=-1 tail=0");
  }
  {
    Options o; o.mg_tail = false; o = resolved(o);
    EXPECT(96, false, o, "96L 48L 24L 12L 6L 3C dense=-1 tail=0");  // the legs also take n <= 32
    EXPECT(2, false, o, "2C dense=-1 tail=0");
    EXPECT(80, true, o, "80L 40L 20P 10C dense=-1 tail=0");
    Options p = o; p.mg_fuse = false; p = resolved(p);
    EXPECT(96, false, p, "96P 48P 24P 12P 6P 3C dense=-1 tail=0");
  }
  {
    Options o; o.mg_dense_tail = false; o = resolved(o);
    EXPECT(96, false, o, "96L 48L 24T 12T 6T 3T dense=-1 tail=4");
    EXPECT(1024, false, o, "1024L 512L 256L 128L 64L 32T 16T 8T 4T 2T dense=-1 tail=5");
    EXPECT(80, true, o, "80L 40L 20P 10C dense=-1 tail=0");
    EXPECT(64, true, o, "64L 32P 16P 8P 4P 2C dense=-1 tail=0");
  }
  {
    Options o; o.mg_sweeps = 3; o = resolved(o);
    EXPECT(96, false, o, "96L 48L 24D 12D 6D 3D dense=2 tail=4");  // the unit square keeps its legs (1 .. 3 sweeps) ...
    EXPECT(80, true, o, "80P 40P 20D 10D dense=2 tail=2");         // ... the periodic square has them for exactly 2
    o.mg_sweeps = 4;
    EXPECT(96, false, o, "96P 48P 24D 12D 6D 3D dense=2 tail=4");
  }
  // ---- side-job weights: every Legs level counts twice (two legs), the finest with cg_xp_w0
  {
    const VertexPlan p = vertex_plan(1024, false, def);
    CHECK(def.cg_xp_w0 == 1.6);
    CHECK(std::fabs(p.side_weight_sum(0, def.cg_xp_w0) - 11.2) < 1e-12);  // 2 * 1.6 + 2 * 4
    CHECK(p.side_weight_sum(1, def.cg_xp_w0) == 8.0);                      // distributed finest level: from level 1
    CHECK(std::fabs(vertex_plan(256, true, def).side_weight_sum(0, 1.6) - 7.2) < 1e-12);
    CHECK(vertex_plan(24, false, def).side_weight_sum(0, 1.6) == 0.0);  // no Legs level: nothing rides
    CHECK(VertexPlan::side_weight(0, 1.6) == 1.6 && VertexPlan::side_weight(3, 1.6) == 1.0);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
