// CPU check of csrc/hdg_options.hpp (compiled by tests/test_host.py with g++): the defaults with an empty environment are the
// values DESIGN.md section 14 states, every kind of value parses, and the switches that imply others resolve in one place.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_options.hpp"

extern char** environ;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("error line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void clear_env() {
  std::vector<std::string> names;
  for (char** e = environ; *e; e++)
    if (std::strncmp(*e, "HDG_", 4) == 0) names.emplace_back(*e, std::strchr(*e, '=') - *e);
  for (const std::string& n : names) unsetenv(n.c_str());
}

int main() {
  clear_env();
  {
    const hdg::Options o = hdg::options_from_env();
    CHECK(o.mg_sweeps == 2 && o.mg_coarse == 2);
    CHECK(o.sstep_max == 6 && o.sstep_per_decade == 1.7);
    CHECK(o.cheb_every == 64 && o.cheb_m == 6 && o.cheb_min_k == 6 && o.cheb_hand_cycle == 8 && o.cheb_max_expected == 64 && o.cheb_fine_step == 2);
    CHECK(o.cheb_flo < 0 && o.cheb_fhi < 0 && o.cheb_ell < 0 && o.cheb_handover < 0);
    CHECK(o.cg_xp_w0 == 1.6 && o.cg_floor_c == 32.0 && o.cg_force_replace == 0);
    CHECK(o.trace_cheb_lo == 0.1 && o.trace_backward_tol == 0.0 && o.trace_smooth_its == 2);
    CHECK(o.trace_tile3 == -1);  // by degree
    CHECK(o.adv_split_lo == 3 && o.adv_split_hi == 3);
    CHECK(o.amg_max_coarse == 2000);
    CHECK(o.row_pad < 0);  // padding rows by the memory-channel rule
    // the fast paths are on, the baseline forms and the opt-in paths off
    CHECK(o.mg_fuse && o.mg_tail && o.mg_dense_tail && o.mg_dense_tail_periodic && !o.mg_replicated);
    CHECK(o.trace_fuse && o.trace_fold && o.trace_tile && o.trace_tile_strips && o.trace_tile_periodic && o.trace_fused_dots);
    CHECK(o.cg_split_update && o.cg_fused_scalars && !o.cg_host_scalars && !o.cg_two_reductions && !o.cg_mass_one_by_one);
    CHECK(o.mfma_schur && o.mfma_lift && o.mfma_adv && !o.mfma_condense && o.lift_pair);
    CHECK(!o.gmres_arnoldi && !o.tail_gmres);
    CHECK(!o.general_csr_lift && !o.general_block_jacobi && !o.general_gmres && o.general_coarse && !o.amg_unfused);
    CHECK(!o.overlap && !o.force_rccl && !o.dbg_nonbr && !o.flow_check && o.ext && o.direct_host);
  }
  {  // one of each kind: flag (presence, whatever the value), negated flag, integer, real, range
    setenv("HDG_TAIL_GMRES", "0", 1);
    setenv("HDG_TRACE_NO_TILE", "", 1);
    setenv("HDG_MG_SWEEPS", "3", 1);
    setenv("HDG_TRACE_TILE3", "0", 1);
    setenv("HDG_CHEB_HANDOVER", "0.45", 1);
    setenv("HDG_TRACE_BACKWARD_TOL", "1e-15", 1);
    setenv("HDG_ADV_SPLIT", "2:4", 1);
    setenv("HDG_ROW_PAD", "0", 1);
    const hdg::Options o = hdg::options_from_env();
    CHECK(o.tail_gmres && !o.trace_tile && o.mg_sweeps == 3 && o.trace_tile3 == 0);
    CHECK(o.cheb_handover == 0.45 && o.trace_backward_tol == 1e-15);
    CHECK(o.adv_split_lo == 2 && o.adv_split_hi == 4);
    CHECK(o.row_pad == 0);  // no padding rows at all: not the same as leaving the variable unset
    CHECK(o.mg_coarse == 2 && o.trace_fuse);  // what was not named keeps its default
    clear_env();
  }
  {  // switches that imply others
    setenv("HDG_MG_NO_TAIL", "1", 1);
    hdg::Options o = hdg::options_from_env();
    CHECK(!o.mg_tail && !o.mg_dense_tail && !o.mg_dense_tail_periodic && o.mg_fuse);
    clear_env();
    setenv("HDG_MG_NO_DENSE_TAIL", "1", 1);
    o = hdg::options_from_env();
    CHECK(o.mg_tail && !o.mg_dense_tail && !o.mg_dense_tail_periodic);
    clear_env();
    setenv("HDG_MG_NO_FUSE", "1", 1);
    o = hdg::options_from_env();
    CHECK(!o.mg_fuse && o.mg_tail && o.mg_dense_tail && !o.mg_dense_tail_periodic);  // the unit square keeps its dense tail
    clear_env();
    setenv("HDG_OVERLAP", "1", 1);
    CHECK(hdg::options_from_env().overlap);
    setenv("HDG_NO_OVERLAP", "1", 1);
    CHECK(!hdg::options_from_env().overlap);
    clear_env();
  }
  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
