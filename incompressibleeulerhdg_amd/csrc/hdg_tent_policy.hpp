// Decisions of the tentative-velocity solver (Engine::cheb_gmres, Engine::sstep_mr) as functions of numbers: the Ritz interval
// and its safety factors, the ellipse of the Chebyshev iteration and its predicted iteration count, the schedule of the
// convergence checks, the growth / stall / slow-tail / hand-over guards with what a stage remembers from solve to solve, and
// the lengths of the s-step cycles.  The engine launches kernels and measures norms; what it does with a norm is decided here.
// Plain C++, no HIP: tests/host/tent_policy_check.cpp compiles it with g++ and states every rule as literal values.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <string>
#include <vector>

#include "hdg_checkpoint.hpp"
#include "hdg_options.hpp"

namespace hdg {

// what the Chebyshev iteration of one stage remembers between solves (checkpoint section 'solver')
struct ChebStage {
  double lmin = -1.0, lmax = -1.0;  // widest interval seen; <= 0: estimate at the next solve
  long count = 0;                   // solves of the stage so far (re-estimate period opt.cheb_every)
  double widen = 1.0;               // factor on the upper safety factor: grows when the iteration grew
  int last = 0;                     // iterations of the last converged Chebyshev solve of the stage (check schedule)
  char slow = 0;                    // the last Chebyshev solve of the stage was slow: GMRES until the next re-estimate
  int hand = 0;                     // learnt hand-over point of the stage: the check after which the Chebyshev rate last turned slow
};

// an engine that has not run a Chebyshev solve yet has no history: its checkpoint holds empty columns
inline bool cheb_history_empty(const std::vector<ChebStage>& st) {
  for (const ChebStage& c : st) if (c.count > 0) return false;
  return true;
}
// The seven columns of the stage records in checkpoint section 'solver', in the order and element types of the format:
// lmin, lmax, widen (double), count (long), last, hand (int), slow (char)
inline void write_cheb_stages(ckpt::ByteWriter& w, const std::vector<ChebStage>& st) {
  std::vector<double> lmin, lmax, widen;
  std::vector<long> count;
  std::vector<int> last, hand;
  std::vector<char> slow;
  for (const ChebStage& c : st) {
    lmin.push_back(c.lmin); lmax.push_back(c.lmax); widen.push_back(c.widen); count.push_back(c.count);
    last.push_back(c.last); hand.push_back(c.hand); slow.push_back(c.slow);
  }
  w.vec(lmin); w.vec(lmax); w.vec(widen); w.vec(count); w.vec(last); w.vec(hand); w.vec(slow);
}
// empty return: read (st is empty, or holds nstage records: a column of length 0 leaves its default); otherwise what is wrong
inline std::string read_cheb_stages(ckpt::ByteReader& r, size_t nstage, std::vector<ChebStage>& st) {
  std::vector<double> lmin, lmax, widen;
  std::vector<long> count;
  std::vector<int> last, hand;
  std::vector<char> slow;
  r.vec(lmin); r.vec(lmax); r.vec(widen); r.vec(count); r.vec(last); r.vec(hand); r.vec(slow);
  st.clear();
  const size_t nh = lmin.size();
  if ((nh != 0 && nh != nstage) || lmax.size() != nh) return "section 'solver': Chebyshev bounds of another stage count";
  for (size_t n : {widen.size(), count.size(), last.size(), hand.size(), slow.size()})
    if (n != 0 && n != nstage) return "section 'solver': Chebyshev history of another stage count";
  if (lmin.size() + widen.size() + count.size() + last.size() + hand.size() + slow.size() == 0) return "";
  st.assign(nstage, ChebStage{});
  for (size_t i = 0; i < nstage; i++) {
    if (!lmin.empty()) { st[i].lmin = lmin[i]; st[i].lmax = lmax[i]; }
    if (!widen.empty()) st[i].widen = widen[i];
    if (!count.empty()) st[i].count = count[i];
    if (!last.empty()) st[i].last = last[i];
    if (!hand.empty()) st[i].hand = hand[i];
    if (!slow.empty()) st[i].slow = slow[i];
  }
  return "";
}

// Interval of the Chebyshev iteration from the Ritz values of the opening Arnoldi cycle; false: no usable interval (the
// stage record is left alone).  Otherwise st.lmin / st.lmax hold it.
// Ritz values lie inside the spectrum: widen; keep the widest interval seen for this stage
// (the hybrid preconditioner's real spectrum starts at 1 -- the non-conforming part is reproduced exactly
//  -- but its upper end, 4.2-5.5 for k = 1..3, is underestimated by 6 Arnoldi steps, ~3.2; the ellipse of
//  convergence is larger than the interval, so 1.3 is enough for k >= 2 (1.5 for k = 1), and a stage whose Chebyshev
//  iteration had to fall back to GMRES widens its own factor for all later solves: ChebStage::widen)
inline bool ritz_interval(const std::vector<std::complex<double>>& ritz, ChebStage& st, const Options& opt, bool hybrid, int degree) {
  double lo = 1e300, hi = -1e300;
  for (auto v : ritz) { lo = std::min(lo, v.real()); hi = std::max(hi, v.real()); }
  if (!(lo > 0) || !(hi > lo)) return false;
  const double e_lo = opt.cheb_flo, e_hi = opt.cheb_fhi;
  const double f_lo = e_lo > 0 ? e_lo : (hybrid ? 0.9 : 0.8);
  const double f_hi = (e_hi > 0 ? e_hi : (hybrid ? (degree == 1 ? 1.5 : 1.3) : 1.15)) * st.widen;
  lo *= f_lo; hi *= f_hi;
  if (st.lmin > 0) { lo = std::min(lo, st.lmin); hi = std::max(hi, st.lmax); }
  st.lmin = lo; st.lmax = hi;
  return true;
}

// Imaginary half-axis / real half-axis of the ellipse.
// The additive preconditioner (SPD) gives a nearly real spectrum (0 is best); the hybrid one is non-symmetric and its
// spectrum fills a fat ellipse (at 128^2: real [1, 4.8] / [1, 4.2] / [1, 5.5], |imag| <= 1.2 / 1.4 / 2.2 for k = 1 / 2 / 3):
// 0.5 is within a few iterations of the best value for k = 1, 2 (measured scan), while 0 loses 10+ iterations.
// k = 2: a THIN ellipse (0.3) for the bulk, then the hand-over to GMRES below; k = 1 (operator so cheap that a GMRES
// iteration costs 3-4 Chebyshev iterations): the wider ellipse that converges on its own (scans: DESIGN.md section 9)
inline double cheb_ellipse_frac(const Options& opt, bool hybrid, int degree) {
  return opt.cheb_ell >= 0 ? opt.cheb_ell : (hybrid ? (degree >= 2 ? 0.3 : 0.5) : 0.0);
}
// Observed rate above which the tail takes over (0: never).
// k = 2: 0.3 with the s-step tail of round 4 (scan at C3, ms/step: 0.1-0.3: 85.5-85.8, 0.35: 91.2, 0.45: 95.6, 0.6: 95.1, 0.8:
// 100.8; with the GMRES(8) tail of round 3 the optimum was 0.6); k >= 3: 0.4 (no sensitivity between 0.25 and 0.6); k = 1: off
inline double cheb_handover_rate(const Options& opt, bool hybrid, int degree) {
  return opt.cheb_handover >= 0.0 ? opt.cheb_handover : (hybrid ? (degree >= 3 ? 0.4 : (degree == 2 ? (opt.tail_gmres ? 0.6 : 0.3) : 0.0)) : 0.0);
}

// Chebyshev for a spectrum inside the ellipse with centre theta, real half-axis aax and imaginary half-axis
// bim = frac aax: foci at theta +- delta, delta^2 = aax^2 - bim^2.
struct ChebEllipse {
  double theta, aax, bim, delta, sigma, rate;
  ChebEllipse(double lo, double hi, double frac)
      : theta(0.5 * (hi + lo)), aax(0.5 * (hi - lo)), bim(frac * aax), delta(std::sqrt(std::max(aax * aax - bim * bim, 1e-24))),
        sigma(theta / delta), rate((aax + bim) / (theta + std::sqrt(std::max(theta * theta - delta * delta, 0.0)))) {}
  // expected iterations for the reduction of the residual by `reduction` (asymptotic rate on the ellipse): the method
  // selection and the stall guard go by it
  int expected(double reduction) const { return (int)(std::log(std::max(reduction, 1e-300)) / std::log(std::min(rate, 0.999))) + 8; }
};

enum class ChebVerdict { Converged, Continue, Growing, Stalled, SlowTail };
inline const char* verdict_name(ChebVerdict v) {
  return v == ChebVerdict::Growing ? "growing" : (v == ChebVerdict::SlowTail ? "slow tail" : "stalled");
}

// Watches one Chebyshev solve of a stage: when the norm of z_k = M(b - A x_k) is measured, and what follows from it.
struct ChebMonitor {
  ChebStage& st;
  const Options& opt;
  const int expected, maxit;
  const double handover, target;  // handover: cheb_handover_rate; target: rtol |M r_0|
  // The norm is only evaluated at check points (z is written out only then: a check costs a vector store, a dot product
  // and a host sync, ~1/4 of an iteration).  With the Chebyshev count of the previous solve of this stage known: every
  // 8th iteration up to 4 before it (enough to catch growth), every opt.cheb_fine_step-th from there on; without
  // history every 4th.  ch_head: iterations of the opening GMRES cycle (0 without an estimate).
  const int kfine;
  double last, stall_ref, nz_prev = 0.0;  // last: the smallest norm seen
  int stall_checks = 0, k_prev = 0;
  // the finishing solver takes the slow tail of this solve (after Growing too, when the growth shows at a learnt
  // hand-over point: the stage record goes by the verdict, the choice of the finishing solver by this)
  bool tail = false;
  ChebMonitor(ChebStage& st_, int ch_head, int expected_, const Options& opt_, double handover_, double target_, double beta, int maxit_)
      : st(st_), opt(opt_), expected(expected_), maxit(maxit_), handover(handover_), target(target_),
        kfine(st_.last > 0 ? std::max(4, (st_.last - ch_head - 4) & ~1) : 0), last(beta), stall_ref(beta) {}
  // is the norm measured in the iteration that starts from iterate k?
  bool check_at(int k) const { return kfine > 0 ? (k < kfine ? (k % 8 == 0) : ((k - kfine) % opt.cheb_fine_step == 0)) : (k % 4 == 0); }
  // nz = |z| measured at a check, k Chebyshev iterations and `its` iterations of the solve done
  ChebVerdict observe(int k, int its, double nz) {
    if (nz <= target) {
      // z belongs to the iterate BEFORE the step just taken; that iterate had converged, and the
      // extra Chebyshev step only reduces the error further
      st.slow = its > opt.cheb_max_expected + opt.cheb_max_expected / 2;  // the prediction was optimistic
      st.last = its;
      return ChebVerdict::Converged;
    }
    // Guards.  Growth (an eigenvalue outside the ellipse of convergence): finish with GMRES and estimate
    // more generously from now on.  No progress over 8 checks (32 iterations), or far beyond the predicted
    // count: finish with GMRES but do NOT widen -- slow convergence is not a wrong interval, and widening on
    // it made every following solve slower still (CFL 1 sweep, tools/robustness_sweep.py).
    const bool growing = nz > 1e2 * last;
    if (nz < 0.5 * stall_ref) { stall_ref = nz; stall_checks = 0; } else stall_checks++;
    // Slow tail: an isolated eigenvalue outside the ellipse (seen at 2048^2: one near 0.3 with a 1e-6 share of
    // the residual) makes the iteration crawl at its own rate (0.87 instead of 0.55 per iteration) once the
    // bulk has converged.  GMRES removes such outliers in a few iterations: hand over when the rate observed
    // since the previous check would need more than 24 further iterations.
    tail = false;
    if (k_prev > 0 && k > k_prev && nz < nz_prev && nz > target) {
      const double obs = std::pow(nz / nz_prev, 1.0 / (k - k_prev));
      const double remaining = std::log(target / nz) / std::log(obs);
      tail = k >= 16 && obs > 0.75 && remaining > 24.0;
      // Deliberate hand-over (HDG_CHEB_HANDOVER = rate threshold, 0 = off): the iteration on a THIN ellipse takes
      // the bulk of the spectrum down at 0.25-0.3 per iteration and then crawls on the few eigenvalues with large
      // imaginary parts that the ellipse leaves out; a GMRES iteration costs 2-3 Chebyshev iterations (Krylov basis
      // traffic) but removes exactly those.  Hand over as soon as the observed rate is worse than what GMRES buys per
      // unit of cost, unless the end is a few iterations away anyway.
      if (handover > 0.0 && k >= opt.cheb_min_k && obs > handover && remaining > 6.0) tail = true;
      if (tail) st.hand = k_prev;  // the segment (k_prev, k] was the slow one: hand over at k_prev next time
    }
    // round 4: with the s-step tail (an iteration of which costs what a Chebyshev iteration costs) the solves that follow
    // hand over AT the learnt point instead of spending two more iterations on confirming the slow rate again
    if (!tail && !opt.tail_gmres && handover > 0.0 && st.hand > 0 && k >= st.hand && nz > target) tail = true;
    k_prev = k; nz_prev = nz;
    const bool stalled = tail || stall_checks >= 8 || k > 6 * expected + 64;
    if (growing || stalled || its >= maxit) {
      if (growing) {
        st.lmin = st.lmax = -1.0;  // wrong interval: re-estimate at the next solve of this stage,
        st.widen = std::min(st.widen * 1.25, 4.0);  // more generously
        return ChebVerdict::Growing;
      }
      if (!tail) {
        st.slow = true;  // right interval, slow iteration: GMRES until the periodic re-estimate
        return ChebVerdict::Stalled;
      }
      st.last = its;  // the next solve of this stage starts its fine checks shortly before this point
      return ChebVerdict::SlowTail;
    }
    last = std::min(last, nz);
    return ChebVerdict::Continue;
  }
};

// ---- s-step minimal-residual cycles
// iterations for the reduction from -> target at GMRES's observed tail rate
inline int sstep_length_for(double from, double target, double per_decade) {
  return (int)std::ceil(per_decade * std::log10(std::max(from / target, 1.0)));
}
// length of a cycle that starts from a residual of norm cur (cur <= 0: not known): chosen from the reduction still needed,
// 1.7 iterations per decade + 1, GMRES's observed 5-6 for 3-4 decades
inline int sstep_first_length(double cur, double target, double per_decade, int smax) {
  return cur > 0.0 ? std::max(2, std::min(smax, sstep_length_for(cur, target, per_decade) + 1)) : std::min(6, smax);
}
// rho: the residual norm the least squares predict for the basis of `built` vectors.  Returns `built` when the step is
// taken with it -- enough (with a margin for the accuracy of the prediction), rank deficient, or no room left -- and the
// longer length to build otherwise
inline int sstep_extend(double rho, double target, int built, int rank, int smax, double per_decade) {
  if (rho <= 0.7 * target || rank < built || built >= smax) return built;
  return std::min(smax, built + std::max(1, sstep_length_for(rho / 0.7, target, per_decade)));
}

}  // namespace hdg
