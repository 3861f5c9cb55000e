// Run-time values -> template arguments: the one mechanism behind every kernel launch of the engine that picks an
// instantiation from a degree, a mode or a flag.  Plain C++ (no HIP header): f is a generic lambda that receives the value as
// a type and uses it as a constant expression,
//   with_int<1, 2, 3, 4>(K, "degree", [&](auto k) { k_gamma_psi<k()><<<grid, block, 0, stream>>>(...); });
// Exactly the listed values are instantiated, each call compiles to a direct launch of the chosen one, and a value outside
// the list throws std::string (HDG_ERR_ARG at the C boundary) -- no site has a default that launches some other kernel.
// Where two run-time cases share one instantiation the call site says so (Engine::rhs_form), so that nesting two with_bool
// calls never instantiates a combination no one launches.
#pragma once
#include <string>
#include <type_traits>

namespace hdg {

// f(std::integral_constant<int, v>{}) for the v of Vs... that equals x
template <int... Vs, class F>
inline void with_int(int x, const char* what, F&& f) {
  const bool found = ((x == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  if (!found) throw std::string(what) + " = " + std::to_string(x) + ": no kernel is built for this value";
}
// f(std::true_type{}) or f(std::false_type{})
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace hdg
