// sf_dem_dispatch.h -- from the run-time pair settings to the template arguments of the kernels, stated once:
//   pair_dispatch(style, cohe, lub, [&](auto st, auto c, auto l) { k_some<st, c, l><<<...>>>(...); });
// The generic lambda is instantiated for every combination it can be called with; each launches its own kernel.
#pragma once
#include <type_traits>

namespace sf {

template <int N> using int_c = std::integral_constant<int, N>;

// STYLE of the kernels: 0 no contact law, 1 Hookean, 2 hertzFix.  Plain gran/hooke (GranParams::style 3) runs the
// Hookean kernels: the law itself branches on GranParams::style.
template <class F>
void style_dispatch(int style, F&& f)
{
  if (style == 2) f(int_c<2>{});
  else if (style == 1 || style == 3) f(int_c<1>{});
  else f(int_c<0>{});
}

template <class F>
void flag_dispatch(bool on, F&& f) { on ? f(std::true_type{}) : f(std::false_type{}); }

// (pair style, fix cohesive, pair lubricate/poly) -> f(STYLE, COHE, LUB) as compile-time constants
template <class F>
void pair_dispatch(int style, bool cohe, bool lub, F&& f)
{
  style_dispatch(style, [&](auto st) {
    flag_dispatch(cohe, [&](auto c) { flag_dispatch(lub, [&](auto l) { f(st, c, l); }); });
  });
}

}  // namespace sf
