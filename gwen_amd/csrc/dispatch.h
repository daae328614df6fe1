// Run-time value -> template argument, for the launchers:
//   return gwen::dispatch(gwen::ints<16, 32, 64>{}, Fin, [&](auto fi) { return launch<decltype(fi)::value>(args); });
// calls f(std::integral_constant<int, V>{}) for the V of the list that equals v and returns what f returns; no V
// equals v: returns not_found.  Every V of the list instantiates f, so what must not exist for some V (a kernel that
// is not built) is excluded inside f, with `if constexpr`.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "../../include/gwen_hip.h"

namespace gwen {

template <int... Vs> struct ints {};

template <int... Vs, class F>
inline int dispatch(ints<Vs...>, int64_t v, F &&f, int not_found = GWEN_EINVAL) {
  int rc = not_found;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return rc;
}

}  // namespace gwen
