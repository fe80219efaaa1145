// Run-time value -> compile-time constant, for picking a kernel instantiation.  Host only, no HIP dependency.
//
//   with_bool(plain, [&](auto PL) { launch<kernel<decltype(PL)::value>>(...); });
//   ARVAE_REQUIRE(with_int<4, 8, 16>(rows, [&](auto RW) { launch<kernel<decltype(RW)::value>>(...); }), "rows %d", rows);
//
// A generic lambda instantiates its body for every listed value: where only some combinations exist as kernels, guard the body
// with `if constexpr` or list the pairs.
#pragma once
#include <type_traits>

namespace arvae {

// f(std::true_type{}) or f(std::false_type{})
template <class F> inline void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the listed V equal to v, and true; no call and false when v is not listed
template <int... V, class F> inline bool with_int(int v, F &&f) {
    return (... || (v == V ? ((void)f(std::integral_constant<int, V>{}), true) : false));
}

}  // namespace arvae
