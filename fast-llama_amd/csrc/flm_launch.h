// flm_launch.h -- from a run-time choice to ONE instantiation of a kernel template.  A fused kernel exists in a fixed set of instantiations (quant type x rounds class x
// split heads x ...).  That set is written down once, as a list of Variant<template arguments...>; launch sites name the tuple they want and dispatch() hands the
// matching entry to a generic lambda as a type, so a launch is one statement; whoever has to visit every instantiation (the dynamic-LDS limit) walks the same list.
// Nothing outside a list can be launched, and nothing in a list is instantiated anywhere else.
#pragma once

namespace fh {

template <int... V> struct Variant {
    static constexpr int v[sizeof...(V)] = {V...};
    static bool is(const int (&want)[sizeof...(V)]) { for (size_t i = 0; i < sizeof...(V); ++i) if (v[i] != want[i]) return false; return true; }
};
template <class... Vs> struct Variants {};

// cross_t<A, B>: every entry of list A continued by every entry of list B
template <int... a, int... b> Variant<a..., b...> join(Variant<a...>, Variant<b...>) { return {}; }
template <class... A, class... B> Variants<A..., B...> cat(Variants<A...>, Variants<B...>) { return {}; }
template <class A, class... B> Variants<decltype(join(A{}, B{}))...> each(A, Variants<B...>) { return {}; }
template <class A0, class... A, class LB> auto cross(Variants<A0, A...>, LB lb) {
    if constexpr (sizeof...(A) == 0) return each(A0{}, lb); else return cat(each(A0{}, lb), cross(Variants<A...>{}, lb));
}
template <class LA, class LB> using cross_t = decltype(cross(LA{}, LB{}));

// f(entry) for the entry of the list that equals `want`; false: the list has none
template <class... Vs, int N, class F> bool dispatch(Variants<Vs...>, const int (&want)[N], F&& f) { return (... || (Vs::is(want) && (f(Vs{}), true))); }
template <class... Vs, class F> void for_each_variant(Variants<Vs...>, F&& f) { (f(Vs{}), ...); }

}  // namespace fh
