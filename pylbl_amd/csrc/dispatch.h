// Run-time values as compile-time constants: what turns an entry's booleans and its angle count
// into the template arguments of the kernel it launches.  No HIP here: plain C++17.
//
//   dispatch(f, b0, b1, ...)          calls f(B0{}, B1{}, ...) once, Bi = std::true_type where bi
//                                     and std::false_type where not, in argument order;
//   dispatch_range<N>(f, k, b0, ...)  for 1 <= k <= N calls f(std::integral_constant<int, k>{},
//                                     B0{}, ...) once and returns true; for any other k calls
//                                     nothing and returns false (the caller has checked k, or
//                                     makes false its own error).
// f is a generic callable (auto parameters) and is instantiated for every combination, so a
// launch site names 2^bools (times N) kernels.
#pragma once

#include <type_traits>
#include <utility>

namespace lbl {

template <typename F>
void dispatch(F && f)
{
    f();
}

template <typename F, typename... Rest>
void dispatch(F && f, bool first, Rest... rest)
{
    if (first)
    {
        dispatch([&](auto... constants) { f(std::true_type{}, constants...); }, rest...);
    }
    else
    {
        dispatch([&](auto... constants) { f(std::false_type{}, constants...); }, rest...);
    }
}

// (dispatch_range's: one comparison per K = I + 1; the first that holds dispatches)
template <typename F, int... I, typename... Bools>
bool dispatch_one_of(std::integer_sequence<int, I...>, F & f, int value, Bools... bools)
{
    return ((value == I + 1 &&
             (dispatch([&](auto... constants) {
                  f(std::integral_constant<int, I + 1>{}, constants...);
              }, bools...), true)) || ...);
}

template <int N, typename F, typename... Bools>
bool dispatch_range(F && f, int value, Bools... bools)
{
    return dispatch_one_of(std::make_integer_sequence<int, N>{}, f, value, bools...);
}

}  // namespace lbl
