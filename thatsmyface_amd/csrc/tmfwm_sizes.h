// The block sizes the library is compiled for -- the only such list on the C++ side -- and the
// step from a run-time block size to the code of that size (host side).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace tmf {

using BlockSizes = std::integer_sequence<int, 4, 6, 8, 10, 12, 14, 16>;

// (a left fold: f is instantiated for the sizes in ascending order, and the kernels it launches are
// emitted in that order; a right fold reverses the order of the kernels in the code object)
template <class R, class F, int... Bs>
inline R block_value_in(int block, R other, F &&f, std::integer_sequence<int, Bs...>)
{
    (void)(... || (block == Bs ? (other = f(std::integral_constant<int, Bs>{}), true) : false));
    return other;
}

// f(std::integral_constant<int, B>{}) for B == block; `other` for a size that is not compiled
template <class R, class F>
inline R block_value(int block, R other, F &&f)
{
    return block_value_in(block, other, f, BlockSizes{});
}

// the same for a launcher: f's hipError_t, hipErrorInvalidValue for a size that is not compiled
template <class F>
inline hipError_t for_block(int block, F &&f)
{
    return block_value(block, hipErrorInvalidValue, f);
}

}  // namespace tmf
