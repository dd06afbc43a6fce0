// read_codes.hpp -- read bytes -> 2-bit codes and the bit helpers of the kernels that compare reads with the text units
// (hamming.hip, edit_distance.hip, align.hip).  Device code only; verify.hpp builds the read loader read_chunk on it.
#pragma once
#include <cstdint>

namespace gdx {

// four read bytes -> their 2-bit codes in 8 bits (byte 0 in bits 1:0) and, in bits 0..3 of `bad`, which of them are not
// one of the dense symbols 1..4.  Args carries IndexView's perm_code_lo / _hi, perm_exp_lo / _hi and perm_mask (VerifyArgs).
template <class Args>
__device__ __forceinline__ uint32_t pack4_perm(const Args &a, uint32_t c, uint32_t &bad)
{
    const uint32_t sel = c & 0x07070707u;
    const uint32_t code = __builtin_amdgcn_perm(a.perm_code_hi, a.perm_code_lo, sel);
    const uint32_t expect = __builtin_amdgcn_perm(a.perm_exp_hi, a.perm_exp_lo, sel);
    uint32_t t = (c & a.perm_mask) ^ expect;  // a non-zero byte: not one of the four
    t |= t >> 4;
    t |= t >> 2;
    t |= t >> 1;
    bad = ((t & 0x01010101u) * 0x01020408u) >> 24;  // bit 8 k -> bit k (the sixteen partial products never meet)
    uint32_t p = (code << 6) | code;
    p = (p << 12) | p;
    return (p >> 18) & 0xffu;
}
__device__ __forceinline__ uint32_t pack4_lds(const uint8_t *s_dense, uint32_t c, uint32_t &bad)
{
    uint32_t out = 0;
    bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t d = static_cast<uint32_t>(s_dense[(c >> (8u * k)) & 0xffu]) - 1u;
        bad |= (d > 3u ? 1u : 0u) << k;
        out |= (d & 3u) << (2u * k);
    }
    return out;
}

// the even bits of x (bit 2 i -> bit i)
__device__ __forceinline__ uint32_t even_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    return (x | (x >> 8)) & 0xffffu;
}

__device__ __forceinline__ uint32_t low_bits(uint32_t n) { return n >= 32u ? 0xffffffffu : (1u << n) - 1u; }

}  // namespace gdx
