// f110_replay_bits.h -- the packed frame format of the replay ring (f110_replay.h: bit k of word w = pixel 64 w + k), for the
// replay kernels and for the consumers that read the bits themselves (f110_bitconv.h).  No kernels.  Without hipcc only the
// frame's dimensions remain (f110_bitconv_plan.h).
#pragma once
#include "f110_launch.h" // F110_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#pragma clang fp contract(off)
#endif

namespace f110 {

constexpr int REPLAY_MAX_DIM = 16384;        // rows, cols: the kernels count a frame's 16-pixel chunks in 32 bits

F110_HD inline int replay_words(int cols) { return (cols + 63) >> 6; }

#ifdef __HIPCC__
// 4 pixels -> 4 bits, bit i = (byte i == 255): a byte is 255 iff its low 7 bits carry into bit 7 and bit 7 is set; the four
// bits 7 are gathered by one multiply (exponents 8 i + 7 (j + 1) are pairwise distinct: no carries, bits 28..31 = byte 0..3).
__device__ inline unsigned replay_bits4(unsigned x)
{
    const unsigned m = ((x & 0x7f7f7f7fu) + 0x01010101u) & x & 0x80808080u;
    return ((m >> 7) * 0x10204080u) >> 28;
}
__device__ inline unsigned replay_bits16(uint4 v)
{
    return replay_bits4(v.x) | (replay_bits4(v.y) << 4) | (replay_bits4(v.z) << 8) | (replay_bits4(v.w) << 12);
}
#endif

} // namespace f110
