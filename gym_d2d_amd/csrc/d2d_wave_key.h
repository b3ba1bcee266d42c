// The 64-bit key reduction of the kernels that choose by packed keys: d2d_color.hip (the next link, its RB) and d2d_stable.hip (a
// link's next proposal).  A key packs what is compared, most significant first, into one unsigned 64-bit word, so one reduction to
// the largest or the smallest word is the whole lexicographic choice.
#pragma once

#include <hip/hip_runtime.h>

namespace d2d {

// One step of a wave reduction by data-parallel primitives: every lane's key as the DPP control moves it, `ident` in both halves
// where the control or the row mask gives a lane no source.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_key(unsigned long long k, unsigned ident) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)ident, (int)(unsigned)k, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)ident, (int)(unsigned)(k >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}

// The largest (MAX) or smallest key of the wave, to every lane as a scalar.  All 64 lanes are active at every call.  A prefix
// scan inside each row of 16 lanes (row_shr 1, 2, 4, 8), lane 15 into row 1 and lane 47 into row 3 (row_bcast 15), lane 31 into
// rows 2 and 3 (row_bcast 31): lane 63 holds the wave's.  Register moves on the VALU, where __shfl_xor is twelve ds_bpermute_b32
// round trips per reduction.
template <bool MAX>
__device__ __forceinline__ unsigned long long wave_reduce(unsigned long long k) {
    constexpr unsigned ident = MAX ? 0u : ~0u;
    unsigned long long o;
#define D2D_WAVE_KEY_STEP(CTRL, ROW_MASK) o = dpp_key<CTRL, ROW_MASK>(k, ident); k = MAX ? (o > k ? o : k) : (o < k ? o : k);
    D2D_WAVE_KEY_STEP(0x111, 0xf)                 // row_shr:1
    D2D_WAVE_KEY_STEP(0x112, 0xf)                 // row_shr:2
    D2D_WAVE_KEY_STEP(0x114, 0xf)                 // row_shr:4
    D2D_WAVE_KEY_STEP(0x118, 0xf)                 // row_shr:8
    D2D_WAVE_KEY_STEP(0x142, 0xa)                 // row_bcast:15 into rows 1 and 3
    D2D_WAVE_KEY_STEP(0x143, 0xc)                 // row_bcast:31 into rows 2 and 3
#undef D2D_WAVE_KEY_STEP
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

}  // namespace d2d
