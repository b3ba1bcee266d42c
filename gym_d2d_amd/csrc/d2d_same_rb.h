// The same-RB staging of the kernels that sort an env's links by (rb, link index) in LDS: d2d_sense.hip, d2d_bestrb.hip,
// d2d_marginal.hip, d2d_powerctl.hip, d2d_evaluate.hip and d2d_balance.hip.  Three steps, each a workgroup-wide loop between the barriers the calling
// kernel places (it knows which bytes its keys share with what): the packed keys rb * 2048 + j, the rank of one key among all of
// them (four keys per ds_read_b128 at a wave-uniform address: stable, free of atomics, the same order on every call), and
// start[r] = the first sorted entry of RB r.  What a kernel puts into a link's slot is its own and stays in the kernel.
#pragma once

#include <hip/hip_runtime.h>

namespace d2d {

constexpr int SAME_RB_MAX_LINKS = 2048;                          // every kernel asserts its public D2D_*_MAX_LINKS / _MAX_RBS against these
constexpr int SAME_RB_MAX_RBS = 8192;
constexpr unsigned KEY_SHIFT = 11;                               // key = rb << 11 | j, j < 2048
static_assert((1 << KEY_SHIFT) == SAME_RB_MAX_LINKS, "the key packs the link index into KEY_SHIFT bits");
static_assert((unsigned long long)(SAME_RB_MAX_RBS + 1) << KEY_SHIFT < 0xFFFFFFFFull, "keys are 32 bits, all ones is the padding");

__host__ __device__ inline unsigned round16(unsigned x) { return (x + 15u) & ~15u; }

// keys: (rb, link index) into key[0 .. n4), n4 = N rounded up to 4; a link whose rb is outside [0, R) takes the pseudo RB R behind
// every real one, the padding behind N is all ones
template <int THREADS>
__device__ __forceinline__ void same_rb_keys(unsigned* key, const int* rb_row, int N, int n4, int R) {
    for (int j = (int)threadIdx.x; j < n4; j += THREADS) {
        unsigned k = 0xFFFFFFFFu;
        if (j < N) {
            const int r = rb_row[j];
            k = ((unsigned)((unsigned)r < (unsigned)R ? r : R) << KEY_SHIFT) | (unsigned)j;
        }
        key[j] = k;
    }
}

// rank: the slot of the link whose key is mine = #{keys below it}; the keys are distinct, so the slots are a permutation
__device__ __forceinline__ int same_rb_rank(const unsigned* key, int n4, unsigned mine) {
    int slot = 0;
    const uint4* k4 = reinterpret_cast<const uint4*>(key);
    for (int q = 0; q < (n4 >> 2); ++q) {
        const uint4 k = k4[q];
        slot += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine);
    }
    return slot;
}

// start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB.  srb[k] is the RB of sorted
// entry k (mine >> KEY_SHIFT).  Every word of start[0 .. R] is written: the ranges (prev, cur] of k = 0 .. N tile [0, R].
template <int THREADS, typename T>
__device__ __forceinline__ void same_rb_starts(int* start, const T* srb, int N, int R) {
    for (int k = (int)threadIdx.x; k <= N; k += THREADS) {
        const int prev = k == 0 ? -1 : (int)srb[k - 1];
        const int cur = k == N ? R : (int)srb[k];
        for (int r = prev + 1; r <= cur; ++r) start[r] = k;
    }
}

}  // namespace d2d
