// libd2d_episode.so (include/d2d_episode.h): the two per-step kernels of VecD2DEnv's autoreset around d2d_step.  gfx950.
//
// merge_kernel is a streaming copy of the [B, A] int32 action block into the handle's action buffer, 16 bytes per lane, in which
// the rows of pending envs are replaced by their reset's random actions (the splitmix64 stream of envs/_rng.py, per env at its own
// episode).  advance_kernel is one lane per env for the counters; a wave then zeroes the reward rows of its reset envs together,
// one row after the other, so a step in which no env resets writes 14 bytes per env and nothing else.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "d2d_addon.h"
#include "d2d_episode.h"

namespace {

constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ull, M1 = 0xBF58476D1CE4E5B9ull, M2 = 0x94D049BB133111EBull;

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long x) {     // splitmix64's finaliser (_rng._mix_int)
    x = (x ^ (x >> 30)) * M1;
    x = (x ^ (x >> 27)) * M2;
    return x ^ (x >> 31);
}

struct MergeArgs {
    unsigned long long total;       // n_envs * n_cols
    unsigned long long first_env;
    unsigned long long seed_mix;    // mix64(seed): the episode key is mix64(seed_mix ^ (episode + 1) * golden) (_rng.stream_key)
    unsigned n_cols;
    int narrow;                     // total < 2^32: 32-bit index arithmetic
};

// _rng.uniform_ints_numpy's value at (env first_env + b, column c) for the episode key `key`
__device__ __forceinline__ int reset_action(const MergeArgs& a, unsigned long long key, unsigned long long b, unsigned c, int high) {
    const unsigned long long x = mix64(key + ((a.first_env + b) * a.n_cols + c + 1ull) * GOLDEN);
    return (int)((x >> 11) % (unsigned long long)(unsigned)high);
}

__device__ __forceinline__ unsigned long long episode_key(const MergeArgs& a, unsigned e) {
    return mix64(a.seed_mix ^ (((unsigned long long)e + 1ull) * GOLDEN));
}

// VEC = 4: int4 loads and stores (both pointers 16-byte aligned), the last total % 4 elements by one lane; VEC = 1 otherwise.
// in may equal out: every element is read and written by the same lane.
template <int VEC>
__global__ __launch_bounds__(256) void merge_kernel(const int* in, int* out, const int* __restrict__ pending,
                                                    const unsigned* __restrict__ episode, const int* __restrict__ high,
                                                    const MergeArgs a) {
    using V = typename std::conditional<VEC == 4, int4, int>::type;
    const unsigned long long nvec = a.total / VEC;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256u + threadIdx.x; v < nvec; v += stride) {
        const unsigned long long k0 = v * VEC;
        unsigned long long b;
        unsigned c;
        if (a.narrow) {
            const unsigned q = (unsigned)k0 / a.n_cols;
            b = q; c = (unsigned)k0 - q * a.n_cols;
        } else {
            b = k0 / a.n_cols; c = (unsigned)(k0 - b * a.n_cols);
        }
        V w = reinterpret_cast<const V*>(in)[v];
        int* x = reinterpret_cast<int*>(&w);
        int p = pending[b];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (p) x[e] = reset_action(a, episode_key(a, episode[b]), b, c, high[c]);
            if (++c == a.n_cols && e + 1 < VEC) { c = 0; ++b; p = pending[b]; }     // the next element exists: b < n_envs
        }
        reinterpret_cast<V*>(out)[v] = w;
    }
    if (VEC > 1 && blockIdx.x == 0 && threadIdx.x == 0) {
        for (unsigned long long k = nvec * VEC; k < a.total; ++k) {
            const unsigned long long b = k / a.n_cols;
            const unsigned c = (unsigned)(k - b * a.n_cols);
            out[k] = pending[b] ? reset_action(a, episode_key(a, episode[b]), b, c, high[c]) : in[k];
        }
    }
}

struct AdvanceArgs {
    int* pending;
    unsigned* episode;
    int* elapsed;
    unsigned char* done;
    unsigned char* reset_out;
    float* reward;                  // [n_envs, reward_cols] or null
    unsigned reward_cols;
    unsigned long long n_envs;
    int length;
};

__global__ __launch_bounds__(256) void advance_kernel(const AdvanceArgs a) {
    const unsigned long long b = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    bool reset = false;
    if (b < a.n_envs) {
        if (a.pending[b]) {
            a.elapsed[b] = 0; a.episode[b] += 1u; a.pending[b] = 0; a.reset_out[b] = 1; a.done[b] = 0;
            reset = true;
        } else {
            const int e = a.elapsed[b] + 1;
            const int d = e >= a.length;
            a.elapsed[b] = e; a.done[b] = (unsigned char)d; a.pending[b] = d; a.reset_out[b] = 0;
        }
    }
    if (!a.reward) return;
    // the reward rows of this wave's reset envs, each zeroed by all 64 lanes (coalesced) - a loop only where some env reset
    unsigned long long mask = __ballot(reset);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long wave_env = b - lane;
    while (mask) {
        const unsigned j = (unsigned)__ffsll((long long)mask) - 1u;
        mask &= mask - 1ull;
        float* row = a.reward + (wave_env + j) * a.reward_cols;
        for (unsigned i = lane; i < a.reward_cols; i += 64u) row[i] = 0.0f;
    }
}

int device_cus() {
    static std::mutex mu;
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 256; }
    std::lock_guard<std::mutex> lock(mu);
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
        cus[dev] = n;
    }
    return cus[dev];
}

}  // namespace

extern "C" int d2d_episode_merge_actions(const int32_t* actions_in, int32_t* actions_out, const int32_t* pending, const uint32_t* episode,
                                         const int32_t* high, int64_t n_envs, int32_t n_cols, uint64_t first_env, uint64_t seed,
                                         void* hip_stream) try {
    if (n_envs < 0 || n_cols < 0) return fail("n_envs and n_cols must be >= 0");
    if (n_envs == 0 || n_cols == 0) return 0;
    if (!actions_in || !actions_out || !pending || !episode || !high) return fail("null device pointer");
    MergeArgs a;
    a.total = (unsigned long long)n_envs * (unsigned long long)n_cols;
    a.first_env = first_env;
    a.seed_mix = mix64(seed);
    a.n_cols = (unsigned)n_cols;
    a.narrow = a.total < (1ull << 32);
    const bool vec = reinterpret_cast<uintptr_t>(actions_in) % 16 == 0 && reinterpret_cast<uintptr_t>(actions_out) % 16 == 0;
    unsigned long long blocks = (a.total / (vec ? 4 : 1) + 255) / 256;
    const unsigned long long cap = (unsigned long long)device_cus() * 32;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;                                  // fewer elements than one vector: the tail lane alone
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const unsigned* ep = reinterpret_cast<const unsigned*>(episode);
    if (vec) hipLaunchKernelGGL(merge_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, actions_in, actions_out, pending, ep, high, a);
    else hipLaunchKernelGGL(merge_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, actions_in, actions_out, pending, ep, high, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("merge_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

extern "C" int d2d_episode_advance(int32_t* pending, uint32_t* episode, int32_t* elapsed, uint8_t* done, uint8_t* reset_out, float* reward,
                                   int32_t reward_cols, int64_t n_envs, int32_t episode_length, void* hip_stream) try {
    if (n_envs < 0) return fail("n_envs must be >= 0");
    if (episode_length < 1) return fail("episode_length must be >= 1");
    if (reward && reward_cols < 1) return fail("reward_cols must be >= 1 with a reward");
    if (n_envs == 0) return 0;
    if (!pending || !episode || !elapsed || !done || !reset_out) return fail("null device pointer");
    AdvanceArgs a{pending, reinterpret_cast<unsigned*>(episode), elapsed, done, reset_out, reward, reward ? (unsigned)reward_cols : 0u,
                  (unsigned long long)n_envs, episode_length};
    hipLaunchKernelGGL(advance_kernel, dim3((unsigned)(((unsigned long long)n_envs + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("advance_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_episode_last_error)
