// libd2d_probe.so, second source - the device functions the kernels share (d2d_step_device.h, d2d_wave_key.h, d2d_same_rb.h), one at
// a time behind thin wrapper kernels, for tests/test_gpu_devfn.py (declared in include/d2d_hip_diag.h).  Measurement equipment, NOT
// the product library.  Nothing a test compares is DEFINED here: every kernel loads its arguments, calls the header's function and
// stores what it returns.  Bounded loops, no atomics, no global store outside out0 / out1.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "d2d_hip_diag.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"
#include "d2d_wave_key.h"

namespace d2d {

int probe_fail(const std::string& msg) noexcept;         // d2d_probe.hip: the library's one error text

namespace {

constexpr int DEVFN_THREADS = 256;                       // the elementwise wrappers: one element per thread
constexpr int SAME_RB_THREADS = 256;                     // the one THREADS value every same-RB kernel of csrc/ instantiates

__device__ __forceinline__ size_t element() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_pow10_kernel(const int* p, float* out, size_t n) {
    const size_t i = element();
    if (i < n) out[i] = pow10_tenth(p[i]);
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_pow_half_kernel(const float* d2, const float* head, const float* tail, float* out, size_t n) {
    const size_t i = element();
    if (i < n) out[i] = pow_neg_half(d2[i], make_float2(head[i], tail[i]));
}

// NP pairs per thread, consecutive; the last thread's pairs behind n repeat pair n - 1 and are not stored
template <int NP, int KC>
__global__ __launch_bounds__(DEVFN_THREADS) void devfn_pow_k_kernel(const float* d2, const float* phi, float* out, size_t n, int k) {
    const size_t i0 = element() * NP;
    if (i0 >= n) return;
    float d[NP], f[NP], g[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const size_t i = i0 + p < n ? i0 + p : n - 1;
        d[p] = d2[i]; f[p] = phi[i];
    }
    pow_k_gains<NP, KC>(d, f, k, g);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (i0 + p < n) out[i0 + p] = g[p];
    }
}

template <int MODE>
__global__ __launch_bounds__(DEVFN_THREADS) void devfn_pair_gain_kernel(const float* d2, const float* head, const float* tail, float* out, size_t n, int k) {
    const size_t i = element();
    if (i < n) out[i] = pair_gain<MODE>(d2[i], make_float2(head[i], tail[i]), k);
}

template <bool PRECISE>
__global__ __launch_bounds__(DEVFN_THREADS) void devfn_div_kernel(const float* x, const float* y, float* out, size_t n) {
    const size_t i = element();
    if (i < n) out[i] = PRECISE ? precise_div(x[i], y[i]) : fast_div(x[i], y[i]);
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_cos_kernel(const float* u, float* out, size_t n) {
    const size_t i = element();
    if (i < n) out[i] = cos_turns(u[i]);
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_philox_kernel(const uint4* ctr, const uint2* key, unsigned* o0, unsigned* o1, size_t n) {
    const size_t i = element();
    if (i >= n) return;
    const uint4 c = ctr[i];
    const uint2 k = key[i];
    unsigned w0, w1;
    philox_step(c.x, c.y, c.z, c.w, k.x, k.y, w0, w1);
    o0[i] = w0; o1[i] = w1;
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_normal_kernel(const uint4* ctr, const uint2* key, float* out, size_t n) {
    const size_t i = element();
    if (i >= n) return;
    const uint4 c = ctr[i];
    const uint2 k = key[i];
    out[i] = philox_normal(c.x, c.y, c.z, c.w, k.x, k.y);
}

// the wave functions: the host launches whole workgroups only (n a multiple of the block), so all 64 lanes of every wave are active
__global__ __launch_bounds__(DEVFN_THREADS) void devfn_wave_sum_kernel(const float* in, float* out) {
    const size_t i = element();
    out[i] = wave_sum(in[i]);
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_wave_halves_kernel(const float* in, float* out_lo, float* out_hi) {
    const size_t i = element();
    float lo, hi;
    wave_sum_halves(in[i], lo, hi);
    out_lo[i] = lo; out_hi[i] = hi;
}

template <bool MAX>
__global__ __launch_bounds__(DEVFN_THREADS) void devfn_wave_key_kernel(const unsigned long long* in, unsigned long long* out) {
    const size_t i = element();
    out[i] = wave_reduce<MAX>(in[i]);
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_sort8_kernel(const unsigned* in, unsigned* out, size_t n) {
    const size_t i = element();
    if (i >= n) return;
    unsigned v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = in[i * 8 + q];
    sort8(v);
#pragma unroll
    for (int q = 0; q < 8; ++q) out[i * 8 + q] = v[q];
}

__global__ __launch_bounds__(DEVFN_THREADS) void devfn_obs_col_kernel(const unsigned* f, const unsigned* row, unsigned* out, size_t n) {
    const size_t i = element();
    if (i < n) out[i] = obs_src_col(f[i], row[i]);
}

// dynamic LDS: key u32[n4] | srb int[N] | (16-byte aligned) start int[R + 2], the last word a sentinel nothing may touch
unsigned same_rb_start_offset(unsigned N) { return round16((((N + 3u) & ~3u) + N) * 4u); }
unsigned same_rb_lds_bytes(unsigned N, unsigned R) { return same_rb_start_offset(N) + (R + 2u) * 4u; }

// One workgroup per env, staged as d2d_sense.hip and its kin stage it: keys, barrier, rank (every link's slot, and the sorted RB
// values), barrier, starts, barrier.  slot_out[b][j] = the slot of link j; start_out[b][0 .. R + 1] = the LDS words from start[0] on.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void devfn_same_rb_kernel(const int* rb, int* slot_out, int* start_out, int N, int R) {
    extern __shared__ __attribute__((aligned(16))) unsigned char devfn_smem[];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int n4 = (N + 3) & ~3;
    unsigned* key = reinterpret_cast<unsigned*>(devfn_smem);
    int* srb = reinterpret_cast<int*>(key + n4);
    int* start = reinterpret_cast<int*>(devfn_smem + round16((unsigned)(n4 + N) * 4u));
    for (int r = tid; r < R + 2; r += THREADS) start[r] = D2D_DEVFN_SENTINEL;
    same_rb_keys<THREADS>(key, rb + b * (size_t)N, N, n4, R);
    __syncthreads();
    for (int j = tid; j < N; j += THREADS) {
        const unsigned mine = key[j];
        const int slot = same_rb_rank(key, n4, mine);
        srb[slot] = (int)(mine >> KEY_SHIFT);
        slot_out[b * (size_t)N + j] = slot;
    }
    __syncthreads();
    same_rb_starts<THREADS>(start, srb, N, R);
    __syncthreads();
    for (int r = tid; r < R + 2; r += THREADS) start_out[b * (size_t)(R + 2) + r] = start[r];
}

const char* const kNames[D2D_DEVFN_COUNT] = {"pow10_tenth", "pow_neg_half", "pow_k_gains", "pair_gain", "precise_div", "fast_div", "cos_turns",
                                             "philox_step", "philox_normal", "wave_sum", "wave_sum_halves", "wave_reduce<true>",
                                             "wave_reduce<false>", "sort8", "obs_src_col", "same_rb"};
// the pointers each function takes: bit 0 a, 1 b, 2 c, 3 out0, 4 out1
const unsigned kPointers[D2D_DEVFN_COUNT] = {0x09, 0x0F, 0x0B, 0x0F, 0x0B, 0x0B, 0x09, 0x1B, 0x0B, 0x09, 0x19, 0x09, 0x09, 0x09, 0x0B, 0x19};

}  // namespace
}  // namespace d2d

extern "C" int d2d_probe_device_fn(int32_t fn, const void* a, const void* b, const void* c, void* out0, void* out1, int64_t n, int32_t k0,
                                   int32_t k1, void* hip_stream) try {
    using namespace d2d;
    if (fn < 0 || fn >= D2D_DEVFN_COUNT) return probe_fail("d2d_probe_device_fn: unknown fn");
    const std::string name = std::string("d2d_probe_device_fn(") + kNames[fn] + "): ";
    if (n < 0) return probe_fail(name + "n must not be negative");
    if (n >= (int64_t)1 << 31) return probe_fail(name + "n must be below 2^31");
    const bool wave = fn == D2D_DEVFN_WAVE_SUM || fn == D2D_DEVFN_WAVE_SUM_HALVES || fn == D2D_DEVFN_WAVE_MAX || fn == D2D_DEVFN_WAVE_MIN;
    if (wave) {
        if (k0 != 64 && k0 != 256) return probe_fail(name + "the block (k0) must be 64 or 256");
        if (n % k0 != 0) return probe_fail(name + "n must be a multiple of the block: all 64 lanes of every wave are active");
    }
    if (fn == D2D_DEVFN_POW_K_GAINS) {
        if (k0 < 1 || k0 > 8) return probe_fail(name + "pow_k must be in [1, 8]");
        if (k1 < 0 || k1 > 2) return probe_fail(name + "the form (k1) must be 0, 1 or 2");
        if (k1 == 2 && k0 != 4) return probe_fail(name + "form 2 is compiled for k == 4");
    }
    if (fn == D2D_DEVFN_PAIR_GAIN) {
        if (k0 != PL_INV_SQUARE && k0 != PL_POWER && k0 != PL_POWK) return probe_fail(name + "the mode (k0) must be 0, 1 or 4");
        if (k0 == PL_POWK && (k1 < 1 || k1 > 8)) return probe_fail(name + "pow_k must be in [1, 8]");
    }
    unsigned lds = 0;
    if (fn == D2D_DEVFN_SAME_RB) {
        if (k0 < 1 || k0 > SAME_RB_MAX_LINKS) return probe_fail(name + "N (k0) must be in [1, 2048]");
        if (k1 < 1 || k1 > SAME_RB_MAX_RBS) return probe_fail(name + "R (k1) must be in [1, 8192]");
        lds = same_rb_lds_bytes((unsigned)k0, (unsigned)k1);
        if (lds > 64u * 1024u) return probe_fail(name + "N and R need more than 64 KiB of LDS");
    }
    const void* const ptrs[5] = {a, b, c, out0, out1};
    static const char* const ptr_names[5] = {"a", "b", "c", "out0", "out1"};
    for (int q = 0; q < 5; ++q) {
        if ((kPointers[fn] >> q & 1u) && !ptrs[q]) return probe_fail(name + "null device pointer: " + ptr_names[q]);
    }
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t cnt = (size_t)n;
    const dim3 block(wave ? (unsigned)k0 : (unsigned)DEVFN_THREADS);
    const dim3 grid((unsigned)((cnt + block.x - 1) / block.x));
    const float *fa = static_cast<const float*>(a), *fb = static_cast<const float*>(b), *fc = static_cast<const float*>(c);
    float *f0 = static_cast<float*>(out0), *f1 = static_cast<float*>(out1);
    const uint4* ctr = static_cast<const uint4*>(a);
    const uint2* key = static_cast<const uint2*>(b);
    const unsigned long long* ka = static_cast<const unsigned long long*>(a);
    unsigned long long* k0out = static_cast<unsigned long long*>(out0);
    switch (fn) {
        case D2D_DEVFN_POW10_TENTH: hipLaunchKernelGGL(devfn_pow10_kernel, grid, block, 0, s, static_cast<const int*>(a), f0, cnt); break;
        case D2D_DEVFN_POW_NEG_HALF: hipLaunchKernelGGL(devfn_pow_half_kernel, grid, block, 0, s, fa, fb, fc, f0, cnt); break;
        case D2D_DEVFN_POW_K_GAINS:
            if (k1 == 0) hipLaunchKernelGGL((devfn_pow_k_kernel<1, 0>), grid, block, 0, s, fa, fb, f0, cnt, k0);
            else if (k1 == 1) hipLaunchKernelGGL((devfn_pow_k_kernel<4, 0>), dim3((unsigned)(((cnt + 3) / 4 + block.x - 1) / block.x)), block, 0, s, fa, fb, f0, cnt, k0);
            else hipLaunchKernelGGL((devfn_pow_k_kernel<1, 4>), grid, block, 0, s, fa, fb, f0, cnt, k0);
            break;
        case D2D_DEVFN_PAIR_GAIN:
            if (k0 == PL_INV_SQUARE) hipLaunchKernelGGL((devfn_pair_gain_kernel<PL_INV_SQUARE>), grid, block, 0, s, fa, fb, fc, f0, cnt, k1);
            else if (k0 == PL_POWER) hipLaunchKernelGGL((devfn_pair_gain_kernel<PL_POWER>), grid, block, 0, s, fa, fb, fc, f0, cnt, k1);
            else hipLaunchKernelGGL((devfn_pair_gain_kernel<PL_POWK>), grid, block, 0, s, fa, fb, fc, f0, cnt, k1);
            break;
        case D2D_DEVFN_PRECISE_DIV: hipLaunchKernelGGL((devfn_div_kernel<true>), grid, block, 0, s, fa, fb, f0, cnt); break;
        case D2D_DEVFN_FAST_DIV: hipLaunchKernelGGL((devfn_div_kernel<false>), grid, block, 0, s, fa, fb, f0, cnt); break;
        case D2D_DEVFN_COS_TURNS: hipLaunchKernelGGL(devfn_cos_kernel, grid, block, 0, s, fa, f0, cnt); break;
        case D2D_DEVFN_PHILOX_STEP:
            hipLaunchKernelGGL(devfn_philox_kernel, grid, block, 0, s, ctr, key, static_cast<unsigned*>(out0), static_cast<unsigned*>(out1), cnt);
            break;
        case D2D_DEVFN_PHILOX_NORMAL: hipLaunchKernelGGL(devfn_normal_kernel, grid, block, 0, s, ctr, key, f0, cnt); break;
        case D2D_DEVFN_WAVE_SUM: hipLaunchKernelGGL(devfn_wave_sum_kernel, grid, block, 0, s, fa, f0); break;
        case D2D_DEVFN_WAVE_SUM_HALVES: hipLaunchKernelGGL(devfn_wave_halves_kernel, grid, block, 0, s, fa, f0, f1); break;
        case D2D_DEVFN_WAVE_MAX: hipLaunchKernelGGL((devfn_wave_key_kernel<true>), grid, block, 0, s, ka, k0out); break;
        case D2D_DEVFN_WAVE_MIN: hipLaunchKernelGGL((devfn_wave_key_kernel<false>), grid, block, 0, s, ka, k0out); break;
        case D2D_DEVFN_SORT8: hipLaunchKernelGGL(devfn_sort8_kernel, grid, block, 0, s, static_cast<const unsigned*>(a), static_cast<unsigned*>(out0), cnt); break;
        case D2D_DEVFN_OBS_SRC_COL:
            hipLaunchKernelGGL(devfn_obs_col_kernel, grid, block, 0, s, static_cast<const unsigned*>(a), static_cast<const unsigned*>(b), static_cast<unsigned*>(out0), cnt);
            break;
        default:
            hipLaunchKernelGGL((devfn_same_rb_kernel<SAME_RB_THREADS>), dim3((unsigned)cnt), dim3(SAME_RB_THREADS), lds, s, static_cast<const int*>(a),
                               static_cast<int*>(out0), static_cast<int*>(out1), k0, k1);
            break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return probe_fail(name + "launch: " + hipGetErrorString(e));
    return 0;
} catch (...) { return d2d::probe_fail("C++ exception"); }
