// libd2d_channel.so (include/d2d_channel.h): the spatially consistent channel - median + correlated shadowing + block fading - of
// every (transmitter link, receiver link) pair of every env, into the live dB table the step kernel reads.  gfx950.
//
// Two launches per fill.
//   channel_phase_kernel   the shadowing's phases, the only part that needs double: one workgroup per (env, slab of 64 links) draws the
//                          env's 2 M_s wave vectors into LDS (Philox, turns per metre, double), then forms k . p of every (link,
//                          sinusoid) in double, reduces it to a fraction of a turn exactly and writes cos / sin as float32:
//                          [B][N][M_s] float4 (cos a, sin a, cos b, sin b), a the transmitter-side phase (phi_m included), b the
//                          receiver-side one.  B N M_s items in all - 1 / N of the table's entries.
//   channel_fill_kernel    one wave per (env, 32 transmitter rows x 64 receiver columns).  A lane owns ONE receiver column and holds its
//                          2 M_s cos / sin values in registers for the whole tile; the tile's transmitter-side pairs and row records
//                          sit in LDS (9 KB at M_s = 32) and are read as broadcasts, so an entry's shadow is 2 M_s FMAs,
//                          cos(a + b) = ca cb - sa sb.  A row's 64 entries leave as one 256-byte store; the lane on the diagonal
//                          writes row N too.  The workgroups of one env are numbered onto one XCD, so the env's pairs are read
//                          from that XCD's L2.
// No atomics, no scratch memory, every word written by the one lane that owns it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "d2d_addon.h"
#include "d2d_channel.h"
#include "d2d_step_device.h"

namespace {

constexpr int TILE_ROWS = 32;       // transmitter rows per workgroup
constexpr int TILE_COLS = 64;       // receiver columns per workgroup: one per lane
constexpr int SLAB_LINKS = 64;      // links per workgroup of the phase kernel
constexpr float INV_2_24 = 5.9604644775390625e-08f;

struct FillArgs {
    const float* pos_x;
    const float* pos_y;
    const int* link_tx;
    const int* link_rx;
    const double* a_tx;
    const double* a_rx;
    const double* expo;
    const int* elapsed_env;         // per-env clock (reset_env != null), else the scalars step / episode
    int* start_env;
    const unsigned* episode_env;
    const int* reset_env;
    float4* phases;                 // [B][N][M] (cos a, sin a, cos b, sin b)
    void* table;                    // [B][N + 1][N], float or double
    double wave_scale;              // 1 / (2 pi decorrelation_m): turns per metre
    unsigned B, D, N;
    unsigned row_tiles, col_tiles;
    unsigned first_env, shadow_lo, shadow_hi, fade_lo, fade_hi, step, episode;
    float amp, mu, s;
};

struct Clock {
    unsigned env, episode, t;
    bool pending;
};

__device__ __forceinline__ Clock env_clock(const FillArgs& a, unsigned b) {
    Clock c;
    c.env = a.first_env + b;
    c.pending = false;
    if (a.reset_env) {
        const unsigned next = a.episode_env[b];
        if (a.reset_env[b] != 0) { c.episode = next; c.t = 0u; c.pending = true; }
        else { c.episode = next - 1u; c.t = (unsigned)(a.elapsed_env[b] - a.start_env[b]) + 1u; }
    } else {
        c.episode = a.episode; c.t = a.step;
    }
    return c;
}

// (sin, cos)(2 pi u) for u in [0, 1), exact quadrant reduction: cos_turns (d2d_step_device.h) with both of its polynomials returned
__device__ __forceinline__ float2 sincos_turns(float u) {
    const float t = 4.0f * u;
    float q = floorf(t);
    float f = t - q;
    if (f > 0.5f) { f -= 1.0f; q += 1.0f; }
    const float x = f * 1.5707963267948966f, z = x * x;
    const float s = fmaf(x * z, fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), x);
    const float c = fmaf(z * z, fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), fmaf(-0.5f, z, 1.0f));
    const int k = (int)q;
    const float cb = (k & 1) ? s : c, sb = (k & 1) ? c : s;             // quarter turns: (c, s) -> (-s, c) -> (-c, -s) -> (s, -c)
    return make_float2((k & 2) ? -sb : sb, ((k + 1) & 2) ? -cb : cb);
}

// -ln(u1), u1 = (k + 0.5) 2^-24: philox_normal's two halves, each with an exact argument (d2d_step_device.h)
__device__ __forceinline__ float neg_log_u1(unsigned k1) {
    const float lo_half = logf(((float)(k1 & 0x7FFFFFu) + 0.5f) * INV_2_24);
    const float hi_half = log1pf(-(((float)(0x1000000u - k1) - 0.5f) * INV_2_24));
    return -(k1 < 0x800000u ? lo_half : hi_half);
}

// log2 x as exponent + log2 of the mantissa in [1/2, 1): v_log's error then is relative to a value below 1, not to |log2 x| ~ 17, which
// a slope of 3.5 * 5 log10(2) would turn into 1e-5 dB - the whole headroom of a float32 entry near 128 dB (ulp 7.6e-6).  log2(0) = -inf.
__device__ __forceinline__ double log2_split(float x) {
    return (double)__builtin_amdgcn_frexp_expf(x) + (double)log2f(__builtin_amdgcn_frexp_mantf(x));
}

// One wave vector in turns per metre, double: Philox words -> (kx, ky)
__device__ __forceinline__ void wave_vector(const FillArgs& a, const Clock& c, unsigned m, unsigned side, double& kx, double& ky) {
    unsigned w0, w1;
    d2d::philox_step(c.env, c.episode, m, side, a.shadow_lo, a.shadow_hi, w0, w1);
    const double one_minus_u = ((double)(0x1000000u - (w0 >> 8)) - 0.5) * 5.9604644775390625e-08;     // exact
    const double theta = (double)(w1 >> 8) * 5.9604644775390625e-08;
    const double k = a.wave_scale * sqrt(1.0 / (one_minus_u * one_minus_u) - 1.0);
    double sn, cs;
    sincospi(2.0 * theta, &sn, &cs);
    kx = k * cs; ky = k * sn;
}

template <int M>
__global__ __launch_bounds__(256) void channel_phase_kernel(const FillArgs a) {
    __shared__ double s_k[M][5];                                         // k^tx (x, y), k^rx (x, y), phi
    const unsigned slabs = (a.N + SLAB_LINKS - 1) / SLAB_LINKS;
    const unsigned b = blockIdx.x / slabs, l0 = (blockIdx.x % slabs) * SLAB_LINKS;
    const Clock c = env_clock(a, b);
    if (threadIdx.x < 2u * M) {
        const unsigned m = threadIdx.x >> 1, side = threadIdx.x & 1u;
        double kx, ky;
        wave_vector(a, c, m, side, kx, ky);
        s_k[m][2 * side] = kx; s_k[m][2 * side + 1] = ky;
        if (side == 0u) {
            unsigned w0, w1;
            d2d::philox_step(c.env, c.episode, m, 2u, a.shadow_lo, a.shadow_hi, w0, w1);
            s_k[m][4] = (double)(w0 >> 8) * 5.9604644775390625e-08;
        }
    }
    __syncthreads();
    const unsigned links = min((unsigned)SLAB_LINKS, a.N - l0);
    const size_t base = (size_t)b * a.D;
    for (unsigned it = threadIdx.x; it < links * M; it += 256u) {
        const unsigned l = l0 + it / M, m = it % M;
        const unsigned u = (unsigned)a.link_tx[l], v = (unsigned)a.link_rx[l];
        const double ux = a.pos_x[base + u], uy = a.pos_y[base + u], vx = a.pos_x[base + v], vy = a.pos_y[base + v];
        double ta = fma(s_k[m][0], ux, fma(s_k[m][1], uy, s_k[m][4]));   // turns
        double tb = fma(s_k[m][2], vx, s_k[m][3] * vy);
        ta -= rint(ta); tb -= rint(tb);                                  // exact: a fraction of a turn in [-1/2, 1/2]
        double sa, ca, sb, cb;
        sincospi(2.0 * ta, &sa, &ca);
        sincospi(2.0 * tb, &sb, &cb);
        a.phases[((size_t)b * a.N + l) * M + m] = make_float4((float)ca, (float)sa, (float)cb, (float)sb);
    }
}

template <int M, int FADE, class T>
__global__ __launch_bounds__(64) void channel_fill_kernel(const FillArgs a) {
    __shared__ float2 s_pos[TILE_ROWS];                                  // p_u
    __shared__ double2 s_law[TILE_ROWS];                                 // a_tx[u], exponent[u] * 5 log10(2)
    __shared__ unsigned s_dev[TILE_ROWS];
    __shared__ float2 s_tx[M ? TILE_ROWS * M : 1];                       // (cos a, sin a) of the tile's rows
    // workgroup -> (env, tile): consecutive workgroup ids go round the 8 XCDs, so an env's tiles take the ids of ONE residue class
    const unsigned xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const unsigned tiles = a.row_tiles * a.col_tiles;
    const unsigned b = (slot / tiles) * 8u + xcd, tile = slot % tiles;
    if (b >= a.B) return;
    const unsigned j0 = (tile / a.col_tiles) * TILE_ROWS, lane = threadIdx.x;
    const unsigned i = (tile % a.col_tiles) * TILE_COLS + lane;
    const bool live = i < a.N;
    const unsigned ic = live ? i : a.N - 1u;
    const Clock c = env_clock(a, b);
    if (c.pending && tile == 0u && lane == 0u) a.start_env[b] = 0;      // read by envs that are not pending only: never this env's
    const size_t base = (size_t)b * a.D;
    const unsigned rows = min((unsigned)TILE_ROWS, a.N - j0);
    if (lane < rows) {
        const unsigned u = (unsigned)a.link_tx[j0 + lane];
        s_dev[lane] = u;
        s_pos[lane] = make_float2(a.pos_x[base + u], a.pos_y[base + u]);
        s_law[lane] = make_double2(a.a_tx[u], a.expo[u] * 1.5051499783199060);
    }
    float cb[M ? M : 1], sb[M ? M : 1];
    if (M) {
        const float4* mine = a.phases + ((size_t)b * a.N + ic) * M;
#pragma unroll
        for (int m = 0; m < M; ++m) { const float4 p = mine[m]; cb[m] = p.z; sb[m] = p.w; }
        const float4* src = a.phases + ((size_t)b * a.N + j0) * M;
        for (unsigned k = lane; k < rows * M; k += TILE_COLS) { const float4 p = src[k]; s_tx[k] = make_float2(p.x, p.y); }
    }
    const unsigned v = (unsigned)a.link_rx[ic];
    const double vx = a.pos_x[base + v], vy = a.pos_y[base + v], arx = a.a_rx[v];
    __syncthreads();
    T* out = static_cast<T*>(a.table) + (size_t)b * (a.N + 1u) * a.N + i;
    for (unsigned r = 0; r < rows; ++r) {
        // the terms are summed in double and rounded at most ONCE, to a float32 entry: each float32 rounding of a ~100 dB partial
        // sum would cost half an ulp of the entry again (a float64 entry is stored as it is).  10 n log10 d = n 5 log10(2) log2 d^2; the differences are exact in double.
        const float2 pu = s_pos[r];
        const double2 law = s_law[r];
        const double dx = (double)pu.x - vx, dy = (double)pu.y - vy;
        double pl = fma(law.y, log2_split((float)fma(dx, dx, dy * dy)), law.x + arx);
        if (M) {
            float acc = 0.0f;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float2 t = s_tx[r * M + m];
                acc = fmaf(t.x, cb[m], acc);
                acc = fmaf(-t.y, sb[m], acc);
            }
            pl = fma((double)a.amp, (double)acc, pl);
        }
        if (FADE) {
            unsigned w0, w1;
            d2d::philox_step(c.env, c.t, s_dev[r] | (v << 16), c.episode, a.fade_lo, a.fade_hi, w0, w1);
            const float nl = neg_log_u1(w0 >> 8);
            float h2 = nl;                                               // Rayleigh: Exp(1)
            if (FADE == D2D_CHANNEL_FADING_RICIAN) {
                const float2 sc = sincos_turns((float)(w1 >> 8) * INV_2_24);
                const float sr = a.s * sqrtf(2.0f * nl);
                const float x = fmaf(sr, sc.y, a.mu), y = sr * sc.x;
                h2 = fmaf(x, x, y * y);
            }
            pl = fma(-3.0102999566398120, log2_split(h2), pl);
        }
        if (live) {
            out[(size_t)(j0 + r) * a.N] = (T)pl;
            if (j0 + r == i) out[(size_t)a.N * a.N] = (T)pl;             // row N: the link's own path, the same channel
        }
    }
}

template <int M, class T>
void launch_fill_as(const FillArgs& a, int fading, unsigned blocks, hipStream_t s) {
    if (fading == D2D_CHANNEL_FADING_NONE) hipLaunchKernelGGL((channel_fill_kernel<M, 0, T>), dim3(blocks), dim3(64), 0, s, a);
    else if (fading == D2D_CHANNEL_FADING_RAYLEIGH) hipLaunchKernelGGL((channel_fill_kernel<M, 1, T>), dim3(blocks), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((channel_fill_kernel<M, 2, T>), dim3(blocks), dim3(64), 0, s, a);
}

template <int M>
void launch_fill(const FillArgs& a, int fading, bool f64, unsigned blocks, hipStream_t s) {
    if (f64) launch_fill_as<M, double>(a, fading, blocks, s);
    else launch_fill_as<M, float>(a, fading, blocks, s);
}

}  // namespace

extern "C" int d2d_channel_fill(const float* pos_x, const float* pos_y, const int32_t* link_tx, const int32_t* link_rx,
                                const double* a_tx_db, const double* a_rx_db, const double* exponent, int64_t n_envs, int32_t n_dev,
                                int32_t n_links, uint64_t first_env, int32_t num_sinusoids, float shadow_amp_db, double wave_scale,
                                int32_t fading, float rician_mu, float rician_s, uint64_t shadow_seed, uint64_t fading_seed,
                                uint32_t step, uint32_t episode, const int32_t* elapsed_env, int32_t* start_env,
                                const uint32_t* episode_env, const int32_t* reset_env, float* phase_scratch, void* table,
                                int32_t table_dtype, void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_links < 1 || n_links > 2048) return fail("n_links must be in [1, 2048]");
    if (n_dev < 1 || n_dev >= 65536) return fail("n_dev must be in [1, 65536): the fading counter holds two device indices in one word");
    if (first_env + (uint64_t)n_envs > (1ull << 32)) return fail("first_env + n_envs must not exceed 2^32 (the env counter word)");
    if (num_sinusoids != 0 && num_sinusoids != 8 && num_sinusoids != 16 && num_sinusoids != 32)
        return fail("num_sinusoids must be 0 (no shadowing), 8, 16 or 32");
    if (fading < D2D_CHANNEL_FADING_NONE || fading > D2D_CHANNEL_FADING_RICIAN) return fail("fading must be a D2D_CHANNEL_FADING_* value");
    if (table_dtype != D2D_CHANNEL_F32 && table_dtype != D2D_CHANNEL_F64) return fail("table_dtype must be D2D_CHANNEL_F32 or D2D_CHANNEL_F64");
    if (num_sinusoids && (!std::isfinite(shadow_amp_db) || !(wave_scale > 0.0) || !std::isfinite(wave_scale)))
        return fail("shadow_amp_db must be finite and wave_scale finite and > 0");
    if (fading == D2D_CHANNEL_FADING_RICIAN && (!(rician_mu >= 0.0f) || !(rician_s > 0.0f) || !std::isfinite(rician_mu) || !std::isfinite(rician_s)))
        return fail("rician_mu must be finite and >= 0, rician_s finite and > 0");
    if (!pos_x || !pos_y || !link_tx || !link_rx || !a_tx_db || !a_rx_db || !exponent || !table) return fail("null device pointer");
    if (num_sinusoids && !phase_scratch) return fail("null device pointer: phase_scratch is needed when num_sinusoids != 0");
    if (((uintptr_t)table | (uintptr_t)phase_scratch) & 15u) return fail("table and phase_scratch must be 16-byte aligned");
    if (reset_env && (!elapsed_env || !start_env || !episode_env)) return fail("the per-env clock needs elapsed_env, start_env and episode_env");
    if (n_envs == 0) return 0;
    FillArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.link_tx = link_tx; a.link_rx = link_rx; a.a_tx = a_tx_db; a.a_rx = a_rx_db; a.expo = exponent;
    a.elapsed_env = elapsed_env; a.start_env = start_env; a.episode_env = episode_env; a.reset_env = reset_env;
    a.phases = reinterpret_cast<float4*>(phase_scratch); a.table = table; a.wave_scale = wave_scale;
    a.B = (unsigned)n_envs; a.D = (unsigned)n_dev; a.N = (unsigned)n_links;
    a.row_tiles = (a.N + TILE_ROWS - 1) / TILE_ROWS; a.col_tiles = (a.N + TILE_COLS - 1) / TILE_COLS;
    a.first_env = (unsigned)first_env;
    a.shadow_lo = (unsigned)(shadow_seed & 0xFFFFFFFFull); a.shadow_hi = (unsigned)(shadow_seed >> 32);
    a.fade_lo = (unsigned)(fading_seed & 0xFFFFFFFFull); a.fade_hi = (unsigned)(fading_seed >> 32);
    a.step = step; a.episode = episode;
    a.amp = shadow_amp_db; a.mu = rician_mu; a.s = rician_s;
    const unsigned long long blocks = (unsigned long long)((a.B + 7u) / 8u) * 8ull * a.row_tiles * a.col_tiles;
    if (blocks >= 0x7FFFFFFFull) return fail("n_envs * tiles must stay below 2^31 workgroups");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (num_sinusoids) {
        const dim3 grid(((a.N + SLAB_LINKS - 1) / SLAB_LINKS) * a.B);       // fewer workgroups than the fill has
        if (num_sinusoids == 8) hipLaunchKernelGGL(channel_phase_kernel<8>, grid, dim3(256), 0, s, a);
        else if (num_sinusoids == 16) hipLaunchKernelGGL(channel_phase_kernel<16>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(channel_phase_kernel<32>, grid, dim3(256), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(std::string("channel_phase_kernel launch: ") + hipGetErrorString(e));
    }
    switch (num_sinusoids) {
        case 0: launch_fill<0>(a, fading, table_dtype == D2D_CHANNEL_F64, (unsigned)blocks, s); break;
        case 8: launch_fill<8>(a, fading, table_dtype == D2D_CHANNEL_F64, (unsigned)blocks, s); break;
        case 16: launch_fill<16>(a, fading, table_dtype == D2D_CHANNEL_F64, (unsigned)blocks, s); break;
        default: launch_fill<32>(a, fading, table_dtype == D2D_CHANNEL_F64, (unsigned)blocks, s); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("channel_fill_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_channel_last_error)
