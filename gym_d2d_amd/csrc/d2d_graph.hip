// libd2d_graph.so (include/d2d_graph.h): the interference graph - the dense coupling matrix, every receiver's K strongest
// interferers, and the per-step gather of the neighbours' planes.  gfx950.
//
// All three kernels are receiver-major: [b][i][j] / [b][i][m], one agent's row contiguous.  A pair is evaluated by couple() below -
// the step's fmaf(dx, dx, dy * dy) and pair_gain (d2d_step_device.h), then (tx_lin * gain) * rx_pl - and turned into dB by lin_to_db(),
// in every kernel alike: a value the selection returns is an entry of the dense matrix bit for bit.
//
// coupling_kernel   LANES OWN TRANSMITTERS: a lane keeps the tuples of four transmitters j in registers (4 lane + q in the 16-byte
//                   form, lane + 64 q otherwise) and the wave walks its 32 receivers, whose (x, y, rx_pl) are LDS broadcasts; every
//                   receiver is four pair evaluations and one nontemporal 16-byte store per lane, 1 KiB of one output row per wave
//                   instruction (the cube is written once and not read by the GPU here).
// neighbors_kernel  A WAVE OWNS A RECEIVER: the workgroup stages the env's N transmitter tuples in LDS once and serves 64 receivers;
//                   for one receiver lane l evaluates the pairs j = l + 64 q, parks the keys (bits of the positive linear coupling,
//                   + 1 so that 0 means "taken / not a candidate") in its wave's LDS column and keeps its own best.  Then K rounds:
//                   a wave-wide maximum over the packed 64-bit key (bits << 32 | ~j) - DPP within rows, row broadcasts across,
//                   v_readlane at the end, no LDS crossbar - names the winner, with equal couplings resolved towards the smaller
//                   j by the ~j; the lane that owned it clears the entry and rescans its N / 64 keys.  No lane reads a key another
//                   lane wrote, so the selection needs no barrier, and nothing is atomic: the same bits on every call.
// neighbor_obs_kernel  one thread per 16-byte group of the observation: group 0 of a row is the link's own four values, group 1 + m
//                   gathers neighbour m's planes through idx (8 MB planes at full size: L2 / Infinity-Cache reads).
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_graph.h"
#include "d2d_sense.h"
#include "d2d_step_device.h"
#include "d2d_store.h"

namespace {

using namespace d2d;

constexpr int GRAPH_THREADS = 256;
constexpr int GRAPH_WAVES = GRAPH_THREADS / 64;
constexpr int COUPLING_ROWS = 128;                               // receivers per workgroup of coupling_kernel: 32 per wave
constexpr int NEIGHBOR_ROWS = 64;                                // receivers per workgroup of neighbors_kernel: 16 per wave
static_assert(D2D_GRAPH_MAX_K <= 64, "a lane holds one rank of the result");
static_assert(D2D_GRAPH_MAX_LINKS == D2D_SENSE_MAX_LINKS, "one link limit");
static_assert(D2D_SENSE_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_SENSE_LAW_POWER == LAW_POWER && D2D_SENSE_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");

struct GraphArgs {
    const float* pos_x;
    const float* pos_y;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    int D, N;
    int pow_k;
};

// linear coupling of transmitter tuple (x, y, tx_lin) with law constants h into the receiver at (rx_x, rx_y): positive, or inf / NaN
// for a zero distance as in the step
template <int MODE>
__device__ __forceinline__ float couple(float tx_x, float tx_y, float tx_lin, float2 h, float rx_x, float rx_y, float rx_pl, int pow_k) {
    const float dx = tx_x - rx_x, dy = tx_y - rx_y;
    const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, pow_k);
    return (tx_lin * g) * rx_pl;
}

// 10 log10(c) to within the float32 rounding of the result.  One v_log_f32 of c itself carries an ulp of log2(c) - at log2 ~ -50 that is
// 3.8e-6, 1.1e-5 dB - where the couplings of the steeper laws (-128 .. -175 dB, ulp 1.5e-5 dB) have no bits to spare: a user who
// rebuilds an SINR from two of them is at the project's 1e-5 bar before any arithmetic.  So the exponent is taken exactly and only
// the mantissa goes through v_log_f32 ([-1, 0): absolute 6e-8): 10 log10(2) = DB_HI + DB_LO with 12 significant bits in DB_HI, whose
// product with the integer exponent (|e| <= 150) is exact; one rounding at the end.  inf, NaN and 0 pass through as the logarithm
// gives them.
__device__ __forceinline__ float lin_to_db(float c) {
#pragma clang fp contract(off)
    constexpr float DB_HI = 3.009765625f;                                // 3082 / 1024
    constexpr float DB_LO = 5.3433163981195e-4f;                         // 3.01029995663981195 - DB_HI
    const float e = (float)__builtin_amdgcn_frexp_expf(c);
    const float l = __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(c));
    return fmaf(e, DB_HI, fmaf(e, DB_LO, 3.01029995663981195f * l));
}

// ------------------------------------------------------------------------------------------------------------------ dense matrix
template <int MODE, bool VEC>
__global__ __launch_bounds__(GRAPH_THREADS) void coupling_kernel(const GraphArgs a, float* __restrict__ out) {
    __shared__ float4 rxs[COUPLING_ROWS];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int N = a.N, D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;
    const int i0 = (int)blockIdx.y * COUPLING_ROWS;
    const int rows = min(COUPLING_ROWS, N - i0);
    for (int r = tid; r < rows; r += GRAPH_THREADS) {
        const int rxd = a.link_rx[i0 + r];
        rxs[r] = make_float4(px[rxd], py[rxd], a.cols[D + rxd], 0.0f);
    }
    __syncthreads();
    const int r_begin = wave * (COUPLING_ROWS / GRAPH_WAVES), r_end = min(r_begin + COUPLING_ROWS / GRAPH_WAVES, rows);
    for (int c0 = 0; c0 < N; c0 += 256) {
        int j[4];
        float tx_x[4], tx_y[4], tx_lin[4];
        float2 h[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            j[q] = VEC ? c0 + 4 * lane + q : c0 + lane + 64 * q;
            const int txd = a.link_tx[min(j[q], N - 1)];               // lanes past the last link shadow it; nothing of theirs is stored
            tx_x[q] = px[txd]; tx_y[q] = py[txd]; tx_lin[q] = a.cols[txd];
            h[q] = POWLAW ? make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]) : make_float2(-1.0f, 0.0f);
        }
        for (int r = r_begin; r < r_end; ++r) {
            const float4 rx = rxs[r];                                   // wave-uniform address: an LDS broadcast
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = lin_to_db(couple<MODE>(tx_x[q], tx_y[q], tx_lin[q], h[q], rx.x, rx.y, rx.z, a.pow_k));
            float* row = out + (b * (size_t)N + (size_t)(i0 + r)) * (size_t)N;
            if (VEC) {
                // N % 4 == 0 and out is 16-byte aligned: a group of four starts inside the row or not at all
                if (j[0] < N) store16<1>(reinterpret_cast<f32x4*>(row + j[0]), f32x4{v[0], v[1], v[2], v[3]});
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j[q] < N) __builtin_nontemporal_store(v[q], row + j[q]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ selection
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xF, BOUND);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xF, BOUND);
    return ((u64)hi << 32) | lo;
}

// Maximum over the 64 lanes, returned wave-uniform: the tree of wave_sum (d2d_step_device.h) with max for +.  A lane a row
// broadcast does not reach takes 0, the identity of max over unsigned keys.
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    v = max(v, dpp_u64<0xB1, 0xF, true>(v));            // quad_perm:[1,0,3,2]
    v = max(v, dpp_u64<0x4E, 0xF, true>(v));            // quad_perm:[2,3,0,1]
    v = max(v, dpp_u64<0x141, 0xF, true>(v));           // row_half_mirror
    v = max(v, dpp_u64<0x140, 0xF, true>(v));           // row_mirror
    v = max(v, dpp_u64<0x142, 0xA, false>(v));          // row_bcast:15 -> rows 1, 3
    v = max(v, dpp_u64<0x143, 0xC, false>(v));          // row_bcast:31 -> rows 2, 3
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

struct NeighborArgs {
    GraphArgs g;
    const unsigned char* env_mask;
    int* idx;
    float* coupling_db;
    int K;
    unsigned off_hh, off_keys;      // byte offsets of the LDS arrays behind the tuples
    unsigned n64;                   // N rounded up to 64: keys per wave
};

// dynamic LDS: tuples float4[N] | hh float2[N] (power laws) | keys u32[4 waves][n64]
template <int MODE>
__global__ __launch_bounds__(GRAPH_THREADS) void neighbors_kernel(const NeighborArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its only barrier
    const int N = a.g.N, D = a.g.D, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* px = a.g.pos_x + b * (size_t)D;
    const float* py = a.g.pos_y + b * (size_t)D;
    float4* txl = reinterpret_cast<float4*>(smem);
    float2* hh = reinterpret_cast<float2*>(smem + a.off_hh);
    unsigned* keys = reinterpret_cast<unsigned*>(smem + a.off_keys) + (unsigned)wave * a.n64;
    for (int j = tid; j < N; j += GRAPH_THREADS) {
        const int txd = a.g.link_tx[j];
        txl[j] = make_float4(px[txd], py[txd], a.g.cols[txd], 0.0f);
        if (POWLAW) hh[j] = make_float2(a.g.cols[4 * D + txd], a.g.cols[5 * D + txd]);
    }
    __syncthreads();
    const int i_begin = (int)blockIdx.y * NEIGHBOR_ROWS, i_end = min(i_begin + NEIGHBOR_ROWS, N);
    const int n64 = (int)a.n64;
    for (int i = i_begin + wave; i < i_end; i += GRAPH_WAVES) {
        const int rxd = a.g.link_rx[i];
        const float rx_x = px[rxd], rx_y = py[rxd], rx_pl = a.g.cols[D + rxd];
        unsigned best = 0u, best_j = 0u;
        for (int j = lane; j < n64; j += 64) {
            unsigned key = 0u;
            if (j < N && j != i) {
                const float4 t = txl[j];
                const float c = couple<MODE>(t.x, t.y, t.z, POWLAW ? hh[j] : make_float2(-1.0f, 0.0f), rx_x, rx_y, rx_pl, a.g.pow_k);
                key = min(__float_as_uint(c), 0xFFFFFFFEu) + 1u;         // >= 1: every candidate can be told from a taken entry
            }
            keys[j] = key;
            if (key > best) { best = key; best_j = (unsigned)j; }        // strict: of a lane's equal keys the smallest j
        }
        unsigned mine_j = 0u, mine_key = 1u;
        for (int m = 0; m < K; ++m) {
            const u64 top = wave_max_u64(((u64)best << 32) | (unsigned)~best_j);
            const unsigned win_j = ~(unsigned)top, win_key = (unsigned)(top >> 32);
            if (lane == m) { mine_j = win_j; mine_key = win_key; }
            if (win_key != 0u && (int)(win_j & 63u) == lane) {     // (k <= N - 1 candidates with keys >= 1: a winner always exists)
                keys[win_j] = 0u;
                best = 0u; best_j = 0u;
                for (int j = lane; j < n64; j += 64) {
                    const unsigned key = keys[j];
                    if (key > best) { best = key; best_j = (unsigned)j; }
                }
            }
        }
        if (lane < K) {
            const size_t o = (b * (size_t)N + (size_t)i) * (size_t)K + (size_t)lane;
            a.idx[o] = (int)mine_j;
            a.coupling_db[o] = lin_to_db(__uint_as_float(mine_key - 1u));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ per-step gather
struct NeighborObsArgs {
    const int* idx;
    const float* coupling_db;
    const int* rb;
    const int* pwr;
    const float* sinr;
    const float* snr;
    float* out;
    unsigned long long groups;      // n_envs * N * (K + 1)
    int N, K;
    int vec_ok;                     // out is 16-byte aligned
};

__global__ __launch_bounds__(GRAPH_THREADS) void neighbor_obs_kernel(const NeighborObsArgs a) {
    const unsigned N = (unsigned)a.N, K = (unsigned)a.K, W = K + 1u;
    const u64 stride = (u64)gridDim.x * GRAPH_THREADS;
    for (u64 g = (u64)blockIdx.x * GRAPH_THREADS + threadIdx.x; g < a.groups; g += stride) {
        const u64 link = g / W;                                          // b * N + i
        const unsigned t = (unsigned)(g - link * W);
        f32x4 v;
        if (t == 0u) {
            v = f32x4{(float)a.rb[link], (float)a.pwr[link], a.sinr[link], a.snr[link]};
        } else {
            const u64 e = link * K + (t - 1u);
            const unsigned j = (unsigned)a.idx[e];
            const float nan = __builtin_nanf("");
            v = f32x4{a.coupling_db[e], nan, nan, nan};
            if (j < N) {
                const u64 o = (link / N) * N + j;                        // b * N + j
                v.y = (float)a.rb[o]; v.z = (float)a.pwr[o]; v.w = a.sinr[o];
            }
        }
        float* dst = a.out + g * 4u;
        if (a.vec_ok) {
            store16<1>(reinterpret_cast<f32x4*>(dst), v);
        } else {
            __builtin_nontemporal_store(v.x, dst); __builtin_nontemporal_store(v.y, dst + 1);
            __builtin_nontemporal_store(v.z, dst + 2); __builtin_nontemporal_store(v.w, dst + 3);
        }
    }
}

const char* check_common(int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links) {
    if (const char* why = check_sizes(n_envs, n_links, D2D_GRAPH_MAX_LINKS, 0, 0, n_dev)) return why;
    return check_law(law, pow_k);
}

template <int MODE>
hipError_t launch_coupling(const GraphArgs& a, float* out, bool vec, dim3 grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((coupling_kernel<MODE, true>), grid, dim3(GRAPH_THREADS), 0, s, a, out);
    else hipLaunchKernelGGL((coupling_kernel<MODE, false>), grid, dim3(GRAPH_THREADS), 0, s, a, out);
    return hipGetLastError();
}

GraphArgs graph_args(const float* pos_x, const float* pos_y, const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols,
                     int32_t pow_k, int32_t n_dev, int32_t n_links) {
    GraphArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.D = n_dev; a.N = n_links; a.pow_k = pow_k;
    return a;
}

}  // namespace

extern "C" int d2d_graph_coupling(const float* pos_x, const float* pos_y, const int32_t* link_tx, const int32_t* link_rx,
                                  const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links,
                                  float* out, void* hip_stream) try {
    if (const char* why = check_common(law, pow_k, n_envs, n_dev, n_links)) return fail(why);
    if (!pos_x || !pos_y || !link_tx || !link_rx || !dev_cols || !out) return fail("null device pointer");
    if (n_envs == 0) return 0;
    const GraphArgs a = graph_args(pos_x, pos_y, link_tx, link_rx, dev_cols, pow_k, n_dev, n_links);
    const bool vec = reinterpret_cast<uintptr_t>(out) % 16 == 0 && n_links % 4 == 0;
    const dim3 grid((unsigned)n_envs, ((unsigned)n_links + COUPLING_ROWS - 1) / COUPLING_ROWS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const hipError_t e = law == D2D_SENSE_LAW_INV_SQUARE ? launch_coupling<PL_INV_SQUARE>(a, out, vec, grid, s)
                         : law == D2D_SENSE_LAW_POWER    ? launch_coupling<PL_POWER>(a, out, vec, grid, s)
                                                         : launch_coupling<PL_POWK>(a, out, vec, grid, s);
    if (e != hipSuccess) return fail(std::string("coupling_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

extern "C" int d2d_graph_neighbors(const float* pos_x, const float* pos_y, const int32_t* link_tx, const int32_t* link_rx,
                                   const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links,
                                   int32_t k, const uint8_t* env_mask, int32_t* idx, float* coupling_db, void* hip_stream) try {
    if (const char* why = check_common(law, pow_k, n_envs, n_dev, n_links)) return fail(why);
    const int k_max = n_links - 1 < D2D_GRAPH_MAX_K ? n_links - 1 : D2D_GRAPH_MAX_K;
    if (k < 1 || k > k_max) return fail("k must be in [1, min(n_links - 1, " + std::to_string(D2D_GRAPH_MAX_K) + ")]");
    if (!pos_x || !pos_y || !link_tx || !link_rx || !dev_cols || !idx || !coupling_db) return fail("null device pointer");
    if (n_envs == 0) return 0;
    NeighborArgs a;
    a.g = graph_args(pos_x, pos_y, link_tx, link_rx, dev_cols, pow_k, n_dev, n_links);
    a.env_mask = env_mask; a.idx = idx; a.coupling_db = coupling_db; a.K = k;
    const unsigned N = (unsigned)n_links;
    a.n64 = (N + 63u) & ~63u;
    a.off_hh = N * 16u;
    a.off_keys = a.off_hh + (law == D2D_SENSE_LAW_INV_SQUARE ? 0u : ((N * 8u + 15u) & ~15u));
    const unsigned lds = a.off_keys + GRAPH_WAVES * a.n64 * 4u;          // 80 KiB at 2048 links
    const dim3 grid((unsigned)n_envs, (N + NEIGHBOR_ROWS - 1) / NEIGHBOR_ROWS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 block(GRAPH_THREADS);
    const hipError_t e = law == D2D_SENSE_LAW_INV_SQUARE ? launch(&neighbors_kernel<PL_INV_SQUARE>, grid, block, lds, s, a)
                         : law == D2D_SENSE_LAW_POWER    ? launch(&neighbors_kernel<PL_POWER>, grid, block, lds, s, a)
                                                         : launch(&neighbors_kernel<PL_POWK>, grid, block, lds, s, a);
    if (e != hipSuccess) return fail(std::string("neighbors_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

extern "C" int d2d_graph_neighbor_obs(const int32_t* idx, const float* coupling_db, const int32_t* rb, const int32_t* pwr_dbm,
                                      const float* sinr_db, const float* snr_db, int64_t n_envs, int32_t n_links, int32_t k, float* out,
                                      void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_links < 1 || n_links > D2D_GRAPH_MAX_LINKS) return fail("n_links must be in [1, 2048]");
    if (k < 0 || k > D2D_GRAPH_MAX_K) return fail("k must be in [0, " + std::to_string(D2D_GRAPH_MAX_K) + "]");
    if (!rb || !pwr_dbm || !sinr_db || !snr_db || !out || (k > 0 && (!idx || !coupling_db))) return fail("null device pointer");
    if (n_envs == 0) return 0;
    NeighborObsArgs a;
    a.idx = idx; a.coupling_db = coupling_db; a.rb = rb; a.pwr = pwr_dbm; a.sinr = sinr_db; a.snr = snr_db; a.out = out;
    a.N = n_links; a.K = k;
    a.groups = (unsigned long long)n_envs * (unsigned long long)n_links * (unsigned long long)(k + 1);
    a.vec_ok = reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const unsigned long long blocks = (a.groups + GRAPH_THREADS - 1) / GRAPH_THREADS;
    const dim3 grid((unsigned)(blocks < (1ull << 20) ? blocks : (1ull << 20)));
    hipLaunchKernelGGL(neighbor_obs_kernel, grid, dim3(GRAPH_THREADS), 0, static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("neighbor_obs_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_graph_last_error)
