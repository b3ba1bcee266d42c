// libd2d_bestrb.so (include/d2d_bestrb.h): every link's best resource block, the SINR it would see there and what the move would
// gain, one launch, without the [B][N][R] block of d2d_sense.hip.  gfx950.
//
// Shape: the sensing kernel's (d2d_sense.hip); the sort both share is d2d_same_rb.h.  grid = (env, block of 256 receivers),
// 256 threads.  The workgroup sorts the env's N links by (rb, link index) into LDS - the rank sort on the packed keys
// rb * 2048 + j, four keys per ds_read_b128 at a wave-uniform address: stable, free of atomics, the same order on every call - as
// transmitter tuples (tx x, tx y, linear EIRP incl. the tx side of the path-loss constant, link index), the per-tx law constants
// beside them and start[r] = the first entry of RB r.  Then LANES OWN RECEIVERS: a wave's 64 lanes walk the sorted list in lockstep
// (every tuple read is an LDS broadcast, the trip counts are wave-uniform: no divergence) and close the running sum at every RB
// boundary.  Where the sensing kernel puts the finished value into a tile, this one compares and selects into three registers:
// the best value so far, its r, and the value of the link's own RB.  No tile, no transpose: LDS holds the tuples, the starts and
// the sort's keys only, and each lane stores its three results once, 256 contiguous bytes per wave and plane.  The pair evaluation
// and the dB value are the sensing kernel's and the step's (d2d_step_device.h: fmaf(dx, dx, dy * dy), pair_gain, float products into
// a double accumulator, precise_div, v_log_f32) on the same operands in the same order, so best_sinr_db is a bit of d2d_sense_rb's
// block and the own-RB value is the step's sinr_db.  Strictly-greater selection in ascending r: equal values keep the lowest r.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_bestrb.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int BEST_THREADS = 256;
constexpr int GROUP_RBS = 32;                                    // one word of the allowed mask
static_assert(D2D_BESTRB_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_BESTRB_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_BESTRB_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_BESTRB_LAW_POWER == LAW_POWER && D2D_BESTRB_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");

struct BestArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const unsigned* allowed;        // [N][words] or null
    const unsigned char* env_mask;  // [B] or null
    int* best_rb;
    float* best_sinr;
    float* gain;
    int D, N, R;
    int pow_k;
    int words;                      // ceil(R / 32)
    unsigned off_hh, off_start, off_key;        // byte offsets of the LDS arrays behind the tuples
};

// dynamic LDS: tuples float4[N] | hh float2[N] (power laws) | start int[R + 1] | keys u32[N rounded up to 4] | sorted rb int[N]

template <int MODE>
__global__ __launch_bounds__(BEST_THREADS) void bestrb_kernel(const BestArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float4* txl = reinterpret_cast<float4*>(smem);
    float2* hh = reinterpret_cast<float2*>(smem + a.off_hh);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    unsigned* key = reinterpret_cast<unsigned*>(smem + a.off_key);
    const int n4 = (N + 3) & ~3;
    int* srb = reinterpret_cast<int*>(key + n4);
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one
    same_rb_keys<BEST_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += BEST_THREADS) {
        const int txd = a.link_tx[j];
        const float x = px[txd], y = py[txd];
        const float pw = pow10_tenth(pwr_row[j]) * a.cols[txd];                  // the step's tuple.z (d2d_step.hip, pass 1)
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const unsigned mine = key[j];
        const int slot = same_rb_rank(key, n4, mine);
        txl[slot] = make_float4(x, y, pw, __int_as_float(j));
        if (POWLAW) hh[slot] = h;
        srb[slot] = (int)(mine >> KEY_SHIFT);
    }
    __syncthreads();
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB
    same_rb_starts<BEST_THREADS>(start, srb, N, R);
    __syncthreads();

    // ---- lanes own receivers
    const int i0 = (int)blockIdx.y * BEST_THREADS + wave * 64;           // this wave's first receiver
    if (i0 >= N) return;                                                 // (no workgroup barrier below)
    const int i = min(i0 + lane, N - 1);                                 // lanes past the last link shadow it; they store nothing
    const int txd = a.link_tx[i], rxd = a.link_rx[i];
    const float rx_x = px[rxd], rx_y = py[rxd];
    const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
    float sig;
    {
        // own link: simulator.py:93, as the step forms it
        const float tx_x = px[txd], tx_y = py[txd];
        const float me_z = pow10_tenth(pwr_row[i]) * a.cols[txd];
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        sig = me_z * g * rx_pl * rx_lin;
    }
    const int my_rb = rb_row[i];                                         // outside [0, R): matches no r below, own stays NaN
    const unsigned* allowed_row = a.allowed ? a.allowed + (size_t)i * (size_t)a.words : nullptr;
    float best = __builtin_nanf(""), own = __builtin_nanf("");
    int best_r = -1;

    int k = __builtin_amdgcn_readfirstlane(start[0]);
    for (int r0 = 0; r0 < R; r0 += GROUP_RBS) {
        const int cw = min(GROUP_RBS, R - r0);
        const unsigned may = allowed_row ? allowed_row[r0 >> 5] : 0xFFFFFFFFu;
        for (int c = 0; c < cw; ++c) {
            const int r = r0 + c;
            const int k_end = __builtin_amdgcn_readfirstlane(start[r + 1]);
            double acc = 0.0;
            for (; k < k_end; ++k) {
                const float4 o = txl[k];
                const float dx = o.x - rx_x, dy = o.y - rx_y;
                const float d2 = fmaf(dx, dx, dy * dy);
                const float g = pair_gain<MODE>(d2, POWLAW ? hh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
                const float term = o.z * g;                                  // simulator.py:97-101, linear mW
                acc += __float_as_int(o.w) != i ? (double)term : 0.0;        // j != i by link index
            }
            const float accf = (float)acc;
            const float v = 3.01029995663981195f * __builtin_amdgcn_logf(precise_div(sig, fmaf(accf, rx_pl, noise)));
            const bool take = ((may >> c) & 1u) && (best_r < 0 || v > best);  // strictly greater: equal values keep the lowest r
            best = take ? v : best;
            best_r = take ? r : best_r;
            own = r == my_rb ? v : own;
        }
    }
    if (i0 + lane < N) {
        const size_t o = b * (size_t)N + (size_t)i;
        a.best_rb[o] = best_r;
        a.best_sinr[o] = best;                                           // NaN where nothing was allowed
        a.gain[o] = best - own;                                          // NaN where either is
    }
}

}  // namespace

extern "C" int d2d_best_rb(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                           const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                           int32_t n_links, int32_t n_rbs, const uint32_t* allowed, const uint8_t* env_mask, int32_t* best_rb,
                           float* best_sinr_db, float* gain_db, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_BESTRB_MAX_LINKS, n_rbs, D2D_BESTRB_MAX_RBS, n_dev)) return fail(why);
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !best_rb || !best_sinr_db || !gain_db)
        return fail("null device pointer");
    if (static_cast<void*>(best_rb) == static_cast<void*>(best_sinr_db) || static_cast<void*>(best_rb) == static_cast<void*>(gain_db) ||
        best_sinr_db == gain_db)
        return fail("best_rb, best_sinr_db and gain_db must be three planes");
    if (n_envs == 0) return 0;
    BestArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.allowed = allowed; a.env_mask = env_mask; a.best_rb = best_rb; a.best_sinr = best_sinr_db; a.gain = gain_db;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k;
    a.words = (n_rbs + 31) / 32;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_hh = N * 16u;
    a.off_start = a.off_hh + (law == D2D_BESTRB_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_key = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned lds = a.off_key + n4 * 4u + N * 4u;                   // at most 96 KiB + 32 bytes (2048 links, 8192 RBs, a power law)
    if (lds > 160u * 1024u) return fail("n_links and n_rbs need more than the 160 KiB of LDS a workgroup can have");
    const dim3 grid((unsigned)n_envs, (N + BEST_THREADS - 1) / BEST_THREADS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_BESTRB_LAW_INV_SQUARE) e = launch(&bestrb_kernel<PL_INV_SQUARE>, grid, dim3(BEST_THREADS), lds, s, a);
    else if (law == D2D_BESTRB_LAW_POWER) e = launch(&bestrb_kernel<PL_POWER>, grid, dim3(BEST_THREADS), lds, s, a);
    else e = launch(&bestrb_kernel<PL_POWK>, grid, dim3(BEST_THREADS), lds, s, a);
    if (e != hipSuccess) return fail(std::string("bestrb_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_bestrb_last_error)
