// libd2d_evaluate.so (include/d2d_evaluate.h): the SINR / capacity planes and the total capacity of K candidate joint assignments
// per env, one launch.  gfx950.
//
// Shape: grid = (env, chunk of EVAL_CHUNK candidates), 256 threads.  The workgroup stages what no candidate changes - per link the
// transmitter's position and tx constant, the exponent pair (power laws), the receiver's position, rx_pl, noise, rx_lin, bandwidth
// and sensitivity - in LDS ONCE, then evaluates its candidates one after the other against it.  A candidate is phase 1 of
// d2d_marginal.hip: keys (rb, link index), d2d_sense.hip's rank sort (stable, no atomics) into transmitter tuples with start[r] =
// the first entry of RB r, then THREADS OWN SORTED SLOTS and walk their RB's members in ascending link index, float products into a
// double accumulator - the step's own sum - and form sinr_db and capacity by the step's own operations (d2d_step.hip, pass 2): the
// step's planes, bit for bit.  The total is the double sum of the float capacities: per thread in slot order, a fixed xor tree over
// the wave, the four wave sums in wave order by thread 0.  Global memory is touched per candidate for its (rb, pwr) rows and its
// outputs only; every output word is written once by its owner, no floating-point read-modify-write anywhere.
//
// Between candidates every per-candidate LDS array is rewritten (key, sorted tuples, srb, start, wsum); the four barriers of a
// candidate order each rewrite behind the last read of the candidate before it - see the notes at the barriers.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_evaluate.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_WAVES = EVAL_THREADS / 64;
constexpr int EVAL_CHUNK = D2D_EVALUATE_CHUNK;
static_assert(D2D_EVALUATE_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_EVALUATE_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_EVALUATE_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_EVALUATE_LAW_POWER == LAW_POWER && D2D_EVALUATE_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_EVALUATE_MAX_CANDIDATES == 65535 * EVAL_CHUNK, "the grid's second dimension holds 65535 chunks");

struct EvaluateArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;                  // [B][K][N]
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* cap_cols;          // [2][D]
    float* sinr;                    // [B][K][N] or null
    float* cap;                     // [B][K][N] or null
    float* total;                   // [B][K]
    int D, N, R, K;
    int pow_k;
    unsigned off_rxa, off_rxb, off_hh, off_txl, off_shh, off_key, off_srb, off_start, off_wsum;     // byte offsets behind stx
};

// dynamic LDS.  Staged once per workgroup, by link index j:
//   stx float4[N] (tx x, tx y, tx constant, bw_mhz) | rxa float4[N] (rx x, rx y, rx_pl, noise) | rxb float2[N] (rx_lin, sens_db)
//   | hh float2[N] (power laws)
// rewritten by every candidate, by sorted slot:
//   txl float4[N] (tx x, tx y, linear EIRP incl. the tx constant, link index) | shh float2[N] (power laws) | key u32[N rounded up
//   to 4] | srb int[N] | start int[R + 1] | wsum double[4]

template <int MODE>
__global__ __launch_bounds__(EVAL_THREADS) void evaluate_kernel(const EvaluateArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int N = a.N, R = a.R, D = a.D, K = a.K;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    float4* stx = reinterpret_cast<float4*>(smem);
    float4* rxa = reinterpret_cast<float4*>(smem + a.off_rxa);
    float2* rxb = reinterpret_cast<float2*>(smem + a.off_rxb);
    float2* hh = reinterpret_cast<float2*>(smem + a.off_hh);
    float4* txl = reinterpret_cast<float4*>(smem + a.off_txl);
    float2* shh = reinterpret_cast<float2*>(smem + a.off_shh);
    unsigned* key = reinterpret_cast<unsigned*>(smem + a.off_key);
    int* srb = reinterpret_cast<int*>(smem + a.off_srb);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    double* wsum = reinterpret_cast<double*>(smem + a.off_wsum);
    const int n4 = (N + 3) & ~3;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- what no candidate changes, once per workgroup
    for (int j = tid; j < N; j += EVAL_THREADS) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        stx[j] = make_float4(px[txd], py[txd], a.cols[txd], a.cap_cols[txd]);
        rxa[j] = make_float4(px[rxd], py[rxd], a.cols[D + rxd], a.cols[3 * D + rxd]);
        rxb[j] = make_float2(a.cols[2 * D + rxd], a.cap_cols[D + rxd]);
        if (POWLAW) hh[j] = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
    }
    // (no barrier of its own: the first candidate's barrier behind the keys stands between these writes and their first reads)

    const int k0 = (int)blockIdx.y * EVAL_CHUNK;
    const int k1 = min(k0 + EVAL_CHUNK, K);
    for (int kc = k0; kc < k1; ++kc) {
        const size_t row = (b * (size_t)K + (size_t)kc) * (size_t)N;
        const int* rb_row = a.rb + row;
        const int* pwr_row = a.pwr + row;

        // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one.
        // key was last read by the sort of the candidate before, which lies behind two barriers.
        same_rb_keys<EVAL_THREADS>(key, rb_row, N, n4, R);
        __syncthreads();
        // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation and every
        // word of txl / shh / srb is rewritten.  Their last readers (the walk of the candidate before) lie behind barrier 4.
        for (int j = tid; j < N; j += EVAL_THREADS) {
            const float4 t = stx[j];
            const float pw = pow10_tenth(pwr_row[j]) * t.z;                          // the step's tuple.z (d2d_step.hip, pass 1)
            const unsigned mine = key[j];
            const int slot = same_rb_rank(key, n4, mine);
            txl[slot] = make_float4(t.x, t.y, pw, __int_as_float(j));
            if (POWLAW) shh[slot] = hh[j];
            srb[slot] = (int)(mine >> KEY_SHIFT);
        }
        __syncthreads();
        // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB.  Every word of
        // start[0..R] is rewritten: the ranges (prev, cur] of k = 0..N tile [0, R].
        same_rb_starts<EVAL_THREADS>(start, srb, N, R);
        __syncthreads();

        // ---- the walk: the slot's link as receiver (d2d_marginal.hip, phase 1)
        double part = 0.0;
        for (int s = tid; s < N; s += EVAL_THREADS) {
            const float4 me = txl[s];
            const int j = __float_as_int(me.w);
            const int r = srb[s];
            const float4 ra = rxa[j];
            const float2 rb2 = rxb[j];
            const float rx_x = ra.x, rx_y = ra.y, rx_pl = ra.z, noise = ra.w, rx_lin = rb2.x, sens = rb2.y;
            const float bw_mhz = stx[j].w;
            int k = 0, k_end = 0;
            if (r < R) { k = start[r]; k_end = start[r + 1]; }
            double acc = 0.0;
            for (; k < k_end; ++k) {
                const float4 o = txl[k];
                const float dx = o.x - rx_x, dy = o.y - rx_y;
                const float d2 = fmaf(dx, dx, dy * dy);
                const float g = pair_gain<MODE>(d2, POWLAW ? shh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
                const float term = o.z * g;                                  // simulator.py:97-101, linear mW
                acc += k != s ? (double)term : 0.0;
            }
            // own link and its capacity: the step's operations in the step's order (d2d_step.hip, pass 2)
            const float dx = me.x - rx_x, dy = me.y - rx_y;
            const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), POWLAW ? shh[s] : make_float2(-1.0f, 0.0f), a.pow_k);
            const float sig = me.z * g * rx_pl * rx_lin;
            const float accf = (float)acc;
            const float sinr_lin = precise_div(sig, fmaf(accf, rx_pl, noise));
            const float sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
            const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
            const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
            const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
            const bool ok = sinr_db > sens;                                  // simulator.py:123,149
            const float cap = ok ? bw_mhz * sh : 0.0f;                       // simulator.py:150-151
            if (a.sinr) a.sinr[row + (size_t)j] = sinr_db;
            if (a.cap) a.cap[row + (size_t)j] = cap;
            part += (double)cap;
        }
        // ---- the total: a fixed xor tree over the wave's 64 partial sums, then the wave sums in wave order
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
        if ((tid & 63) == 0) wsum[tid >> 6] = part;
        __syncthreads();                 // barrier 4: the walk is over - txl, shh, srb and start may be rewritten
        if (tid == 0) {
            double t = wsum[0];
#pragma unroll
            for (int w = 1; w < EVAL_WAVES; ++w) t += wsum[w];
            a.total[b * (size_t)K + (size_t)kc] = (float)t;
        }
        // wsum is rewritten behind the next candidate's three barriers, which thread 0 reaches only after this read
    }
}

}  // namespace

extern "C" int d2d_evaluate(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                            const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                            int64_t n_envs, int32_t n_cand, int32_t n_dev, int32_t n_links, int32_t n_rbs, float* sinr_db,
                            float* capacity_mbps, float* total_mbps, void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_cand < 1 || n_cand > D2D_EVALUATE_MAX_CANDIDATES) return fail("n_cand must be in [1, " + std::to_string(D2D_EVALUATE_MAX_CANDIDATES) + "]");
    if (const char* why = check_sizes(n_envs, n_links, D2D_EVALUATE_MAX_LINKS, n_rbs, D2D_EVALUATE_MAX_RBS, n_dev)) return fail(why);
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !total_mbps)
        return fail("null device pointer");
    if (sinr_db && sinr_db == capacity_mbps) return fail("sinr_db and capacity_mbps must be two planes");
    EvaluateArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.sinr = sinr_db; a.cap = capacity_mbps; a.total = total_mbps;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.K = n_cand; a.pow_k = pow_k;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    const unsigned h = law == D2D_EVALUATE_LAW_INV_SQUARE ? 0u : round16(N * 8u);
    a.off_rxa = N * 16u;
    a.off_rxb = a.off_rxa + N * 16u;
    a.off_hh = a.off_rxb + round16(N * 8u);
    a.off_txl = a.off_hh + h;
    a.off_shh = a.off_txl + N * 16u;
    a.off_key = a.off_shh + h;
    a.off_srb = a.off_key + n4 * 4u;
    a.off_start = a.off_srb + round16(N * 4u);
    a.off_wsum = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned lds = a.off_wsum + (unsigned)(EVAL_WAVES * sizeof(double));
    if (lds > (unsigned)D2D_EVALUATE_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                             std::to_string(D2D_EVALUATE_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs, (unsigned)((n_cand + EVAL_CHUNK - 1) / EVAL_CHUNK));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_EVALUATE_LAW_INV_SQUARE) e = launch(&evaluate_kernel<PL_INV_SQUARE>, grid, dim3(EVAL_THREADS), lds, s, a);
    else if (law == D2D_EVALUATE_LAW_POWER) e = launch(&evaluate_kernel<PL_POWER>, grid, dim3(EVAL_THREADS), lds, s, a);
    else e = launch(&evaluate_kernel<PL_POWK>, grid, dim3(EVAL_THREADS), lds, s, a);
    if (e != hipSuccess) return fail(std::string("evaluate_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_evaluate_last_error)
