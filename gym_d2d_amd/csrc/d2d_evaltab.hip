// libd2d_evaltab.so (include/d2d_evaltab.h): the SINR / capacity planes and the total capacity of K candidate joint assignments
// per env on a dB path-loss TABLE by (tx link, rx link), one launch.  gfx950.
//
// Shape: d2d_evaluate.hip's.  grid = (env, chunk of ET_CHUNK candidates), 256 threads.  The workgroup stages what no candidate
// changes - per link the tx constant, bandwidth, rx_lin, noise and sensitivity; no positions, no exponents - in LDS ONCE, then
// evaluates its candidates one after the other against it.  A candidate: keys (rb, link index), the rank sort of d2d_same_rb.h
// (stable, every word written by one owner) into (power, link index) tuples with start[r] = the first entry of RB r, then THREADS OWN SORTED SLOTS and
// walk their RB's members in ascending link index.  Entry [j][i] of the env's block comes from global memory (L2: the candidates of
// a chunk read the same block) and is converted where it is read, as the step's PL_TABLE_DB mode converts it; float products into a
// double accumulator - the step's own sum - and sinr_db and capacity by the step's own operations (d2d_step.hip, pass 2) with the
// table modes' columns (a_tx = a_rx = 0: rx_pl is exactly 1.0f and is dropped): the step's planes, bit for bit.  The total is
// d2d_evaluate.hip's: per thread in slot order, a fixed xor tree over the wave, the four wave sums in wave order by thread 0.  The
// domain flag is a bit per thread, a ballot per wave, one word per wave in LDS, and thread 0 writes.  Every output word is written
// once by its owner; no read-modify-write on memory anywhere, no scratch.
//
// Known limit: a thread with a long group walks G entries with a double exp2 each, and the reads of one receiver's column are
// strided by a table row (converting the table once into a float32 gain block is the option not built).
//
// Between candidates every per-candidate LDS array is rewritten (key, txl, srb, start, wsum, wdom); the four barriers of a
// candidate order each rewrite behind the last read of the candidate before it - see the notes at the barriers.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_evaltab.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int ET_THREADS = 256;
constexpr int ET_WAVES = ET_THREADS / 64;
constexpr int ET_CHUNK = D2D_EVALTAB_CHUNK;
static_assert(D2D_EVALTAB_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_EVALTAB_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_EVALTAB_MAX_CANDIDATES == 65535 * ET_CHUNK, "the grid's second dimension holds 65535 chunks");

struct EvalTabArgs {
    const void* table;              // [B][rows][N], float or double
    const int* rb;                  // [B][K][N]
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [3][D]: tx_lin, rx_lin, noise_mw
    const float* cap_cols;          // [2][D]
    float* sinr;                    // [B][K][N] or null
    float* cap;                     // [B][K][N] or null
    float* total;                   // [B][K]
    int* domain;                    // [B][K]
    int D, N, R, K, rows;
    unsigned off_sens, off_txl, off_key, off_srb, off_start, off_wsum, off_wdom;     // byte offsets behind ca
};

// dynamic LDS.  Staged once per workgroup, by link index j:
//   ca float4[N] (tx constant, bw_mhz, rx_lin, noise) | sens float[N]
// rewritten by every candidate, by sorted slot:
//   txl float2[N] (linear EIRP incl. the tx constant, link index) | key u32[N rounded up to 4] | srb int[N] | start int[R + 1]
//   | wsum double[4] | wdom u32[4]

// One dB entry -> linear gain: table_gain_db of d2d_step_device.h restated (that one takes the step's argument block) - the
// exponential in double, rounded once.  An entry that is NaN or -inf raises the flag, and only when it is read.
template <typename T>
__device__ __forceinline__ float entry_gain(const T* tab, size_t k, int& bad) {
    const double x = (double)tab[k];
    if (!(x > -__builtin_huge_val())) bad = 1;
    return (float)exp2(-0.33219280948873623478703194294894 * x);
}

template <typename T>
__global__ __launch_bounds__(ET_THREADS) void evaltab_kernel(const EvalTabArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = a.N, R = a.R, D = a.D, K = a.K;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    float4* ca = reinterpret_cast<float4*>(smem);
    float* sens_l = reinterpret_cast<float*>(smem + a.off_sens);
    float2* txl = reinterpret_cast<float2*>(smem + a.off_txl);
    unsigned* key = reinterpret_cast<unsigned*>(smem + a.off_key);
    int* srb = reinterpret_cast<int*>(smem + a.off_srb);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    double* wsum = reinterpret_cast<double*>(smem + a.off_wsum);
    unsigned* wdom = reinterpret_cast<unsigned*>(smem + a.off_wdom);
    const int n4 = (N + 3) & ~3;
    const T* tab = static_cast<const T*>(a.table) + b * (size_t)a.rows * (size_t)N;      // this env's block; rows >= N, row N never read

    // ---- what no candidate changes, once per workgroup
    for (int j = tid; j < N; j += ET_THREADS) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        ca[j] = make_float4(a.cols[txd], a.cap_cols[txd], a.cols[D + rxd], a.cols[2 * D + rxd]);
        sens_l[j] = a.cap_cols[D + rxd];
    }
    // (no barrier of its own: the first candidate's barrier behind the keys stands between these writes and their first reads)

    const int k0 = (int)blockIdx.y * ET_CHUNK;
    const int k1 = min(k0 + ET_CHUNK, K);
    for (int kc = k0; kc < k1; ++kc) {
        const size_t row = (b * (size_t)K + (size_t)kc) * (size_t)N;
        const int* rb_row = a.rb + row;
        const int* pwr_row = a.pwr + row;

        // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one.
        // key was last read by the sort of the candidate before, which lies behind two barriers.
        same_rb_keys<ET_THREADS>(key, rb_row, N, n4, R);
        __syncthreads();
        // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation and every
        // word of txl / srb is rewritten.  Their last readers (the walk of the candidate before) lie behind barrier 4.
        for (int j = tid; j < N; j += ET_THREADS) {
            const float pw = pow10_tenth(pwr_row[j]) * ca[j].x;                      // the step's tuple.z (d2d_step.hip, pass 1)
            const unsigned mine = key[j];
            const int slot = same_rb_rank(key, n4, mine);
            txl[slot] = make_float2(pw, __int_as_float(j));
            srb[slot] = (int)(mine >> KEY_SHIFT);
        }
        __syncthreads();
        // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB.  Every word of
        // start[0..R] is rewritten: the ranges (prev, cur] of k = 0..N tile [0, R].
        same_rb_starts<ET_THREADS>(start, srb, N, R);
        __syncthreads();

        // ---- the walk: the slot's link as receiver i, column i of the env's block
        double part = 0.0;
        int bad = 0;
        for (int s = tid; s < N; s += ET_THREADS) {
            const float2 me = txl[s];
            const int i = __float_as_int(me.y);
            const int r = srb[s];
            const float4 c = ca[i];
            const float bw_mhz = c.y, rx_lin = c.z, noise = c.w;
            const float sens = sens_l[i];
            int k = 0, k_end = 0;
            if (r < R) { k = start[r]; k_end = start[r + 1]; }
            double acc = 0.0;
#pragma unroll 1
            for (; k < k_end; ++k) {
                if (k == s) continue;                                        // .difference({action}), simulator.py:95
                const float2 o = txl[k];
                const float g = entry_gain(tab, (size_t)__float_as_int(o.y) * (size_t)N + (size_t)i, bad);
                acc += (double)(o.x * g);                                    // simulator.py:97-101, linear mW
            }
            // own link and its capacity: the step's operations in the step's order (d2d_step.hip, pass 2) with rx_pl == 1.0f:
            // me.z * g * rx_pl * rx_lin is (me.z * g) * rx_lin and fmaf(accf, rx_pl, noise) is accf + noise, both exactly
            const float g = entry_gain(tab, (size_t)i * (size_t)N + (size_t)i, bad);
            const float sig = me.x * g * rx_lin;
            const float accf = (float)acc;
            const float sinr_lin = precise_div(sig, fmaf(accf, 1.0f, noise));
            const float sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
            const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
            const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
            const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
            const bool ok = sinr_db > sens;                                  // simulator.py:123,149
            const float cap = ok ? bw_mhz * sh : 0.0f;                       // simulator.py:150-151
            if (a.sinr) a.sinr[row + (size_t)i] = sinr_db;
            if (a.cap) a.cap[row + (size_t)i] = cap;
            part += (double)cap;
        }
        // ---- the total: a fixed xor tree over the wave's 64 partial sums, then the wave sums in wave order; the flag: one ballot
        // per wave (every lane is here: the loop above has closed)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
        const unsigned long long any_bad = __builtin_amdgcn_ballot_w64(bad != 0);
        if ((tid & 63) == 0) { wsum[tid >> 6] = part; wdom[tid >> 6] = any_bad != 0ull ? 1u : 0u; }
        __syncthreads();                 // barrier 4: the walk is over - txl, srb and start may be rewritten
        if (tid == 0) {
            double t = wsum[0];
            unsigned f = wdom[0];
#pragma unroll
            for (int w = 1; w < ET_WAVES; ++w) { t += wsum[w]; f |= wdom[w]; }
            a.total[b * (size_t)K + (size_t)kc] = (float)t;
            a.domain[b * (size_t)K + (size_t)kc] = (int)f;
        }
        // wsum / wdom are rewritten behind the next candidate's three barriers, which thread 0 reaches only after this read
    }
}

}  // namespace

extern "C" int d2d_evaluate_table(const void* table, int32_t table_dtype, int32_t table_rows, const int32_t* rb, const int32_t* pwr_dbm,
                                  const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols,
                                  int64_t n_envs, int32_t n_cand, int32_t n_dev, int32_t n_links, int32_t n_rbs, float* sinr_db,
                                  float* capacity_mbps, float* total_mbps, int32_t* domain, void* hip_stream) try {
    if (n_cand < 1 || n_cand > D2D_EVALTAB_MAX_CANDIDATES) return fail("n_cand must be in [1, " + std::to_string(D2D_EVALTAB_MAX_CANDIDATES) + "]");
    if (const char* why = check_sizes(n_envs, n_links, D2D_EVALTAB_MAX_LINKS, n_rbs, D2D_EVALTAB_MAX_RBS, n_dev)) return fail(why);
    if (table_dtype != D2D_EVALTAB_F32 && table_dtype != D2D_EVALTAB_F64) return fail("table_dtype must be D2D_EVALTAB_F32 or D2D_EVALTAB_F64");
    if (table_rows != n_links && table_rows != n_links + 1) return fail("table_rows must be n_links or n_links + 1");
    if (!table || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !total_mbps || !domain)
        return fail("null device pointer");
    if (sinr_db && sinr_db == capacity_mbps) return fail("sinr_db and capacity_mbps must be two planes");
    EvalTabArgs a;
    a.table = table; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols; a.cap_cols = cap_cols;
    a.sinr = sinr_db; a.cap = capacity_mbps; a.total = total_mbps; a.domain = domain;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.K = n_cand; a.rows = table_rows;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_sens = N * 16u;
    a.off_txl = a.off_sens + round16(N * 4u);
    a.off_key = a.off_txl + round16(N * 8u);
    a.off_srb = a.off_key + n4 * 4u;
    a.off_start = a.off_srb + round16(N * 4u);
    a.off_wsum = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    a.off_wdom = a.off_wsum + (unsigned)(ET_WAVES * sizeof(double));
    const unsigned lds = a.off_wdom + (unsigned)(ET_WAVES * sizeof(unsigned));
    if (lds > (unsigned)D2D_EVALTAB_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                             std::to_string(D2D_EVALTAB_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs, (unsigned)((n_cand + ET_CHUNK - 1) / ET_CHUNK));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (table_dtype == D2D_EVALTAB_F64) e = launch(&evaltab_kernel<double>, grid, dim3(ET_THREADS), lds, s, a);
    else e = launch(&evaltab_kernel<float>, grid, dim3(ET_THREADS), lds, s, a);
    if (e != hipSuccess) return fail(std::string("evaltab_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_evaltab_last_error)
