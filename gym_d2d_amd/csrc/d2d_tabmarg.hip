// libd2d_tabmarg.so (include/d2d_tabmarg.h): every link's leave-one-out harm and difference reward on a dB path-loss TABLE by
// (tx link, rx link), one launch.  gfx950.
//
// Shape: d2d_marginal.hip's two phases on d2d_evaltab.hip's staging.  grid = env, 256 threads.  The workgroup sorts the env's N
// links by (rb, link index) - the rank sort of d2d_same_rb.h: stable, every word written by one owner - into (linear EIRP incl. the
// tx constant, link index) tuples with start[r] = the first entry of RB r.  From there on THREADS OWN SORTED SLOTS.
//   phase 1, the slot's link as RECEIVER j: evaltab_kernel's walk and closing - column j of the env's block, every entry converted
//            where it is read, float products in ascending link index into a double accumulator, sinr_db and capacity by the step's
//            own operations with rx_pl == 1.0f dropped: d2d_evaluate_table's capacity_mbps, bit for bit - and I_j (double), S_j,
//            bw_mhz, sens_db, noise and ok parked in LDS by sorted slot;
//   phase 2, the slot's link as TRANSMITTER i: marginal_kernel's, term for term, with rx_pl = 1 - row i of the env's block, t_ij the
//            identical float phase 1 added to I_j, I_j - t_ij IN DOUBLE, and the capacity victim j regains as ONE log2(1 + x) term,
//            x = S t / ((I' + noise) (I + noise + S)), or the whole capacity when only the removal lifts j over its threshold; the
//            terms of a link are summed in double in ascending j and rounded once.
// The entries are read in place (L2 / HBM): phase 1's reads of a receiver's column are strided by a table row (DESIGN.md 4.26's
// known limit), phase 2's reads of a transmitter's row are consecutive in j.  No float32 gain block (on the fading
// routes the table changes every step, and the conversion would cost more than the N G entries read twice).
// The domain flag is a bit per thread, a ballot per wave, one word per wave in LDS, and thread 0 writes.  Every output word is
// written once by its owner; no read-modify-write on memory anywhere, no scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"
#include "d2d_tabmarg.h"

namespace {

using namespace d2d;

constexpr int TM_THREADS = 256;
constexpr int TM_WAVES = TM_THREADS / 64;
static_assert(D2D_TABMARG_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_TABMARG_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");

struct TabMargArgs {
    const void* table;              // [B][rows][N], float or double
    const int* rb;                  // [B][N]
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [3][D]: tx_lin, rx_lin, noise_mw
    const float* cap_cols;          // [2][D]
    float* harm;                    // [B][N]
    float* diff;                    // [B][N]
    int* domain;                    // [B]
    int D, N, R, rows;
    unsigned off_txl, off_acc, off_noise, off_cap, off_srb, off_start, off_wdom;     // byte offsets behind v1
};

// dynamic LDS, by sorted slot:
//   v1 float4[N] (S_j, bw_mhz, sens_db, ok) | txl float2[N] (linear EIRP incl. the tx constant, link index) | acc double[n4], whose
//   bytes first hold the sort's keys u32[N rounded up to 4] | noise float[N] | cap float[N] | srb int[N] | start int[R + 1] | wdom u32[4]

// One dB entry -> linear gain: d2d_evaltab.hip's line (table_gain_db of d2d_step_device.h restated) - the exponential in double,
// rounded once.  An entry that is NaN or -inf raises the flag, and only when it is read.
template <typename T>
__device__ __forceinline__ float entry_gain(const T* tab, size_t k, int& bad) {
    const double x = (double)tab[k];
    if (!(x > -__builtin_huge_val())) bad = 1;
    return (float)exp2(-0.33219280948873623478703194294894 * x);
}

// log2(1 + x) with relative accuracy for small x: d2d_marginal.hip's (the step's form of its Shannon term)
__device__ __forceinline__ float log2_1p(float x) {
    const float u = 1.0f + x, um1 = u - 1.0f;
    const float big = __builtin_amdgcn_logf(u) * precise_div(x, um1 == 0.0f ? 1.0f : um1);
    return um1 == 0.0f ? x * 1.44269504088896340736f : big;
}

template <typename T>
__global__ __launch_bounds__(TM_THREADS) void tabmarg_kernel(const TabMargArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = a.N, R = a.R, D = a.D;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    float4* v1 = reinterpret_cast<float4*>(smem);
    float2* txl = reinterpret_cast<float2*>(smem + a.off_txl);
    double* accl = reinterpret_cast<double*>(smem + a.off_acc);
    unsigned* key = reinterpret_cast<unsigned*>(smem + a.off_acc);
    float* noise_l = reinterpret_cast<float*>(smem + a.off_noise);
    float* capl = reinterpret_cast<float*>(smem + a.off_cap);
    int* srb = reinterpret_cast<int*>(smem + a.off_srb);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    unsigned* wdom = reinterpret_cast<unsigned*>(smem + a.off_wdom);
    const int n4 = (N + 3) & ~3;
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const T* tab = static_cast<const T*>(a.table) + b * (size_t)a.rows * (size_t)N;      // this env's block; rows >= N, row N never read

    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one
    same_rb_keys<TM_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += TM_THREADS) {
        const float pw = pow10_tenth(pwr_row[j]) * a.cols[a.link_tx[j]];             // the step's tuple.z (d2d_step.hip, pass 1)
        const unsigned mine = key[j];
        const int slot = same_rb_rank(key, n4, mine);
        txl[slot] = make_float2(pw, __int_as_float(j));
        srb[slot] = (int)(mine >> KEY_SHIFT);
    }
    __syncthreads();                 // the last use of key: its bytes are the interference sums from here on
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB
    same_rb_starts<TM_THREADS>(start, srb, N, R);
    __syncthreads();

    int bad = 0;
    // ---- phase 1: the slot's link as receiver i, column i of the env's block (evaltab_kernel's walk and closing)
    for (int s = tid; s < N; s += TM_THREADS) {
        const float2 me = txl[s];
        const int i = __float_as_int(me.y);
        const int r = srb[s];
        const int txd = a.link_tx[i], rxd = a.link_rx[i];
        const float bw_mhz = a.cap_cols[txd], rx_lin = a.cols[D + rxd], noise = a.cols[2 * D + rxd];
        const float sens = a.cap_cols[D + rxd];
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
        v1[s] = make_float4(sig, bw_mhz, sens, ok ? 1.0f : 0.0f);
        noise_l[s] = noise;
        accl[s] = acc;
        capl[s] = cap;
    }
    __syncthreads();

    // ---- phase 2: the slot's link as transmitter i, row i of the env's block (marginal_kernel's, rx_pl = 1)
    for (int s = tid; s < N; s += TM_THREADS) {
        const float2 me = txl[s];
        const int i = __float_as_int(me.y);
        const int r = srb[s];
        int k = 0, k_end = 0;
        if (r < R) { k = start[r]; k_end = start[r + 1]; }
        double harm = 0.0;
#pragma unroll 1
        for (; k < k_end; ++k) {
            if (k == s) continue;
            const float4 q = v1[k];
            const double acc = accl[k];
            const int j = __float_as_int(txl[k].y);
            const float g = entry_gain(tab, (size_t)i * (size_t)N + (size_t)j, bad);
            const float t = me.x * g;                                    // the float phase 1 added to acc of slot k
            const double td = (double)t, noise = (double)noise_l[k], sig = (double)q.x;
            const double den = acc + noise;                              // with link i on the air
            const double denp = (acc - td) + noise;                      // without it
            const bool ok = q.w != 0.0f;
            // ok before: the gain of capacity is log2(1 + S t / (den' (den + S))); not ok before: the whole capacity without
            // link i, if that clears the threshold (the step's test, simulator.py:123, on the SINR without link i)
            const double num = ok ? sig * td : sig;
            const double dd = ok ? denp * (den + sig) : denp;
            const float x = (float)(num / dd);
            const bool ok_after = ok || 3.01029995663981195f * __builtin_amdgcn_logf(x) > q.z;
            const float term = ok_after ? q.y * log2_1p(x) : 0.0f;
            harm += (double)term;
        }
        const float harm_f = (float)harm;
        const size_t o = b * (size_t)N + (size_t)i;
        a.harm[o] = harm_f;
        a.diff[o] = capl[s] - harm_f;
    }
    // ---- the flag: one ballot per wave (every lane is here: the loops above have closed), the four words by thread 0
    const unsigned long long any_bad = __builtin_amdgcn_ballot_w64(bad != 0);
    if ((tid & 63) == 0) wdom[tid >> 6] = any_bad != 0ull ? 1u : 0u;
    __syncthreads();
    if (tid == 0) {
        unsigned f = wdom[0];
#pragma unroll
        for (int w = 1; w < TM_WAVES; ++w) f |= wdom[w];
        a.domain[b] = (int)f;
    }
}

}  // namespace

extern "C" int d2d_table_marginal(const void* table, int32_t table_dtype, int32_t table_rows, const int32_t* rb, const int32_t* pwr_dbm,
                                  const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols,
                                  int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, float* harm_mbps,
                                  float* difference_mbps, int32_t* domain, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_TABMARG_MAX_LINKS, n_rbs, D2D_TABMARG_MAX_RBS, n_dev)) return fail(why);
    if (table_dtype != D2D_TABMARG_F32 && table_dtype != D2D_TABMARG_F64) return fail("table_dtype must be D2D_TABMARG_F32 or D2D_TABMARG_F64");
    if (table_rows != n_links && table_rows != n_links + 1) return fail("table_rows must be n_links or n_links + 1");
    if (!table || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !harm_mbps || !difference_mbps || !domain)
        return fail("null device pointer");
    if (harm_mbps == difference_mbps) return fail("harm_mbps and difference_mbps must be two planes");
    TabMargArgs a;
    a.table = table; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols; a.cap_cols = cap_cols;
    a.harm = harm_mbps; a.diff = difference_mbps; a.domain = domain;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.rows = table_rows;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_txl = N * 16u;
    a.off_acc = a.off_txl + round16(N * 8u);
    a.off_noise = a.off_acc + n4 * 8u;                                   // doubles; the sort's keys (n4 * 4 bytes) fit inside
    a.off_cap = a.off_noise + round16(N * 4u);
    a.off_srb = a.off_cap + round16(N * 4u);
    a.off_start = a.off_srb + round16(N * 4u);
    a.off_wdom = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned lds = a.off_wdom + (unsigned)(TM_WAVES * sizeof(unsigned));
    if (lds > (unsigned)D2D_TABMARG_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                             std::to_string(D2D_TABMARG_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (table_dtype == D2D_TABMARG_F64) e = launch(&tabmarg_kernel<double>, grid, dim3(TM_THREADS), lds, s, a);
    else e = launch(&tabmarg_kernel<float>, grid, dim3(TM_THREADS), lds, s, a);
    if (e != hipSuccess) return fail(std::string("tabmarg_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_tabmarg_last_error)
