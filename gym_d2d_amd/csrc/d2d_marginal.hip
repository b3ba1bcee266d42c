// libd2d_marginal.so (include/d2d_marginal.h): every link's leave-one-out harm and difference reward, one launch.  gfx950.
//
// Shape: grid = env, 256 threads.  The workgroup sorts the env's N links by (rb, link index) into LDS - d2d_sense.hip's rank sort on
// the packed keys rb * 2048 + j: stable, so the members of an RB stand in ascending j, and free of atomics, so the order is the same
// on every call - as transmitter tuples (tx x, tx y, linear EIRP incl. the tx side of the path-loss constant, link index) with
// start[r] = the first entry of RB r.  From there on THREADS OWN SORTED SLOTS, so the lanes of a wave stand in the same or in
// neighbouring RBs: their walks over an RB's members have nearly the same bounds and read nearly the same LDS words.
//   phase 1, the slot's link as RECEIVER j: I_j over the other members of its RB in ascending link index, float products into a
//            double accumulator - the step's own sum, so that the capacity formed from it by the step's own operations
//            (d2d_step.hip, pass 2) is the step's plane, bit for bit - parked in LDS as a double beside the receiver's tuple
//            (rx x, rx y, rx_pl, noise | S_j, bw_mhz, sens_db, ok);
//   phase 2, the slot's link as TRANSMITTER i: over the same members as victims j, t_ij by the same pair function on the same
//            operands (the identical float phase 1 added), I_j - t_ij IN DOUBLE, and the capacity victim j regains as ONE
//            log2(1 + x) term, x = S t rx_pl / ((I' rx_pl + noise) (I rx_pl + noise + S)), or the whole capacity when only the
//            removal lifts j over its threshold; the terms of a link are summed in double in ascending j.
// No floating-point read-modify-write on memory anywhere; every output word is written once by its owner.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_marginal.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int MARG_THREADS = 256;
static_assert(D2D_MARGINAL_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_MARGINAL_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_MARGINAL_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_MARGINAL_LAW_POWER == LAW_POWER && D2D_MARGINAL_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");

struct MarginalArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* cap_cols;          // [2][D]
    float* harm;
    float* diff;
    int D, N, R;
    int pow_k;
    unsigned off_hh, off_v0, off_v1, off_acc, off_cap, off_srb, off_start;      // byte offsets of the LDS arrays behind the tuples
};

// dynamic LDS: tuples float4[N] | hh float2[N] (power laws) | v0 float4[N] | v1 float4[N] | acc double[N], whose bytes first hold the
// sort's keys u32[N rounded up to 4] | cap float[N] | srb int[N] | start int[R + 1]

// log2(1 + x) with relative accuracy for small x: log2(u) * x / (u - 1), u = fl(1 + x) (the step's form of its Shannon term)
__device__ __forceinline__ float log2_1p(float x) {
    const float u = 1.0f + x, um1 = u - 1.0f;
    const float big = __builtin_amdgcn_logf(u) * precise_div(x, um1 == 0.0f ? 1.0f : um1);
    return um1 == 0.0f ? x * 1.44269504088896340736f : big;
}

template <int MODE>
__global__ __launch_bounds__(MARG_THREADS) void marginal_kernel(const MarginalArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int N = a.N, R = a.R, D = a.D;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    float4* txl = reinterpret_cast<float4*>(smem);
    float2* hh = reinterpret_cast<float2*>(smem + a.off_hh);
    float4* v0 = reinterpret_cast<float4*>(smem + a.off_v0);
    float4* v1 = reinterpret_cast<float4*>(smem + a.off_v1);
    double* accl = reinterpret_cast<double*>(smem + a.off_acc);
    unsigned* key = reinterpret_cast<unsigned*>(smem + a.off_acc);
    float* capl = reinterpret_cast<float*>(smem + a.off_cap);
    int* srb = reinterpret_cast<int*>(smem + a.off_srb);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    const int n4 = (N + 3) & ~3;
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one
    same_rb_keys<MARG_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += MARG_THREADS) {
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
    __syncthreads();                 // the last use of key: its bytes are the interference sums from here on
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB
    same_rb_starts<MARG_THREADS>(start, srb, N, R);
    __syncthreads();

    // ---- phase 1: the slot's link as receiver
    for (int s = tid; s < N; s += MARG_THREADS) {
        const float4 me = txl[s];
        const int j = __float_as_int(me.w);
        const int r = srb[s];
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float rx_x = px[rxd], rx_y = py[rxd];
        const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
        const float bw_mhz = a.cap_cols[txd], sens = a.cap_cols[D + rxd];
        int k = 0, k_end = 0;
        if (r < R) { k = start[r]; k_end = start[r + 1]; }
        double acc = 0.0;
        for (; k < k_end; ++k) {
            const float4 o = txl[k];
            const float dx = o.x - rx_x, dy = o.y - rx_y;
            const float d2 = fmaf(dx, dx, dy * dy);
            const float g = pair_gain<MODE>(d2, POWLAW ? hh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
            const float term = o.z * g;                                  // simulator.py:97-101, linear mW
            acc += k != s ? (double)term : 0.0;
        }
        // own link and its capacity: the step's operations in the step's order (d2d_step.hip, pass 2)
        const float dx = me.x - rx_x, dy = me.y - rx_y;
        const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), POWLAW ? hh[s] : make_float2(-1.0f, 0.0f), a.pow_k);
        const float sig = me.z * g * rx_pl * rx_lin;
        const float accf = (float)acc;
        const float sinr_lin = precise_div(sig, fmaf(accf, rx_pl, noise));
        const float sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
        const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
        const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
        const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
        const bool ok = sinr_db > sens;                                  // simulator.py:123,149
        const float cap = ok ? bw_mhz * sh : 0.0f;                       // simulator.py:150-151
        v0[s] = make_float4(rx_x, rx_y, rx_pl, noise);
        v1[s] = make_float4(sig, bw_mhz, sens, ok ? 1.0f : 0.0f);
        accl[s] = acc;
        capl[s] = cap;
    }
    __syncthreads();

    // ---- phase 2: the slot's link as transmitter
    for (int s = tid; s < N; s += MARG_THREADS) {
        const float4 me = txl[s];
        const int i = __float_as_int(me.w);
        const int r = srb[s];
        const float2 h = POWLAW ? hh[s] : make_float2(-1.0f, 0.0f);
        int k = 0, k_end = 0;
        if (r < R) { k = start[r]; k_end = start[r + 1]; }
        double harm = 0.0;
        for (; k < k_end; ++k) {
            const float4 p = v0[k], q = v1[k];
            const double acc = accl[k];
            const float dx = me.x - p.x, dy = me.y - p.y;
            const float d2 = fmaf(dx, dx, dy * dy);
            const float g = pair_gain<MODE>(d2, h, a.pow_k);
            const float t = me.z * g;                                    // the float phase 1 added to acc of slot k
            const double td = (double)t, rx_pl = (double)p.z, noise = (double)p.w, sig = (double)q.x;
            const double den = fma(acc, rx_pl, noise);                   // with link i on the air
            const double denp = fma(acc - td, rx_pl, noise);             // without it
            const bool ok = q.w != 0.0f;
            // ok before: the gain of capacity is log2(1 + S t rx_pl / (den' (den + S))); not ok before: the whole capacity without
            // link i, if that clears the threshold (the step's test, simulator.py:123, on the SINR without link i)
            const double num = ok ? sig * rx_pl * td : sig;
            const double dd = ok ? denp * (den + sig) : denp;
            const float x = (float)(num / dd);
            const bool ok_after = ok || 3.01029995663981195f * __builtin_amdgcn_logf(x) > q.z;
            const float term = ok_after ? q.y * log2_1p(x) : 0.0f;
            harm += k != s ? (double)term : 0.0;
        }
        const float harm_f = (float)harm;
        const size_t o = b * (size_t)N + (size_t)i;
        a.harm[o] = harm_f;
        a.diff[o] = capl[s] - harm_f;
    }
}

}  // namespace

extern "C" int d2d_marginal_capacity(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm,
                                     const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols,
                                     int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs,
                                     float* harm_mbps, float* difference_mbps, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_MARGINAL_MAX_LINKS, n_rbs, D2D_MARGINAL_MAX_RBS, n_dev)) return fail(why);
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !harm_mbps || !difference_mbps)
        return fail("null device pointer");
    if (harm_mbps == difference_mbps) return fail("harm_mbps and difference_mbps must be two planes");
    if (n_envs == 0) return 0;
    MarginalArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.harm = harm_mbps; a.diff = difference_mbps;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_hh = N * 16u;
    a.off_v0 = a.off_hh + (law == D2D_MARGINAL_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_v1 = a.off_v0 + N * 16u;
    a.off_acc = a.off_v1 + N * 16u;
    a.off_cap = a.off_acc + round16(n4 * 8u);                            // doubles; the sort's keys (n4 * 4 bytes) fit inside
    a.off_srb = a.off_cap + round16(N * 4u);
    a.off_start = a.off_srb + round16(N * 4u);
    const unsigned lds = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    if (lds > 160u * 1024u) return fail("n_links and n_rbs need more than the 160 KiB of LDS a workgroup can have");
    const dim3 grid((unsigned)n_envs);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_MARGINAL_LAW_INV_SQUARE) e = launch(&marginal_kernel<PL_INV_SQUARE>, grid, dim3(MARG_THREADS), lds, s, a);
    else if (law == D2D_MARGINAL_LAW_POWER) e = launch(&marginal_kernel<PL_POWER>, grid, dim3(MARG_THREADS), lds, s, a);
    else e = launch(&marginal_kernel<PL_POWK>, grid, dim3(MARG_THREADS), lds, s, a);
    if (e != hipSuccess) return fail(std::string("marginal_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_marginal_last_error)
