// libd2d_powerctl.so (include/d2d_powerctl.h): the constrained target-SINR power iteration on the integer dBm alphabet, every sweep
// of every env in one launch.  gfx950.
//
// Shape: ONE workgroup of 256 threads per env - the iteration couples exactly the links of one env - that stages the env once and
// then sweeps in LDS.  Staging is the sensing / best-response kernels' (d2d_sense.hip, d2d_bestrb.hip), whose sort all
// of them take from d2d_same_rb.h: the rank sort of the packed keys rb * 2048 + j (four keys per ds_read_b128 at a wave-uniform address:
// stable, free of atomics, the same order on every call) puts every link's constants into its sorted slot - transmitter tuple (tx x,
// tx y, the folded tx column, link index), the power-law head / tail, receiver tuple (rx x, rx y, rx side of the path-loss constant,
// noise), (own-pair gain, rx gain), target, bounds, start power - and start[r] = the first slot of RB r, folded per slot into the
// pair (first, last + 1) of the link's own RB.  Then LANES OWN SLOTS, a lane with several of them loops: neighbouring lanes own
// neighbouring slots, so the lanes of a wave mostly walk the same RB's members (identical LDS addresses broadcast) and a wave runs
// as long as its longest RB group.  A sweep reads the linear powers of the old vector z[cur], writes the new ones to z[cur ^ 1]
// (Jacobi) and ends in ONE barrier that also carries the "anything changed" flag: each wave's ballot goes into a word of LDS, every
// thread reads the four words behind the barrier.  No global access inside the sweep loop, no atomics, no scratch, no [B][N][N] or
// [B][N][R] buffer: global memory is read while staging and written once behind the last sweep.
//
// The pair gains are recomputed in every sweep - only z changes between sweeps, but a lane's gains would be (links per lane) x (RB
// group length) registers, which has no bound short of N^2 / 256; the RB groups of the shapes this serves are short (2 links at 512
// x 256), and the long-group cases pay v_rcp / v_exp per pair as the step does.  The pair evaluation and the dB value are the step's
// (d2d_step_device.h: fmaf(dx, dx, dy * dy), pair_gain, float products into a double accumulator in ascending j, precise_div,
// v_log_f32, one multiply) on the same operands in the same order, so s is the step's sinr_db for those powers bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_powerctl.h"
#include "d2d_powerctl_device.h"
#include "d2d_same_rb.h"

namespace {

using namespace d2d;

constexpr int PC_THREADS = 256;
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr unsigned NO_RB = PC_NO_RB;                             // range word of a link on no RB (d2d_powerctl_device.h)
static_assert(D2D_POWERCTL_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_POWERCTL_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_POWERCTL_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_POWERCTL_LAW_POWER == LAW_POWER && D2D_POWERCTL_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_POWERCTL_MAX_LINKS < (1 << 15), "a range word packs two slot indices into 16 bits each under the NO_RB bit");

struct PowerArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* target;            // [N]
    const int* p_min;               // [N]
    const int* p_max;               // [N]
    const unsigned char* adjustable;  // [N] or null
    const unsigned char* env_mask;  // [B] or null
    int* power;
    float* sinr;
    int* iters;
    unsigned char* converged;
    int D, N, R;
    int pow_k;
    int max_iters;
    // byte offsets of the LDS arrays behind the transmitter tuples
    unsigned off_rxa, off_rxb, off_lohi, off_hh, off_tgt, off_p, off_range, off_z0, off_z1, off_start, off_flag;
};

// dynamic LDS, by sorted slot: tx float4[N] | rxa float4[N] | rxb float2[N] | lohi int2[N] | hh float2[N] (power laws) | target f32[n4]
// | p i32[n4] | range u32[n4] (the sorted rb until start[] exists) | z0 f32[n4] | z1 f32[n4] (the sort's keys until the first sweep) |
// start i32[R + 1] | flag i32[2][4]

struct Lds {
    float4* tx; float4* rxa; float2* rxb; int2* lohi; float2* hh; float* tgt; int* p; unsigned* range; float* z0; float* z1; int* start; int* flag;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const PowerArgs& a) {
    Lds s;
    s.tx = reinterpret_cast<float4*>(smem);
    s.rxa = reinterpret_cast<float4*>(smem + a.off_rxa);
    s.rxb = reinterpret_cast<float2*>(smem + a.off_rxb);
    s.lohi = reinterpret_cast<int2*>(smem + a.off_lohi);
    s.hh = reinterpret_cast<float2*>(smem + a.off_hh);
    s.tgt = reinterpret_cast<float*>(smem + a.off_tgt);
    s.p = reinterpret_cast<int*>(smem + a.off_p);
    s.range = reinterpret_cast<unsigned*>(smem + a.off_range);
    s.z0 = reinterpret_cast<float*>(smem + a.off_z0);
    s.z1 = reinterpret_cast<float*>(smem + a.off_z1);
    s.start = reinterpret_cast<int*>(smem + a.off_start);
    s.flag = reinterpret_cast<int*>(smem + a.off_flag);
    return s;
}

template <int MODE>
__global__ __launch_bounds__(PC_THREADS) void powerctl_kernel(const PowerArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    unsigned* key = reinterpret_cast<unsigned*>(s.z1);
    const int n4 = (N + 3) & ~3;
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one
    same_rb_keys<PC_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += PC_THREADS) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float tx_x = px[txd], tx_y = py[txd], rx_x = px[rxd], rx_y = py[rxd];
        const float c0 = a.cols[txd];
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g_own = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        const unsigned mine = key[j];
        const bool on_rb = (int)(mine >> KEY_SHIFT) < R;
        const bool adj = on_rb && (!a.adjustable || a.adjustable[j] != 0);
        const int held = pwr_row[j];
        const int lo = adj ? a.p_min[j] : held, hi = adj ? a.p_max[j] : held;
        const float tgt = a.target[j];
        const int slot = same_rb_rank(key, n4, mine);
        s.tx[slot] = make_float4(tx_x, tx_y, c0, __int_as_float(j));
        s.rxa[slot] = make_float4(rx_x, rx_y, rx_pl, noise);
        s.rxb[slot] = make_float2(g_own, rx_lin);
        s.lohi[slot] = make_int2(lo, hi);
        if (POWLAW) s.hh[slot] = h;
        s.tgt[slot] = tgt;
        s.p[slot] = lo;                                                  // p0: p_min where adjustable, the held power elsewhere
        s.z0[slot] = pow10_tenth(lo) * c0;                             // the step's tuple.z (d2d_step.hip, pass 1)
        s.range[slot] = mine >> KEY_SHIFT;                               // the sorted rb, until start[] exists
    }
    __syncthreads();
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB
    same_rb_starts<PC_THREADS>(s.start, s.range, N, R);
    __syncthreads();
    // ---- every slot's own RB group as (first | last + 1 << 16); from here on a slot is touched by its owner lane only, z aside
    for (int k = tid; k < N; k += PC_THREADS) {
        const int r = (int)s.range[k];
        s.range[k] = r < R ? (unsigned)s.start[r] | ((unsigned)s.start[r + 1] << 16) : NO_RB;
    }
    // (the keys in z[1] were last read before the second barrier above; sweep 0 is the first to write z[1])

    // ---- the sweeps
    int cur = 0, sweeps = 0, fixed = 0;
    for (int t = 0; t < a.max_iters; ++t) {
        const float* z = cur ? s.z1 : s.z0;
        float* zn = cur ? s.z0 : s.z1;
        bool changed = false;
        for (int k = tid; k < N; k += PC_THREADS) {
            const unsigned range = s.range[k];
            const int p = s.p[k];
            int pn = p;
            if (range != NO_RB) {
                const float v = slot_sinr_db<MODE>(s, z, k, range, a.pow_k);
                const float need = ceilf((float)p + (s.tgt[k] - v));
                const int2 lh = s.lohi[k];
                // min(p_max, max(p_min, (int)need)) with the clamp taken on the float: need is a whole number, the bounds are exact
                const int want = (int)fminf(fmaxf(need, (float)lh.x), (float)lh.y);
                pn = need == need ? max(p, want) : p;                    // never lowered; NaN need: unchanged
            }
            if (pn != p) {
                changed = true;
                s.p[k] = pn;
                zn[k] = pow10_tenth(pn) * s.tx[k].z;
            } else {
                zn[k] = z[k];
            }
        }
        const bool wave_changed = __ballot(changed) != 0ull;
        int* flag = s.flag + (t & 1) * PC_WAVES;
        if (lane == 0) flag[wave] = wave_changed ? 1 : 0;
        __syncthreads();                                                 // the sweep's one barrier: z[cur ^ 1] and the flags
        const int any = flag[0] | flag[1] | flag[2] | flag[3];
        if (!any) { fixed = 1; break; }                                  // workgroup-uniform; z[cur ^ 1] == z[cur]
        cur ^= 1;
        ++sweeps;
    }

    // ---- the SINR at the powers the iteration stopped at, and the results
    const int* p_out = s.p;
    const float* z = cur ? s.z1 : s.z0;
    const size_t row = b * (size_t)N;
    for (int k = tid; k < N; k += PC_THREADS) {
        const unsigned range = s.range[k];
        const int i = __float_as_int(s.tx[k].w);
        const float v = range != NO_RB ? slot_sinr_db<MODE>(s, z, k, range, a.pow_k) : __builtin_nanf("");
        a.power[row + (size_t)i] = p_out[k];
        a.sinr[row + (size_t)i] = v;
    }
    if (tid == 0) {
        a.iters[b] = sweeps;
        a.converged[b] = (unsigned char)fixed;
    }
}

}  // namespace

extern "C" int d2d_power_control(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                 const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                                 int32_t n_links, int32_t n_rbs, const float* target_db, const int32_t* p_min, const int32_t* p_max,
                                 const uint8_t* adjustable, int32_t max_iters, const uint8_t* env_mask, int32_t* power_dbm,
                                 float* sinr_db, int32_t* iters, uint8_t* converged, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_POWERCTL_MAX_LINKS, n_rbs, D2D_POWERCTL_MAX_RBS, n_dev)) return fail(why);
    if (max_iters < 1) return fail("max_iters must be >= 1");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !target_db || !p_min || !p_max || !power_dbm ||
        !sinr_db || !iters || !converged)
        return fail("null device pointer");
    const void* outs[4] = {power_dbm, sinr_db, iters, converged};
    for (int x = 0; x < 4; ++x)
        for (int y = x + 1; y < 4; ++y)
            if (outs[x] == outs[y]) return fail("power_dbm, sinr_db, iters and converged must be four arrays");
    PowerArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.target = target_db; a.p_min = p_min; a.p_max = p_max; a.adjustable = adjustable; a.env_mask = env_mask;
    a.power = power_dbm; a.sinr = sinr_db; a.iters = iters; a.converged = converged;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k; a.max_iters = max_iters;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_rxa = N * 16u;
    a.off_rxb = a.off_rxa + N * 16u;
    a.off_lohi = a.off_rxb + round16(N * 8u);
    a.off_hh = a.off_lohi + round16(N * 8u);
    a.off_tgt = a.off_hh + (law == D2D_POWERCTL_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_p = a.off_tgt + n4 * 4u;
    a.off_range = a.off_p + n4 * 4u;
    a.off_z0 = a.off_range + n4 * 4u;
    a.off_z1 = a.off_z0 + n4 * 4u;
    a.off_start = a.off_z1 + n4 * 4u;
    a.off_flag = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned lds = a.off_flag + 2u * PC_WAVES * 4u;
    if (lds > 160u * 1024u) return fail("n_links and n_rbs need more than the 160 KiB of LDS a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_POWERCTL_LAW_INV_SQUARE) e = launch(&powerctl_kernel<PL_INV_SQUARE>, grid, dim3(PC_THREADS), lds, st, a);
    else if (law == D2D_POWERCTL_LAW_POWER) e = launch(&powerctl_kernel<PL_POWER>, grid, dim3(PC_THREADS), lds, st, a);
    else e = launch(&powerctl_kernel<PL_POWK>, grid, dim3(PC_THREADS), lds, st, a);
    if (e != hipSuccess) return fail(std::string("powerctl_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_powerctl_last_error)
