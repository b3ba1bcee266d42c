// libd2d_balance.so (include/d2d_balance.h): max-min SINR balancing - the bisection over a grid of target levels, every probe the
// whole power iteration of d2d_powerctl.hip, every probe of every env in one launch.  gfx950.
//
// Shape: d2d_powerctl.hip's - ONE workgroup of 256 threads per env that stages the env once (the sort of d2d_same_rb.h, every link's
// constants into its sorted slot, every slot's own RB group as a range word) and then works in LDS with lanes owning slots.  What
// is new is the outer loop: a probe re-initialises p and z[0] from p_min, runs the sweeps (slot_sinr_db of d2d_powerctl_device.h,
// that kernel's update restated, the target formed as base + margin, one float32 addition), evaluates the pass rule on the plane
// it stopped at and, where it passed, copies p into p_best.  The target array of d2d_powerctl.hip is not kept: its place is the
// base's, which with the floor and p_best makes 8 bytes per link more than that kernel has - 2048 links on 256 RBs still fit.
//
// Uniformity: every decision that steers a loop is read by all threads from LDS behind a barrier - the sweep's "anything changed"
// words as in d2d_powerctl.hip, the probe's "any link failed" words likewise, and (lo, hi), which thread 0 writes behind the pass
// words' barrier and everyone reads behind the next probe's first one.  So the probe loop, the sweep loop and every
// __syncthreads() are workgroup-uniform.  Both loops are bounded: by max_iters and by MAX_PROBES.  No global access inside the
// loops beyond margins[mid], no atomics, no scratch; global memory is written once behind the search.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_balance.h"
#include "d2d_powerctl_device.h"
#include "d2d_same_rb.h"

namespace {

using namespace d2d;

constexpr int BAL_THREADS = 256;
constexpr int BAL_WAVES = BAL_THREADS / 64;
constexpr int MAX_PROBES = 13;                                   // probe 0, then at most ceil(log2 4096) = 12 halvings
constexpr unsigned ADJ_BIT = 0x80000000u;                        // in the link-index word of a slot's tx tuple: the link is adjustable
static_assert(D2D_BALANCE_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_BALANCE_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_BALANCE_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_BALANCE_LAW_POWER == LAW_POWER && D2D_BALANCE_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_BALANCE_MAX_LINKS < (1 << 15), "a range word packs two slot indices into 16 bits each under the NO_RB bit");
static_assert((1 << (MAX_PROBES - 1)) >= D2D_BALANCE_MAX_MARGINS, "the halvings reach hi - lo == 1 within MAX_PROBES - 1 probes");
static_assert(D2D_BALANCE_MAX_LDS_BYTES == 160 * 1024, "what a workgroup can have");

struct BalanceArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* base;              // [N]
    const float* floor;             // [N] or null
    const float* margins;           // [K]
    const int* p_min;               // [N]
    const int* p_max;               // [N]
    const unsigned char* adjustable;  // [N] or null
    const unsigned char* env_mask;  // [B] or null
    int* power;
    float* sinr;
    float* margin;
    int* level;
    int* probes;
    int D, N, R, K;
    int pow_k;
    int max_iters;
    // byte offsets of the LDS arrays behind the transmitter tuples
    unsigned off_rxa, off_rxb, off_lohi, off_hh, off_base, off_floor, off_p, off_best, off_range, off_z0, off_z1, off_start, off_flag;
};

// dynamic LDS, by sorted slot: tx float4[N] | rxa float4[N] | rxb float2[N] | lohi int2[N] | hh float2[N] (power laws) | base f32[n4]
// | floor f32[n4] | p i32[n4] | p_best i32[n4] | range u32[n4] (the sorted rb until start[] exists) | z0 f32[n4] | z1 f32[n4] (the
// sort's keys until the first sweep) | start i32[R + 1] | flag i32[2][4] | bad i32[4] | ctl i32[4] (lo, hi)

struct Lds {
    float4* tx; float4* rxa; float2* rxb; int2* lohi; float2* hh; float* base; float* floor; int* p; int* best; unsigned* range;
    float* z0; float* z1; int* start; int* flag; int* bad; int* ctl;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const BalanceArgs& a) {
    Lds s;
    s.tx = reinterpret_cast<float4*>(smem);
    s.rxa = reinterpret_cast<float4*>(smem + a.off_rxa);
    s.rxb = reinterpret_cast<float2*>(smem + a.off_rxb);
    s.lohi = reinterpret_cast<int2*>(smem + a.off_lohi);
    s.hh = reinterpret_cast<float2*>(smem + a.off_hh);
    s.base = reinterpret_cast<float*>(smem + a.off_base);
    s.floor = reinterpret_cast<float*>(smem + a.off_floor);
    s.p = reinterpret_cast<int*>(smem + a.off_p);
    s.best = reinterpret_cast<int*>(smem + a.off_best);
    s.range = reinterpret_cast<unsigned*>(smem + a.off_range);
    s.z0 = reinterpret_cast<float*>(smem + a.off_z0);
    s.z1 = reinterpret_cast<float*>(smem + a.off_z1);
    s.start = reinterpret_cast<int*>(smem + a.off_start);
    s.flag = reinterpret_cast<int*>(smem + a.off_flag);
    s.bad = s.flag + 2 * BAL_WAVES;
    s.ctl = s.bad + BAL_WAVES;
    return s;
}

// p^t+1 of a link at power p whose SINR is v and whose target is tgt, inside its bounds lh = (p_min, p_max): d2d_powerctl.hip's
// expression (include/d2d_powerctl.h), restated
__device__ __forceinline__ int raised_power(int p, float tgt, float v, int2 lh) {
    const float need = ceilf((float)p + (tgt - v));
    // min(p_max, max(p_min, (int)need)) with the clamp taken on the float: need is a whole number, the bounds are exact
    const int want = (int)fminf(fmaxf(need, (float)lh.x), (float)lh.y);
    return need == need ? max(p, want) : p;                              // never lowered; NaN need: unchanged
}

template <int MODE>
__global__ __launch_bounds__(BAL_THREADS) void balance_kernel(const BalanceArgs a) {
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

    // ---- staging, as d2d_powerctl.hip: keys, rank sort, every link's constants into its slot
    same_rb_keys<BAL_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    for (int j = tid; j < N; j += BAL_THREADS) {
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
        const int slot = same_rb_rank(key, n4, mine);
        s.tx[slot] = make_float4(tx_x, tx_y, c0, __int_as_float((int)((unsigned)j | (adj ? ADJ_BIT : 0u))));   // bits only, never arithmetic
        s.rxa[slot] = make_float4(rx_x, rx_y, rx_pl, noise);
        s.rxb[slot] = make_float2(g_own, rx_lin);
        s.lohi[slot] = make_int2(lo, hi);
        if (POWLAW) s.hh[slot] = h;
        s.base[slot] = a.base[j];
        s.floor[slot] = a.floor ? a.floor[j] : -__builtin_inff();
        s.range[slot] = mine >> KEY_SHIFT;                               // the sorted rb, until start[] exists
    }
    if (tid == 0) { s.ctl[0] = 0; s.ctl[1] = a.K; }
    __syncthreads();
    same_rb_starts<BAL_THREADS>(s.start, s.range, N, R);
    __syncthreads();
    // ---- every slot's own RB group as (first | last + 1 << 16); from here on a slot is touched by its owner lane only, z aside
    for (int k = tid; k < N; k += BAL_THREADS) {
        const int r = (int)s.range[k];
        s.range[k] = r < R ? (unsigned)s.start[r] | ((unsigned)s.start[r + 1] << 16) : PC_NO_RB;
    }
    // (the keys in z[1] were last read before the second barrier above; a probe's sweep 0 is the first to write z[1])

    // ---- the search: probe 0, then the halvings.  One pass of the loop more than there are probes: it ends the search.
    int lo = 0, probes = 0;
    for (int it = 0; it <= MAX_PROBES; ++it) {
        // cold start: p0 = p_min where adjustable, the held power elsewhere; z[0] the step's tuple.z (d2d_step.hip, pass 1).  The
        // last reads of z by the probe before lie before the barrier that carried its pass words.
        for (int k = tid; k < N; k += BAL_THREADS) {
            const int p0 = s.lohi[k].x;
            s.p[k] = p0;
            s.z0[k] = pow10_tenth(p0) * s.tx[k].z;
        }
        __syncthreads();                                                 // z[0], and (lo, hi) as thread 0 left them
        lo = s.ctl[0];
        const int hi = s.ctl[1];
        if (it > 0 && hi - lo <= 1) break;                               // workgroup-uniform: (lo, hi) come from LDS
        const int mid = it == 0 ? 0 : (lo + hi) >> 1;                    // 0 <= mid < K
        const float margin = a.margins[mid];
        ++probes;

        // ---- the sweeps of d2d_powerctl.hip for the target base + margin
        int cur = 0, fixed = 0;
        for (int t = 0; t < a.max_iters; ++t) {
            const float* z = cur ? s.z1 : s.z0;
            float* zn = cur ? s.z0 : s.z1;
            bool changed = false;
            for (int k = tid; k < N; k += BAL_THREADS) {
                const unsigned range = s.range[k];
                const int p = s.p[k];
                int pn = p;
                if (range != PC_NO_RB) {
                    const float v = slot_sinr_db<MODE>(s, z, k, range, a.pow_k);
                    pn = raised_power(p, s.base[k] + margin, v, s.lohi[k]);
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
            int* flag = s.flag + (t & 1) * BAL_WAVES;
            if (lane == 0) flag[wave] = wave_changed ? 1 : 0;
            __syncthreads();                                             // the sweep's one barrier: z[cur ^ 1] and the flags
            const int any = flag[0] | flag[1] | flag[2] | flag[3];
            if (!any) { fixed = 1; break; }                              // workgroup-uniform; z[cur ^ 1] == z[cur]
            cur ^= 1;
        }

        // ---- the pass rule on the plane the probe stopped at
        const float* z = cur ? s.z1 : s.z0;
        bool bad = false;
        for (int k = tid; k < N; k += BAL_THREADS) {
            const unsigned range = s.range[k];
            if (range == PC_NO_RB) continue;
            const float v = slot_sinr_db<MODE>(s, z, k, range, a.pow_k);
            const bool adj = ((unsigned)__float_as_int(s.tx[k].w) & ADJ_BIT) != 0u;
            const bool short_at_max = adj && s.p[k] == s.lohi[k].y && v < s.base[k] + margin;
            bad = bad || short_at_max || v < s.floor[k];                 // a NaN comparison is false
        }
        const bool wave_bad = __ballot(bad) != 0ull;
        if (lane == 0) s.bad[wave] = wave_bad ? 1 : 0;
        __syncthreads();                                                 // the pass words; every read of z and p of this probe
        const bool pass = fixed && !(s.bad[0] | s.bad[1] | s.bad[2] | s.bad[3]);
        if (pass || it == 0)                                             // an infeasible env reports probe 0
            for (int k = tid; k < N; k += BAL_THREADS) s.best[k] = s.p[k];
        if (tid == 0) {                                                  // read by everyone behind the next barrier
            if (it == 0) { s.ctl[0] = pass ? 0 : -1; s.ctl[1] = pass ? a.K : 0; }
            else if (pass) s.ctl[0] = mid;
            else s.ctl[1] = mid;
        }
    }

    // ---- the SINR at the kept powers, and the results.  The pass that broke out of the loop left z[0] behind its barrier and
    // nobody has read it since: every owner lane rewrites its slots.
    for (int k = tid; k < N; k += BAL_THREADS) s.z0[k] = pow10_tenth(s.best[k]) * s.tx[k].z;
    __syncthreads();
    const size_t row = b * (size_t)N;
    for (int k = tid; k < N; k += BAL_THREADS) {
        const unsigned range = s.range[k];
        const int i = (int)((unsigned)__float_as_int(s.tx[k].w) & ~ADJ_BIT);
        const float v = range != PC_NO_RB ? slot_sinr_db<MODE>(s, s.z0, k, range, a.pow_k) : __builtin_nanf("");
        a.power[row + (size_t)i] = s.best[k];
        a.sinr[row + (size_t)i] = v;
    }
    if (tid == 0) {
        a.margin[b] = lo >= 0 ? a.margins[lo] : -__builtin_inff();
        a.level[b] = lo;
        a.probes[b] = probes;
    }
}

}  // namespace

extern "C" int d2d_balance_sinr(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                                int32_t n_links, int32_t n_rbs, const float* base_db, const float* floor_db, const float* margins_db,
                                int32_t n_margins, const int32_t* p_min, const int32_t* p_max, const uint8_t* adjustable,
                                int32_t max_iters, const uint8_t* env_mask, int32_t* power_dbm, float* sinr_db, float* margin_db,
                                int32_t* level, int32_t* probes, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_BALANCE_MAX_LINKS, n_rbs, D2D_BALANCE_MAX_RBS, n_dev)) return fail(why);
    if (n_margins < 1 || n_margins > D2D_BALANCE_MAX_MARGINS)
        return fail("n_margins must be in [1, " + std::to_string(D2D_BALANCE_MAX_MARGINS) + "]");
    if (max_iters < 1) return fail("max_iters must be >= 1");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !base_db || !margins_db || !p_min || !p_max ||
        !power_dbm || !sinr_db || !margin_db || !level || !probes)
        return fail("null device pointer");
    const void* outs[5] = {power_dbm, sinr_db, margin_db, level, probes};
    for (int x = 0; x < 5; ++x)
        for (int y = x + 1; y < 5; ++y)
            if (outs[x] == outs[y]) return fail("power_dbm, sinr_db, margin_db, level and probes must be five arrays");
    BalanceArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.base = base_db; a.floor = floor_db; a.margins = margins_db; a.p_min = p_min; a.p_max = p_max; a.adjustable = adjustable;
    a.env_mask = env_mask; a.power = power_dbm; a.sinr = sinr_db; a.margin = margin_db; a.level = level; a.probes = probes;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.K = n_margins; a.pow_k = pow_k; a.max_iters = max_iters;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_rxa = N * 16u;
    a.off_rxb = a.off_rxa + N * 16u;
    a.off_lohi = a.off_rxb + round16(N * 8u);
    a.off_hh = a.off_lohi + round16(N * 8u);
    a.off_base = a.off_hh + (law == D2D_BALANCE_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_floor = a.off_base + n4 * 4u;
    a.off_p = a.off_floor + n4 * 4u;
    a.off_best = a.off_p + n4 * 4u;
    a.off_range = a.off_best + n4 * 4u;
    a.off_z0 = a.off_range + n4 * 4u;
    a.off_z1 = a.off_z0 + n4 * 4u;
    a.off_start = a.off_z1 + n4 * 4u;
    a.off_flag = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned lds = a.off_flag + 4u * BAL_WAVES * 4u;               // flag[2][4], bad[4], ctl[4]
    if (lds > (unsigned)D2D_BALANCE_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                    std::to_string(D2D_BALANCE_MAX_LDS_BYTES) + " (D2D_BALANCE_MAX_LDS_BYTES) a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_BALANCE_LAW_INV_SQUARE) e = launch(&balance_kernel<PL_INV_SQUARE>, grid, dim3(BAL_THREADS), lds, st, a);
    else if (law == D2D_BALANCE_LAW_POWER) e = launch(&balance_kernel<PL_POWER>, grid, dim3(BAL_THREADS), lds, st, a);
    else e = launch(&balance_kernel<PL_POWK>, grid, dim3(BAL_THREADS), lds, st, a);
    if (e != hipSuccess) return fail(std::string("balance_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_balance_last_error)
