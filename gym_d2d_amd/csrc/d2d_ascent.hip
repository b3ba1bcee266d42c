// libd2d_ascent.so (include/d2d_ascent.h): coordinate ascent on the total capacity of every RB group over the integer dBm alphabet,
// with SINR floors, every turn of every round of every env in one launch.  gfx950.
//
// Shape: ONE workgroup of 256 threads per env that stages the env once - d2d_powerctl.hip's staging: the rank sort of d2d_same_rb.h
// puts every link's constants into its sorted slot (transmitter tuple, receiver tuple, own-pair gain / rx gain / bandwidth /
// sensitivity, the power-law pair, floor, bounds, current power and its linear value) with start[r] = the first slot of RB r - and
// then ascends in LDS.  A WAVE OWNS AN RB GROUP: wave w takes the RBs w, w + 4, ... that have an adjustable member, one after the
// other, and runs the group's rounds to their end; groups do not interact, so no wave reads a slot another wave writes.  THE 64
// LANES OWN THE POWER LEVELS of the link whose turn it is: lane q walks the group's members and, per member, the group's
// transmitters as evaluate_kernel does (d2d_evaluate.hip: float products into a double accumulator in ascending link index, the
// receiver's own slot adding 0.0, precise_div, v_log_f32 and the capacity by the step's operations) with the turn's link at level
// q's linear power - the members and transmitters are the same for every lane, so every LDS read is a broadcast.  The lane sums the
// capacities in double and keeps its admissibility bit; the choice is ONE 64-bit wave reduction of the order-preserving image of
// the double (d2d_wave_key.h), a ballot on equality and the lowest set lane.  No global access, no workgroup barrier and no
// atomics inside the ascent; one barrier behind it, then every slot's owner thread writes the three planes of the final vector and
// thread 0 combines the waves' (rounds, moves, converged) words in wave order.
//
// The pair gains are recomputed at every level of every turn: cached they would be (group size)^2 floats per wave with no bound
// short of N^2.  A group of G links costs G^2 pair evaluations per turn on one wave; one long group is not spread over the waves.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "d2d_addon.h"
#include "d2d_ascent.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"
#include "d2d_wave_key.h"

namespace {

using namespace d2d;

constexpr int AS_THREADS = 256;
constexpr int AS_WAVES = AS_THREADS / 64;
constexpr int AS_LEVELS = D2D_ASCENT_MAX_LEVELS;
constexpr int NO_TURN = 1;                                       // bounds word of a link that takes no turn: lo = 1 > hi = 0
static_assert(D2D_ASCENT_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_ASCENT_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_ASCENT_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_ASCENT_LAW_POWER == LAW_POWER && D2D_ASCENT_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_ASCENT_MAX_LINKS < (1 << 15), "a range word packs two slot indices into 16 bits each");
static_assert(AS_LEVELS == 64, "one lane per level");

struct AscentArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* cap_cols;          // [2][D]
    const int* p_min;               // [N]
    const int* p_max;               // [N]
    const unsigned char* adjustable;  // [N] or null
    const float* floor;             // [N] or null
    const unsigned char* env_mask;  // [B] or null
    int* power;
    float* sinr;
    float* cap;
    int* rounds;
    int* moves;
    unsigned char* converged;
    double min_gain;
    int D, N, R;
    int pow_k;
    int start;
    int max_rounds;
    // byte offsets of the LDS arrays behind the transmitter tuples
    unsigned off_rxa, off_rxb, off_hh, off_floor, off_p, off_z, off_range, off_lohi, off_start, off_flag;
};

// dynamic LDS, by sorted slot: tx float4[N] (tx x, tx y, tx constant, link index) | rxa float4[N] (rx x, rx y, rx_pl, noise) | rxb
// float4[N] (own-pair gain, rx_lin, bw_mhz, sens_db) | hh float2[N] (power laws) | floor f32[n4] | p i32[n4] | z f32[n4] (the linear
// powers; the sort's keys until start[] exists) | range u32[n4] (first | last + 1 << 16 of the link's group; the sorted rb until
// start[] exists) | lohi i32[n4] (p_min in the low half, p_max in the high one; NO_TURN: the link takes no turn) | start i32[R + 1] |
// flag i32[4][4]

struct Lds {
    float4* tx; float4* rxa; float4* rxb; float2* hh; float* floor; int* p; float* z; unsigned* range; int* lohi; int* start; int* flag;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const AscentArgs& a) {
    Lds s;
    s.tx = reinterpret_cast<float4*>(smem);
    s.rxa = reinterpret_cast<float4*>(smem + a.off_rxa);
    s.rxb = reinterpret_cast<float4*>(smem + a.off_rxb);
    s.hh = reinterpret_cast<float2*>(smem + a.off_hh);
    s.floor = reinterpret_cast<float*>(smem + a.off_floor);
    s.p = reinterpret_cast<int*>(smem + a.off_p);
    s.z = reinterpret_cast<float*>(smem + a.off_z);
    s.range = reinterpret_cast<unsigned*>(smem + a.off_range);
    s.lohi = reinterpret_cast<int*>(smem + a.off_lohi);
    s.start = reinterpret_cast<int*>(smem + a.off_start);
    s.flag = reinterpret_cast<int*>(smem + a.off_flag);
    return s;
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// sinr_db and capacity_mbps of the link in slot m, whose group is the slots [first, last), under the linear powers z with slot
// `turn` at zq instead (turn = -1: z as it is): evaluate_kernel's walk and the step's operations in the step's order
// (d2d_evaluate.hip; d2d_step.hip, pass 2).  An empty range (a link on no RB) gives the link's SNR, as evaluate_kernel does.
template <int MODE>
__device__ __forceinline__ void member_planes(const Lds& s, int m, int first, int last, int turn, float zq, int pow_k, float& sinr_db,
                                              float& cap) {
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const float4 rx = s.rxa[m];                                          // rx x, rx y, rx_pl, noise
    const float4 own = s.rxb[m];                                         // own-pair gain, rx_lin, bw_mhz, sens_db
    double acc = 0.0;
    for (int o = first; o < last; ++o) {
        const float4 t = s.tx[o];
        const float dx = t.x - rx.x, dy = t.y - rx.y;
        const float d2 = fmaf(dx, dx, dy * dy);
        const float g = pair_gain<MODE>(d2, POWLAW ? s.hh[o] : make_float2(-1.0f, 0.0f), pow_k);
        const float zo = o == turn ? zq : s.z[o];
        const float term = zo * g;                                       // simulator.py:97-101, linear mW
        acc += o != m ? (double)term : 0.0;
    }
    const float zm = m == turn ? zq : s.z[m];
    const float sig = zm * own.x * rx.z * own.y;
    const float accf = (float)acc;
    const float sinr_lin = precise_div(sig, fmaf(accf, rx.z, rx.w));
    sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
    const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
    const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
    const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
    const bool ok = sinr_db > own.w;                                     // simulator.py:123,149
    cap = ok ? own.z * sh : 0.0f;                                        // simulator.py:150-151
}

// The order-preserving image of a double in the unsigned 64-bit words: a < b as doubles iff image(a) < image(b), above the two
// words the choice keeps for itself - 0, wave_reduce<true>'s identity (an inadmissible lane), and 1 (a NaN): -inf maps to 2^52 - 1.
__device__ __forceinline__ unsigned long long ordered_image(double t) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(t);
    return t != t ? 1ull : ((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}

template <int MODE>
__global__ __launch_bounds__(AS_THREADS) void ascent_kernel(const AscentArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    unsigned* key = reinterpret_cast<unsigned*>(s.z);
    const int n4 = (N + 3) & ~3;
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one
    same_rb_keys<AS_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += AS_THREADS) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float tx_x = px[txd], tx_y = py[txd], rx_x = px[rxd], rx_y = py[rxd];
        const float c0 = a.cols[txd];
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
        const float bw_mhz = a.cap_cols[txd], sens = a.cap_cols[D + rxd];
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g_own = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        const int slot = same_rb_rank(key, n4, key[j]);
        s.tx[slot] = make_float4(tx_x, tx_y, c0, __int_as_float(j));
        s.rxa[slot] = make_float4(rx_x, rx_y, rx_pl, noise);
        s.rxb[slot] = make_float4(g_own, rx_lin, bw_mhz, sens);
        if (POWLAW) s.hh[slot] = h;
    }
    // (a second loop, and the rank taken twice: one loop over both halves keeps every argument of the launch in scalar registers at
    // once, more than the pow-k instantiation has)
    for (int j = tid; j < N; j += AS_THREADS) {
        const unsigned mine = key[j];
        const bool on_rb = (int)(mine >> KEY_SHIFT) < R;
        const int held = pwr_row[j];
        const int lo = a.p_min[j], hi = a.p_max[j];
        // the links that take turns: on an RB, marked, an alphabet of 1 .. 64 levels that 16 bits hold, and a start inside it
        bool adj = on_rb && (!a.adjustable || a.adjustable[j] != 0) && lo <= hi && (long long)hi - lo < AS_LEVELS && lo > -4096 && hi < 4096;
        if (a.start == D2D_ASCENT_START_HELD) adj = adj && held >= lo && held <= hi;
        const int p0 = !adj ? held : (a.start == D2D_ASCENT_START_MIN ? lo : (a.start == D2D_ASCENT_START_MAX ? hi : held));
        const int slot = same_rb_rank(key, n4, mine);
        s.floor[slot] = a.floor ? a.floor[j] : -INFINITY;
        s.p[slot] = p0;
        s.lohi[slot] = adj ? (int)(((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16)) : NO_TURN;
        s.range[slot] = mine >> KEY_SHIFT;                               // the sorted rb, until start[] exists
    }
    __syncthreads();
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB
    same_rb_starts<AS_THREADS>(s.start, s.range, N, R);
    __syncthreads();
    // ---- every slot's own RB group as (first | last + 1 << 16), empty for a link on no RB, and its linear power: the step's tuple.z
    // (d2d_step.hip, pass 1).  The keys in z were last read before the second barrier above.
    for (int k = tid; k < N; k += AS_THREADS) {
        const int r = (int)s.range[k];
        s.range[k] = r < R ? (unsigned)s.start[r] | ((unsigned)s.start[r + 1] << 16) : (unsigned)k | ((unsigned)k << 16);
        s.z[k] = pow10_tenth(s.p[k]) * s.tx[k].z;
    }
    __syncthreads();                                                     // the staging is over: waves read each other's slots

    // ---- the ascent: wave w takes the RBs w, w + 4, ...; every value that steers it is wave-uniform
    int w_rounds = 0, w_moves = 0, w_quiet = 1;
    for (int r = wave; r < R; r += AS_WAVES) {
        const int first = uniform(s.start[r]), last = uniform(s.start[r + 1]);
        unsigned long long takes = 0ull;
        for (int k0 = first; k0 < last; k0 += 64) {
            const int k = k0 + lane;
            takes |= __ballot(k < last && s.lohi[k] != NO_TURN);
        }
        if (takes == 0ull) continue;                                     // nobody here takes a turn
        int g_rounds = 0, quiet = 0;
        for (int t = 0; t < a.max_rounds; ++t) {
            int moved = 0;
            for (int k = first; k < last; ++k) {
                const int bounds = uniform(s.lohi[k]);
                if (bounds == NO_TURN) continue;
                const int lo = (int)(short)(bounds & 0xFFFF), hi = bounds >> 16;
                const int levels = hi - lo + 1;                          // 1 .. 64 by the staging
                const int cur = uniform(s.p[k]) - lo;                    // the lane of the current level, in [0, levels)
                // a lane past the alphabet evaluates the top level again and is never admissible: all 64 lanes stay active
                const int level = lo + min(lane, levels - 1);
                const float zq = pow10_tenth(level) * s.tx[k].z;
                double total = 0.0;
                bool adm = true;
                for (int m = first; m < last; ++m) {
                    float sinr, cap;
                    member_planes<MODE>(s, m, first, last, k, zq, a.pow_k, sinr, cap);
                    total += (double)cap;
                    const float fl = s.floor[m];
                    const float at_cur = __shfl(sinr, cur, 64);
                    adm = adm && (!(fl > -INFINITY) || sinr >= fl || at_cur < fl);      // float32, NaN compares false
                }
                adm = (adm || lane == cur) && lane < levels;
                const unsigned long long mine = adm ? ordered_image(total) : 0ull;
                const unsigned long long top = wave_reduce<true>(mine);
                if (top <= 1ull) continue;                               // every admissible total is NaN
                const int win = __ffsll((unsigned long long)__ballot(mine == top)) - 1;     // the lowest level at the maximum
                if (win == cur) continue;
                const double gain = __shfl(total, win, 64) - __shfl(total, cur, 64);
                if (!(gain > a.min_gain)) continue;
                if (lane == win) {
                    s.p[k] = level;
                    s.z[k] = zq;
                }
                // The wave's own later reads of p[k] and z[k] must see this write; no other wave reads the slot before the
                // barrier behind the ascent.  A wave's LDS instructions are executed in the order it issues them, and the
                // wavefront-scope fence keeps the compiler from moving a read of the slot above the winning lane's write.
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                moved = 1;
                ++w_moves;
            }
            if (!moved) { quiet = 1; break; }
            ++g_rounds;
        }
        w_rounds = max(w_rounds, g_rounds);
        w_quiet &= quiet;
    }
    if (lane == 0) {
        s.flag[4 * wave] = w_rounds;
        s.flag[4 * wave + 1] = w_moves;
        s.flag[4 * wave + 2] = w_quiet;
    }
    __syncthreads();                                                     // the one barrier behind the ascent: p, z and the flags

    // ---- the planes of the final vector, every slot by its owner thread, and the env's three words in wave order
    const size_t row = b * (size_t)N;
    for (int k = tid; k < N; k += AS_THREADS) {
        const unsigned range = s.range[k];
        const int i = __float_as_int(s.tx[k].w);
        float sinr, cap;
        member_planes<MODE>(s, k, (int)(range & 0xFFFFu), (int)(range >> 16), -1, 0.0f, a.pow_k, sinr, cap);
        a.power[row + (size_t)i] = s.p[k];
        a.sinr[row + (size_t)i] = sinr;
        a.cap[row + (size_t)i] = cap;
    }
    if (tid == 0) {
        int rounds = 0, moves = 0, quiet = 1;
#pragma unroll
        for (int w = 0; w < AS_WAVES; ++w) {
            rounds = max(rounds, s.flag[4 * w]);
            moves += s.flag[4 * w + 1];
            quiet &= s.flag[4 * w + 2];
        }
        a.rounds[b] = rounds;
        a.moves[b] = moves;
        a.converged[b] = (unsigned char)quiet;
    }
}

}  // namespace

extern "C" int d2d_power_ascent(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                                int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max,
                                const uint8_t* adjustable, const float* floor_db, int32_t start, double min_gain_mbps, int32_t max_rounds,
                                const uint8_t* env_mask, int32_t* power_dbm, float* sinr_db, float* capacity_mbps, int32_t* rounds,
                                int32_t* moves, uint8_t* converged, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_ASCENT_MAX_LINKS, n_rbs, D2D_ASCENT_MAX_RBS, n_dev)) return fail(why);
    if (max_rounds < 1 || max_rounds > D2D_ASCENT_MAX_ROUNDS) return fail("max_rounds must be in [1, " + std::to_string(D2D_ASCENT_MAX_ROUNDS) + "]");
    if (start != D2D_ASCENT_START_HELD && start != D2D_ASCENT_START_MIN && start != D2D_ASCENT_START_MAX) return fail("unknown start");
    if (!std::isfinite(min_gain_mbps) || min_gain_mbps < 0.0) return fail("min_gain_mbps must be finite and >= 0");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !p_min || !p_max || !power_dbm ||
        !sinr_db || !capacity_mbps || !rounds || !moves || !converged)
        return fail("null device pointer");
    const void* outs[6] = {power_dbm, sinr_db, capacity_mbps, rounds, moves, converged};
    for (int x = 0; x < 6; ++x)
        for (int y = x + 1; y < 6; ++y)
            if (outs[x] == outs[y]) return fail("power_dbm, sinr_db, capacity_mbps, rounds, moves and converged must be six arrays");
    AscentArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.p_min = p_min; a.p_max = p_max; a.adjustable = adjustable; a.floor = floor_db; a.env_mask = env_mask;
    a.power = power_dbm; a.sinr = sinr_db; a.cap = capacity_mbps; a.rounds = rounds; a.moves = moves; a.converged = converged;
    a.min_gain = min_gain_mbps;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k; a.start = start; a.max_rounds = max_rounds;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_rxa = N * 16u;
    a.off_rxb = a.off_rxa + N * 16u;
    a.off_hh = a.off_rxb + N * 16u;
    a.off_floor = a.off_hh + (law == D2D_ASCENT_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_p = a.off_floor + n4 * 4u;
    a.off_z = a.off_p + n4 * 4u;
    a.off_range = a.off_z + n4 * 4u;
    a.off_lohi = a.off_range + n4 * 4u;
    a.off_start = a.off_lohi + n4 * 4u;
    a.off_flag = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned lds = a.off_flag + 4u * AS_WAVES * 4u;
    if (lds > (unsigned)D2D_ASCENT_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                    std::to_string(D2D_ASCENT_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_ASCENT_LAW_INV_SQUARE) e = launch(&ascent_kernel<PL_INV_SQUARE>, grid, dim3(AS_THREADS), lds, st, a);
    else if (law == D2D_ASCENT_LAW_POWER) e = launch(&ascent_kernel<PL_POWER>, grid, dim3(AS_THREADS), lds, st, a);
    else e = launch(&ascent_kernel<PL_POWK>, grid, dim3(AS_THREADS), lds, st, a);
    if (e != hipSuccess) return fail(std::string("ascent_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_ascent_last_error)
