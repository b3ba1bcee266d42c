// libd2d_goodput.so (include/d2d_goodput.h): queue-aware goodput ascent - a link moves its RB or its power to where the weighted
// bits the env can deliver out of its backlogs gain most, with SINR floors - every turn of every round of every env in one launch.
// gfx950.
//
// Shape: ONE workgroup of at most 256 threads per env that stages the env once and then takes turns in LDS.  Staging is by link
// index, no sort, one 96-byte record per link: d2d_rbascent.hip's transmitter tuple (tx x, tx y, linear power x the folded tx
// column c0, and c0 itself - a power candidate forms pow10_tenth(q) * c0 as d2d_ascent.hip does), its receiver tuple (rx x, rx y, rx
// side of the path-loss constant, noise), d2d_ascent.hip's closing tuple (own-pair gain, rx gain, bandwidth, sensitivity), the
// power-law pair, floor, weight, the current rb, the turn word (-1: the link never takes a turn, else the levels of its power
// alphabet, 0: it has no power candidate), the held power, p_min and the demand; then the allowed words and the membership bitset
// bits[w][r], bit j & 31 of word j / 32 = link j sits on RB r.
//
// A link's turn: THE CANDIDATES ARE ONE FLAT LIST dealt over the threads, RB candidates first, then power candidates (a thread with
// several loops).  Every candidate is one call of one walk: the members of the affected group - group(r) and link i - as receivers
// in ascending link index and, per receiver, the same set as transmitters in ascending index, with evaluate_kernel's pair
// arithmetic on the same operands in the same order (d2d_evaluate.hip) into TWO double accumulators, one per state: A is the
// candidate s', B the current state s; link i's slot takes its term at its place in the order under its power in that state, or
// adds 0.0 where it is not on the RB in that state (as the receiver's own slot does).  Both close by evaluate_kernel's operations;
// the integer part (budget, min with the demand, weight, int64 sum) follows the closing.  What link i's LEAVING does to group(c) is
// the same walk with A = "gone", B = "now", made once per turn by every thread on the same words (every LDS read a broadcast),
// not per candidate; a power candidate leaves nothing.  The members of the column are the copies of d2d_rbascent.hip's helpers
// (member_word, nonzero_words, next_member; closing and pair_term restated for a power that varies) - a later refactor may share
// them; that kernel's code generation is pinned, so they are not moved now.
//
// The choice is a reduction of two 64-bit keys - Delta with its sign bit flipped (|Delta| < 2^62, so 0 ranks below every value: no
// admissible candidate), then the complement of (q - p_min) << 16 | r - across the wave by data-parallel primitives
// (d2d_wave_key.h) and across the waves through LDS.  One barrier per turn; every thread then takes the same decision from the same
// words, and a move - two bit flips and rb[i], or the power and its linear value - is applied behind a second barrier that only
// turns that move pay.  A link whose last evaluation is newer than the env's last move is not evaluated again.  No global access
// inside the turn loop, no read-modify-write on memory another thread owns, no scratch, nothing that depends on scheduling.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "d2d_addon.h"
#include "d2d_goodput.h"
#include "d2d_step_device.h"
#include "d2d_wave_key.h"

namespace {

using namespace d2d;

constexpr int GP_MAX_THREADS = 256;
constexpr int GP_MAX_WAVES = GP_MAX_THREADS / 64;
constexpr int GP_LEVELS = D2D_GOODPUT_MAX_LEVELS;
constexpr unsigned GP_RED_BYTES = 208u;                              // keys u64[2][4] | nr u32[2][4] | vsum i64[4] | the results' pointers [9], pad
constexpr unsigned long long GP_SIGN = 0x8000000000000000ull;
static_assert(D2D_GOODPUT_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_GOODPUT_LAW_POWER == LAW_POWER && D2D_GOODPUT_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_GOODPUT_MAX_RBS <= (1 << 16) && GP_LEVELS <= (1 << 15), "the second key packs the level above 16 bits of RB");
static_assert((unsigned long long)D2D_GOODPUT_MAX_LINKS * D2D_GOODPUT_MAX_WEIGHT * 0x7FFFFFFFull < (1ull << 62), "V < 2^62");

struct Results {
    int* rb_out;
    int* power;
    float* sinr;
    float* cap;
    int* served;
    long long* value;
    int* rounds;
    int* moves;
    unsigned char* converged;
};

struct GoodputArgs {
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
    const unsigned* weight;         // [B][N] or null
    const int* demand;              // [B][N] or null
    const unsigned* allowed;        // [N][words] or null
    const unsigned char* movable;   // [N] or null
    const float* floor;             // [N] or null
    const unsigned char* env_mask;  // [B] or null
    Results out;
    double bits_per_mbps;
    long long min_gain;
    int D, N, R;
    int pow_k;
    int words;                      // ceil(R / 32) with an allowed mask, 0 without: the turn loop asks this word, not the pointer
    int W;                          // ceil(N / 32)
    int max_rounds;
    int move_mask;
    // byte offsets of the LDS arrays behind the link records
    unsigned off_al, off_bits, off_red;
};

// dynamic LDS: link Link[N] | allowed u32[N * words] (with a mask) | bits u32[W][R] | keys u64[2][4], nr u32[2][4], vsum i64[4], the
// nine result pointers (parked here across the turn loop: held in scalar registers they are eighteen the pow-k instantiation
// does not have).
// One record of six 16-byte rows per link, so that every field of every link is the record's address plus a constant: separate
// arrays would each hold a base in a scalar register across the turn loop, more than the kernel has.
struct Link {
    float4 tx;                      // tx x, tx y, linear power x c0, c0
    float4 rxa;                     // rx x, rx y, rx_pl, noise
    float4 rxb;                     // own-pair gain, rx_lin, bw_mhz, sens_db
    float2 hh;                      // the power-law pair
    float floor;
    unsigned weight;
    int rb, turn, p, pmin;          // turn: -1 - the link never takes a turn, else the levels of its power alphabet (0: no power candidate)
    int demand, pad0, pad1, pad2;
};
static_assert(sizeof(Link) == 96, "the header's 96 n_links");

struct Lds {
    Link* link; unsigned* al; unsigned* bits; unsigned long long* key; unsigned* nr; long long* vsum; Results* out;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const GoodputArgs& a) {
    Lds s;
    s.link = reinterpret_cast<Link*>(smem);
    s.al = reinterpret_cast<unsigned*>(smem + a.off_al);
    s.bits = reinterpret_cast<unsigned*>(smem + a.off_bits);
    s.key = reinterpret_cast<unsigned long long*>(smem + a.off_red);
    s.nr = reinterpret_cast<unsigned*>(smem + a.off_red + 2u * GP_MAX_WAVES * 8u);
    s.vsum = reinterpret_cast<long long*>(smem + a.off_red + 2u * GP_MAX_WAVES * 8u + 2u * GP_MAX_WAVES * 4u);
    s.out = reinterpret_cast<Results*>(smem + a.off_red + 128u);
    return s;
}

// evaluate_kernel's closing operations (d2d_evaluate.hip; d2d_step.hip, pass 2) on the interference sum acc of a receiver with the
// tuples rx (rx x, rx y, rx_pl, noise) and own (own-pair gain, rx_lin, bw_mhz, sens_db) whose transmitter sends at the linear power z
__device__ __forceinline__ void closing(float4 rx, float4 own, float z, double acc, float& sinr_db, float& cap) {
    const float sig = z * own.x * rx.z * own.y;
    const float accf = (float)acc;
    const float sinr_lin = precise_div(sig, fmaf(accf, rx.z, rx.w));
    sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
    const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
    const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
    const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
    const bool ok = sinr_db > own.w;                                     // simulator.py:123,149
    cap = ok ? own.z * sh : 0.0f;                                        // simulator.py:150-151
}

// rule 5 of include/d2d_queue.h (d2d_queue.hip, service_budget), then the min with the demand
__device__ __forceinline__ int served_bits(float capacity_mbps, double bits_per_mbps, int demand) {
    const double x = (double)capacity_mbps * bits_per_mbps;
    const int budget = !(x > 0.0) ? 0 : (x >= 2147483647.0 ? 2147483647 : (int)x);      // x > 0: the conversion truncates = floor
    return min(budget, demand);
}

// the gain of the pair (transmitter o, the receiver of tuple rx): evaluate_kernel's
template <int MODE>
__device__ __forceinline__ float pair_g(const Lds& s, int o, float4 t, float4 rx, int pow_k) {
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const float dx = t.x - rx.x, dy = t.y - rx.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    return pair_gain<MODE>(d2, POWLAW ? s.link[o].hh : make_float2(-1.0f, 0.0f), pow_k);
}

// The members of RB r, link i forced in (bit_i = 0: nobody), in ascending link index.  `nz` marks the words of the RB's column that
// hold a member, so that a thread steps from member to member (d2d_rbascent.hip).
struct Members {
    unsigned long long nz;
    unsigned cur;
    int w;
};
static_assert(D2D_GOODPUT_MAX_LINKS <= 64 * 32, "one bit of a 64-bit word per word of the column");

__device__ __forceinline__ unsigned member_word(const Lds& s, int w, int r, int R, int wi, unsigned bit_i) {
    const unsigned m = s.bits[w * R + r];
    return w == wi ? m | bit_i : m;
}

__device__ __forceinline__ unsigned long long nonzero_words(const Lds& s, int r, int R, int W, int wi, unsigned bit_i) {
    unsigned long long nz = 0ull;
    for (int w = 0; w < W; ++w) nz |= (unsigned long long)(member_word(s, w, r, R, wi, bit_i) != 0u) << w;
    return nz;
}

__device__ __forceinline__ bool next_member(const Lds& s, Members& it, int r, int R, int wi, unsigned bit_i, int& m) {
    if (it.cur == 0u) {
        if (it.nz == 0ull) return false;
        it.w = __builtin_ctzll(it.nz);
        it.nz &= it.nz - 1ull;
        it.cur = member_word(s, it.w, r, R, wi, bit_i);                  // not zero: nz says so
    }
    m = (it.w << 5) + __builtin_ctz(it.cur);
    it.cur &= it.cur - 1u;
    return true;
}

// sinr_db and capacity_mbps of link m on RB r with the members the bitset holds (m among them) at the powers tx[].z holds:
// evaluate_kernel's walk.  A link on no RB (r outside [0, R)) gets its SNR, as evaluate_kernel gives it.
template <int MODE>
__device__ __forceinline__ void link_planes(const Lds& s, int m, int r, int R, int W, int pow_k, float& sinr_db, float& cap) {
    const float4 rx = s.link[m].rxa;
    double acc = 0.0;
    if ((unsigned)r < (unsigned)R) {
        Members it = {nonzero_words(s, r, R, W, -1, 0u), 0u, 0};
        int o;
        while (next_member(s, it, r, R, -1, 0u, o)) {
            const float4 t = s.link[o].tx;
            const float term = t.z * pair_g<MODE>(s, o, t, rx, pow_k);   // simulator.py:97-101, linear mW
            acc += o != m ? (double)term : 0.0;
        }
    }
    closing(rx, s.link[m].rxb, s.link[m].tx.z, acc, sinr_db, cap);
}

// One walk over group(r) u {i} under two states that differ in link i alone.  State A (the candidate s'): link i sends at z_a if
// in_a, else it is not on r.  State B (the current state s): link i sends at z_b if in_b, else it is not on r.  sum_a, sum_b: the
// int64 sums of term_m over the members a state has on r.  adm: every member m that state A has on r and that has a floor passes
// sinr_m(A) >= floor or sinr_m(s) < floor, float32, NaN compares false - sinr_m(s) is the walk's own B value, but for link i where
// B does not have it on r: there it is sinr_prev_i.  sinr_b_i: link i's sinr_db in state B (read only where in_b).
template <int MODE>
__device__ __forceinline__ void walk(const Lds& s, int r, int i, float z_a, bool in_a, float z_b, bool in_b, float sinr_prev_i, int R, int W,
                                     int pow_k, double bits_per_mbps, long long& sum_a, long long& sum_b, bool& adm, float& sinr_b_i) {
    const int wi = i >> 5;
    const unsigned bit_i = 1u << (i & 31);
    sum_a = 0;
    sum_b = 0;
    adm = true;
    sinr_b_i = 0.0f;
    const unsigned long long nz = nonzero_words(s, r, R, W, wi, bit_i);
    Members rxs = {nz, 0u, 0};
    int m;
    while (next_member(s, rxs, r, R, wi, bit_i, m)) {
        const float4 rx = s.link[m].rxa;
        double acc_a = 0.0, acc_b = 0.0;
        Members txs = {nz, 0u, 0};
        int o;
        while (next_member(s, txs, r, R, wi, bit_i, o)) {
            const float4 t = s.link[o].tx;
            const float g = pair_g<MODE>(s, o, t, rx, pow_k);
            const bool is_i = o == i, other = o != m;                    // the receiver's own slot adds 0.0
            const float term_a = (is_i ? z_a : t.z) * g, term_b = (is_i ? z_b : t.z) * g;       // simulator.py:97-101, linear mW
            acc_a += other && (!is_i || in_a) ? (double)term_a : 0.0;    // link i not on r in that state: its slot adds 0.0
            acc_b += other && (!is_i || in_b) ? (double)term_b : 0.0;
        }
        const float4 own = s.link[m].rxb;
        const bool me = m == i;
        const float zm = s.link[m].tx.z;
        float sinr_a, cap_a, sinr_b, cap_b;
        closing(rx, own, me ? z_a : zm, acc_a, sinr_a, cap_a);
        closing(rx, own, me ? z_b : zm, acc_b, sinr_b, cap_b);
        const long long wgt = (long long)s.link[m].weight;
        const int dem = s.link[m].demand;
        const long long term_a = wgt * (long long)served_bits(cap_a, bits_per_mbps, dem);
        const long long term_b = wgt * (long long)served_bits(cap_b, bits_per_mbps, dem);
        sum_a += !me || in_a ? term_a : 0ll;
        sum_b += !me || in_b ? term_b : 0ll;
        const float fl = s.link[m].floor;
        const float before = me && !in_b ? sinr_prev_i : sinr_b;
        adm = adm && ((me && !in_a) || !(fl > -INFINITY) || sinr_a >= fl || before < fl);      // float32, NaN compares false
        sinr_b_i = me ? sinr_b : sinr_b_i;
    }
}

template <int MODE>
__global__ __launch_bounds__(GP_MAX_THREADS) void goodput_kernel(const GoodputArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D, W = a.W, words = a.words;
    const int T = (int)blockDim.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    const size_t row = b * (size_t)N;
    const int* rb_row = a.rb + row;
    const int* pwr_row = a.pwr + row;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- per-link constants by link index, and an empty bitset
    for (int j = tid; j < N; j += T) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float tx_x = px[txd], tx_y = py[txd], rx_x = px[rxd], rx_y = py[rxd];
        const float c0 = a.cols[txd];
        const float me_z = pow10_tenth(pwr_row[j]) * c0;                 // the step's tuple.z (d2d_step.hip, pass 1)
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
        const float bw_mhz = a.cap_cols[txd], sens = a.cap_cols[D + rxd];
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g_own = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        s.link[j].tx = make_float4(tx_x, tx_y, me_z, c0);
        s.link[j].rxa = make_float4(rx_x, rx_y, rx_pl, noise);
        s.link[j].rxb = make_float4(g_own, rx_lin, bw_mhz, sens);
        s.link[j].hh = h;
    }
    // (a second loop: one loop over both halves keeps every argument of the launch in scalar registers at once)
    for (int j = tid; j < N; j += T) {
        const int r = rb_row[j], held = pwr_row[j];
        const int lo = a.p_min[j], hi = a.p_max[j];
        // the levels of a link that has power candidates: an alphabet of 1 .. 64 levels that 16 bits hold, the held power inside it
        const bool alphabet = lo <= hi && (long long)hi - lo < GP_LEVELS && lo > -4096 && hi < 4096 && held >= lo && held <= hi;
        bool some = words == 0;                                          // an allowed RB
        for (int w = 0; w < words; ++w) {
            unsigned m = a.allowed[(size_t)j * (size_t)words + (size_t)w];
            if (w == words - 1 && (R & 31)) m &= (1u << (R & 31)) - 1u;
            some = some || m != 0u;
        }
        const bool takes = (unsigned)r < (unsigned)R && (!a.movable || a.movable[j] != 0) && ((a.move_mask & D2D_GOODPUT_MOVE_POWER) || some);
        const unsigned wgt = a.weight ? a.weight[row + (size_t)j] : 1u;
        const int dem = a.demand ? a.demand[row + (size_t)j] : 0x7FFFFFFF;
        s.link[j].rb = r;
        s.link[j].turn = takes ? (alphabet ? hi - lo + 1 : 0) : -1;
        s.link[j].floor = a.floor ? a.floor[j] : -INFINITY;
        s.link[j].p = held;
        s.link[j].pmin = lo;
        s.link[j].weight = min(wgt, (unsigned)D2D_GOODPUT_MAX_WEIGHT);
        s.link[j].demand = max(dem, 0);
    }
    for (int k = tid; k < N * words; k += T) s.al[k] = a.allowed[k];
    for (int k = tid; k < W * R; k += T) s.bits[k] = 0u;
    if (tid == 0) *s.out = a.out;
    // the slots of the waves a launch does not have stay 0 - no candidate, no bits - so that every combine below reads all four
    if (tid < 2 * GP_MAX_WAVES) { s.key[tid] = 0ull; s.nr[tid] = 0u; }
    if (tid < GP_MAX_WAVES) s.vsum[tid] = 0ll;
    __syncthreads();
    // ---- membership: thread w owns column w of the bitset (links 32 w .. 32 w + 31), so no two threads touch one word
    for (int w = tid; w < W; w += T) {
        const int j_end = min(N, (w + 1) << 5);
        for (int j = w << 5; j < j_end; ++j) {
            const int r = s.link[j].rb;
            if ((unsigned)r < (unsigned)R) s.bits[w * R + r] |= 1u << (j & 31);
        }
    }
    __syncthreads();

    // ---- the rounds
    int moves = 0, parity = 0;
    int last_move = -1;                                                  // the turn index t * N + i of the env's last move
    const int n_rb = (a.move_mask & D2D_GOODPUT_MOVE_RB) && R > 1 ? R : 0;             // the RB half of the flat candidate list
    int t = 0;                                                           // the rounds that moved a link
    for (; t < a.max_rounds; ++t) {
        for (int i = 0; i < N; ++i) {
            const int levels = __builtin_amdgcn_readfirstlane(s.link[i].turn);
            if (levels < 0) continue;                                    // never moves: no turn
            const int turn = t * N + i;
            // evaluated since the last move, which was another link's: it stays, and so does the rest.  (The link that made the last
            // move takes its turn again: after an RB move a power may gain, and the other way round.)
            if (t > 0 && turn - N > last_move) break;
            // the same words in every lane, kept in vector registers: the scalar ones are spoken for
            const int cur = s.link[i].rb, p = s.link[i].p, lo = s.link[i].pmin;
            const float4 me = s.link[i].tx;                                   // me.z: the linear power now, me.w: c0
            const int held_level = levels > 0 ? p - lo : 0;
            const int n_pw = (a.move_mask & D2D_GOODPUT_MOVE_POWER) ? levels : 0;
            // One loop, one walk.  Its first pass, made by every thread on the same words when there are RB candidates, is what link
            // i's leaving does to group(c) - A = "gone", B = "now" - for every RB candidate alike; the passes behind it are the
            // thread's candidates of the flat list.
            long long leave = 0ll;
            bool adm_leave = true;
            float sinr_now = 0.0f;
            unsigned long long key = 0ull;                               // 0: no admissible candidate
            unsigned key_lr = 0u;
            for (int k = n_rb ? -1 : tid; k < n_rb + n_pw; k = k < 0 ? tid : k + T) {
                const bool leaving = k < 0, is_rb = k < n_rb;
                const int r = is_rb && !leaving ? k : cur;
                const int level = is_rb ? held_level : k - n_rb;
                bool skip = false;
                if (!leaving) skip = is_rb ? r == cur || !(words == 0 || ((s.al[i * words + (r >> 5)] >> (r & 31)) & 1u)) : lo + level == p;
                if (skip) continue;
                const float z_a = is_rb ? me.z : pow10_tenth(lo + level) * me.w;
                long long sum_a, sum_b;
                bool adm;
                float sinr_b_i;
                walk<MODE>(s, r, i, z_a, !leaving, me.z, leaving || !is_rb, sinr_now, R, W, a.pow_k, a.bits_per_mbps, sum_a, sum_b, adm, sinr_b_i);
                if (leaving) {
                    leave = sum_a - sum_b;
                    adm_leave = adm;
                    sinr_now = sinr_b_i;
                    continue;
                }
                if (!(adm && (adm_leave || !is_rb))) continue;
                const long long delta = sum_a - sum_b + (is_rb ? leave : 0ll);
                const unsigned long long kd = (unsigned long long)delta ^ GP_SIGN;
                const unsigned lr = 0xFFFFFFFFu - (((unsigned)level << 16) | (unsigned)r);
                if (kd > key || (kd == key && lr > key_lr)) { key = kd; key_lr = lr; }
            }
            // the largest Delta of the wave, then the lowest (power, RB) among the lanes that hold it
            const unsigned long long top_w = wave_reduce<true>(key);
            const unsigned long long nr_w = wave_reduce<true>(key == top_w && key != 0ull ? (unsigned long long)key_lr : 0ull);
            if (lane == 0) {
                s.key[parity * GP_MAX_WAVES + wave] = top_w;
                s.nr[parity * GP_MAX_WAVES + wave] = (unsigned)nr_w;
            }
            __syncthreads();                                             // the turn's one barrier: the keys and their (power, RB)
            unsigned long long top = s.key[parity * GP_MAX_WAVES];
            unsigned nr = s.nr[parity * GP_MAX_WAVES];
#pragma unroll
            for (int w = 1; w < GP_MAX_WAVES; ++w) {
                const unsigned long long k = s.key[parity * GP_MAX_WAVES + w];
                const unsigned n = s.nr[parity * GP_MAX_WAVES + w];
                const bool better = k > top || (k == top && n > nr);
                top = better ? k : top;
                nr = better ? n : nr;
            }
            int to = -1;                                                 // level << 16 | rb of the move, or -1
            if (top != 0ull && (long long)(top ^ GP_SIGN) > a.min_gain) to = (int)(0xFFFFFFFFu - nr);
            to = __builtin_amdgcn_readfirstlane(to);                     // every thread read the same words: the decision is scalar
            parity ^= 1;
            if (to >= 0) {
                const int to_rb = to & 0xFFFF;
                if (to_rb != cur) {                                      // an RB move: the power stays
                    const int wi = i >> 5;
                    const unsigned bit = 1u << (i & 31);
                    if (tid == cur % T) s.bits[wi * R + cur] &= ~bit;
                    if (tid == to_rb % T) s.bits[wi * R + to_rb] |= bit;
                    if (tid == 0) s.link[i].rb = to_rb;
                } else if (tid == 0) {                                   // a power move: the RB stays
                    const int q = lo + (to >> 16);
                    s.link[i].p = q;
                    s.link[i].tx.z = pow10_tenth(q) * me.w;
                }
                ++moves;
                last_move = turn;
                __syncthreads();                                         // the next turn reads the bitset, rb[], p[] and tx[].z
            }
        }
        if (last_move < t * N) break;                                    // a round that moved nobody: t < max_rounds
    }

    // ---- evaluate_kernel's planes for the state the ascent stopped at, every link, the served bits, V, and the results
    // (the env's index and its row are formed again, from a workgroup id the compiler cannot match with the one above: held across the
    // turn loop they are scalar registers the pow-k instantiation does not have)
    const Results out = *s.out;
    unsigned wg = blockIdx.x;
    asm volatile("" : "+s"(wg));
    const size_t env = wg, out_row = env * (size_t)N;
    long long v = 0ll;
    for (int i = tid; i < N; i += T) {
        const int r = s.link[i].rb;
        float sinr, cap;
        link_planes<MODE>(s, i, r, R, W, a.pow_k, sinr, cap);
        const int served = served_bits(cap, a.bits_per_mbps, s.link[i].demand);
        v += (long long)s.link[i].weight * (long long)served;
        out.rb_out[out_row + (size_t)i] = r;
        out.power[out_row + (size_t)i] = s.link[i].p;
        out.sinr[out_row + (size_t)i] = sinr;
        out.cap[out_row + (size_t)i] = cap;
        out.served[out_row + (size_t)i] = served;
    }
    // V: integer sums are order-free - across the wave by shuffles, across the waves through LDS
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane == 0) s.vsum[wave] = v;
    __syncthreads();
    if (tid == 0) {
        long long total = 0ll;
#pragma unroll
        for (int w = 0; w < GP_MAX_WAVES; ++w) total += s.vsum[w];
        out.value[env] = total;
        out.rounds[env] = t;
        out.moves[env] = moves;
        out.converged[env] = (unsigned char)(t < a.max_rounds);
    }
}

}  // namespace

extern "C" int d2d_goodput_ascent(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                  const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                                  int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max,
                                  const uint32_t* weight, const int32_t* demand_bits, double bits_per_mbps, const uint32_t* allowed,
                                  const uint8_t* movable, const float* floor_db, int32_t move_mask, int64_t min_gain, int32_t max_rounds,
                                  const uint8_t* env_mask, int32_t* rb_out, int32_t* power_dbm, float* sinr_db, float* capacity_mbps,
                                  int32_t* served_bits, int64_t* value, int32_t* rounds, int32_t* moves, uint8_t* converged,
                                  void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_GOODPUT_MAX_LINKS, n_rbs, D2D_GOODPUT_MAX_RBS, n_dev)) return fail(why);
    if (max_rounds < 1 || max_rounds > D2D_GOODPUT_MAX_ROUNDS)
        return fail("max_rounds must be in [1, " + std::to_string(D2D_GOODPUT_MAX_ROUNDS) + "]");
    if (move_mask < 1 || move_mask > (D2D_GOODPUT_MOVE_RB | D2D_GOODPUT_MOVE_POWER)) return fail("move_mask must be 1 (RBs), 2 (powers) or 3 (both)");
    if (min_gain < 0 || min_gain >= (int64_t)1 << 62) return fail("min_gain must be in [0, 2^62)");
    if (!std::isfinite(bits_per_mbps) || !(bits_per_mbps > 0.0)) return fail("bits_per_mbps must be finite and > 0");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !p_min || !p_max || !rb_out || !power_dbm ||
        !sinr_db || !capacity_mbps || !served_bits || !value || !rounds || !moves || !converged)
        return fail("null device pointer");
    const void* outs[9] = {rb_out, power_dbm, sinr_db, capacity_mbps, served_bits, value, rounds, moves, converged};
    for (int x = 0; x < 9; ++x)
        for (int y = x + 1; y < 9; ++y)
            if (outs[x] == outs[y])
                return fail("rb_out, power_dbm, sinr_db, capacity_mbps, served_bits, value, rounds, moves and converged must be nine arrays");
    GoodputArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.p_min = p_min; a.p_max = p_max; a.weight = weight; a.demand = demand_bits; a.allowed = allowed;
    a.movable = movable; a.floor = floor_db; a.env_mask = env_mask;
    a.out.rb_out = rb_out; a.out.power = power_dbm; a.out.sinr = sinr_db; a.out.cap = capacity_mbps; a.out.served = served_bits;
    a.out.value = reinterpret_cast<long long*>(value); a.out.rounds = rounds; a.out.moves = moves; a.out.converged = converged;
    a.bits_per_mbps = bits_per_mbps;
    a.min_gain = min_gain;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k; a.max_rounds = max_rounds; a.move_mask = move_mask;
    a.words = allowed ? (n_rbs + 31) / 32 : 0;
    a.W = (n_links + 31) / 32;
    const unsigned long long N = (unsigned long long)n_links;
    // 64-bit until the limit is checked: 2048 links x 8192 RBs would be 2 MiB of bitset alone
    unsigned long long off = N * sizeof(Link);
    a.off_al = (unsigned)off; off += (N * (unsigned long long)a.words * 4ull + 15ull) & ~15ull;
    a.off_bits = (unsigned)off; off += ((unsigned long long)a.W * (unsigned long long)n_rbs * 4ull + 15ull) & ~15ull;
    a.off_red = (unsigned)off; off += GP_RED_BYTES;
    if (off > (unsigned long long)D2D_GOODPUT_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_GOODPUT_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const unsigned lds = (unsigned)off;
    // the flat candidate list of a turn: the RBs, then the levels - no more waves than it needs
    const int list = ((move_mask & D2D_GOODPUT_MOVE_RB) ? n_rbs : 0) + ((move_mask & D2D_GOODPUT_MOVE_POWER) ? GP_LEVELS : 0);
    const unsigned threads = (unsigned)min(GP_MAX_THREADS, (list + 63) & ~63);
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_GOODPUT_LAW_INV_SQUARE) e = launch(&goodput_kernel<PL_INV_SQUARE>, grid, dim3(threads), lds, st, a);
    else if (law == D2D_GOODPUT_LAW_POWER) e = launch(&goodput_kernel<PL_POWER>, grid, dim3(threads), lds, st, a);
    else e = launch(&goodput_kernel<PL_POWK>, grid, dim3(threads), lds, st, a);
    if (e != hipSuccess) return fail(std::string("goodput_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_goodput_last_error)
