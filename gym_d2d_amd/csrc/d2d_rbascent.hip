// libd2d_rbascent.so (include/d2d_rbascent.h): cooperative local search on the RB half of the action - a link moves to the RB where
// the TOTAL capacity gains most, with SINR floors - every turn of every round of every env in one launch.  gfx950.
//
// Shape: ONE workgroup of at most 256 threads per env that stages the env once and then takes turns in LDS.  Staging is
// d2d_brdyn.hip's, by link index, no sort: the transmitter tuple (tx x, tx y, linear power x the folded tx column), the receiver
// tuple (rx x, rx y, rx side of the path-loss constant, noise), the closing tuple (own signal, bandwidth, sensitivity, floor), the
// power-law pair, the current rb, the first allowed RB (-1: the link never takes a turn), the allowed words, and the membership
// bitset bits[w][r], bit j & 31 of word j / 32 = link j sits on RB r.
//
// A link's turn: LANES OWN RBs (a lane with several of them loops).  A lane walks group(r) u {i} as receivers in ascending link
// index and, per receiver, the same set as transmitters in ascending index - stepping from member to member by a 64-bit mask of
// the column's words that hold one, so that a wave runs as many bodies as its longest group has members, not as many as its lanes'
// groups have words between them - with evaluate_kernel's pair arithmetic on the same
// operands in the same order (d2d_evaluate.hip) into TWO double accumulators: one takes link i's term at its place in the order,
// one skips it (adding 0.0, as the receiver's own slot does).  Both close by evaluate_kernel's operations, so one walk gives
// With(r), Without(r), both SINRs of the floor test and D(r) = With(r) - Without(r); the lane of the link's own RB c gives D(c) the
// same way.  The choice is a reduction of keys - the order-preserving image of the double D (64 bits), then the complement of r -
// across the wave by data-parallel primitives (d2d_wave_key.h) and across the waves through LDS; the image takes all 64 bits of a
// word, so the complement of r travels in a second word, reduced among the lanes that hold the top image.  One barrier per turn;
// every thread then takes the same decision from the same words, and a move - two bit flips and rb[i] - is applied behind a second
// barrier that only turns that move pay.  A link whose last evaluation is newer than the env's last move is not evaluated again.
// No global access inside the turn loop, no read-modify-write on memory another thread owns, no scratch, nothing that depends on
// scheduling.  A lane with a long group does G^2 pair evaluations while the others wait.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <string>

#include "d2d_addon.h"
#include "d2d_rbascent.h"
#include "d2d_step_device.h"
#include "d2d_wave_key.h"

namespace {

using namespace d2d;

constexpr int RA_MAX_THREADS = 256;
constexpr int RA_MAX_WAVES = RA_MAX_THREADS / 64;
constexpr unsigned RA_RED_BYTES = 112u;                              // keys u64[2][4] | d_cur f64[2] | nr u32[2][4]
static_assert(D2D_RBASCENT_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_RBASCENT_LAW_POWER == LAW_POWER && D2D_RBASCENT_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");

struct Results {
    int* rb_out;
    float* sinr;
    float* cap;
    int* rounds;
    int* moves;
    unsigned char* converged;
};

struct RbAscentArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* cap_cols;          // [2][D]
    const unsigned* allowed;        // [N][words] or null
    const unsigned char* movable;   // [N] or null
    const float* floor;             // [N] or null
    const unsigned char* env_mask;  // [B] or null
    Results out;
    double min_gain;
    int D, N, R;
    int pow_k;
    int words;                      // ceil(R / 32) with an allowed mask, 0 without: the turn loop asks this word, not the pointer
    int W;                          // ceil(N / 32)
    int max_rounds;
    // byte offsets of the LDS arrays behind the transmitter tuples
    unsigned off_hh, off_rb, off_al, off_bits, off_red;
};

// dynamic LDS, by link index: tx float4[N] (tx x, tx y, linear power x tx constant, unused) | rxa float4[N] (rx x, rx y, rx_pl,
// noise) | rxb float4[N] (own signal, bw_mhz, sens_db, floor) | hh float2[N] (power laws) | rb i32[n4] | first i32[n4] | allowed
// u32[N * words] (with a mask) | bits u32[W][R] | keys u64[2][4], d_cur f64[2], nr u32[2][4]

struct Lds {
    float4* tx; float4* rxa; float4* rxb; float2* hh; int* rb; int* first; unsigned* al; unsigned* bits;
    unsigned long long* key; double* dcur; unsigned* nr;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const RbAscentArgs& a) {
    Lds s;
    s.tx = reinterpret_cast<float4*>(smem);
    s.rxa = s.tx + a.N;                                              // the three float4 arrays are one block: one base
    s.rxb = s.tx + 2 * a.N;
    s.hh = reinterpret_cast<float2*>(smem + a.off_hh);
    s.rb = reinterpret_cast<int*>(smem + a.off_rb);
    s.first = s.rb + ((a.N + 3) & ~3);
    s.al = reinterpret_cast<unsigned*>(smem + a.off_al);
    s.bits = reinterpret_cast<unsigned*>(smem + a.off_bits);
    s.key = reinterpret_cast<unsigned long long*>(smem + a.off_red);
    s.dcur = reinterpret_cast<double*>(smem + a.off_red + 2u * RA_MAX_WAVES * 8u);
    s.nr = reinterpret_cast<unsigned*>(smem + a.off_red + 2u * RA_MAX_WAVES * 8u + 16u);
    return s;
}

// evaluate_kernel's closing operations (d2d_evaluate.hip; d2d_step.hip, pass 2) on the interference sum acc of a receiver with the
// tuples rx (rx x, rx y, rx_pl, noise) and cl (own signal, bw_mhz, sens_db, floor)
__device__ __forceinline__ void closing(float4 rx, float4 cl, double acc, float& sinr_db, float& cap) {
    const float accf = (float)acc;
    const float sinr_lin = precise_div(cl.x, fmaf(accf, rx.z, rx.w));
    sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
    const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
    const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
    const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
    const bool ok = sinr_db > cl.z;                                      // simulator.py:123,149
    cap = ok ? cl.y * sh : 0.0f;                                         // simulator.py:150-151
}

template <int MODE>
__device__ __forceinline__ float pair_term(const Lds& s, int o, float4 rx, int pow_k) {
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const float4 t = s.tx[o];
    const float dx = t.x - rx.x, dy = t.y - rx.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    const float g = pair_gain<MODE>(d2, POWLAW ? s.hh[o] : make_float2(-1.0f, 0.0f), pow_k);
    return t.z * g;                                                      // simulator.py:97-101, linear mW
}

// The members of RB r, link i forced in (bit_i = 0: nobody), in ascending link index.  `nz` marks the words of the RB's column that
// hold a member, so that a lane steps from member to member: walking the W words in lockstep, a wave whose lanes own RBs with
// members in different words would run the body once per word ANY lane has a member in - W^2 bodies for the two nested walks where
// the longest group asks for G^2.
struct Members {
    unsigned long long nz;
    unsigned cur;
    int w;
};
static_assert(D2D_RBASCENT_MAX_LINKS <= 64 * 32, "one bit of a 64-bit word per word of the column");

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

// sinr_db and capacity_mbps of link m on RB r with the members the bitset holds (m among them): evaluate_kernel's walk.  A link on
// no RB (r outside [0, R)) gets its SNR, as evaluate_kernel gives it.
template <int MODE>
__device__ __forceinline__ void link_planes(const Lds& s, int m, int r, int R, int W, int pow_k, float& sinr_db, float& cap) {
    const float4 rx = s.rxa[m];
    double acc = 0.0;
    if ((unsigned)r < (unsigned)R) {
        Members it = {nonzero_words(s, r, R, W, -1, 0u), 0u, 0};
        int o;
        while (next_member(s, it, r, R, -1, 0u, o)) {
            const float term = pair_term<MODE>(s, o, rx, pow_k);
            acc += o != m ? (double)term : 0.0;
        }
    }
    closing(rx, s.rxb[m], acc, sinr_db, cap);
}

// One walk over group(r) u {i}: with = With(r), without = Without(r), adm = r is admissible for link i, whose sinr_db on its own RB
// is sinr_cur_i (read only where link i has a floor).
template <int MODE>
__device__ __forceinline__ void rb_walk(const Lds& s, int r, int i, float sinr_cur_i, int R, int W, int pow_k, double& with,
                                        double& without, bool& adm) {
    const int wi = i >> 5;
    const unsigned bit_i = 1u << (i & 31);
    with = 0.0;
    without = 0.0;
    adm = true;
    const unsigned long long nz = nonzero_words(s, r, R, W, wi, bit_i);
    Members rxs = {nz, 0u, 0};
    int m;
    while (next_member(s, rxs, r, R, wi, bit_i, m)) {
        const float4 rx = s.rxa[m];
        double acc_with = 0.0, acc_without = 0.0;
        Members txs = {nz, 0u, 0};
        int o;
        while (next_member(s, txs, r, R, wi, bit_i, o)) {
            const float term = pair_term<MODE>(s, o, rx, pow_k);
            const double dt = o != m ? (double)term : 0.0;               // the receiver's own slot adds 0.0
            acc_with += dt;
            acc_without += o != i ? dt : 0.0;                            // link i not on r: its slot adds 0.0
        }
        const float4 cl = s.rxb[m];
        float sinr_with, cap_with, sinr_without, cap_without;
        closing(rx, cl, acc_with, sinr_with, cap_with);
        closing(rx, cl, acc_without, sinr_without, cap_without);
        with += (double)cap_with;
        without += m != i ? (double)cap_without : 0.0;
        const float fl = cl.w;
        const float before = m == i ? sinr_cur_i : sinr_without;         // sinr^c_m: link i where it is now
        adm = adm && (!(fl > -INFINITY) || sinr_with >= fl || before < fl);          // float32, NaN compares false
    }
}

// The six result pointers, read from the kernel-argument segment BEHIND the turn loop: taken from the argument struct they are
// loaded with the rest at the kernel's start and held in twelve scalar registers across the loop, more than the pow-k
// instantiation has.  The empty statement keeps the loads below it.
__device__ __forceinline__ Results results_behind_the_loop() {
    typedef __attribute__((address_space(4))) const unsigned char* KernargBytes;
    typedef __attribute__((address_space(4))) const unsigned long long* KernargWords;
    KernargBytes ka = (KernargBytes)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const KernargWords w = (KernargWords)(ka + offsetof(RbAscentArgs, out));
    static_assert(sizeof(Results) == 6 * sizeof(unsigned long long), "six pointers");
    Results out;
    out.rb_out = reinterpret_cast<int*>(w[0]);
    out.sinr = reinterpret_cast<float*>(w[1]);
    out.cap = reinterpret_cast<float*>(w[2]);
    out.rounds = reinterpret_cast<int*>(w[3]);
    out.moves = reinterpret_cast<int*>(w[4]);
    out.converged = reinterpret_cast<unsigned char*>(w[5]);
    return out;
}

// The order-preserving image of a double in the unsigned 64-bit words: a < b as doubles iff image(a) < image(b), above the two
// words the choice keeps for itself - 0 (no candidate) and 1 (a NaN): -inf maps to 2^52 - 1.  -0.0 takes the image of +0.0.
__device__ __forceinline__ unsigned long long ordered_image(double t) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(t + 0.0);
    return t != t ? 1ull : ((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}

__device__ __forceinline__ double image_value(unsigned long long o) {
    return __longlong_as_double((long long)((o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o));
}

template <int MODE>
__global__ __launch_bounds__(RA_MAX_THREADS) void rbascent_kernel(const RbAscentArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D, W = a.W, words = a.words;
    const int T = (int)blockDim.x, n_waves = T >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- per-link constants by link index, and an empty bitset
    for (int j = tid; j < N; j += T) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float tx_x = px[txd], tx_y = py[txd], rx_x = px[rxd], rx_y = py[rxd];
        const float me_z = pow10_tenth(pwr_row[j]) * a.cols[txd];        // the step's tuple.z (d2d_step.hip, pass 1)
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
        const float bw_mhz = a.cap_cols[txd], sens = a.cap_cols[D + rxd];
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        s.tx[j] = make_float4(tx_x, tx_y, me_z, 0.0f);
        s.rxa[j] = make_float4(rx_x, rx_y, rx_pl, noise);
        s.rxb[j] = make_float4(me_z * g * rx_pl * rx_lin, bw_mhz, sens, a.floor ? a.floor[j] : -INFINITY);     // own link: as evaluate_kernel forms it
        if (POWLAW) s.hh[j] = h;
    }
    // (a second loop: one loop over both halves keeps every argument of the launch in scalar registers at once, more than the pow-k
    // instantiation has)
    for (int j = tid; j < N; j += T) {
        const int r = rb_row[j];
        int first = -1;                                                  // the first allowed RB of a link that takes turns
        if ((unsigned)r < (unsigned)R && (!a.movable || a.movable[j] != 0)) {
            if (words == 0) first = 0;
            for (int w = 0; w < words; ++w) {
                unsigned m = a.allowed[(size_t)j * (size_t)words + (size_t)w];
                if (w == words - 1 && (R & 31)) m &= (1u << (R & 31)) - 1u;
                if (m) { first = (w << 5) + __builtin_ctz(m); break; }
            }
        }
        s.rb[j] = r;
        s.first[j] = first;
    }
    for (int k = tid; k < N * words; k += T) s.al[k] = a.allowed[k];
    for (int k = tid; k < W * R; k += T) s.bits[k] = 0u;
    __syncthreads();
    // ---- membership: thread w owns column w of the bitset (links 32 w .. 32 w + 31), so no two threads touch one word
    for (int w = tid; w < W; w += T) {
        const int j_end = min(N, (w + 1) << 5);
        for (int j = w << 5; j < j_end; ++j) {
            const int r = s.rb[j];
            if ((unsigned)r < (unsigned)R) s.bits[w * R + r] |= 1u << (j & 31);
        }
    }
    __syncthreads();

    // ---- the rounds
    int rounds = 0, moves = 0, fixed = 0, parity = 0;
    int last_move = -1;                                                  // the turn index t * N + i of the env's last move
    for (int t = 0; t < a.max_rounds; ++t) {
        bool moved = false;
        for (int i = 0; i < N; ++i) {
            const int fa = __builtin_amdgcn_readfirstlane(s.first[i]);
            if (fa < 0) continue;                                        // never moves: no turn
            const int turn = t * N + i;
            if (t > 0 && turn - N >= last_move) break;                   // evaluated since the last move: it stays, and so does the rest
            const int cur = __builtin_amdgcn_readfirstlane(s.rb[i]);
            // sinr^c_i, for the floor test of link i itself on another RB: every thread walks group(c) on the same words
            float sinr_cur = 0.0f;
            if (s.rxb[i].w > -INFINITY) {
                float cap_cur;
                link_planes<MODE>(s, i, cur, R, W, a.pow_k, sinr_cur, cap_cur);
            }
            unsigned long long key = 0ull;                               // 0: no candidate
            unsigned key_r = 0u;
            for (int r = tid; r < R; r += T) {
                const bool may = words == 0 || ((s.al[i * words + (r >> 5)] >> (r & 31)) & 1u);
                if (!may && r != cur) continue;
                double with, without;
                bool adm;
                rb_walk<MODE>(s, r, i, sinr_cur, R, W, a.pow_k, with, without, adm);
                const double d = with - without;
                if (r == cur) { s.dcur[parity] = d; continue; }
                const unsigned long long k = ordered_image(d);
                if (adm && k > 1ull && k > key) { key = k; key_r = (unsigned)r; }       // ascending r: equal images keep the lowest
            }
            // the largest image of the wave, then the lowest r among the lanes that hold it
            const unsigned long long top_w = wave_reduce<true>(key);
            const unsigned long long nr_w = wave_reduce<true>(key == top_w && key != 0ull ? (unsigned long long)(0xFFFFFFFFu - key_r) : 0ull);
            if (lane == 0) {
                s.key[parity * RA_MAX_WAVES + wave] = top_w;
                s.nr[parity * RA_MAX_WAVES + wave] = (unsigned)nr_w;
            }
            __syncthreads();                                             // the turn's one barrier: keys, their RBs, D(c)
            unsigned long long top = s.key[parity * RA_MAX_WAVES];
            unsigned nr = s.nr[parity * RA_MAX_WAVES];
            for (int w = 1; w < n_waves; ++w) {
                const unsigned long long k = s.key[parity * RA_MAX_WAVES + w];
                const unsigned n = s.nr[parity * RA_MAX_WAVES + w];
                const bool better = k > top || (k == top && n > nr);
                top = better ? k : top;
                nr = better ? n : nr;
            }
            int to = -1;
            if (top != 0ull) {
                const double gain = image_value(top) - s.dcur[parity];
                to = gain > a.min_gain ? (int)(0xFFFFFFFFu - nr) : -1;  // NaN gain: stays
            }
            to = __builtin_amdgcn_readfirstlane(to);                     // every thread read the same words: the decision is scalar
            parity ^= 1;
            if (to >= 0) {
                const int wi = i >> 5;
                const unsigned bit = 1u << (i & 31);
                if (tid == cur % T) s.bits[wi * R + cur] &= ~bit;
                if (tid == to % T) s.bits[wi * R + to] |= bit;
                if (tid == 0) s.rb[i] = to;
                moved = true;
                ++moves;
                last_move = turn;
                __syncthreads();                                         // the next turn reads the bitset and rb[]
            }
        }
        if (!moved) { fixed = 1; break; }
        ++rounds;
    }

    // ---- evaluate_kernel's planes for the RBs the ascent stopped at, every link, and the results
    const Results out = results_behind_the_loop();
    const size_t row = b * (size_t)N;
    for (int i = tid; i < N; i += T) {
        const int r = s.rb[i];
        float sinr, cap;
        link_planes<MODE>(s, i, r, R, W, a.pow_k, sinr, cap);
        out.rb_out[row + (size_t)i] = r;
        out.sinr[row + (size_t)i] = sinr;
        out.cap[row + (size_t)i] = cap;
    }
    if (tid == 0) {
        out.rounds[b] = rounds;
        out.moves[b] = moves;
        out.converged[b] = (unsigned char)fixed;
    }
}

}  // namespace

extern "C" int d2d_rb_ascent(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                             const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                             int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const uint32_t* allowed,
                             const uint8_t* movable, const float* floor_db, double min_gain_mbps, int32_t max_rounds,
                             const uint8_t* env_mask, int32_t* rb_out, float* sinr_db, float* capacity_mbps, int32_t* rounds,
                             int32_t* moves, uint8_t* converged, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_RBASCENT_MAX_LINKS, n_rbs, D2D_RBASCENT_MAX_RBS, n_dev)) return fail(why);
    if (max_rounds < 1 || max_rounds > D2D_RBASCENT_MAX_ROUNDS)
        return fail("max_rounds must be in [1, " + std::to_string(D2D_RBASCENT_MAX_ROUNDS) + "]");
    if (!std::isfinite(min_gain_mbps) || min_gain_mbps < 0.0) return fail("min_gain_mbps must be finite and >= 0");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !rb_out || !sinr_db || !capacity_mbps ||
        !rounds || !moves || !converged)
        return fail("null device pointer");
    const void* outs[6] = {rb_out, sinr_db, capacity_mbps, rounds, moves, converged};
    for (int x = 0; x < 6; ++x)
        for (int y = x + 1; y < 6; ++y)
            if (outs[x] == outs[y]) return fail("rb_out, sinr_db, capacity_mbps, rounds, moves and converged must be six arrays");
    RbAscentArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.allowed = allowed; a.movable = movable; a.floor = floor_db; a.env_mask = env_mask;
    a.out.rb_out = rb_out; a.out.sinr = sinr_db; a.out.cap = capacity_mbps; a.out.rounds = rounds; a.out.moves = moves;
    a.out.converged = converged;
    a.min_gain = min_gain_mbps;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k; a.max_rounds = max_rounds;
    a.words = allowed ? (n_rbs + 31) / 32 : 0;
    a.W = (n_links + 31) / 32;
    const unsigned long long N = (unsigned long long)n_links, n4 = (N + 3ull) & ~3ull;
    // 64-bit until the limit is checked: 2048 links x 8192 RBs would be 2 MiB of bitset alone
    unsigned long long off = N * 16ull;
    off += 2ull * N * 16ull;                                             // rxa, rxb: behind tx, one block
    a.off_hh = (unsigned)off; off += law == D2D_RBASCENT_LAW_INV_SQUARE ? 0ull : (N * 8ull + 15ull) & ~15ull;
    a.off_rb = (unsigned)off; off += 2ull * n4 * 4ull;                   // rb, first
    a.off_al = (unsigned)off; off += (N * (unsigned long long)a.words * 4ull + 15ull) & ~15ull;
    a.off_bits = (unsigned)off; off += ((unsigned long long)a.W * (unsigned long long)n_rbs * 4ull + 15ull) & ~15ull;
    a.off_red = (unsigned)off; off += RA_RED_BYTES;
    if (off > (unsigned long long)D2D_RBASCENT_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_RBASCENT_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const unsigned lds = (unsigned)off;
    const unsigned threads = (unsigned)min(RA_MAX_THREADS, (n_rbs + 63) & ~63);     // lanes own RBs: no more waves than RBs need
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_RBASCENT_LAW_INV_SQUARE) e = launch(&rbascent_kernel<PL_INV_SQUARE>, grid, dim3(threads), lds, st, a);
    else if (law == D2D_RBASCENT_LAW_POWER) e = launch(&rbascent_kernel<PL_POWER>, grid, dim3(threads), lds, st, a);
    else e = launch(&rbascent_kernel<PL_POWK>, grid, dim3(threads), lds, st, a);
    if (e != hipSuccess) return fail(std::string("rbascent_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_rbascent_last_error)
