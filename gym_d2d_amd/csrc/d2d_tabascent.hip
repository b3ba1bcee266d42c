// libd2d_tabascent.so (include/d2d_tabascent.h): d2d_rbascent.hip's cooperative local search on the RB half of the action - a link
// moves to the RB where the TOTAL capacity gains most, with SINR floors - on a dB path-loss TABLE by (tx link, rx link).  Two
// launches.  gfx950.
//
// (1) tabgain_kernel: ONE workgroup of 256 threads per env converts the env's N x N dB block into float32 linear gains in the
// caller's work space, each entry by the step's one-line conversion (d2d_evaltab.hip, entry_gain), and transposes it on the way:
// the table is (tx j, rx i), the work space RECEIVER-major, G[b][i][j], so the ascent's walk over the transmitters of one receiver
// runs along one row.  Tiles of 32 x 32 go through LDS (a row of 33 words: no bank conflict either way), so both the reads and the
// writes are 32 consecutive words.  An entry that fails x > -inf marks its thread; a ballot per wave, a word per wave in LDS, and
// thread 0 writes domain[b]: one writer per word, no atomics.
//
// (2) tabascent_kernel: d2d_rbascent.hip's shape and decisions.  ONE workgroup of at most 256 threads per env stages the env once -
// per link tz = linear power x the folded tx column, the closing tuple (own signal, noise, bandwidth, sensitivity), the floor, the
// current rb, the first allowed RB (-1: the link never takes a turn), the allowed words, and the membership bitset bits[w][r], bit
// j & 31 of word j / 32 = link j sits on RB r - and then takes turns in LDS.  A link's turn: LANES OWN RBs (a lane with several of
// them loops).  A lane walks group(r) u {i} as receivers in ascending link index and, per receiver, the same set as transmitters
// in ascending index, stepping from member to member by a 64-bit mask of the column's words that hold one, with
// evaltab_kernel's pair arithmetic - the float product tz[o] * G[m][o], one load from the work space - into TWO double
// accumulators: one takes link i's term at its place in the order, one skips it (adding 0.0, as the receiver's own slot does).
// Both close by evaltab_kernel's operations (rx_pl == 1.0f dropped: the denominator is accf + noise), so one walk gives With(r),
// Without(r), both SINRs of the floor test and D(r) = With(r) - Without(r); the lane of the link's own RB c gives D(c) the same
// way.  The choice is d2d_rbascent.hip's reduction of keys - the order-preserving image of the double D, then the complement of r
// in a second word - across the wave (d2d_wave_key.h) and across the waves through LDS.  One barrier per turn; every thread then
// takes the same decision from the same words, and a move - two bit flips and rb[i] - is applied behind a second barrier that only
// turns that move pay.  A link whose last evaluation is newer than the env's last move is not evaluated again: nothing it read has
// changed, so the unskipped loop would decide the same.  No global write and no atomic inside the turn loop, no scratch, nothing
// that depends on scheduling.  A lane with a long group does G^2 pair loads while the others wait.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <string>

#include "d2d_addon.h"
#include "d2d_step_device.h"
#include "d2d_tabascent.h"
#include "d2d_wave_key.h"

namespace {

using namespace d2d;

constexpr int TA_MAX_THREADS = 256;
constexpr int TA_MAX_WAVES = TA_MAX_THREADS / 64;
constexpr unsigned TA_RED_BYTES = 112u;                              // keys u64[2][4] | d_cur f64[2] | nr u32[2][4]
constexpr int CV_THREADS = 256;
constexpr int CV_WAVES = CV_THREADS / 64;
constexpr int CV_TILE = 32;
constexpr int CV_ROWS = CV_THREADS / CV_TILE;                        // tile rows one pass of the workgroup covers

// ---------------------------------------------------------------------------------------------------------------- the conversion
struct GainArgs {
    const void* table;              // [B][rows][N], float or double, (tx j, rx i)
    const unsigned char* env_mask;  // [B] or null
    float* gains;                   // [B][N][N], (rx i, tx j)
    int* domain;                    // [B]
    int N, rows;
};

template <typename T>
__global__ __launch_bounds__(CV_THREADS) void tabgain_kernel(const GainArgs a) {
    __shared__ float tile[CV_TILE][CV_TILE + 1];
    __shared__ unsigned wbad[CV_WAVES];
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N;
    const int tid = threadIdx.x, tx = tid & (CV_TILE - 1), ty = tid / CV_TILE;
    const T* tab = static_cast<const T*>(a.table) + b * (size_t)a.rows * (size_t)N;      // rows >= N, row N never read
    float* g = a.gains + b * (size_t)N * (size_t)N;
    const int tiles = (N + CV_TILE - 1) / CV_TILE;
    int bad = 0;
    for (int tj = 0; tj < tiles; ++tj) {
        for (int ti = 0; ti < tiles; ++ti) {
            // in: rows j of the table, 32 consecutive receivers i each
#pragma unroll
            for (int q = 0; q < CV_TILE; q += CV_ROWS) {
                const int j = tj * CV_TILE + ty + q, i = ti * CV_TILE + tx;
                if (j < N && i < N) {
                    const double x = (double)tab[(size_t)j * (size_t)N + (size_t)i];
                    if (!(x > -__builtin_huge_val())) bad = 1;
                    tile[ty + q][tx] = (float)exp2(-0.33219280948873623478703194294894 * x);
                }
            }
            __syncthreads();
            // out: rows i of the work space, 32 consecutive transmitters j each; the words read are the ones written above (the
            // two bounds are the same pair)
#pragma unroll
            for (int q = 0; q < CV_TILE; q += CV_ROWS) {
                const int i = ti * CV_TILE + ty + q, j = tj * CV_TILE + tx;
                if (i < N && j < N) g[(size_t)i * (size_t)N + (size_t)j] = tile[tx][ty + q];
            }
            __syncthreads();                                             // the next tile rewrites `tile`
        }
    }
    const unsigned long long any_bad = __builtin_amdgcn_ballot_w64(bad != 0);
    if ((tid & 63) == 0) wbad[tid >> 6] = any_bad != 0ull ? 1u : 0u;
    __syncthreads();
    if (tid == 0) {
        unsigned f = wbad[0];
#pragma unroll
        for (int w = 1; w < CV_WAVES; ++w) f |= wbad[w];
        a.domain[b] = (int)f;
    }
}

// -------------------------------------------------------------------------------------------------------------------- the ascent
struct Results {
    int* rb_out;
    float* sinr;
    float* cap;
    int* rounds;
    int* moves;
    unsigned char* converged;
};

struct TabAscentArgs {
    const float* gains;             // [B][N][N], (rx i, tx j): tabgain_kernel's
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [3][D]: tx_lin, rx_lin, noise_mw
    const float* cap_cols;          // [2][D]
    const unsigned* allowed;        // [N][words] or null
    const unsigned char* movable;   // [N] or null
    const float* floor;             // [N] or null
    const unsigned char* env_mask;  // [B] or null
    Results out;
    double min_gain;
    int D, N, R;
    int words;                      // ceil(R / 32) with an allowed mask, 0 without: the turn loop asks this word, not the pointer
    int W;                          // ceil(N / 32)
    int max_rounds;
    // byte offsets of the LDS arrays behind the closing tuples
    unsigned off_tz, off_fl, off_rb, off_al, off_bits, off_red;
};

// dynamic LDS, by link index: cl float4[N] (own signal, noise, bw_mhz, sens_db) | tz float[N] (linear power x tx constant) | fl
// float[N] (floor) | rb i32[n4] | first i32[n4] | allowed u32[N * words] (with a mask) | bits u32[W][R] | keys u64[2][4], d_cur
// f64[2], nr u32[2][4]

struct Lds {
    float4* cl; float* tz; float* fl; int* rb; int* first; unsigned* al; unsigned* bits;
    unsigned long long* key; double* dcur; unsigned* nr;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const TabAscentArgs& a) {
    Lds s;
    s.cl = reinterpret_cast<float4*>(smem);
    s.tz = reinterpret_cast<float*>(smem + a.off_tz);
    s.fl = reinterpret_cast<float*>(smem + a.off_fl);
    s.rb = reinterpret_cast<int*>(smem + a.off_rb);
    s.first = s.rb + ((a.N + 3) & ~3);
    s.al = reinterpret_cast<unsigned*>(smem + a.off_al);
    s.bits = reinterpret_cast<unsigned*>(smem + a.off_bits);
    s.key = reinterpret_cast<unsigned long long*>(smem + a.off_red);
    s.dcur = reinterpret_cast<double*>(smem + a.off_red + 2u * TA_MAX_WAVES * 8u);
    s.nr = reinterpret_cast<unsigned*>(smem + a.off_red + 2u * TA_MAX_WAVES * 8u + 16u);
    return s;
}

// evaltab_kernel's closing operations (d2d_evaltab.hip; d2d_step.hip, pass 2, with rx_pl == 1.0f) on the interference sum acc of a
// receiver with the tuple cl (own signal, noise, bw_mhz, sens_db)
__device__ __forceinline__ void closing(float4 cl, double acc, float& sinr_db, float& cap) {
    const float accf = (float)acc;
    const float sinr_lin = precise_div(cl.x, accf + cl.y);
    sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
    const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
    const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
    const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
    const bool ok = sinr_db > cl.w;                                      // simulator.py:123,149
    cap = ok ? cl.z * sh : 0.0f;                                         // simulator.py:150-151
}

// The members of RB r, link i forced in (bit_i = 0: nobody), in ascending link index: d2d_rbascent.hip's member stepping.  `nz`
// marks the words of the RB's column that hold a member, so that a lane steps from member to member.
struct Members {
    unsigned long long nz;
    unsigned cur;
    int w;
};
static_assert(D2D_TABASCENT_MAX_LINKS <= 64 * 32, "one bit of a 64-bit word per word of the column");

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

// sinr_db and capacity_mbps of link m on RB r with the members the bitset holds (m among them): evaltab_kernel's walk along row m
// of the env's gain block g.  A link on no RB (r outside [0, R)) gets its SNR, as evaltab_kernel gives it.
__device__ __forceinline__ void link_planes(const Lds& s, const float* g, int m, int r, int N, int R, int W, float& sinr_db, float& cap) {
    const float* row = g + (size_t)m * (size_t)N;
    double acc = 0.0;
    if ((unsigned)r < (unsigned)R) {
        Members it = {nonzero_words(s, r, R, W, -1, 0u), 0u, 0};
        int o;
        while (next_member(s, it, r, R, -1, 0u, o)) {
            const float term = s.tz[o] * row[o];                         // o < N: a bit of the bitset is a link
            acc += o != m ? (double)term : 0.0;
        }
    }
    closing(s.cl[m], acc, sinr_db, cap);
}

// One walk over group(r) u {i}: with = With(r), without = Without(r), adm = r is admissible for link i, whose sinr_db on its own RB
// is sinr_cur_i (read only where link i has a floor).
__device__ __forceinline__ void rb_walk(const Lds& s, const float* g, int r, int i, float sinr_cur_i, int N, int R, int W, double& with,
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
        const float* row = g + (size_t)m * (size_t)N;
        double acc_with = 0.0, acc_without = 0.0;
        Members txs = {nz, 0u, 0};
        int o;
        while (next_member(s, txs, r, R, wi, bit_i, o)) {
            const float term = s.tz[o] * row[o];
            const double dt = o != m ? (double)term : 0.0;               // the receiver's own slot adds 0.0
            acc_with += dt;
            acc_without += o != i ? dt : 0.0;                            // link i not on r: its slot adds 0.0
        }
        const float4 cl = s.cl[m];
        float sinr_with, cap_with, sinr_without, cap_without;
        closing(cl, acc_with, sinr_with, cap_with);
        closing(cl, acc_without, sinr_without, cap_without);
        with += (double)cap_with;
        without += m != i ? (double)cap_without : 0.0;
        const float fl = s.fl[m];
        const float before = m == i ? sinr_cur_i : sinr_without;         // sinr^c_m: link i where it is now
        adm = adm && (!(fl > -INFINITY) || sinr_with >= fl || before < fl);          // float32, NaN compares false
    }
}

// The six result pointers, read from the kernel-argument segment BEHIND the turn loop (d2d_rbascent.hip's device): taken from the
// argument struct they are loaded with the rest at the kernel's start and held in twelve scalar registers across the loop, more
// than the kernel has without spilling.  The empty statement keeps the loads below it.
__device__ __forceinline__ Results results_behind_the_loop() {
    typedef __attribute__((address_space(4))) const unsigned char* KernargBytes;
    typedef __attribute__((address_space(4))) const unsigned long long* KernargWords;
    KernargBytes ka = (KernargBytes)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const KernargWords w = (KernargWords)(ka + offsetof(TabAscentArgs, out));
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

__global__ __launch_bounds__(TA_MAX_THREADS) void tabascent_kernel(const TabAscentArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D, W = a.W, words = a.words;
    const int T = (int)blockDim.x, n_waves = T >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* g = a.gains + b * (size_t)N * (size_t)N;               // this env's gain block, (rx, tx)

    // ---- per-link constants by link index, and an empty bitset
    for (int j = tid; j < N; j += T) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float tz = pow10_tenth(pwr_row[j]) * a.cols[txd];          // the step's tuple.z (d2d_step.hip, pass 1)
        const float rx_lin = a.cols[D + rxd], noise = a.cols[2 * D + rxd];
        const float own = g[(size_t)j * (size_t)N + (size_t)j];
        s.tz[j] = tz;
        s.cl[j] = make_float4(tz * own * rx_lin, noise, a.cap_cols[txd], a.cap_cols[D + rxd]);   // own link: as evaltab_kernel forms it
        s.fl[j] = a.floor ? a.floor[j] : -INFINITY;
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
            if (s.fl[i] > -INFINITY) {
                float cap_cur;
                link_planes(s, g, i, cur, N, R, W, sinr_cur, cap_cur);
            }
            unsigned long long key = 0ull;                               // 0: no candidate
            unsigned key_r = 0u;
            for (int r = tid; r < R; r += T) {
                const bool may = words == 0 || ((s.al[i * words + (r >> 5)] >> (r & 31)) & 1u);
                if (!may && r != cur) continue;
                double with, without;
                bool adm;
                rb_walk(s, g, r, i, sinr_cur, N, R, W, with, without, adm);
                const double d = with - without;
                if (r == cur) { s.dcur[parity] = d; continue; }
                const unsigned long long k = ordered_image(d);
                if (adm && k > 1ull && k > key) { key = k; key_r = (unsigned)r; }       // ascending r: equal images keep the lowest
            }
            // the largest image of the wave, then the lowest r among the lanes that hold it
            const unsigned long long top_w = wave_reduce<true>(key);
            const unsigned long long nr_w = wave_reduce<true>(key == top_w && key != 0ull ? (unsigned long long)(0xFFFFFFFFu - key_r) : 0ull);
            if (lane == 0) {
                s.key[parity * TA_MAX_WAVES + wave] = top_w;
                s.nr[parity * TA_MAX_WAVES + wave] = (unsigned)nr_w;
            }
            __syncthreads();                                             // the turn's one barrier: keys, their RBs, D(c)
            unsigned long long top = s.key[parity * TA_MAX_WAVES];
            unsigned nr = s.nr[parity * TA_MAX_WAVES];
            for (int w = 1; w < n_waves; ++w) {
                const unsigned long long k = s.key[parity * TA_MAX_WAVES + w];
                const unsigned n = s.nr[parity * TA_MAX_WAVES + w];
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

    // ---- evaltab_kernel's planes for the RBs the ascent stopped at, every link, and the results
    const Results out = results_behind_the_loop();
    const size_t row = b * (size_t)N;
    for (int i = tid; i < N; i += T) {
        const int r = s.rb[i];
        float sinr, cap;
        link_planes(s, g, i, r, N, R, W, sinr, cap);
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

unsigned long long up16(unsigned long long x) { return (x + 15ull) & ~15ull; }

}  // namespace

extern "C" int d2d_table_rb_ascent(const void* table, int32_t table_dtype, int32_t table_rows, const int32_t* rb, const int32_t* pwr_dbm,
                                   const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols,
                                   int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const uint32_t* allowed,
                                   const uint8_t* movable, const float* floor_db, double min_gain_mbps, int32_t max_rounds,
                                   const uint8_t* env_mask, float* gains, int32_t* rb_out, float* sinr_db, float* capacity_mbps,
                                   int32_t* rounds, int32_t* moves, uint8_t* converged, int32_t* domain, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_TABASCENT_MAX_LINKS, n_rbs, D2D_TABASCENT_MAX_RBS, n_dev)) return fail(why);
    if (max_rounds < 1 || max_rounds > D2D_TABASCENT_MAX_ROUNDS)
        return fail("max_rounds must be in [1, " + std::to_string(D2D_TABASCENT_MAX_ROUNDS) + "]");
    if (!std::isfinite(min_gain_mbps) || min_gain_mbps < 0.0) return fail("min_gain_mbps must be finite and >= 0");
    if (table_dtype != D2D_TABASCENT_F32 && table_dtype != D2D_TABASCENT_F64) return fail("table_dtype must be D2D_TABASCENT_F32 or D2D_TABASCENT_F64");
    if (table_rows != n_links && table_rows != n_links + 1) return fail("table_rows must be n_links or n_links + 1");
    if (!table || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !gains || !rb_out || !sinr_db || !capacity_mbps ||
        !rounds || !moves || !converged || !domain)
        return fail("null device pointer");
    const void* outs[8] = {rb_out, sinr_db, capacity_mbps, rounds, moves, converged, domain, gains};
    for (int x = 0; x < 8; ++x)
        for (int y = x + 1; y < 8; ++y)
            if (outs[x] == outs[y]) return fail("rb_out, sinr_db, capacity_mbps, rounds, moves, converged, domain and gains must be eight arrays");
    TabAscentArgs a;
    a.gains = gains; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols; a.cap_cols = cap_cols;
    a.allowed = allowed; a.movable = movable; a.floor = floor_db; a.env_mask = env_mask;
    a.out.rb_out = rb_out; a.out.sinr = sinr_db; a.out.cap = capacity_mbps; a.out.rounds = rounds; a.out.moves = moves;
    a.out.converged = converged;
    a.min_gain = min_gain_mbps;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.max_rounds = max_rounds;
    a.words = allowed ? (n_rbs + 31) / 32 : 0;
    a.W = (n_links + 31) / 32;
    const unsigned long long N = (unsigned long long)n_links, n4 = (N + 3ull) & ~3ull;
    // 64-bit until the limit is checked: 2048 links x 8192 RBs would be 2 MiB of bitset alone
    unsigned long long off = N * 16ull;                                  // cl
    a.off_tz = (unsigned)off; off += up16(N * 4ull);
    a.off_fl = (unsigned)off; off += up16(N * 4ull);
    a.off_rb = (unsigned)off; off += 2ull * n4 * 4ull;                   // rb, first
    a.off_al = (unsigned)off; off += up16(N * (unsigned long long)a.words * 4ull);
    a.off_bits = (unsigned)off; off += up16((unsigned long long)a.W * (unsigned long long)n_rbs * 4ull);
    a.off_red = (unsigned)off; off += TA_RED_BYTES;
    if (off > (unsigned long long)D2D_TABASCENT_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_TABASCENT_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    GainArgs c;
    c.table = table; c.env_mask = env_mask; c.gains = gains; c.domain = domain; c.N = n_links; c.rows = table_rows;
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (table_dtype == D2D_TABASCENT_F64) e = launch(&tabgain_kernel<double>, grid, dim3(CV_THREADS), 0u, st, c);
    else e = launch(&tabgain_kernel<float>, grid, dim3(CV_THREADS), 0u, st, c);
    if (e != hipSuccess) return fail(std::string("tabgain_kernel launch: ") + hipGetErrorString(e));
    const unsigned lds = (unsigned)off;
    const unsigned threads = (unsigned)min(TA_MAX_THREADS, (n_rbs + 63) & ~63);     // lanes own RBs: no more waves than RBs need
    e = launch(&tabascent_kernel, grid, dim3(threads), lds, st, a);
    if (e != hipSuccess) return fail(std::string("tabascent_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_tabascent_last_error)
