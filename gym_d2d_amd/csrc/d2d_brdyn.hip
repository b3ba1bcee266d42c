// libd2d_brdyn.so (include/d2d_brdyn.h): sequential (Gauss-Seidel) best response on the RB half of the action, every turn of every
// round of every env in one launch.  gfx950.
//
// Shape: ONE workgroup per env - the dynamics couple exactly the links of one env - that stages the env once and then takes turns
// in LDS.  Staging is the power-control kernel's (d2d_powerctl.hip) minus the sort (d2d_same_rb.h), which nothing
// here needs: per link, by link index, the transmitter tuple (tx x, tx y, linear power x the folded tx column), the power-law head /
// tail, the receiver tuple (rx x, rx y, rx side of the path-loss constant, noise), the own-pair signal, the current rb, and the
// first allowed RB (-1: the link never takes a turn).  RB membership is a bitset word[w][r], bit j & 31 of word j / 32 = link j
// sits on RB r: neighbouring lanes read neighbouring words, a move is two bit flips, and a find-first-set loop over w = 0, 1, ...
// enumerates an RB's members in ascending j - the order the step adds them in.
//
// A link's turn: LANES OWN RBs (a lane with several of them loops).  Each lane walks its RB's members, the link itself left out,
// with the step's pair arithmetic on the same operands in the same order (d2d_step_device.h: fmaf(dx, dx, dy * dy), pair_gain,
// float products into ONE double accumulator in ascending j) and closes as d2d_bestrb.hip does ((float)acc, fmaf(acc, rx_pl,
// noise), precise_div, v_log_f32, one multiply), so every value is a value of the sensed block bit for bit.  The allowed values
// are reduced as 64-bit keys (order-preserving bits of the value, then the complement of r): the largest key is the highest
// value at the lowest r, which is what strictly-greater selection in ascending r gives; the lane of the link's own RB and the lane
// of its first allowed RB leave the own value and "the first value is NaN" (the one case in which the ascending scan ends on a
// NaN) beside the keys.  One barrier per turn; every thread then takes the same decision from the same words, and a move - two
// bit flips and rb[i] - is applied behind a second barrier that only turns that move pay.  A link whose last evaluation is newer
// than the env's last move is not evaluated again (its answer is "stay"), which ends the last, quiet round at its first turn.  No
// global access inside the turn loop, no atomics, no scratch, no [B][N][N] or [B][N][R] buffer, nothing that depends on scheduling.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_brdyn.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int BR_MAX_THREADS = 256;
constexpr int BR_MAX_WAVES = BR_MAX_THREADS / 64;
static_assert(D2D_BRDYN_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_BRDYN_LAW_POWER == LAW_POWER && D2D_BRDYN_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");

struct DynArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const unsigned* allowed;        // [N][words] or null
    const unsigned char* movable;   // [N] or null
    const unsigned char* env_mask;  // [B] or null
    int* rb_out;
    float* sinr;
    int* rounds;
    int* moves;
    unsigned char* converged;
    int D, N, R;
    int pow_k;
    int words;                      // ceil(R / 32)
    int W;                          // ceil(N / 32)
    int max_rounds;
    float min_gain;
    // byte offsets of the LDS arrays behind the transmitter tuples
    unsigned off_rx, off_hh, off_sig, off_rb, off_first, off_al, off_bits, off_red;
};

// dynamic LDS, by link index: tx float4[N] | rx float4[N] | hh float2[N] (power laws) | sig f32[n4] | rb i32[n4] | first i32[n4] |
// allowed u32[N * words] (with a mask) | bits u32[W][R] | keys u64[2][4], own f32[2], nan-first i32[2]

struct Lds {
    float4* tx; float4* rx; float2* hh; float* sig; int* rb; int* first; unsigned* al; unsigned* bits;
    unsigned long long* key; float* own; int* nanf;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const DynArgs& a) {
    Lds s;
    s.tx = reinterpret_cast<float4*>(smem);
    s.rx = reinterpret_cast<float4*>(smem + a.off_rx);
    s.hh = reinterpret_cast<float2*>(smem + a.off_hh);
    s.sig = reinterpret_cast<float*>(smem + a.off_sig);
    s.rb = reinterpret_cast<int*>(smem + a.off_rb);
    s.first = reinterpret_cast<int*>(smem + a.off_first);
    s.al = reinterpret_cast<unsigned*>(smem + a.off_al);
    s.bits = reinterpret_cast<unsigned*>(smem + a.off_bits);
    s.key = reinterpret_cast<unsigned long long*>(smem + a.off_red);
    s.own = reinterpret_cast<float*>(smem + a.off_red + 2u * BR_MAX_WAVES * 8u);
    s.nanf = reinterpret_cast<int*>(smem + a.off_red + 2u * BR_MAX_WAVES * 8u + 8u);
    return s;
}

// the sinr_db link i (receiver tuple rx, signal sig) has on RB r with the members the bitset holds, i itself left out
template <int MODE>
__device__ __forceinline__ float rb_sinr_db(const Lds& s, int r, int i, float4 rx, float sig, int R, int W, int pow_k) {
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int wi = i >> 5;
    const unsigned not_i = ~(1u << (i & 31));
    double acc = 0.0;
    for (int w = 0; w < W; ++w) {
        unsigned m = s.bits[w * R + r];
        m = w == wi ? m & not_i : m;                                     // j != i
        while (m) {
            const int j = (w << 5) + __builtin_ctz(m);
            m &= m - 1u;
            const float4 o = s.tx[j];
            const float dx = o.x - rx.x, dy = o.y - rx.y;
            const float d2 = fmaf(dx, dx, dy * dy);
            const float g = pair_gain<MODE>(d2, POWLAW ? s.hh[j] : make_float2(-1.0f, 0.0f), pow_k);
            const float term = o.z * g;                                  // simulator.py:97-101, linear mW
            acc += (double)term;
        }
    }
    const float accf = (float)acc;
    return 3.01029995663981195f * __builtin_amdgcn_logf(precise_div(sig, fmaf(accf, rx.z, rx.w)));
}

// bits that order as the floats do (no NaN comes here); -0 and +0, which compare equal, get the same bits
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}

__device__ __forceinline__ float ordered_value(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? o & 0x7FFFFFFFu : ~o);
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long k) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, d, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

template <int MODE>
__global__ __launch_bounds__(BR_MAX_THREADS) void brdyn_kernel(const DynArgs a) {
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
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        const int r = rb_row[j];
        int first = -1;                                                  // the first allowed RB of a link that takes turns
        if ((unsigned)r < (unsigned)R && (!a.movable || a.movable[j] != 0)) {
            if (!a.allowed) first = 0;
            for (int w = 0; a.allowed && w < words; ++w) {
                unsigned m = a.allowed[(size_t)j * (size_t)words + (size_t)w];
                if (w == words - 1 && (R & 31)) m &= (1u << (R & 31)) - 1u;
                if (m) { first = (w << 5) + __builtin_ctz(m); break; }
            }
        }
        s.tx[j] = make_float4(tx_x, tx_y, me_z, 0.0f);
        s.rx[j] = make_float4(rx_x, rx_y, rx_pl, noise);
        if (POWLAW) s.hh[j] = h;
        s.sig[j] = me_z * g * rx_pl * rx_lin;                            // own link: simulator.py:93, as the step forms it
        s.rb[j] = r;
        s.first[j] = first;
    }
    if (a.allowed)
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
            const float4 rx = s.rx[i];
            const float sig = s.sig[i];
            const int cur = __builtin_amdgcn_readfirstlane(s.rb[i]);
            unsigned long long key = 0ull;                               // 0: no candidate
            for (int r = tid; r < R; r += T) {
                const bool may = !a.allowed || ((s.al[i * words + (r >> 5)] >> (r & 31)) & 1u);
                if (!may && r != cur) continue;
                const float v = rb_sinr_db<MODE>(s, r, i, rx, sig, R, W, a.pow_k);
                if (r == cur) s.own[parity] = v;
                if (r == fa) s.nanf[parity] = v != v ? 1 : 0;
                if (may && v == v) {
                    const unsigned long long k = ((unsigned long long)ordered_bits(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)r);
                    key = k > key ? k : key;
                }
            }
            key = wave_max(key);
            if (lane == 0) s.key[parity * BR_MAX_WAVES + wave] = key;
            __syncthreads();                                             // the turn's one barrier: keys, own value, NaN flag
            unsigned long long top = s.key[parity * BR_MAX_WAVES];
            for (int w = 1; w < n_waves; ++w) {
                const unsigned long long k = s.key[parity * BR_MAX_WAVES + w];
                top = k > top ? k : top;
            }
            int to = -1;
            if (top != 0ull && s.nanf[parity] == 0) {
                const float gain = ordered_value((unsigned)(top >> 32)) - s.own[parity];
                const int r = (int)(0xFFFFFFFFu - (unsigned)top);
                to = gain > a.min_gain && r != cur ? r : -1;             // NaN gain: stays
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

    // ---- the step's plane for the RBs the dynamics stopped at, and the results
    const size_t row = b * (size_t)N;
    for (int i = tid; i < N; i += T) {
        const int r = s.rb[i];
        const float v = (unsigned)r < (unsigned)R ? rb_sinr_db<MODE>(s, r, i, s.rx[i], s.sig[i], R, W, a.pow_k) : __builtin_nanf("");
        a.rb_out[row + (size_t)i] = r;
        a.sinr[row + (size_t)i] = v;
    }
    if (tid == 0) {
        a.rounds[b] = rounds;
        a.moves[b] = moves;
        a.converged[b] = (unsigned char)fixed;
    }
}

}  // namespace

extern "C" int d2d_best_response_dynamics(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm,
                                          const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, int32_t law,
                                          int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs,
                                          const uint32_t* allowed, const uint8_t* movable, float min_gain_db, int32_t max_rounds,
                                          const uint8_t* env_mask, int32_t* rb_out, float* sinr_db, int32_t* rounds, int32_t* moves,
                                          uint8_t* converged, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_BRDYN_MAX_LINKS, n_rbs, D2D_BRDYN_MAX_RBS, n_dev)) return fail(why);
    if (max_rounds < 0 || max_rounds > D2D_BRDYN_MAX_ROUNDS)
        return fail("max_rounds must be in [0, " + std::to_string(D2D_BRDYN_MAX_ROUNDS) + "]");
    if (!(min_gain_db >= 0.0f)) return fail("min_gain_db must be >= 0 and not NaN");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !rb_out || !sinr_db || !rounds || !moves || !converged)
        return fail("null device pointer");
    const void* outs[5] = {rb_out, sinr_db, rounds, moves, converged};
    for (int x = 0; x < 5; ++x)
        for (int y = x + 1; y < 5; ++y)
            if (outs[x] == outs[y]) return fail("rb_out, sinr_db, rounds, moves and converged must be five arrays");
    DynArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.allowed = allowed; a.movable = movable; a.env_mask = env_mask;
    a.rb_out = rb_out; a.sinr = sinr_db; a.rounds = rounds; a.moves = moves; a.converged = converged;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k; a.max_rounds = max_rounds; a.min_gain = min_gain_db;
    a.words = (n_rbs + 31) / 32;
    a.W = (n_links + 31) / 32;
    const unsigned long long N = (unsigned long long)n_links, n4 = (N + 3ull) & ~3ull;
    // 64-bit until the limit is checked: 2048 links x 8192 RBs would be 2 MiB of bitset alone
    unsigned long long off = N * 16ull;
    a.off_rx = (unsigned)off; off += N * 16ull;
    a.off_hh = (unsigned)off; off += law == D2D_BRDYN_LAW_INV_SQUARE ? 0ull : (N * 8ull + 15ull) & ~15ull;
    a.off_sig = (unsigned)off; off += n4 * 4ull;
    a.off_rb = (unsigned)off; off += n4 * 4ull;
    a.off_first = (unsigned)off; off += n4 * 4ull;
    a.off_al = (unsigned)off; off += allowed ? (N * (unsigned long long)a.words * 4ull + 15ull) & ~15ull : 0ull;
    a.off_bits = (unsigned)off; off += ((unsigned long long)a.W * (unsigned long long)n_rbs * 4ull + 15ull) & ~15ull;
    a.off_red = (unsigned)off; off += 2ull * BR_MAX_WAVES * 8ull + 16ull;
    if (off > (unsigned long long)D2D_BRDYN_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                          std::to_string(D2D_BRDYN_MAX_LDS_BYTES) + " (D2D_BRDYN_MAX_LDS_BYTES) a workgroup can have");
    if (n_envs == 0) return 0;
    const unsigned lds = (unsigned)off;
    const unsigned threads = (unsigned)min(BR_MAX_THREADS, (n_rbs + 63) & ~63);      // lanes own RBs: no more waves than RBs need
    const dim3 grid((unsigned)n_envs);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_BRDYN_LAW_INV_SQUARE) e = launch(&brdyn_kernel<PL_INV_SQUARE>, grid, dim3(threads), lds, st, a);
    else if (law == D2D_BRDYN_LAW_POWER) e = launch(&brdyn_kernel<PL_POWER>, grid, dim3(threads), lds, st, a);
    else e = launch(&brdyn_kernel<PL_POWK>, grid, dim3(threads), lds, st, a);
    if (e != hipSuccess) return fail(std::string("brdyn_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_brdyn_last_error)
