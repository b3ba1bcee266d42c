// libd2d_deviate.so (include/d2d_deviate.h): the unilateral-deviation gains of every selected link over every (RB, power) action -
// what the env's total capacity would gain if that link alone had played it, with SINR floors - as a table, or reduced to every
// link's best deviation and the env's regret.  gfx950.
//
// Shape: the grid is (env, chunk of selected links), at most 256 threads per workgroup.  Nothing here is sequential, so an env is
// served by as many workgroups as its selection has chunks.  Each workgroup stages the env once, by link index, no sort, as
// d2d_goodput.hip does: one 80-byte record per link - the transmitter tuple (tx x, tx y, linear power x the folded tx column c0,
// and c0 itself: a level q sends at pow10_tenth(q) * c0), the receiver tuple (rx x, rx y, rx side of the path-loss constant,
// noise), the closing tuple (own-pair gain, rx gain, bandwidth, sensitivity), the power-law pair, the held rb and power, p_min and
// the levels - then the allowed words and the membership bitset bits[w][r], bit j & 31 of word j / 32 = link j sits on RB r.
//
// THE HELD STATE s IS EVALUATED ONCE, not per entry: behind the bitset every link gets evaluate_kernel's two values for s, and the
// record keeps cap_m(s) and the link's EFFECTIVE floor - its floor, or -inf where sinr_m(s) < floor already ("a link already under
// its floor constrains nothing"; a NaN sinr compares false and keeps the floor).  Groups do not interact, so cap_m(s) of a member of
// r is its value "without i" for every link i that is not on r: Without(r) is a sum of stored values, in ascending link index.
//
// Pass 1, one thread per link of the chunk: what link i's LEAVING does to group(c) - one walk of the state "i gone" gives
// Without(c); With(c,p) is the sum of the stored cap(s) over group(c); so D(c,p) - into LDS, once per link, not per entry.
//
// Pass 2: every entry (link, r, l) is one call of one walk of ONE state, s^(r,q): the members of group(r) and link i as receivers in
// ascending link index and, per receiver, the same set as transmitters in ascending index, with evaluate_kernel's pair arithmetic
// on the same operands in the same order (d2d_evaluate.hip) into one double accumulator.  Link i's slot takes its term at its place
// in the order (its term is never added to a finished sum), the receiver's own slot adds 0.0, and the sum closes by
// evaluate_kernel's operations: one closing per member, where two states would take two.  The same loop adds the members' stored
// cap(s) into Without(r) and compares sinr(s^(r,q)) with the effective floors.
//
// The table kernel deals the chunk's entries FLAT over the threads: entry e of the chunk is (link e / (R L), r, l) with l fastest,
// which is the order the table has in memory, so consecutive lanes store consecutive floats and the table leaves in full rows.  The
// levels of one (link, r) are adjacent lanes: they run the same walk in lockstep - every LDS read a broadcast, the pair gain one
// instruction for all of them - and differ in the linear power alone.
//
// The best kernel takes the chunk's links one after another; a link's (r, l) entries are dealt over the threads, and the choice
// is d2d_goodput.hip's reduction of two 64-bit keys - the order-preserving image of the double gain (0: no open entry, 1: a NaN),
// then the complement of l << 16 | r - across the wave by data-parallel primitives (d2d_wave_key.h) and across the waves through
// LDS, one barrier per link.  A second kernel, one workgroup per env, writes the rows of the links that are not selected and
// reduces gain_link to regret and leader by the same keys.  No read-modify-write on memory another thread owns, no scratch, nothing
// that depends on scheduling.
// The members of a column are the copies of d2d_rbascent.hip's helpers, as d2d_goodput.hip's are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "d2d_addon.h"
#include "d2d_deviate.h"
#include "d2d_step_device.h"
#include "d2d_wave_key.h"

namespace {

using namespace d2d;

constexpr int DV_MAX_THREADS = 256;
constexpr int DV_MAX_WAVES = DV_MAX_THREADS / 64;
constexpr int DV_CHUNK = DV_MAX_THREADS;                             // the links of one chunk, at most: pass 1 gives each a thread
constexpr int DV_CHUNK_ENTRIES = 4096;                               // a chunk takes links until it has about this many entries
constexpr unsigned DV_TAIL_BYTES = 5216u;                            // wo f64[256] | dcur f64[256] | sel i32[256] | keys u64[2][4] | nr u32[2][4]
static_assert(D2D_DEVIATE_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_DEVIATE_LAW_POWER == LAW_POWER && D2D_DEVIATE_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_DEVIATE_MAX_RBS <= (1 << 16) && D2D_DEVIATE_MAX_LEVELS <= (1 << 15), "the second key packs the level above 16 bits of RB");
static_assert(DV_TAIL_BYTES == DV_CHUNK * (8u + 8u + 4u) + 2u * DV_MAX_WAVES * (8u + 4u), "the header's 5216");

struct DeviateArgs {
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
    const int* links;               // [M]
    const unsigned* allowed;        // [N][words] or null
    const float* floor;             // [N] or null
    const unsigned char* env_mask;  // [B] or null
    float* table;                   // [B][M][R][L]            (the table kernel)
    int* rb_out;                    // [B][N]                  (the best kernel, and the three below)
    int* pwr_out;
    double* gain_link;
    double min_gain;
    int D, N, R, M, L;
    int pow_k;
    int words;                      // ceil(R / 32) with an allowed mask, 0 without
    int W;                          // ceil(N / 32)
    int chunk;                      // the selected links of one workgroup
    // byte offsets of the LDS arrays behind the link records
    unsigned off_al, off_bits, off_tail;
};

// dynamic LDS: link Link[N] | allowed u32[N * words] (with a mask) | bits u32[W][R] | the tail (DV_TAIL_BYTES)
struct Link {
    float4 tx;                      // tx x, tx y, linear power x c0, c0
    float4 rxa;                     // rx x, rx y, rx_pl, noise
    float4 rxb;                     // own-pair gain, rx_lin, bw_mhz, sens_db
    float2 hh;                      // the power-law pair
    float floor;                    // the effective floor: -inf where the link has none or is under it in the held state
    int rb;
    int p, pmin, levels;            // levels: min(max(L_i, 0), L)
    float cap;                      // cap_m(s): evaluate_kernel's capacity in the held state
};
static_assert(sizeof(Link) == 80, "the header's 80 n_links");

struct Lds {
    Link* link; unsigned* al; unsigned* bits; double* wo; double* dcur; int* sel; unsigned long long* key; unsigned* nr;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const DeviateArgs& a) {
    Lds s;
    s.link = reinterpret_cast<Link*>(smem);
    s.al = reinterpret_cast<unsigned*>(smem + a.off_al);
    s.bits = reinterpret_cast<unsigned*>(smem + a.off_bits);
    unsigned char* tail = smem + a.off_tail;
    s.wo = reinterpret_cast<double*>(tail);
    s.dcur = s.wo + DV_CHUNK;
    s.sel = reinterpret_cast<int*>(s.dcur + DV_CHUNK);
    s.key = reinterpret_cast<unsigned long long*>(s.sel + DV_CHUNK);
    s.nr = reinterpret_cast<unsigned*>(s.key + 2 * DV_MAX_WAVES);
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

// the gain of the pair (transmitter o, the receiver of tuple rx): evaluate_kernel's
template <int MODE>
__device__ __forceinline__ float pair_g(const Lds& s, int o, float4 t, float4 rx, int pow_k) {
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const float dx = t.x - rx.x, dy = t.y - rx.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    return pair_gain<MODE>(d2, POWLAW ? s.link[o].hh : make_float2(-1.0f, 0.0f), pow_k);
}

// The members of RB r, link i forced in, in ascending link index.  `nz` marks the words of the RB's column that hold a member, so
// that a thread steps from member to member (d2d_rbascent.hip).
struct Members {
    unsigned long long nz;
    unsigned cur;
    int w;
};
static_assert(D2D_DEVIATE_MAX_LINKS <= 64 * 32, "one bit of a 64-bit word per word of the column");

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

// One walk over group(r) u {i} in the state that has link i on r at the linear power z_i (in_a) or on no RB (!in_a: "i gone").
// sum_a: the double sum, in ascending link index, of (double)cap_m of that state over the members it has on r.  sum_s: the same sum
// of the stored cap_m(s) over group(r), link i counted iff count_me (it is on r in the held state).  adm: every member m that the
// state has on r passes sinr_m >= its effective floor, float32, NaN compares false (no floor: -inf).
template <int MODE>
__device__ __forceinline__ void walk(const Lds& s, int r, int i, float z_i, bool in_a, bool count_me, int R, int W, int pow_k,
                                     double& sum_a, double& sum_s, bool& adm) {
    const int wi = i >> 5;
    const unsigned bit_i = 1u << (i & 31);
    sum_a = 0.0;
    sum_s = 0.0;
    adm = true;
    const unsigned long long nz = nonzero_words(s, r, R, W, wi, bit_i);
    Members rxs = {nz, 0u, 0};
    int m;
    while (next_member(s, rxs, r, R, wi, bit_i, m)) {
        const float4 rx = s.link[m].rxa;
        double acc = 0.0;
        Members txs = {nz, 0u, 0};
        int o;
        while (next_member(s, txs, r, R, wi, bit_i, o)) {
            const float4 t = s.link[o].tx;
            const float g = pair_g<MODE>(s, o, t, rx, pow_k);
            const bool is_i = o == i;
            const float term = (is_i ? z_i : t.z) * g;                   // simulator.py:97-101, linear mW
            acc += o != m && (!is_i || in_a) ? (double)term : 0.0;       // the receiver's own slot adds 0.0; so does link i's where it is gone
        }
        const bool me = m == i;
        float sinr_a, cap_a;
        closing(rx, s.link[m].rxb, me ? z_i : s.link[m].tx.z, acc, sinr_a, cap_a);
        sum_a += !me || in_a ? (double)cap_a : 0.0;
        sum_s += !me || count_me ? (double)s.link[m].cap : 0.0;
        const float fl = s.link[m].floor;
        adm = adm && ((me && !in_a) || !(fl > -INFINITY) || sinr_a >= fl);       // float32, NaN compares false
    }
}

// The entry (r, level l) of the chunk's link t: is it open, is it the held action, and its double gain.
template <int MODE>
__device__ __forceinline__ void entry(const Lds& s, const DeviateArgs& a, int t, int r, int l, bool& open, bool& held, double& gain) {
    open = false;
    held = false;
    gain = 0.0;
    const int i = s.sel[t];
    if (i < 0) return;                                                   // no link of this env, or a link on no RB
    const Link& me = s.link[i];
    const int cur = me.rb;
    if (l >= me.levels) return;
    const bool stays = r == cur;
    if (!stays && a.words != 0 && !((s.al[i * a.words + (r >> 5)] >> (r & 31)) & 1u)) return;
    const int q = me.pmin + l;
    const float4 tx = me.tx;
    const float z_a = pow10_tenth(q) * tx.w;
    double sum_a, sum_s;
    bool adm;
    walk<MODE>(s, r, i, z_a, true, false, a.R, a.W, a.pow_k, sum_a, sum_s, adm);
    const double d = sum_a - (stays ? s.wo[t] : sum_s);                  // D(r,q) = With(r,q) - Without(r)
    gain = d - s.dcur[t];
    held = stays && q == me.p;
    open = held || adm;
}

// The order-preserving image of a double in the unsigned 64-bit words (d2d_rbascent.hip): a < b as doubles iff image(a) <
// image(b), above the two words the choice keeps for itself - 0 (no entry) and 1 (a NaN).  -0.0 takes the image of +0.0.
__device__ __forceinline__ unsigned long long ordered_image(double t) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(t + 0.0);
    return t != t ? 1ull : ((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}

__device__ __forceinline__ double image_value(unsigned long long o) {
    return __longlong_as_double((long long)((o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o));
}

template <int MODE, bool BEST>
__global__ __launch_bounds__(DV_MAX_THREADS) void deviate_kernel(const DeviateArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;                        // the whole workgroup, before its first barrier
    const int N = a.N, R = a.R, D = a.D, W = a.W, words = a.words, L = a.L;
    const int T = (int)blockDim.x;
    const int tid = threadIdx.x;
    const Lds s = carve_lds(smem, a);
    const size_t row = b * (size_t)N;
    const int* rb_row = a.rb + row;
    const int* pwr_row = a.pwr + row;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;
    const int k0 = (int)blockIdx.y * a.chunk;                            // the chunk: selected links k0 .. k0 + nl - 1
    const int nl = min(a.chunk, a.M - k0);

    // ---- per-link constants by link index, an empty bitset, the chunk's links
    for (int j = tid; j < N; j += T) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        const float tx_x = px[txd], tx_y = py[txd], rx_x = px[rxd], rx_y = py[rxd];
        const float c0 = a.cols[txd];
        const int held = pwr_row[j];
        const float me_z = pow10_tenth(held) * c0;                       // the step's tuple.z (d2d_step.hip, pass 1)
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
        const float bw_mhz = a.cap_cols[txd], sens = a.cap_cols[D + rxd];
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g_own = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        const int lo = a.p_min[j], hi = a.p_max[j];
        const long long lv = (long long)hi - lo + 1;
        Link& k = s.link[j];
        k.tx = make_float4(tx_x, tx_y, me_z, c0);
        k.rxa = make_float4(rx_x, rx_y, rx_pl, noise);
        k.rxb = make_float4(g_own, rx_lin, bw_mhz, sens);
        k.hh = h;
        k.floor = a.floor ? a.floor[j] : -INFINITY;                     // made effective behind the bitset
        k.rb = rb_row[j];
        k.p = held;
        k.pmin = lo;
        k.levels = (int)min(max(lv, 0ll), (long long)L);
    }
    for (int k = tid; k < N * words; k += T) s.al[k] = a.allowed[k];
    for (int k = tid; k < W * R; k += T) s.bits[k] = 0u;
    // the slots of the waves a launch does not have stay 0 - no entry - so that every combine below reads all four
    if (tid < 2 * DV_MAX_WAVES) { s.key[tid] = 0ull; s.nr[tid] = 0u; }
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
    // ---- the held state, once: cap_m(s), and the floor of a link that is under it already constrains nothing.  (A thread writes
    // its own link's two words, which no walk of another thread reads here.)
    for (int j = tid; j < N; j += T) {
        float sinr, cap;
        link_planes<MODE>(s, j, s.link[j].rb, R, W, a.pow_k, sinr, cap);
        const float fl = s.link[j].floor;
        s.link[j].cap = cap;
        s.link[j].floor = sinr < fl ? -INFINITY : fl;                    // NaN compares false: the floor stays
    }
    __syncthreads();

    // ---- pass 1: what leaving c does, once per link of the chunk.  sel[t] = -1: every entry of the link is closed
    for (int t = tid; t < nl; t += T) {
        const int i = a.links[k0 + t];
        int sel = -1;
        double wo = 0.0, dcur = 0.0;
        if ((unsigned)i < (unsigned)N) {
            const int cur = s.link[i].rb;
            if ((unsigned)cur < (unsigned)R) {
                double with_now;
                bool adm;
                walk<MODE>(s, cur, i, s.link[i].tx.z, false, true, R, W, a.pow_k, wo, with_now, adm);
                dcur = with_now - wo;                                    // D(c,p) = With(c,p) - Without(c)
                sel = i;
            }
        }
        s.sel[t] = sel;
        s.wo[t] = wo;
        s.dcur[t] = dcur;
    }
    __syncthreads();

    // ---- pass 2
    const int E = R * L;                                                 // the entries of one link
    if (!BEST) {
        // the chunk's entries, flat: consecutive lanes own consecutive (r, l), the order of the table's memory
        float* out = a.table + (b * (size_t)a.M + (size_t)k0) * (size_t)E;
        const int total = nl * E;
        for (int e = tid; e < total; e += T) {
            const int t = e / E, rem = e - t * E;
            const int r = rem / L, l = rem - r * L;
            bool open, held;
            double gain;
            entry<MODE>(s, a, t, r, l, open, held, gain);
            out[e] = open ? (float)gain : -INFINITY;                    // rounded once; a NaN stays NaN
        }
    } else {
        const int lane = tid & 63, wave = tid >> 6;
        int parity = 0;
        for (int t = 0; t < nl; ++t) {
            unsigned long long key = 0ull;                               // 0: no open entry
            unsigned key_lr = 0u;
            for (int e = tid; e < E; e += T) {
                const int r = e / L, l = e - r * L;
                bool open, held;
                double gain;
                entry<MODE>(s, a, t, r, l, open, held, gain);
                const unsigned long long kd = ordered_image(gain);
                const unsigned lr = 0xFFFFFFFFu - (((unsigned)l << 16) | (unsigned)r);
                if (open && !held && kd > 1ull && (kd > key || (kd == key && lr > key_lr))) { key = kd; key_lr = lr; }
            }
            // the largest gain of the wave, then the lowest (power, RB) among the lanes that hold it
            const unsigned long long top_w = wave_reduce<true>(key);
            const unsigned long long nr_w = wave_reduce<true>(key == top_w && key != 0ull ? (unsigned long long)key_lr : 0ull);
            if (lane == 0) {
                s.key[parity * DV_MAX_WAVES + wave] = top_w;
                s.nr[parity * DV_MAX_WAVES + wave] = (unsigned)nr_w;
            }
            __syncthreads();                                             // the link's one barrier: the keys and their (power, RB)
            if (tid == 0) {
                unsigned long long top = s.key[parity * DV_MAX_WAVES];
                unsigned nr = s.nr[parity * DV_MAX_WAVES];
#pragma unroll
                for (int w = 1; w < DV_MAX_WAVES; ++w) {
                    const unsigned long long k = s.key[parity * DV_MAX_WAVES + w];
                    const unsigned n = s.nr[parity * DV_MAX_WAVES + w];
                    const bool better = k > top || (k == top && n > nr);
                    top = better ? k : top;
                    nr = better ? n : nr;
                }
                const int i = a.links[k0 + t];
                if ((unsigned)i < (unsigned)N) {
                    int to_rb = s.link[i].rb, to_p = s.link[i].p;
                    double g = 0.0;
                    if (top != 0ull && image_value(top) > a.min_gain) {
                        const unsigned lr = 0xFFFFFFFFu - nr;
                        to_rb = (int)(lr & 0xFFFFu);
                        to_p = s.link[i].pmin + (int)(lr >> 16);
                        g = image_value(top);
                    }
                    a.rb_out[row + (size_t)i] = to_rb;
                    a.pwr_out[row + (size_t)i] = to_p;
                    a.gain_link[row + (size_t)i] = g;
                }
            }
            parity ^= 1;
        }
    }
}

struct RegretArgs {
    const int* rb;                  // [B][N]
    const int* pwr;
    const int* links;               // [M]
    const unsigned char* env_mask;  // [B] or null
    int* rb_out;                    // [B][N]
    int* pwr_out;
    double* gain_link;
    double* regret;                 // [B]
    int* leader;
    int N, M;
};

// One workgroup per env, behind the best kernel on the stream: the links that are not selected keep (rb, pwr) with gain 0.0, and
// regret / leader are the largest gain_link above 0.0 and the lowest link that has it.
__global__ __launch_bounds__(DV_MAX_THREADS) void regret_kernel(const RegretArgs a) {
    __shared__ unsigned char selected[D2D_DEVIATE_MAX_LINKS];
    __shared__ unsigned long long keys[DV_MAX_WAVES];
    __shared__ unsigned nrs[DV_MAX_WAVES];
    const size_t b = blockIdx.x;
    if (a.env_mask && a.env_mask[b] == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N;
    const size_t row = b * (size_t)N;
    for (int j = tid; j < N; j += DV_MAX_THREADS) selected[j] = 0;
    __syncthreads();
    for (int k = tid; k < a.M; k += DV_MAX_THREADS) {
        const int i = a.links[k];
        if ((unsigned)i < (unsigned)N) selected[i] = 1;
    }
    __syncthreads();
    unsigned long long key = 0ull;                                       // 0: nobody would move
    unsigned key_n = 0u;
    for (int j = tid; j < N; j += DV_MAX_THREADS) {
        double g = 0.0;
        if (selected[j]) {
            g = a.gain_link[row + (size_t)j];
        } else {
            a.rb_out[row + (size_t)j] = a.rb[row + (size_t)j];
            a.pwr_out[row + (size_t)j] = a.pwr[row + (size_t)j];
            a.gain_link[row + (size_t)j] = 0.0;
        }
        const unsigned long long kd = ordered_image(g);
        if (g > 0.0 && kd > key) { key = kd; key_n = 0xFFFFFFFFu - (unsigned)j; }      // ascending j: equal images keep the lowest
    }
    const unsigned long long top_w = wave_reduce<true>(key);
    const unsigned long long n_w = wave_reduce<true>(key == top_w && key != 0ull ? (unsigned long long)key_n : 0ull);
    if (lane == 0) { keys[wave] = top_w; nrs[wave] = (unsigned)n_w; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long top = keys[0];
        unsigned nr = nrs[0];
#pragma unroll
        for (int w = 1; w < DV_MAX_WAVES; ++w) {
            const bool better = keys[w] > top || (keys[w] == top && nrs[w] > nr);
            top = better ? keys[w] : top;
            nr = better ? nrs[w] : nr;
        }
        a.regret[b] = top != 0ull ? image_value(top) : 0.0;
        a.leader[b] = top != 0ull ? (int)(0xFFFFFFFFu - nr) : -1;
    }
}

// The checks and the launch geometry both entry points share; 0, or non-zero with the message set.
int prepare(DeviateArgs& a, const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
            const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
            int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max, const int32_t* links, int32_t n_sel,
            int32_t n_levels, const uint32_t* allowed, const float* floor_db, const uint8_t* env_mask, unsigned& lds) {
    if (const char* why = check_sizes(n_envs, n_links, D2D_DEVIATE_MAX_LINKS, n_rbs, D2D_DEVIATE_MAX_RBS, n_dev)) return fail(why);
    if (n_sel < 1 || n_sel > n_links) return fail("n_sel must be in [1, n_links]");
    if (n_levels < 1 || n_levels > D2D_DEVIATE_MAX_LEVELS)
        return fail("n_levels must be in [1, " + std::to_string(D2D_DEVIATE_MAX_LEVELS) + "]");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !p_min || !p_max || !links)
        return fail("null device pointer");
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.p_min = p_min; a.p_max = p_max; a.links = links; a.allowed = allowed; a.floor = floor_db; a.env_mask = env_mask;
    a.table = nullptr; a.rb_out = nullptr; a.pwr_out = nullptr; a.gain_link = nullptr;
    a.min_gain = 0.0;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.M = n_sel; a.L = n_levels; a.pow_k = pow_k;
    a.words = allowed ? (n_rbs + 31) / 32 : 0;
    a.W = (n_links + 31) / 32;
    const int entries = n_rbs * n_levels;                                // at most 8192 x 64
    a.chunk = std::min(std::min(DV_CHUNK, n_sel), std::max(1, (DV_CHUNK_ENTRIES + entries - 1) / entries));
    const unsigned long long N = (unsigned long long)n_links;
    // 64-bit until the limit is checked: 2048 links x 8192 RBs would be 2 MiB of bitset alone
    unsigned long long off = N * sizeof(Link);
    a.off_al = (unsigned)off; off += (N * (unsigned long long)a.words * 4ull + 15ull) & ~15ull;
    a.off_bits = (unsigned)off; off += ((unsigned long long)a.W * (unsigned long long)n_rbs * 4ull + 15ull) & ~15ull;
    a.off_tail = (unsigned)off; off += DV_TAIL_BYTES;
    if (off > (unsigned long long)D2D_DEVIATE_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_DEVIATE_MAX_LDS_BYTES) + " a workgroup can have");
    lds = (unsigned)off;
    return 0;
}

template <bool BEST>
hipError_t launch_deviate(const DeviateArgs& a, int32_t law, int64_t n_envs, unsigned lds, hipStream_t st) {
    const long long work = BEST ? (long long)a.R * a.L : (long long)a.chunk * a.R * a.L;        // what one pass deals over the threads
    const unsigned threads = (unsigned)std::min<long long>(DV_MAX_THREADS, (work + 63) & ~63ll);
    const dim3 grid((unsigned)n_envs, (unsigned)((a.M + a.chunk - 1) / a.chunk));
    if (law == D2D_DEVIATE_LAW_INV_SQUARE) return launch(&deviate_kernel<PL_INV_SQUARE, BEST>, grid, dim3(threads), lds, st, a);
    if (law == D2D_DEVIATE_LAW_POWER) return launch(&deviate_kernel<PL_POWER, BEST>, grid, dim3(threads), lds, st, a);
    return launch(&deviate_kernel<PL_POWK, BEST>, grid, dim3(threads), lds, st, a);
}

}  // namespace

extern "C" int d2d_deviation_gains(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                   const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                                   int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max,
                                   const int32_t* links, int32_t n_sel, int32_t n_levels, const uint32_t* allowed, const float* floor_db,
                                   const uint8_t* env_mask, float* gain_out, void* hip_stream) try {
    DeviateArgs a;
    unsigned lds = 0;
    if (prepare(a, pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, cap_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs, p_min, p_max,
                links, n_sel, n_levels, allowed, floor_db, env_mask, lds))
        return 1;
    if (!gain_out) return fail("null device pointer");
    if (n_envs == 0) return 0;
    a.table = gain_out;
    const hipError_t e = launch_deviate<false>(a, law, n_envs, lds, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(std::string("deviate_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

extern "C" int d2d_best_deviation(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                  const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                                  int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max,
                                  const int32_t* links, int32_t n_sel, int32_t n_levels, const uint32_t* allowed, const float* floor_db,
                                  double min_gain_mbps, const uint8_t* env_mask, int32_t* rb_out, int32_t* pwr_out, double* gain_link,
                                  double* regret, int32_t* leader, void* hip_stream) try {
    DeviateArgs a;
    unsigned lds = 0;
    if (prepare(a, pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, cap_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs, p_min, p_max,
                links, n_sel, n_levels, allowed, floor_db, env_mask, lds))
        return 1;
    if (!std::isfinite(min_gain_mbps) || min_gain_mbps < 0.0) return fail("min_gain_mbps must be finite and >= 0");
    if (!rb_out || !pwr_out || !gain_link || !regret || !leader) return fail("null device pointer");
    const void* outs[5] = {rb_out, pwr_out, gain_link, regret, leader};
    for (int x = 0; x < 5; ++x)
        for (int y = x + 1; y < 5; ++y)
            if (outs[x] == outs[y]) return fail("rb_out, pwr_out, gain_link, regret and leader must be five arrays");
    if (rb_out == rb || pwr_out == pwr_dbm) return fail("rb_out and pwr_out must not be the held planes");
    if (n_envs == 0) return 0;
    a.rb_out = rb_out; a.pwr_out = pwr_out; a.gain_link = gain_link; a.min_gain = min_gain_mbps;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e = launch_deviate<true>(a, law, n_envs, lds, st);
    if (e != hipSuccess) return fail(std::string("deviate_kernel launch: ") + hipGetErrorString(e));
    RegretArgs g;
    g.rb = rb; g.pwr = pwr_dbm; g.links = links; g.env_mask = env_mask; g.rb_out = rb_out; g.pwr_out = pwr_out; g.gain_link = gain_link;
    g.regret = regret; g.leader = leader; g.N = n_links; g.M = n_sel;
    e = launch(&regret_kernel, dim3((unsigned)n_envs), dim3(DV_MAX_THREADS), 0u, st, g);
    if (e != hipSuccess) return fail(std::string("regret_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_deviate_last_error)
