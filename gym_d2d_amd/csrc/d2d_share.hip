// libd2d_share.so (include/d2d_share.h): exact optimal RB sharing for small link groups - the value of every subset of the movable
// links on every RB, and the max-plus subset convolution over the RBs.  gfx950.
//
// share_values_kernel.  Grid (env, RB), 256 threads.  (1) The background members of the RB - the links on it that are not movable -
// are found by one ballot per 64 links, kept as words in LDS: a member's place is the popcount of the bits below it, so the order is
// the link order on every call, without atomics.  (2) Members and movable links are merged in ascending link index into the UNION
// (at most 64 + 12 entries) and staged as evaluate_kernel stages tuples.  (3) The term matrix term[i][j] = what transmitter j puts
// into receiver i, the float evaluate_kernel forms on the fly, is computed once for the whole union, row stride odd.  (4) THREADS
// OWN SUBSETS: for every entry of background + S in union order the others' terms are accumulated in union order into a double,
// the capacity is formed by the step's operations (d2d_evaluate.hip, the walk) and added to the subset's double sum.  Every lane of
// a wave reads the same matrix word (a broadcast: no bank conflicts whatever the stride); the bits of S above the low six are the
// same in a wave, so rows and columns of links no lane holds are skipped by a ballot.  An RB with more than 64 background members
// is closed: its background capacity comes from a plain walk with on-the-fly terms, thread per member, and a sequential sum.
//
// share_solve_kernel.  One workgroup per env, every RB layer in one launch: g[2][2^M] doubles, the layer's values f[2^M] (what is
// not admissible staged as -inf) and the layer's choice words in LDS.  A WAVE OWNS A TARGET T: lane l takes the submasks S of T
// whose low six bits are l - S = Shi | l with Shi running through the submasks of T's high bits - so each step reads f[Shi | l] and
// g[(T \ Shi) \ l], 64 consecutive doubles each, conflict-free, and the work of a target is spread over the wave: T = all ones
// costs 64 steps, not 4096 of one thread.  Each candidate is one double addition; a lane keeps (largest, lowest S) and a fixed xor
// tree reduces the wave by the same rule, so the words do not depend on any order.  The choice words of a layer leave LDS by
// coalesced stores; after the last layer one wave walks them back from T = all ones.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_same_rb.h"
#include "d2d_share.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int SV_THREADS = 256;
constexpr int SV_WAVES = SV_THREADS / 64;
constexpr int SV_MAX_M = D2D_SHARE_MAX_MOVABLE;
constexpr int SV_MAX_BG = D2D_SHARE_MAX_BACKGROUND;
constexpr int SS_MAX_THREADS = 1024;
static_assert(D2D_SHARE_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_SHARE_MAX_RBS == SAME_RB_MAX_RBS, "the limits of every kernel that keeps an env in LDS");
static_assert(D2D_SHARE_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_SHARE_LAW_POWER == LAW_POWER && D2D_SHARE_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(SV_MAX_BG == 64, "a closed RB is one whose members do not fit one ballot word");
static_assert(SV_MAX_BG + SV_MAX_M <= 128, "a subset's union mask is two 64-bit words");
static_assert(26ull * (1ull << SV_MAX_M) <= D2D_SHARE_MAX_LDS_BYTES, "the solver's layers fit the LDS of one workgroup");
static_assert(SV_MAX_M <= 16, "a choice word is 16 bits");

struct ShareValuesArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;                  // [B][N]
    const int* pwr;                 // [B][N]
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* cap_cols;          // [2][D]
    const int* movable;             // [M], ascending link indices
    const unsigned* allowed;        // [N][ceil(R / 32)] or null
    double* values;                 // [B][R][2^M]
    int* closed_rb;                 // [B][R]
    int D, N, R, M;
    int pow_k;
    int stride;                     // the floats of a row of the term matrix: odd
    unsigned off_mbit, off_term, off_txl, off_rxa, off_rxb, off_hh, off_mem, off_capf;     // byte offsets behind the ballot words
};

// dynamic LDS: bal u64[ceil(N / 64)] | mbit i32[U] | term f32[U][stride] | and by union entry (by member, on a closed RB), L = N + 12
// slots each: txl float4 (tx x, tx y, linear EIRP incl. the tx constant, bw_mhz) | rxa float4 (rx x, rx y, rx_pl, noise) |
// rxb float2 (rx_lin, sens_db) | hh float2 (power laws) | mem i32 (the link index) | capf f32 (a closed RB's capacities)

// the step's capacity of a receiver whose own transmitter puts `own` into it and the others `acc`: d2d_evaluate.hip, the walk
__device__ __forceinline__ float capacity_of(float own, double acc, float4 ra, float2 rb2, float bw_mhz) {
    const float rx_pl = ra.z, noise = ra.w, rx_lin = rb2.x, sens = rb2.y;
    const float sig = own * rx_pl * rx_lin;
    const float accf = (float)acc;
    const float sinr_lin = precise_div(sig, fmaf(accf, rx_pl, noise));
    const float sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
    const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
    const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
    const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
    const bool ok = sinr_db > sens;
    return ok ? bw_mhz * sh : 0.0f;
}

template <int MODE>
__global__ __launch_bounds__(SV_THREADS) void share_values_kernel(const ShareValuesArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int N = a.N, R = a.R, D = a.D, M = a.M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const int r = (int)blockIdx.y;
    unsigned long long* bal = reinterpret_cast<unsigned long long*>(smem);
    int* mbit = reinterpret_cast<int*>(smem + a.off_mbit);
    float* term = reinterpret_cast<float*>(smem + a.off_term);
    float4* txl = reinterpret_cast<float4*>(smem + a.off_txl);
    float4* rxa = reinterpret_cast<float4*>(smem + a.off_rxa);
    float2* rxb = reinterpret_cast<float2*>(smem + a.off_rxb);
    float2* hh = reinterpret_cast<float2*>(smem + a.off_hh);
    int* mem = reinterpret_cast<int*>(smem + a.off_mem);
    float* capf = reinterpret_cast<float*>(smem + a.off_capf);
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const int nch = (N + 63) >> 6;
    const int nS = 1 << M;
    double* out = a.values + (b * (size_t)R + (size_t)r) * (size_t)nS;

    // ---- (1) the background members of r: one ballot word per 64 links
    for (int c = wave; c < nch; c += SV_WAVES) {
        const int j = c * 64 + lane;
        bool member = j < N && rb_row[j] == r;
        for (int q = 0; q < M; ++q) member = member && a.movable[q] != j;
        const unsigned long long w = __ballot(member);
        if (lane == 0) bal[c] = w;
    }
    __syncthreads();
    int nb = 0;
    for (int c = 0; c < nch; ++c) nb += __popcll(bal[c]);
    const bool closed = nb > SV_MAX_BG;
    const int U = closed ? nb : nb + M;                                  // the staged entries: at most N + M
    // the members below link j
    auto below = [&](int j) {
        int n = 0;
        for (int c = 0; c < (j >> 6); ++c) n += __popcll(bal[c]);
        return n + __popcll(bal[j >> 6] & ((1ull << (j & 63)) - 1ull));
    };
    auto stage = [&](int p, int j, int bit) {
        const int txd = a.link_tx[j], rxd = a.link_rx[j];
        txl[p] = make_float4(px[txd], py[txd], pow10_tenth(pwr_row[j]) * a.cols[txd], a.cap_cols[txd]);
        rxa[p] = make_float4(px[rxd], py[rxd], a.cols[D + rxd], a.cols[3 * D + rxd]);
        rxb[p] = make_float2(a.cols[2 * D + rxd], a.cap_cols[D + rxd]);
        if (POWLAW) hh[p] = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        mem[p] = j;
        if (!closed) mbit[p] = bit;
    };
    // ---- (2) the union in ascending link index: a member behind the members and the movable links below it, a movable link likewise
    for (int c = wave; c < nch; c += SV_WAVES) {
        const int j = c * 64 + lane;
        if ((bal[c] >> lane) & 1ull) {
            int p = below(j);
            if (!closed)
                for (int q = 0; q < M; ++q) p += a.movable[q] < j ? 1 : 0;
            stage(p, j, -1);
        }
    }
    if (!closed && tid < M) {
        const int j = min(max(a.movable[tid], 0), N - 1);
        stage(tid + below(j), j, tid);
    }
    if (tid == 0) a.closed_rb[b * (size_t)R + (size_t)r] = closed ? 1 : 0;
    __syncthreads();

    if (closed) {
        // ---- a closed RB: the background's capacity by a plain walk, thread per member, and -inf for every other subset
        for (int s = tid; s < nb; s += SV_THREADS) {
            const float4 ra = rxa[s];
            double acc = 0.0;
            float own = 0.0f;
            for (int k = 0; k < nb; ++k) {
                const float4 o = txl[k];
                const float dx = o.x - ra.x, dy = o.y - ra.y;
                const float d2 = fmaf(dx, dx, dy * dy);
                const float g = pair_gain<MODE>(d2, POWLAW ? hh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
                const float t = o.z * g;
                acc += k != s ? (double)t : 0.0;
                own = k == s ? t : own;
            }
            capf[s] = capacity_of(own, acc, ra, rxb[s], txl[s].w);
        }
        for (int S = tid; S < nS; S += SV_THREADS)
            if (S) out[S] = -__builtin_inf();
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int k = 0; k < nb; ++k) tot += (double)capf[k];
            out[0] = tot;
        }
        return;
    }

    // ---- (3) the term matrix: term[i][j] = what transmitter j puts into receiver i, linear mW (evaluate_kernel's `term`)
    const int stride = a.stride;
    for (int e = tid; e < U * U; e += SV_THREADS) {
        const int i = e / U, j = e - i * U;
        const float4 o = txl[j];
        const float4 ra = rxa[i];
        const float dx = o.x - ra.x, dy = o.y - ra.y;
        const float d2 = fmaf(dx, dx, dy * dy);
        const float g = pair_gain<MODE>(d2, POWLAW ? hh[j] : make_float2(-1.0f, 0.0f), a.pow_k);
        term[i * stride + j] = o.z * g;
    }
    // the movable links that are not allowed on r, as a mask
    unsigned forbid = 0u;
    if (a.allowed) {
        const int words = (R + 31) >> 5;
        for (int q = 0; q < M; ++q) {
            const int j = min(max(a.movable[q], 0), N - 1);
            const unsigned w = a.allowed[(size_t)j * (size_t)words + (size_t)(r >> 5)];
            forbid |= ((w >> (r & 31)) & 1u) ? 0u : (1u << q);
        }
    }
    __syncthreads();

    // ---- (4) threads own subsets
    for (int S = tid; S < nS; S += SV_THREADS) {
        double tot = -__builtin_inf();
        if (((unsigned)S & forbid) == 0u) {
            unsigned long long in0 = 0ull, in1 = 0ull;                   // the union entries on the RB under S
            for (int p = 0; p < U; ++p) {
                const int mb = mbit[p];
                const unsigned long long in = (mb < 0 || ((S >> mb) & 1)) ? 1ull : 0ull;
                if (p < 64) in0 |= in << p; else in1 |= in << (p - 64);
            }
            tot = 0.0;
            for (int i = 0; i < U; ++i) {
                const bool in_i = ((i < 64 ? in0 >> i : in1 >> (i - 64)) & 1ull) != 0ull;
                if (__ballot(in_i) == 0ull) continue;                    // no lane of the wave has this link on the RB
                const float* row = term + i * stride;
                double acc = 0.0;
                for (int j = 0; j < U; ++j) {
                    const bool in_j = ((j < 64 ? in0 >> j : in1 >> (j - 64)) & 1ull) != 0ull;
                    if (__ballot(in_j) == 0ull) continue;
                    const float t = row[j];
                    acc += (in_j && j != i) ? (double)t : 0.0;
                }
                const float cap = capacity_of(row[i], acc, rxa[i], rxb[i], txl[i].w);
                tot += in_i ? (double)cap : 0.0;
            }
        }
        out[S] = tot;
    }
}

struct ShareSolveArgs {
    const double* values;           // [B][R][2^M]
    const int* quota;               // [R] or null
    unsigned short* choice;         // [B][R][2^M]
    int* col;                       // [B][M]
    double* value;                  // [B]
    int* feasible;                  // [B]
    int R, M;
};

__device__ __forceinline__ bool finite64(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// dynamic LDS: g f64[2][2^M] | f f64[2^M] | ch u16[2^M]
__global__ __launch_bounds__(SS_MAX_THREADS) void share_solve_kernel(const ShareSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int R = a.R, M = a.M;
    const int nT = 1 << M;
    const int T_ = (int)blockDim.x, nw = T_ >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    double* g = reinterpret_cast<double*>(smem);
    double* f = g + 2 * nT;
    unsigned short* ch = reinterpret_cast<unsigned short*>(f + nT);
    const double NINF = -__builtin_inf();
    const size_t env = b * (size_t)R * (size_t)nT;

    for (int T = tid; T < nT; T += T_) g[T] = T == 0 ? 0.0 : NINF;
    for (int r = 0; r < R; ++r) {
        const size_t layer = env + (size_t)r * (size_t)nT;
        const int q = a.quota ? max(a.quota[r], 0) : M;
        // ---- the layer's values, what is not admissible as -inf.  f was last read before the barrier that ended the layer before
        for (int S = tid; S < nT; S += T_) {
            const double v = a.values[layer + (size_t)S];
            f[S] = (finite64(v) && __popc((unsigned)S) <= q) ? v : NINF;
        }
        __syncthreads();
        const double* gp = g + (r & 1) * nT;
        double* gn = g + ((r & 1) ^ 1) * nT;
        // ---- waves own targets
        for (int T = wave; T < nT; T += nw) {
            const int Thi = T & ~63, Tlo = T & 63;
            double best = NINF;
            int bestS = 0x7FFFFFFF;
            if ((lane & ~Tlo) == 0) {
                const int rest = T ^ lane;                               // T without this lane's low bits
                const int steps = 1 << __popc((unsigned)Thi);            // the submasks of the high bits: a trip count the compiler can unroll on
                int Shi = Thi;
#pragma unroll 4
                for (int it = 0; it < steps; ++it) {                     // descending, so that on equal sums the later, lower S stays
                    const int S = Shi | lane;
                    const double fv = f[S];
                    const double c = gp[rest ^ Shi] + fv;
                    if (fv > NINF && c > NINF && c >= best) { best = c; bestS = S; }
                    Shi = (Shi - 1) & Thi;
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double oc = __shfl_xor(best, m, 64);
                const int oS = __shfl_xor(bestS, m, 64);
                if (oc > best || (oc == best && oS < bestS)) { best = oc; bestS = oS; }
            }
            if (lane == 0) { gn[T] = best; ch[T] = (unsigned short)(best > NINF ? bestS : 0); }
        }
        __syncthreads();
        // ---- the layer's choice words, coalesced; ch is rewritten behind the next layer's barrier
        for (int T = tid; T < nT; T += T_) a.choice[layer + (size_t)T] = ch[T];
    }
    // the choice words are read back by wave 0, which did not write all of them
    __threadfence_block();
    __syncthreads();
    if (wave == 0) {
        const double top = g[(R & 1) * nT + (nT - 1)];
        const bool feas = top > NINF;
        int T = nT - 1, mine = -1;
        if (feas)
            for (int r = R - 1; r >= 0; --r) {
                const int S = a.choice[env + (size_t)r * (size_t)nT + (size_t)T];
                if ((S >> lane) & 1) mine = r;
                T ^= S;
            }
        if (lane < M) a.col[b * (size_t)M + (size_t)lane] = mine;
        if (lane == 0) { a.value[b] = feas ? top : 0.0; a.feasible[b] = feas ? 1 : 0; }
    }
}

unsigned long long bytes16(unsigned long long x) { return (x + 15ull) & ~15ull; }

}  // namespace

extern "C" int d2d_share_values(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                                int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* movable_links,
                                int32_t n_movable, const uint32_t* allowed, double* values, int32_t* closed_rb, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_SHARE_MAX_LINKS, n_rbs, D2D_SHARE_MAX_RBS, n_dev)) return fail(why);
    if (n_movable < 1 || n_movable > D2D_SHARE_MAX_MOVABLE || n_movable > n_links)
        return fail("n_movable must be in [1, " + std::to_string(D2D_SHARE_MAX_MOVABLE) + "] (D2D_SHARE_MAX_MOVABLE) and at most n_links");
    if (n_rbs > 65535) return fail("n_rbs must be at most 65535: the grid's second dimension");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    const unsigned long long block = (unsigned long long)n_envs * (unsigned long long)n_rbs * (10ull << n_movable);
    if (block > (unsigned long long)D2D_SHARE_MAX_BLOCK_BYTES)
        return fail("the value block and the choice words need " + std::to_string(block) + " bytes, more than the " +
                    std::to_string((unsigned long long)D2D_SHARE_MAX_BLOCK_BYTES) + " (D2D_SHARE_MAX_BLOCK_BYTES) one call may hold");
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !movable_links || !values || !closed_rb)
        return fail("null device pointer");
    ShareValuesArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.movable = movable_links; a.allowed = allowed; a.values = values; a.closed_rb = closed_rb;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.M = n_movable; a.pow_k = pow_k;
    const unsigned long long N = (unsigned long long)n_links, L = N + D2D_SHARE_MAX_MOVABLE;
    const unsigned long long U = (N < D2D_SHARE_MAX_BACKGROUND ? N : D2D_SHARE_MAX_BACKGROUND) + (unsigned long long)n_movable;
    a.stride = (int)(U | 1ull);
    unsigned long long off = bytes16(8ull * ((N + 63ull) / 64ull));
    a.off_mbit = (unsigned)off; off += bytes16(4ull * U);
    a.off_term = (unsigned)off; off += bytes16(4ull * U * (U | 1ull));
    a.off_txl = (unsigned)off; off += 16ull * L;
    a.off_rxa = (unsigned)off; off += 16ull * L;
    a.off_rxb = (unsigned)off; off += bytes16(8ull * L);
    a.off_hh = (unsigned)off; off += law == D2D_SHARE_LAW_INV_SQUARE ? 0ull : bytes16(8ull * L);
    a.off_mem = (unsigned)off; off += bytes16(4ull * L);
    a.off_capf = (unsigned)off; off += bytes16(4ull * L);
    if (off > (unsigned long long)D2D_SHARE_MAX_LDS_BYTES)
        return fail("n_links and n_movable need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_SHARE_MAX_LDS_BYTES) + " (D2D_SHARE_MAX_LDS_BYTES) a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs, (unsigned)n_rbs);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    if (law == D2D_SHARE_LAW_INV_SQUARE) e = launch(&share_values_kernel<PL_INV_SQUARE>, grid, dim3(SV_THREADS), (unsigned)off, s, a);
    else if (law == D2D_SHARE_LAW_POWER) e = launch(&share_values_kernel<PL_POWER>, grid, dim3(SV_THREADS), (unsigned)off, s, a);
    else e = launch(&share_values_kernel<PL_POWK>, grid, dim3(SV_THREADS), (unsigned)off, s, a);
    if (e != hipSuccess) return fail(std::string("share_values_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

extern "C" int d2d_share_solve(const double* values, const int32_t* quota, int64_t n_envs, int32_t n_rbs, int32_t n_movable,
                               uint16_t* choice, int32_t* col, double* value, int32_t* feasible, void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_rbs < 1 || n_rbs > D2D_SHARE_MAX_RBS) return fail("n_rbs must be in [1, " + std::to_string(D2D_SHARE_MAX_RBS) + "]");
    if (n_movable < 1 || n_movable > D2D_SHARE_MAX_MOVABLE)
        return fail("n_movable must be in [1, " + std::to_string(D2D_SHARE_MAX_MOVABLE) + "] (D2D_SHARE_MAX_MOVABLE)");
    const unsigned long long block = (unsigned long long)n_envs * (unsigned long long)n_rbs * (10ull << n_movable);
    if (block > (unsigned long long)D2D_SHARE_MAX_BLOCK_BYTES)
        return fail("the value block and the choice words need " + std::to_string(block) + " bytes, more than the " +
                    std::to_string((unsigned long long)D2D_SHARE_MAX_BLOCK_BYTES) + " (D2D_SHARE_MAX_BLOCK_BYTES) one call may hold");
    const unsigned long long lds = 26ull << n_movable;
    if (lds > (unsigned long long)D2D_SHARE_MAX_LDS_BYTES)
        return fail("n_movable needs " + std::to_string(lds) + " bytes of LDS, more than the " + std::to_string(D2D_SHARE_MAX_LDS_BYTES) +
                    " (D2D_SHARE_MAX_LDS_BYTES) a workgroup can have");
    if (!values || !choice || !col || !value || !feasible) return fail("null device pointer");
    if (n_envs == 0) return 0;
    ShareSolveArgs a;
    a.values = values; a.quota = quota; a.choice = choice; a.col = col; a.value = value; a.feasible = feasible;
    a.R = n_rbs; a.M = n_movable;
    const unsigned nT = 1u << n_movable;
    const unsigned threads = nT < 64u ? 64u : (nT > (unsigned)SS_MAX_THREADS ? (unsigned)SS_MAX_THREADS : nT);      // a wave per 64 targets
    const hipError_t e = launch(&share_solve_kernel, dim3((unsigned)n_envs), dim3(threads), (unsigned)lds,
                                static_cast<hipStream_t>(hip_stream), a);
    if (e != hipSuccess) return fail(std::string("share_solve_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_share_last_error)
