// libd2d_assign.so (include/d2d_assign.h): the weight planes of one-to-one RB matching and the maximum-weight matching itself, one
// launch each.  gfx950.
//
// assign_weights_kernel: grid = env, 256 threads.  The workgroup sorts the env's BACKGROUND links by (rb, link index) into LDS with
// the shared sort (d2d_same_rb.h); the movable links take the pseudo RB R and so stand behind start[R] with the links on no RB.
//   phase 1, d2d_marginal.hip's: the slot's link as receiver - I_k over the other background members of its RB in ascending link
//            index, float products into a double accumulator, the capacity by the step's own operations - parked in LDS beside the
//            receiver's tuple;
//   phase 2, the items (a, r): ONE MOVABLE LINK PER WAVE at a time, lanes across r, so a wave's stores into weights[b][a][r ..] are
//            contiguous.  An item walks the members of r once: link a's interference as d2d_evaluate.hip adds it, and per member
//            the capacity it loses to link a as one log2(1 + x) term, x = S t rx_pl / (den (den' + S)), den without link a and
//            den' with it, or its whole capacity when link a pushes it under its threshold.
// assign_solve_kernel: grid = env, 64 or 256 threads that OWN COLUMNS (j = tid, tid + THREADS, ...).  One step of an augmentation is
// one coalesced read of the row weights[b][i][:], the update of the own columns' shortest[] and a workgroup argmin on (value, index).
// Only additions and subtractions of doubles: nothing the compiler could contract.
// No floating-point read-modify-write on memory anywhere; every output word is written once by its owner.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_assign.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int AW_THREADS = 256;
constexpr int AW_WAVES = AW_THREADS / 64;
static_assert(D2D_ASSIGN_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_ASSIGN_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_ASSIGN_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_ASSIGN_LAW_POWER == LAW_POWER && D2D_ASSIGN_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(D2D_ASSIGN_MAX_RBS <= 32 * 256, "a solver thread keeps the scanned marks of its columns in one 32-bit word");

struct WeightsArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    const float* cap_cols;          // [2][D]
    const int* links;               // [M]
    const unsigned* allowed;        // [N][ceil(R / 32)] or null
    float* weights;                 // [B][M][R]
    float* harm;                    // [B][M][R] or null
    int D, N, R, M;
    int pow_k;
    unsigned off_hh, off_v0, off_v1, off_acc, off_cap, off_srb, off_sof, off_start;     // byte offsets of the LDS arrays behind the tuples
};

// dynamic LDS: tuples float4[N] | hh float2[N] (power laws) | v0 float4[N] | v1 float4[N] | acc double[N], whose bytes first hold the
// sort's keys u32[N rounded up to 4] | cap float[N] | srb int[N], which first holds the movable marks | sof int[N] (slot of link) |
// start int[R + 1]

// log2(1 + x) with relative accuracy for small x (d2d_marginal.hip's)
__device__ __forceinline__ float log2_1p(float x) {
    const float u = 1.0f + x, um1 = u - 1.0f;
    const float big = __builtin_amdgcn_logf(u) * precise_div(x, um1 == 0.0f ? 1.0f : um1);
    return um1 == 0.0f ? x * 1.44269504088896340736f : big;
}

template <int MODE, int OBJECTIVE>
__global__ __launch_bounds__(AW_THREADS) void assign_weights_kernel(const WeightsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int N = a.N, R = a.R, D = a.D, M = a.M;
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
    int* sof = reinterpret_cast<int*>(smem + a.off_sof);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    const int n4 = (N + 3) & ~3;
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- the movable marks, in the bytes of srb (rewritten by the sort, behind the last read of a mark)
    for (int j = tid; j < N; j += AW_THREADS) srb[j] = 0;
    __syncthreads();
    for (int m = tid; m < M; m += AW_THREADS) {
        const int j = a.links[m];
        if ((unsigned)j < (unsigned)N) srb[j] = 1;
    }
    __syncthreads();
    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one - and so does every
    // movable link: thread j rewrites the key it has just written
    same_rb_keys<AW_THREADS>(key, rb_row, N, n4, R);
    for (int j = tid; j < N; j += AW_THREADS)
        if (srb[j]) key[j] = ((unsigned)R << KEY_SHIFT) | (unsigned)j;
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += AW_THREADS) {
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
        sof[j] = slot;
    }
    __syncthreads();                 // the last use of key: its bytes are the interference sums from here on
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB or movable
    same_rb_starts<AW_THREADS>(start, srb, N, R);
    __syncthreads();

    // ---- phase 1: the slot's link as receiver (d2d_marginal.hip, phase 1); a slot behind start[R] walks nobody
    for (int s = tid; s < N; s += AW_THREADS) {
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

    // ---- phase 2: movable link a of the wave on RB r of the lane
    const int wave = tid >> 6, lane = tid & 63;
    const int words = (R + 31) >> 5;
    const float ninf = -__builtin_inff();
    for (int m = wave; m < M; m += AW_WAVES) {
        const int i = a.links[m];
        const size_t out = (b * (size_t)M + (size_t)m) * (size_t)R;
        if ((unsigned)i >= (unsigned)N) {                                 // not a link: a row nobody can take
            for (int r = lane; r < R; r += 64) {
                a.weights[out + r] = ninf;
                if (a.harm) a.harm[out + r] = 0.0f;
            }
            continue;
        }
        const int s = sof[i];
        const float4 me = txl[s], p = v0[s], q = v1[s];
        const float2 h = POWLAW ? hh[s] : make_float2(-1.0f, 0.0f);
        const unsigned* may = a.allowed ? a.allowed + (size_t)i * (size_t)words : nullptr;
        for (int r = lane; r < R; r += 64) {
            double acc = 0.0, harm = 0.0;
            const int k_end = start[r + 1];
            for (int k = start[r]; k < k_end; ++k) {
                // member k into link a's receiver: the term d2d_evaluate.hip adds, in its order
                const float4 o = txl[k];
                const float dx = o.x - p.x, dy = o.y - p.y;
                const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), POWLAW ? hh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
                acc += (double)(o.z * g);
                if (OBJECTIVE == D2D_ASSIGN_OBJECTIVE_TOTAL || a.harm) {
                    // link a into member k's receiver: what k loses
                    const float4 vp = v0[k], vq = v1[k];
                    const double ik = accl[k];
                    const float ex = me.x - vp.x, ey = me.y - vp.y;
                    const float gv = pair_gain<MODE>(fmaf(ex, ex, ey * ey), h, a.pow_k);
                    const float t = me.z * gv;
                    const double td = (double)t, rx_pl = (double)vp.z, noise = (double)vp.w, sig = (double)vq.x;
                    const double den = fma(ik, rx_pl, noise);                // without link a
                    const double denw = fma(ik + td, rx_pl, noise);          // with it
                    float loss = 0.0f;
                    if (vq.w != 0.0f) {                                       // under its threshold already: nothing to lose
                        // still over it with link a (the step's test, simulator.py:123): log2(1 + S t rx_pl / (den (den' + S)))
                        const float sw = (float)(sig / denw);
                        const bool ok_with = 3.01029995663981195f * __builtin_amdgcn_logf(sw) > vq.z;
                        const float x = (float)(sig * rx_pl * td / (den * (denw + sig)));
                        loss = ok_with ? vq.y * log2_1p(x) : capl[k];
                    }
                    harm += (double)loss;
                }
            }
            // link a's capacity on r: the step's operations in the step's order, as d2d_evaluate.hip forms it
            const float accf = (float)acc;
            const float sinr_lin = precise_div(q.x, fmaf(accf, p.z, p.w));
            const float sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
            const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
            const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
            const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
            const float cap = sinr_db > q.z ? q.y * sh : 0.0f;
            const bool free_rb = !may || ((may[r >> 5] >> (r & 31)) & 1u);
            const float w = OBJECTIVE == D2D_ASSIGN_OBJECTIVE_OWN ? cap : (float)((double)cap - harm);
            a.weights[out + r] = free_rb ? w : ninf;
            if (a.harm) a.harm[out + r] = (float)harm;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the matching
struct SolveArgs {
    const float* w;                 // [B][M][R]
    int* col;                       // [B][M]
    float* value;                   // [B]
    unsigned char* feasible;        // [B]
    int M, R;
    unsigned off_v, off_short, off_path, off_r4c, off_c4r, off_red;            // byte offsets behind u
};

// dynamic LDS: u double[M] | v double[R] | shortest double[R] | path int[R] | row4col int[R] | col4row int[M] | the argmin's
// scratch, two buffers taken in turn: value double[4] and index int[4] each

template <int THREADS>
__global__ __launch_bounds__(THREADS) void assign_solve_kernel(const SolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WAVES = THREADS / 64;
    const int M = a.M, R = a.R;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    double* u = reinterpret_cast<double*>(smem);
    double* v = reinterpret_cast<double*>(smem + a.off_v);
    double* shortest = reinterpret_cast<double*>(smem + a.off_short);
    int* path = reinterpret_cast<int*>(smem + a.off_path);
    int* row4col = reinterpret_cast<int*>(smem + a.off_r4c);
    int* col4row = reinterpret_cast<int*>(smem + a.off_c4r);
    double* red_v = reinterpret_cast<double*>(smem + a.off_red);               // [2][4]
    int* red_j = reinterpret_cast<int*>(smem + a.off_red + 2 * 4 * sizeof(double));   // [2][4]
    const float* w = a.w + b * (size_t)M * (size_t)R;
    const double inf = __builtin_inf();

    for (int i = tid; i < M; i += THREADS) { u[i] = 0.0; col4row[i] = -1; }
    for (int j = tid; j < R; j += THREADS) { v[j] = 0.0; row4col[j] = -1; }
    __syncthreads();

    bool feasible = true;
    unsigned turn = 0;                                                         // which argmin buffer the next step writes
    for (int cur = 0; cur < M && feasible; ++cur) {
        unsigned scanned = 0;                                                  // bit q: the thread's q-th column, tid + q THREADS
        for (int j = tid; j < R; j += THREADS) shortest[j] = inf;              // own columns only: no barrier
        double minval = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            const double ui = u[i];
            const float* row = w + (size_t)i * (size_t)R;
            double best = inf;
            int bj = 0x7FFFFFFF;
            unsigned bit = 1u;
            for (int j = tid; j < R; j += THREADS, bit <<= 1) {
                if (scanned & bit) continue;
                const float wf = row[j];
                const double cost = (__builtin_fabsf(wf) < __builtin_inff()) ? -(double)wf : inf;      // NaN compares false
                const double red = ((minval + cost) - ui) - v[j];
                double sh = shortest[j];
                if (red < sh) { sh = red; shortest[j] = red; path[j] = i; }
                if (sh < best) { best = sh; bj = j; }                          // ascending j: equal values keep the lowest
            }
            // the workgroup's (value, index) minimum, equal values to the lowest index
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ov = __shfl_xor(best, m, 64);
                const int oj = __shfl_xor(bj, m, 64);
                if (ov < best || (ov == best && oj < bj)) { best = ov; bj = oj; }
            }
            if (WAVES > 1) {
                double* rv = red_v + 4 * (turn & 1u);
                int* rj = red_j + 4 * (turn & 1u);
                if ((tid & 63) == 0) { rv[tid >> 6] = best; rj[tid >> 6] = bj; }
                __syncthreads();     // the other buffer is written a step later, behind this barrier: nobody still reads it
                best = rv[0]; bj = rj[0];
#pragma unroll
                for (int q = 1; q < WAVES; ++q) {
                    const double ov = rv[q];
                    const int oj = rj[q];
                    if (ov < best || (ov == best && oj < bj)) { best = ov; bj = oj; }
                }
                ++turn;
            }
            if (!(best < inf)) { feasible = false; break; }                    // no column left to reach: the same in every thread
            minval = best;
            if ((bj % THREADS) == tid) scanned |= 1u << (bj / THREADS);
            const int owner = row4col[bj];                                     // row4col does not change inside an augmentation
            if (owner < 0) sink = bj; else i = owner;
        }
        if (!feasible) break;
        // ---- the duals: every scanned column j but the sink hands minval - shortest[j] to its row (col4row[row4col[j]] == j) and
        // takes it off v[j]; the sink's difference is 0
        {
            unsigned bit = 1u;
            for (int j = tid; j < R; j += THREADS, bit <<= 1) {
                if (!(scanned & bit) || j == sink) continue;
                const double d = minval - shortest[j];
                u[row4col[j]] += d;                                            // one scanned column per assigned row
                v[j] -= d;
            }
            if (tid == 0) u[cur] += minval;                                    // cur is unassigned: no column's row
        }
        __syncthreads();
        // ---- flip the path from the sink back to cur
        if (tid == 0) {
            int j = sink;
            while (true) {
                const int r = path[j];
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }

    // ---- results
    if (feasible) {
        for (int r = tid; r < M; r += THREADS) a.col[b * (size_t)M + (size_t)r] = col4row[r];
        if (tid == 0) {
            double t = 0.0;
            for (int r = 0; r < M; ++r) t += (double)w[(size_t)r * (size_t)R + (size_t)col4row[r]];
            a.value[b] = (float)t;
            a.feasible[b] = 1;
        }
    } else {
        for (int r = tid; r < M; r += THREADS) a.col[b * (size_t)M + (size_t)r] = -1;
        if (tid == 0) { a.value[b] = 0.0f; a.feasible[b] = 0; }
    }
}

}  // namespace

extern "C" int d2d_assign_weights(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                                  const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                                  int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* movable_links,
                                  int32_t n_movable, const uint32_t* allowed, int32_t objective, float* weights, float* harm,
                                  void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_ASSIGN_MAX_LINKS, n_rbs, D2D_ASSIGN_MAX_RBS, n_dev)) return fail(why);
    if (n_movable < 1 || n_movable > n_links) return fail("n_movable must be in [1, n_links]");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (objective != D2D_ASSIGN_OBJECTIVE_TOTAL && objective != D2D_ASSIGN_OBJECTIVE_OWN) return fail("unknown objective");
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !movable_links || !weights)
        return fail("null device pointer");
    if (harm == weights) return fail("weights and harm must be two planes");
    WeightsArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.links = movable_links; a.allowed = allowed; a.weights = weights; a.harm = harm;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.M = n_movable; a.pow_k = pow_k;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_hh = N * 16u;
    a.off_v0 = a.off_hh + (law == D2D_ASSIGN_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_v1 = a.off_v0 + N * 16u;
    a.off_acc = a.off_v1 + N * 16u;
    a.off_cap = a.off_acc + round16(n4 * 8u);                            // doubles; the sort's keys (n4 * 4 bytes) fit inside
    a.off_srb = a.off_cap + round16(N * 4u);
    a.off_sof = a.off_srb + round16(N * 4u);
    a.off_start = a.off_sof + round16(N * 4u);
    const unsigned lds = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    if (lds > (unsigned)D2D_ASSIGN_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                    std::to_string(D2D_ASSIGN_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs), block(AW_THREADS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    const bool own = objective == D2D_ASSIGN_OBJECTIVE_OWN;
    if (law == D2D_ASSIGN_LAW_INV_SQUARE)
        e = own ? launch(&assign_weights_kernel<PL_INV_SQUARE, D2D_ASSIGN_OBJECTIVE_OWN>, grid, block, lds, s, a)
                : launch(&assign_weights_kernel<PL_INV_SQUARE, D2D_ASSIGN_OBJECTIVE_TOTAL>, grid, block, lds, s, a);
    else if (law == D2D_ASSIGN_LAW_POWER)
        e = own ? launch(&assign_weights_kernel<PL_POWER, D2D_ASSIGN_OBJECTIVE_OWN>, grid, block, lds, s, a)
                : launch(&assign_weights_kernel<PL_POWER, D2D_ASSIGN_OBJECTIVE_TOTAL>, grid, block, lds, s, a);
    else
        e = own ? launch(&assign_weights_kernel<PL_POWK, D2D_ASSIGN_OBJECTIVE_OWN>, grid, block, lds, s, a)
                : launch(&assign_weights_kernel<PL_POWK, D2D_ASSIGN_OBJECTIVE_TOTAL>, grid, block, lds, s, a);
    if (e != hipSuccess) return fail(std::string("assign_weights_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

extern "C" int d2d_assign_solve(const float* weights, int64_t n_envs, int32_t n_rows, int32_t n_cols, int32_t* col, float* value,
                                uint8_t* feasible, void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_cols < 1 || n_cols > D2D_ASSIGN_MAX_RBS) return fail("n_cols must be in [1, " + std::to_string(D2D_ASSIGN_MAX_RBS) + "]");
    if (n_rows < 1) return fail("n_rows must be >= 1");
    if (n_rows > n_cols)
        return fail("n_rows = " + std::to_string(n_rows) + " rows cannot be matched one-to-one to n_cols = " + std::to_string(n_cols) +
                    " columns: n_rows must be <= n_cols");
    if (!weights || !col || !value || !feasible) return fail("null device pointer");
    SolveArgs a;
    a.w = weights; a.col = col; a.value = value; a.feasible = feasible; a.M = n_rows; a.R = n_cols;
    const unsigned M = (unsigned)n_rows, R = (unsigned)n_cols;
    a.off_v = round16(M * 8u);
    a.off_short = a.off_v + round16(R * 8u);
    a.off_path = a.off_short + round16(R * 8u);
    a.off_r4c = a.off_path + round16(R * 4u);
    a.off_c4r = a.off_r4c + round16(R * 4u);
    a.off_red = a.off_c4r + round16(M * 4u);
    const unsigned lds = a.off_red + 96u;                                // two buffers of double[4] + int[4]
    if (lds > (unsigned)D2D_ASSIGN_MAX_LDS_BYTES)
        return fail("n_rows and n_cols need " + std::to_string(lds) + " bytes of LDS, more than the " +
                    std::to_string(D2D_ASSIGN_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const hipError_t e = n_cols <= 64 ? launch(&assign_solve_kernel<64>, grid, dim3(64), lds, s, a)
                                      : launch(&assign_solve_kernel<256>, grid, dim3(256), lds, s, a);
    if (e != hipSuccess) return fail(std::string("assign_solve_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_assign_last_error)
