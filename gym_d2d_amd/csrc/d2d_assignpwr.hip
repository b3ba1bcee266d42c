// libd2d_assignpwr.so (include/d2d_assignpwr.h): the best admissible power of every movable link on every RB and its matching weight,
// one launch.  gfx950.
//
// assign_power_weights_kernel: grid = env, 256 threads.  The staging is d2d_assign.hip's: the BACKGROUND links sorted by (rb, link
// index) into LDS with the shared sort (d2d_same_rb.h), the movable links on the pseudo RB R behind start[R].  A movable link's
// tuple.z holds dev_cols[0][tx] alone - the factor its power levels multiply - since nobody walks it as an interferer.
//   phase 1, d2d_assign.hip's, parking additionally (in v1.w) each slot's EFFECTIVE floor: floor_db of its link where the background alone
//            meets it, -inf where there is none or the background already misses it (such a victim constrains nothing);
//   phase 2, the items (a, r): one movable link per wave at a time, lanes across r, both planes stored contiguously.  An item walks
//            the members of r once for link a's interference sum - that and its own-link gain do not depend on the power - and then
//            once per chunk of CHUNK power levels held in registers, MEMBER-OUTER, LEVEL-INNER: the gain a -> victim, the victim's
//            tuples and its denominator without link a are formed once per chunk, the two double quotients once per level; each
//            level's harm is summed in ascending member order.  Behind the walk the chunk's levels are scanned in ascending power
//            with a strict >.
// The expressions per level are d2d_assign.hip's, spelled the same way: without floors a level's weight is that kernel's bit for bit.
// No atomics, no floating-point read-modify-write on memory; every output word is written once by its owner.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_assignpwr.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"

namespace {

using namespace d2d;

constexpr int AP_THREADS = 256;
constexpr int AP_WAVES = AP_THREADS / 64;
constexpr int CHUNK = D2D_ASSIGNPWR_CHUNK;
static_assert(D2D_ASSIGNPWR_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_ASSIGNPWR_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_ASSIGNPWR_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_ASSIGNPWR_LAW_POWER == LAW_POWER && D2D_ASSIGNPWR_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");
static_assert(CHUNK >= 1 && CHUNK <= 32 && D2D_ASSIGNPWR_MAX_LEVELS % CHUNK == 0, "a chunk's inadmissible levels are the bits of one word");

struct PowerWeightsArgs {
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
    const int* p_min;               // [N]
    const int* p_max;               // [N]
    const float* floor_db;          // [N] or null
    float* weights;                 // [B][M][R]
    int* power;                     // [B][M][R]
    int D, N, R, M;
    int pow_k;
    unsigned off_hh, off_v0, off_v1, off_acc, off_cap, off_srb, off_sof, off_start;     // byte offsets of the LDS arrays behind the tuples
};

// dynamic LDS: tuples float4[N] | hh float2[N] (power laws) | v0 float4[N] | v1 float4[N] | acc double[N], whose bytes first hold the
// sort's keys u32[N rounded up to 4] | cap float[N] | srb int[N], which first holds the movable marks | sof int[N] (slot of link) |
// start int[R + 1] - d2d_assign.hip's layout and size.  v1 = (signal, +-bw_mhz, sensitivity, effective floor): the sign of .y says
// whether the background alone holds the link over its sensitivity (+) or not (-), which d2d_assign.hip keeps in .w

// log2(1 + x) with relative accuracy for small x (d2d_assign.hip's)
__device__ __forceinline__ float log2_1p(float x) {
    const float u = 1.0f + x, um1 = u - 1.0f;
    const float big = __builtin_amdgcn_logf(u) * precise_div(x, um1 == 0.0f ? 1.0f : um1);
    return um1 == 0.0f ? x * 1.44269504088896340736f : big;
}

template <int MODE, bool FLOORS>
__global__ __launch_bounds__(AP_THREADS) void assign_power_weights_kernel(const PowerWeightsArgs a) {
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
    const float ninf = -__builtin_inff();

    // ---- the movable marks, in the bytes of srb (rewritten by the sort, behind the last read of a mark)
    for (int j = tid; j < N; j += AP_THREADS) srb[j] = 0;
    __syncthreads();
    for (int m = tid; m < M; m += AP_THREADS) {
        const int j = a.links[m];
        if ((unsigned)j < (unsigned)N) srb[j] = 1;
    }
    __syncthreads();
    // ---- keys: (rb, link index); a link on no RB and every movable link take the pseudo RB R behind every real one
    same_rb_keys<AP_THREADS>(key, rb_row, N, n4, R);
    for (int j = tid; j < N; j += AP_THREADS)
        if (srb[j]) key[j] = ((unsigned)R << KEY_SHIFT) | (unsigned)j;
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}
    for (int j = tid; j < N; j += AP_THREADS) {
        const int txd = a.link_tx[j];
        const float x = px[txd], y = py[txd];
        const unsigned mine = key[j];
        const bool on_rb = (mine >> KEY_SHIFT) < (unsigned)R;
        // a background link on an RB: the step's tuple.z (d2d_step.hip, pass 1); anyone behind start[R] is walked by nobody and keeps
        // the factor alone, which a movable link's levels multiply
        const float pw = on_rb ? pow10_tenth(pwr_row[j]) * a.cols[txd] : a.cols[txd];
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const int slot = same_rb_rank(key, n4, mine);
        txl[slot] = make_float4(x, y, pw, __int_as_float(j));
        if (POWLAW) hh[slot] = h;
        srb[slot] = (int)(mine >> KEY_SHIFT);
        sof[j] = slot;
    }
    __syncthreads();                 // the last use of key: its bytes are the interference sums from here on
    same_rb_starts<AP_THREADS>(start, srb, N, R);
    __syncthreads();

    // ---- phase 1: the slot's link as receiver (d2d_assign.hip, phase 1); a slot behind start[R] walks nobody
    for (int s = tid; s < N; s += AP_THREADS) {
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
        float eff = ninf;
        if (FLOORS) {
            const float f = a.floor_db[j];
            eff = (f > ninf && sinr_db >= f) ? f : ninf;                 // the background alone under its floor: constrains nothing
        }
        v1[s] = make_float4(sig, ok ? bw_mhz : -bw_mhz, sens, eff);
        accl[s] = acc;
        capl[s] = cap;
    }
    __syncthreads();

    // ---- phase 2: movable link a of the wave on RB r of the lane
    const int wave = tid >> 6, lane = tid & 63;
    const int words = (R + 31) >> 5;
    for (int m = wave; m < M; m += AP_WAVES) {
        const int i = a.links[m];
        const size_t out = (b * (size_t)M + (size_t)m) * (size_t)R;
        int lo = 0, P = 0;
        if ((unsigned)i < (unsigned)N) {
            lo = a.p_min[i];
            const int hi = a.p_max[i];
            const long long levels = (long long)hi - (long long)lo + 1;
            const bool in_range = lo > -4096 && hi < 4096;               // the contract of pow10_tenth: |p| < 4096
            P = in_range && levels >= 1 && levels <= D2D_ASSIGNPWR_MAX_LEVELS ? (int)levels : 0;
        }
        if (P == 0) {                                                     // not a link, or an alphabet outside the contract: a row nobody can take
            for (int r = lane; r < R; r += 64) {
                a.weights[out + r] = ninf;
                a.power[out + r] = D2D_ASSIGNPWR_NO_POWER;
            }
            continue;
        }
        const int s = sof[i];
        const float4 me = txl[s], p = v0[s], q = v1[s];
        const float bw_own = __builtin_fabsf(q.y);
        const float2 h = POWLAW ? hh[s] : make_float2(-1.0f, 0.0f);
        const float rx_lin = a.cols[2 * D + a.link_rx[i]];
        const float odx = me.x - p.x, ody = me.y - p.y;
        const float g_own = pair_gain<MODE>(fmaf(odx, odx, ody * ody), h, a.pow_k);
        const float own_floor = FLOORS ? a.floor_db[i] : ninf;
        const bool has_floor = FLOORS && own_floor > ninf;
        const unsigned* may = a.allowed ? a.allowed + (size_t)i * (size_t)words : nullptr;
        for (int r = lane; r < R; r += 64) {
            const int k_begin = start[r], k_end = start[r + 1];
            // the members of r into link a's receiver: the terms d2d_evaluate.hip adds, in its order
            double acc = 0.0;
            for (int k = k_begin; k < k_end; ++k) {
                const float4 o = txl[k];
                const float dx = o.x - p.x, dy = o.y - p.y;
                const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), POWLAW ? hh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
                acc += (double)(o.z * g);
            }
            const float accf = (float)acc;
            const float den_own = fmaf(accf, p.z, p.w);
            float best = ninf;
            int best_p = D2D_ASSIGNPWR_NO_POWER;
            for (int c0 = 0; c0 < P; c0 += CHUNK) {
                float pw[CHUNK];
                double harm[CHUNK];
                unsigned bad = 0u;                                       // bit l: level c0 + l pushes a constrained victim under its floor
#pragma unroll
                for (int l = 0; l < CHUNK; ++l) {
                    pw[l] = pow10_tenth(lo + c0 + l) * me.z;             // the step's tuple.z at that level
                    harm[l] = 0.0;
                }
                for (int k = k_begin; k < k_end; ++k) {
                    // link a into member k's receiver: what k loses, and whether k keeps its floor
                    const float4 vp = v0[k], vq = v1[k];
                    const double ik = accl[k];
                    const float capk = capl[k];
                    const float fk = FLOORS ? vq.w : ninf;
                    const float bw = __builtin_fabsf(vq.y);
                    const bool alive = __float_as_int(vq.y) >= 0;        // under its threshold already: nothing to lose
                    const bool bound = FLOORS && fk > ninf;
                    if (!alive && !bound) continue;
                    const float ex = me.x - vp.x, ey = me.y - vp.y;
                    const float gv = pair_gain<MODE>(fmaf(ex, ex, ey * ey), h, a.pow_k);
                    const double rx_pl = (double)vp.z, noise = (double)vp.w, sig = (double)vq.x;
                    const double den = fma(ik, rx_pl, noise);            // without link a
#pragma unroll
                    for (int l = 0; l < CHUNK; ++l) {
                        if (c0 + l < P) {
                            const float t = pw[l] * gv;
                            const double td = (double)t;
                            const double denw = fma(ik + td, rx_pl, noise);      // with it
                            const float sw = (float)(sig / denw);
                            const float with_db = 3.01029995663981195f * __builtin_amdgcn_logf(sw);
                            if (alive) {
                                // still over its threshold with link a (the step's test, simulator.py:123):
                                // log2(1 + S t rx_pl / (den (den' + S)))
                                const bool ok_with = with_db > vq.z;
                                const float x = (float)(sig * rx_pl * td / (den * (denw + sig)));
                                const float loss = ok_with ? bw * log2_1p(x) : capk;
                                harm[l] += (double)loss;
                            }
                            if (bound && !(with_db >= fk)) bad |= 1u << l;
                        }
                    }
                }
                // link a's capacity on r at every level of the chunk: the step's operations in the step's order, as
                // d2d_evaluate.hip forms it; ascending power, strict >: equal weights go to the lowest power
#pragma unroll
                for (int l = 0; l < CHUNK; ++l) {
                    if (c0 + l < P) {
                        const float sig = pw[l] * g_own * p.z * rx_lin;
                        const float sinr_lin = precise_div(sig, den_own);
                        const float sinr_db = 3.01029995663981195f * __builtin_amdgcn_logf(sinr_lin);
                        const float u1p = 1.0f + sinr_lin, um1 = u1p - 1.0f;
                        const float sh_big = __builtin_amdgcn_logf(u1p) * fast_div(sinr_lin, um1 == 0.0f ? 1.0f : um1);
                        const float sh = um1 == 0.0f ? sinr_lin * 1.44269504088896340736f : sh_big;
                        const float cap = sinr_db > q.z ? bw_own * sh : 0.0f;
                        const float w = (float)((double)cap - harm[l]);
                        const bool admissible = !((bad >> l) & 1u) && (!has_floor || sinr_db >= own_floor);
                        if (admissible && w > best) { best = w; best_p = lo + c0 + l; }
                    }
                }
            }
            const bool free_rb = !may || ((may[r >> 5] >> (r & 31)) & 1u);
            a.weights[out + r] = free_rb ? best : ninf;
            a.power[out + r] = free_rb ? best_p : D2D_ASSIGNPWR_NO_POWER;
        }
    }
}

}  // namespace

extern "C" int d2d_assign_power_weights(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm,
                                        const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols,
                                        int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs,
                                        const int32_t* movable_links, int32_t n_movable, const uint32_t* allowed, const int32_t* p_min,
                                        const int32_t* p_max, const float* floor_db, float* weights, int32_t* power_dbm,
                                        void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_ASSIGNPWR_MAX_LINKS, n_rbs, D2D_ASSIGNPWR_MAX_RBS, n_dev)) return fail(why);
    if (n_movable < 1 || n_movable > n_links) return fail("n_movable must be in [1, n_links]");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !cap_cols || !movable_links || !p_min || !p_max ||
        !weights || !power_dbm)
        return fail("null device pointer");
    if (static_cast<void*>(weights) == static_cast<void*>(power_dbm)) return fail("weights and power_dbm must be two planes");
    PowerWeightsArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols;
    a.cap_cols = cap_cols; a.links = movable_links; a.allowed = allowed; a.p_min = p_min; a.p_max = p_max; a.floor_db = floor_db;
    a.weights = weights; a.power = power_dbm;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.M = n_movable; a.pow_k = pow_k;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_hh = N * 16u;
    a.off_v0 = a.off_hh + (law == D2D_ASSIGNPWR_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_v1 = a.off_v0 + N * 16u;
    a.off_acc = a.off_v1 + N * 16u;
    a.off_cap = a.off_acc + round16(n4 * 8u);                            // doubles; the sort's keys (n4 * 4 bytes) fit inside
    a.off_srb = a.off_cap + round16(N * 4u);
    a.off_sof = a.off_srb + round16(N * 4u);
    a.off_start = a.off_sof + round16(N * 4u);
    const unsigned lds = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    if (lds > (unsigned)D2D_ASSIGNPWR_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(lds) + " bytes of LDS, more than the " +
                    std::to_string(D2D_ASSIGNPWR_MAX_LDS_BYTES) + " a workgroup can have");
    if (n_envs == 0) return 0;
    const dim3 grid((unsigned)n_envs), block(AP_THREADS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e;
    const bool floors = floor_db != nullptr;
    if (law == D2D_ASSIGNPWR_LAW_INV_SQUARE)
        e = floors ? launch(&assign_power_weights_kernel<PL_INV_SQUARE, true>, grid, block, lds, s, a)
                   : launch(&assign_power_weights_kernel<PL_INV_SQUARE, false>, grid, block, lds, s, a);
    else if (law == D2D_ASSIGNPWR_LAW_POWER)
        e = floors ? launch(&assign_power_weights_kernel<PL_POWER, true>, grid, block, lds, s, a)
                   : launch(&assign_power_weights_kernel<PL_POWER, false>, grid, block, lds, s, a);
    else
        e = floors ? launch(&assign_power_weights_kernel<PL_POWK, true>, grid, block, lds, s, a)
                   : launch(&assign_power_weights_kernel<PL_POWK, false>, grid, block, lds, s, a);
    if (e != hipSuccess) return fail(std::string("assign_power_weights_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_assignpwr_last_error)
