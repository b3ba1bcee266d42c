// libd2d_sense.so (include/d2d_sense.h): every link's interference / SINR on every resource block, one launch.  gfx950.
//
// Shape: grid = (env, block of 256 receivers), 256 threads.  The workgroup sorts the env's N links by (rb, link index) into LDS -
// a rank sort on the packed keys rb * 2048 + j, read back four keys per ds_read_b128 at a wave-uniform address: stable, so the
// members of an RB stand in ascending j, and free of atomics, so the order is the same on every call - as transmitter tuples
// (tx x, tx y, linear EIRP incl. the tx side of the path-loss constant, link index), with the per-tx law constants beside them and
// start[r] = the first entry of RB r.  Then LANES OWN RECEIVERS: a wave's 64 lanes walk the sorted list in lockstep (every tuple
// read is an LDS broadcast, the trip counts are wave-uniform: no divergence), close the running sum at every RB boundary and put
// the finished value into a [32 RBs][64 receivers] tile of their wave in LDS (row pitch 65 floats: both the column writes and the
// transposed reads spread over the banks).  After 32 RBs the wave writes the tile out transposed, so that every output row
// out[b][i][r0 .. r0 + 32) leaves as 128 contiguous bytes in 16-byte nontemporal stores (the block is written once and not
// read by the GPU here).  The pair evaluation is the step's (d2d_step_device.h: fmaf(dx, dx, dy * dy), pair_gain, float products
// into a double accumulator, precise_div, v_log_f32), so column rb[b][i] reproduces the step's sinr_db.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_sense.h"
#include "d2d_same_rb.h"
#include "d2d_step_device.h"
#include "d2d_store.h"

namespace {

using namespace d2d;

constexpr int SENSE_THREADS = 256;
constexpr int SENSE_WAVES = SENSE_THREADS / 64;
constexpr int TILE_RBS = 32;
constexpr int TILE_PITCH = 65;                                   // floats per RB row of a wave's tile: 64 receivers + 1
constexpr unsigned TILE_BYTES = TILE_RBS * TILE_PITCH * 4u;      // per wave
static_assert(D2D_SENSE_MAX_LINKS == SAME_RB_MAX_LINKS && D2D_SENSE_MAX_RBS == SAME_RB_MAX_RBS, "the limits of the shared sort (d2d_same_rb.h)");
static_assert(D2D_SENSE_LAW_INV_SQUARE == LAW_INV_SQUARE && D2D_SENSE_LAW_POWER == LAW_POWER && D2D_SENSE_LAW_POW_K == LAW_POW_K, "the laws check_law() knows (d2d_addon.h)");

struct SenseArgs {
    const float* pos_x;
    const float* pos_y;
    const int* rb;
    const int* pwr;
    const int* link_tx;
    const int* link_rx;
    const float* cols;              // [6][D]
    float* out;
    int D, N, R;
    int pow_k;
    int vec_ok;                     // out is 16-byte aligned and R % 4 == 0: a tile whose width is a multiple of 4 goes out in float4
    unsigned off_hh, off_start, off_tile;       // byte offsets of the LDS arrays behind the tuples
};

// dynamic LDS: tuples float4[N] | hh float2[N] (power laws) | start int[R + 1] | tiles float[4][32 * 65], whose bytes first hold the
// sort's keys u32[N rounded up to 4] and the sorted rb values int[N]

template <int MODE, int WHAT>
__global__ __launch_bounds__(SENSE_THREADS) void sense_kernel(const SenseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const int N = a.N, R = a.R, D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    float4* txl = reinterpret_cast<float4*>(smem);
    float2* hh = reinterpret_cast<float2*>(smem + a.off_hh);
    int* start = reinterpret_cast<int*>(smem + a.off_start);
    unsigned* key = reinterpret_cast<unsigned*>(smem + a.off_tile);
    const int n4 = (N + 3) & ~3;
    int* srb = reinterpret_cast<int*>(key + n4);
    const int* rb_row = a.rb + b * (size_t)N;
    const int* pwr_row = a.pwr + b * (size_t)N;
    const float* px = a.pos_x + b * (size_t)D;
    const float* py = a.pos_y + b * (size_t)D;

    // ---- keys: (rb, link index); a link whose rb is outside [0, R) takes the pseudo RB R behind every real one
    same_rb_keys<SENSE_THREADS>(key, rb_row, N, n4, R);
    __syncthreads();
    // ---- rank sort: link j goes to slot #{keys below its own}; the keys are distinct, so the slots are a permutation
    for (int j = tid; j < N; j += SENSE_THREADS) {
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
    }
    __syncthreads();
    // ---- start[r]: the first sorted entry whose RB is >= r, r in [0, R]; entries from start[R] on are on no RB
    same_rb_starts<SENSE_THREADS>(start, srb, N, R);
    __syncthreads();                 // the last use of key / srb: their bytes are the tiles from here on

    // ---- lanes own receivers
    const int i0 = (int)blockIdx.y * SENSE_THREADS + wave * 64;          // this wave's first receiver
    if (i0 >= N) return;                                                 // (no workgroup barrier below)
    const int rows = min(64, N - i0);
    const int i = min(i0 + lane, N - 1);                                 // lanes past the last link shadow it; their rows are not stored
    const int txd = a.link_tx[i], rxd = a.link_rx[i];
    const float rx_x = px[rxd], rx_y = py[rxd];
    const float rx_pl = a.cols[D + rxd], rx_lin = a.cols[2 * D + rxd], noise = a.cols[3 * D + rxd];
    float sig = 0.0f;
    if (WHAT == D2D_SENSE_SINR_DB) {
        // own link: simulator.py:93, as the step forms it
        const float tx_x = px[txd], tx_y = py[txd];
        const float me_z = pow10_tenth(pwr_row[i]) * a.cols[txd];
        float2 h = make_float2(-1.0f, 0.0f);
        if (POWLAW) h = make_float2(a.cols[4 * D + txd], a.cols[5 * D + txd]);
        const float dx = tx_x - rx_x, dy = tx_y - rx_y;
        const float g = pair_gain<MODE>(fmaf(dx, dx, dy * dy), h, a.pow_k);
        sig = me_z * g * rx_pl * rx_lin;
    }
    float* tile = reinterpret_cast<float*>(smem + a.off_tile + (unsigned)wave * TILE_BYTES);
    float* out_wave = a.out + (b * (size_t)N + (size_t)i0) * (size_t)R;

    for (int r0 = 0; r0 < R; r0 += TILE_RBS) {
        const int cw = min(TILE_RBS, R - r0);
        int k = __builtin_amdgcn_readfirstlane(start[r0]);
        for (int c = 0; c < cw; ++c) {
            const int k_end = __builtin_amdgcn_readfirstlane(start[r0 + c + 1]);
            double acc = 0.0;
            for (; k < k_end; ++k) {
                const float4 o = txl[k];
                const float dx = o.x - rx_x, dy = o.y - rx_y;
                const float d2 = fmaf(dx, dx, dy * dy);
                const float g = pair_gain<MODE>(d2, POWLAW ? hh[k] : make_float2(-1.0f, 0.0f), a.pow_k);
                const float term = o.z * g;                                  // simulator.py:97-101, linear mW
                acc += __float_as_int(o.w) != i ? (double)term : 0.0;        // j != i by link index
            }
            const float accf = (float)acc;
            float v;
            if (WHAT == D2D_SENSE_SINR_DB) v = 3.01029995663981195f * __builtin_amdgcn_logf(precise_div(sig, fmaf(accf, rx_pl, noise)));
            else v = accf * rx_pl;
            tile[c * TILE_PITCH + lane] = v;
        }
        // the tile belongs to this wave alone, whose LDS operations complete in issue order
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float* base = out_wave + r0;
        const int total = rows * cw;
        if (a.vec_ok && (cw & 3) == 0) {
            for (int e = lane * 4; e < total; e += 256) {
                int row, col;
                if (cw == TILE_RBS) { row = e >> 5; col = e & 31; }
                else { row = e / cw; col = e - row * cw; }
                const float* t = tile + col * TILE_PITCH + row;
                const f32x4 v = {t[0], t[TILE_PITCH], t[2 * TILE_PITCH], t[3 * TILE_PITCH]};
                store16<1>(reinterpret_cast<f32x4*>(base + (size_t)row * (size_t)R + col), v);
            }
        } else {
            for (int e = lane; e < total; e += 64) {
                const int row = e / cw, col = e - row * cw;
                __builtin_nontemporal_store(tile[col * TILE_PITCH + row], base + (size_t)row * (size_t)R + col);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

extern "C" int d2d_sense_rb(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                            const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                            int32_t n_links, int32_t n_rbs, int32_t what, float* out, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_SENSE_MAX_LINKS, n_rbs, D2D_SENSE_MAX_RBS, n_dev)) return fail(why);
    if (what != D2D_SENSE_SINR_DB && what != D2D_SENSE_INTERFERENCE_MW) return fail("what must be D2D_SENSE_SINR_DB or D2D_SENSE_INTERFERENCE_MW");
    if (const char* why = check_law(law, pow_k)) return fail(why);
    if (!pos_x || !pos_y || !rb || !pwr_dbm || !link_tx || !link_rx || !dev_cols || !out) return fail("null device pointer");
    if (n_envs == 0) return 0;
    SenseArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.rb = rb; a.pwr = pwr_dbm; a.link_tx = link_tx; a.link_rx = link_rx; a.cols = dev_cols; a.out = out;
    a.D = n_dev; a.N = n_links; a.R = n_rbs; a.pow_k = pow_k;
    a.vec_ok = reinterpret_cast<uintptr_t>(out) % 16 == 0 && n_rbs % 4 == 0;
    const unsigned N = (unsigned)n_links, n4 = (N + 3u) & ~3u;
    a.off_hh = N * 16u;
    a.off_start = a.off_hh + (law == D2D_SENSE_LAW_INV_SQUARE ? 0u : round16(N * 8u));
    a.off_tile = a.off_start + round16(((unsigned)n_rbs + 1u) * 4u);
    const unsigned sort_bytes = n4 * 4u + N * 4u, tile_bytes = SENSE_WAVES * TILE_BYTES;
    const unsigned lds = a.off_tile + (sort_bytes > tile_bytes ? sort_bytes : tile_bytes);
    if (lds > 160u * 1024u) return fail("n_links and n_rbs need more than the 160 KiB of LDS a workgroup can have");
    const dim3 grid((unsigned)n_envs, (N + SENSE_THREADS - 1) / SENSE_THREADS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bool sinr = what == D2D_SENSE_SINR_DB;
    void (*kernel)(SenseArgs);
    if (law == D2D_SENSE_LAW_INV_SQUARE) kernel = sinr ? &sense_kernel<PL_INV_SQUARE, D2D_SENSE_SINR_DB> : &sense_kernel<PL_INV_SQUARE, D2D_SENSE_INTERFERENCE_MW>;
    else if (law == D2D_SENSE_LAW_POWER) kernel = sinr ? &sense_kernel<PL_POWER, D2D_SENSE_SINR_DB> : &sense_kernel<PL_POWER, D2D_SENSE_INTERFERENCE_MW>;
    else kernel = sinr ? &sense_kernel<PL_POWK, D2D_SENSE_SINR_DB> : &sense_kernel<PL_POWK, D2D_SENSE_INTERFERENCE_MW>;
    const hipError_t e = launch(kernel, grid, dim3(SENSE_THREADS), lds, s, a);
    if (e != hipSuccess) return fail(std::string("sense_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_sense_last_error)
