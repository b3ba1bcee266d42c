// libd2d_queue.so (include/d2d_queue.h): one step of every link's packet queue of every env, one launch.  gfx950.
//
// Shape: mobility_move_kernel's (d2d_mobility.hip) - one thread per (env, link), every word written by the one thread that owns it:
// no atomics, no scratch.  The two 64-entry threshold tables travel in the kernel's arguments and are staged in 512 bytes of LDS per
// workgroup, where the arrival count is a 7-probe binary search.  The ring is slot-major [D][B][N]: consecutive lanes hold consecutive
// links, so every ring access of a wave is one run of consecutive words.  Memory-bound: the slot that expires is read once, the drain
// reads older slots oldest first only while unserved bits remain ahead of it, and a slot is written only if its value changed - at
// most 8 D bytes of ring traffic per link and step, plus 40 bytes of planes (capacity and backlog read, on read and written, seven
// planes written).  All arithmetic is integer but the budget (one double multiply) and the mean delay (one double divide).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "d2d_addon.h"
#include "d2d_queue.h"
#include "d2d_step_device.h"

namespace {

constexpr int kTable = D2D_QUEUE_TABLE;

struct QueueArgs {
    const float* capacity;
    int* ring;
    int* arrived;
    int* served;
    int* expired;
    int* overflow;
    int* backlog;
    int* hol_age;
    float* mean_delay;
    unsigned char* on;
    const int* elapsed_env;         // per-env clock (reset_env != null), else the scalars step / episode
    int* start_env;
    const unsigned* episode_env;
    const int* reset_env;
    double bits_per_step;
    unsigned links, links_magic;    // links per env, floor(2^32 / links)
    unsigned cues;
    unsigned total;                 // n_envs * links: also the ring's slot stride
    int D, packet_bits, buffer_bits;
    unsigned p_on_to_off, p_off_to_on, p_start_on;
    unsigned first_env, seed_lo, seed_hi, step, episode;
    unsigned table[2 * kTable];
};

// how many of the 64 non-decreasing entries of t are <= w
__device__ __forceinline__ int count_not_above(const unsigned* t, unsigned w) {
    int k = 0;
#pragma unroll
    for (int s = kTable / 2; s; s >>= 1)
        if (t[k + s - 1] <= w) k += s;
    return k + (t[k] <= w ? 1 : 0);                                      // k <= 63 here: the 64th entry
}

__device__ __forceinline__ int service_budget(float capacity_mbps, double bits_per_step) {
    const double x = (double)capacity_mbps * bits_per_step;
    if (!(x > 0.0)) return 0;                                            // NaN, negative, zero
    return x >= 2147483647.0 ? 2147483647 : (int)x;                      // x > 0: the conversion truncates = floor
}

__global__ __launch_bounds__(256) void queue_step_kernel(const QueueArgs a) {
    __shared__ unsigned tab[2 * kTable];
    if (threadIdx.x < 2u * kTable) tab[threadIdx.x] = a.table[threadIdx.x];
    __syncthreads();
    const unsigned gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= a.total) return;
    unsigned b = __umulhi(gid, a.links_magic);                           // gid / links: the estimate is exact or one short
    unsigned i = gid - b * a.links;
    if (i >= a.links) { i -= a.links; ++b; }
    unsigned episode, t;
    if (a.reset_env) {
        const unsigned next = a.episode_env[b];
        if (a.reset_env[b] != 0) {
            episode = next; t = 0u;
            if (i == 0u) a.start_env[b] = 0;                             // read by envs that step only: never by this env in this launch
        } else {
            episode = next - 1u; t = (unsigned)(a.elapsed_env[b] - a.start_env[b]) + 1u;
        }
    } else {
        episode = a.episode; t = a.step;
    }
    unsigned w0, w1;
    d2d::philox_step(a.first_env + b, episode, t, i, a.seed_lo, a.seed_hi, w0, w1);
    const size_t stride = a.total;
    int* const ring = a.ring + gid;                                      // slot s of this link: ring[s * stride]

    if (t == 0u) {                                                       // start of the episode
        for (int s = 0; s < a.D; ++s) ring[(size_t)s * stride] = 0;
        a.arrived[gid] = 0; a.served[gid] = 0; a.expired[gid] = 0; a.overflow[gid] = 0; a.backlog[gid] = 0; a.hol_age[gid] = 0;
        a.mean_delay[gid] = 0.0f;
        a.on[gid] = (a.p_on_to_off == 0u || w0 < a.p_start_on) ? 1 : 0;
        return;
    }

    // 1  on/off source
    bool on = a.on[gid] != 0;
    on = on ? !(w0 < a.p_on_to_off) : (w0 < a.p_off_to_on);
    if (a.p_on_to_off == 0u) on = true;
    // 2  arrivals
    const int k = on ? count_not_above(tab + (i < a.cues ? 0 : kTable), w1) : 0;
    // 3  deadline: slot t mod D holds what arrived at step t - D
    const int s = (int)(t % (unsigned)a.D);
    const int expired = ring[(size_t)s * stride];
    const int kept = a.backlog[gid] - expired;
    // 4  finite buffer, tail drop
    int room = a.buffer_bits - kept;
    if (room < 0) room = 0;
    int n = room / a.packet_bits;
    if (n > k) n = k;
    const int admitted = n * a.packet_bits;
    // 5  service, oldest first
    int budget = service_budget(a.capacity[gid], a.bits_per_step);
    int served = 0, hol = 0;
    long long delay_sum = 0;
    int ahead = kept;                                                    // unserved bits in the cohorts not yet visited
    for (int age = a.D - 1; age >= 1 && ahead > 0; --age) {
        int slot = s - age;
        if (slot < 0) slot += a.D;
        int* const p = ring + (size_t)slot * stride;
        const int v = *p;
        if (v == 0) continue;
        const int take = v < budget ? v : budget;
        if (take) {
            *p = v - take;
            budget -= take; served += take; delay_sum += (long long)take * age;
        }
        ahead -= v;
        if (take < v) { hol = age; break; }                              // the budget is spent: every newer cohort stays as it is
    }
    const int take = admitted < budget ? admitted : budget;
    served += take;
    if (admitted - take != expired) ring[(size_t)s * stride] = admitted - take;

    a.on[gid] = on ? 1 : 0;
    a.arrived[gid] = k * a.packet_bits;
    a.served[gid] = served;
    a.expired[gid] = expired;
    a.overflow[gid] = (k - n) * a.packet_bits;
    a.backlog[gid] = kept + admitted - served;
    a.hol_age[gid] = hol;
    a.mean_delay[gid] = served ? (float)((double)delay_sum / (double)served) : 0.0f;
}

}  // namespace

extern "C" int d2d_queue_step(const float* capacity_mbps, int32_t* ring, int32_t* arrived_bits, int32_t* served_bits,
                              int32_t* expired_bits, int32_t* overflow_bits, int32_t* backlog_bits, int32_t* hol_age_steps,
                              float* mean_delay_steps, uint8_t* on, const uint32_t* thresholds, int64_t n_envs, int32_t n_cues,
                              int32_t n_due_pairs, int32_t deadline_steps, int64_t packet_bits, int64_t buffer_bits,
                              double bits_per_mbps_step, uint32_t p_on_to_off, uint32_t p_off_to_on, uint32_t p_start_on,
                              uint64_t first_env, uint64_t seed, uint32_t step, uint32_t episode, const int32_t* elapsed_env,
                              int32_t* start_env, const uint32_t* episode_env, const int32_t* reset_env, void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_cues < 0 || n_due_pairs < 0 || n_cues > (1 << 24) || n_due_pairs > (1 << 24)) return fail("n_cues and n_due_pairs must be in [0, 2^24]");
    if (first_env + (uint64_t)n_envs > (1ull << 32)) return fail("first_env + n_envs must not exceed 2^32 (the env counter word)");
    if (deadline_steps < 1 || deadline_steps > D2D_QUEUE_MAX_DEADLINE) return fail("deadline_steps must be in [1, 32]");
    if (packet_bits < 1 || packet_bits * kTable >= (1ll << 31)) return fail("packet_bits must be >= 1 and 64 * packet_bits below 2^31");
    if (buffer_bits < 0 || buffer_bits >= (1ll << 31)) return fail("buffer_bits must be in [0, 2^31)");
    if (!(bits_per_mbps_step > 0.0) || !std::isfinite(bits_per_mbps_step)) return fail("bits_per_mbps_step must be finite and > 0");
    if (!thresholds) return fail("thresholds must be a host array of 2 x 64 words");
    for (int c = 0; c < 2; ++c)
        for (int k = 1; k < kTable; ++k)
            if (thresholds[c * kTable + k] < thresholds[c * kTable + k - 1]) return fail("thresholds: a table must not decrease");
    if (!capacity_mbps || !ring || !arrived_bits || !served_bits || !expired_bits || !overflow_bits || !backlog_bits || !hol_age_steps ||
        !mean_delay_steps || !on)
        return fail("null device pointer");
    if (reset_env && (!elapsed_env || !start_env || !episode_env)) return fail("the per-env clock needs elapsed_env, start_env and episode_env");
    const unsigned links = (unsigned)n_cues + (unsigned)n_due_pairs;
    const unsigned long long total = (unsigned long long)n_envs * links;
    if (total >= 0xFFFFFF00ull) return fail("n_envs * (n_cues + n_due_pairs) must stay below 2^32 - 256");
    if (total == 0) return 0;
    QueueArgs a;
    a.capacity = capacity_mbps; a.ring = ring; a.arrived = arrived_bits; a.served = served_bits; a.expired = expired_bits;
    a.overflow = overflow_bits; a.backlog = backlog_bits; a.hol_age = hol_age_steps; a.mean_delay = mean_delay_steps; a.on = on;
    a.elapsed_env = elapsed_env; a.start_env = start_env; a.episode_env = episode_env; a.reset_env = reset_env;
    a.bits_per_step = bits_per_mbps_step;
    a.links = links;
    a.links_magic = links == 1u ? 0xFFFFFFFFu : (unsigned)(0x100000000ull / links);           // one short at most: the kernel corrects
    a.cues = (unsigned)n_cues;
    a.total = (unsigned)total;
    a.D = deadline_steps; a.packet_bits = (int)packet_bits; a.buffer_bits = (int)buffer_bits;
    a.p_on_to_off = p_on_to_off; a.p_off_to_on = p_off_to_on; a.p_start_on = p_start_on;
    a.first_env = (unsigned)first_env;
    a.seed_lo = (unsigned)(seed & 0xFFFFFFFFull); a.seed_hi = (unsigned)(seed >> 32);
    a.step = step; a.episode = episode;
    for (int k = 0; k < 2 * kTable; ++k) a.table[k] = thresholds[k];
    hipLaunchKernelGGL(queue_step_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("queue_step_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_queue_last_error)
