/* libd2d_queue.so - finite-buffer packet traffic with deadlines: every link's on/off source, Poisson arrivals, deadline ring, tail
 * drop and oldest-first service behind the step's capacity, one launch per step
 * (gym_d2d_amd.envs.VecD2DEnv(traffic=PacketTraffic(...))).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.  It
 * reads the plane a handle has bound as D2D_BUF_CAPACITY after the step kernel has written it, and nothing else of the handle.
 *
 * Links of one env, as the step orders them: 0 .. n_cues - 1 the CUE links (class 0), then n_due_pairs DUE links (class 1);
 * n_links = n_cues + n_due_pairs.  All quantities are integers (bits, steps) but mean_delay_steps; nothing on the device touches a
 * floating-point CDF, so a restatement in integers equals the kernel bit for bit.
 *
 * d2d_queue_step, per env b and link i, with the env's clock (episode e, step t, see below) and the two draw words
 * (w0, w1) = words 0 and 1 of Philox4x32-10 at
 *
 *       counter word 0   the GLOBAL env index first_env + b (< 2^32)
 *       counter word 1   e, the episode index
 *       counter word 2   t, the step in the episode; 0 is the start-of-episode draw
 *       counter word 3   i, the link index in the env
 *       key              seed, low word then high word
 *
 *   t == 0, the start of episode e: the link's ring is cleared, every output plane is 0, and the on/off state is drawn from the
 *     stationary distribution:  on = (p_on_to_off == 0) || (w0 < p_start_on).  Nothing arrives and nothing is served.
 *
 *   t >= 1, step t of episode e, in this order:
 *     1  on/off source, a two-state Markov chain: an ON link switches off if w0 < p_on_to_off, an OFF link switches on if
 *        w0 < p_off_to_on.  p_on_to_off == 0: every link is always on.  The new state is the one this step's arrivals see.
 *     2  arrivals: an ON link receives k packets of packet_bits each, k = the number of entries of its class's 64-entry threshold
 *        table that are <= w1 (the table is the Poisson CDF scaled to 2^32, see `thresholds`); an OFF link receives 0.
 *        arrived_bits = k * packet_bits.
 *     3  deadline: the ring holds, per link, the unserved bits of the packets that arrived at each of the last D = deadline_steps
 *        steps, the cohort of step t in slot t mod D.  What slot t mod D still holds arrived at step t - D, has had its D chances
 *        and is expired_bits; the slot is cleared.
 *     4  finite buffer, tail drop: with backlog' = backlog - expired_bits, n = min(k, (buffer_bits - backlog') / packet_bits) whole
 *        packets are admitted into slot t mod D; overflow_bits = (k - n) * packet_bits.  The new packets are the ones that drop.
 *     5  service: budget = floor((double)capacity_mbps[b][i] * bits_per_mbps_step) clipped to [0, 2^31 - 1]; a NaN, negative or
 *        zero capacity gives 0, +inf gives 2^31 - 1.  The budget drains the cohorts oldest first (age D - 1 down to age 0, this
 *        step's arrivals); bits are fluid, a packet may be partly served.  served_bits is what was drained, mean_delay_steps =
 *        sum(bits * age) / served_bits with the sum in int64, the division in double, rounded once to float32; 0.0 if nothing was
 *        served.  backlog_bits is what the ring holds afterwards, hol_age_steps the age of the oldest non-empty cohort (0: empty).
 *
 *   Simplification: a link whose buffer is empty still transmits (and interferes) in the step kernel - that kernel has no off
 *   state; the queue only decides how many of the bits the link could carry were there to be carried.
 *
 *   Nothing of launch geometry or of how a batch is sharded enters: shards given their first_env draw what the whole batch draws.
 *   `seed` is the TRAFFIC seed - keep it apart from the mobility, shadowing and fading seeds, whose streams share the generator.
 *
 * The clock is d2d_mobility.h's.  In lockstep (reset_env == NULL) every env stands at the scalars `episode` and `step`.  With
 * per-env episodes (reset_env != NULL; the three arrays beside it then must not be NULL, `step` and `episode` are ignored):
 *
 *   reset_env[b] != 0   the env is being reset in this step (D2D_BUF_RESET_PENDING): e = episode_env[b], t = 0;
 *                       start_env[b] = 0 is written
 *   reset_env[b] == 0   e = episode_env[b] - 1, t = elapsed_env[b] - start_env[b] + 1
 *
 *   episode_env  u32 [n_envs]  D2D_BUF_EPISODE: the index an env's NEXT reset draws at, hence one more than the episode it stands in
 *   elapsed_env  i32 [n_envs]  steps the env has taken in its episode (d2d_episode_advance's elapsed), read before that step's advance
 *   start_env    i32 [n_envs]  what elapsed_env[b] was when the env's queues were started: the stagger of a first episode, 0 later
 *
 * Planes, all [n_envs][n_links], updated in place: arrived_bits, served_bits, expired_bits, overflow_bits, backlog_bits,
 * hol_age_steps i32; mean_delay_steps f32; on u8.  capacity_mbps f32 [n_envs][n_links] is read only.
 * ring  i32 [D][n_envs][n_links]: SLOT-MAJOR, so that the 64 lanes of a wave - consecutive links of one env - read and write
 *       consecutive words of one slot; a link-major [n_envs][n_links][D] ring would stride every access by 4 D bytes.
 * thresholds  u32 [2][64] in HOST memory (it travels in the kernel's arguments): class 0 the CUE links, class 1 the DUE links;
 *       T_k = min(2^32 - 1, floor(c_k * 2^32)), c_k the running sum of p_0 = exp(-lambda), p_k = p_{k-1} * lambda / k in double,
 *       lambda <= 16 packets per step (the mass beyond 64 entries is then far below 2^-32).  Each table must not decrease.
 * p_on_to_off, p_off_to_on, p_start_on  u32 thresholds min(2^32 - 1, floor(p * 2^32)); "switch" means word < threshold.
 * bits_per_mbps_step  the double 1e6 * dt_s, formed by the caller; finite and > 0.
 *
 * n_envs >= 0 (0: nothing to do), n_cues, n_due_pairs >= 0, first_env + n_envs <= 2^32, 1 <= deadline_steps <= 32,
 * 1 <= packet_bits, 64 * packet_bits < 2^31, 0 <= buffer_bits < 2^31.  Bad arguments are refused before any launch.
 * Returns 0, or non-zero with a message in d2d_queue_last_error().                                                              */
#ifndef D2D_QUEUE_H
#define D2D_QUEUE_H

#include <stdint.h>

#define D2D_QUEUE_MAX_DEADLINE 32
#define D2D_QUEUE_TABLE 64

#ifdef __cplusplus
extern "C" {
#endif

int d2d_queue_step(const float* capacity_mbps, int32_t* ring, int32_t* arrived_bits, int32_t* served_bits, int32_t* expired_bits,
                   int32_t* overflow_bits, int32_t* backlog_bits, int32_t* hol_age_steps, float* mean_delay_steps, uint8_t* on,
                   const uint32_t* thresholds, int64_t n_envs, int32_t n_cues, int32_t n_due_pairs, int32_t deadline_steps,
                   int64_t packet_bits, int64_t buffer_bits, double bits_per_mbps_step, uint32_t p_on_to_off, uint32_t p_off_to_on,
                   uint32_t p_start_on, uint64_t first_env, uint64_t seed, uint32_t step, uint32_t episode,
                   const int32_t* elapsed_env, int32_t* start_env, const uint32_t* episode_env, const int32_t* reset_env,
                   void* hip_stream);
const char* d2d_queue_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_QUEUE_H */
