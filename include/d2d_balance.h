/* libd2d_balance.so - max-min SINR balancing with protected links (gym_d2d_amd.envs.VecD2DEnv.balance_sinr, balance_sinr_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_balance_sinr finds, per env b, the largest level k of an ascending grid margins_db[0 .. n_margins) at which the targets
 * base_db[i] + margins_db[k] can be given to every adjustable link at once with every floor kept, and the least powers that do it.
 *
 * PROBE k is d2d_power_control's iteration (include/d2d_powerctl.h) for the target t_k[i] = base_db[i] + margins_db[k], one float32
 * addition: cold from p_min, at most max_iters sweeps, the same operands in the same order - its final powers, SINRs and
 * converged flag are what d2d_power_control returns for t_k, bit for bit.  There is no warm start.  The probe PASSES iff
 *
 *   it converged, and
 *   no adjustable link on an RB sits at its p_max with sinr_db < t_k[i], and
 *   no link on an RB, adjustable or not, has sinr_db < floor_db[i]
 *
 * in float32 comparisons on the probe's final plane (a NaN comparison is false; a link below its maximum at a fixed point meets its
 * target up to the rounding of ceilf and is not compared).  The floor test is exact: the least fixed point lies componentwise below
 * every power vector that meets the targets, and lower adjustable powers only raise the other links' SINR.
 *
 * THE SEARCH is fixed, so that `probes` is a result:  probe 0 first; if it fails the env is infeasible (level -1, margin_db -inf,
 * power_dbm / sinr_db of probe 0, probes 1).  Otherwise lo = 0, hi = n_margins; while hi - lo > 1: probe mid = (lo + hi) / 2, a
 * pass sets lo = mid, a fail sets hi = mid.  level = lo, margin_db = margins_db[lo], power_dbm / sinr_db those of probe lo.  Without
 * assuming anything monotone: level passes, and level + 1 is n_margins or fails.  At most 1 + ceil(log2 n_margins) <= 13 probes.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_power_control takes them
 *   base_db            f32 [n_links]: every link's target SINR at margin 0, dB
 *   floor_db           f32 [n_links] or NULL: the SINR a link on an RB must keep, dB; -inf: none for that link.  NULL: no floors
 *   margins_db         f32 [n_margins]: the grid, strictly ascending (the caller's promise; the search above is defined without it)
 *   n_margins          1 .. D2D_BALANCE_MAX_MARGINS
 *   p_min, p_max, adjustable, max_iters, env_mask
 *                      as d2d_power_control takes them; the workgroup of an env whose env_mask byte is 0 returns at once and that
 *                      env's rows of the five outputs stay as they were
 *   power_dbm          i32 [n_envs][n_links]: the powers of probe `level` (probe 0 where infeasible)
 *   sinr_db            f32 [n_envs][n_links]: every link's SINR at power_dbm, recomputed from the kept powers (the probe's bits)
 *   margin_db          f32 [n_envs]: margins_db[level], -inf where infeasible
 *   level              i32 [n_envs]: -1 where infeasible
 *   probes             i32 [n_envs]: the probes run
 *
 * One workgroup of 256 threads per env runs the whole search out of LDS; the only global read inside the loops is margins_db[mid].
 * No atomics, no scratch memory.  LDS bytes, with round16(x) = x rounded up to 16 and n4 = n_links rounded up to 4:
 *
 *   32 n_links + (2 + has_power_law) round16(8 n_links) + 28 n4 + round16(4 (n_rbs + 1)) + 64
 *
 * (has_power_law = law != D2D_BALANCE_LAW_INV_SQUARE): d2d_power_control's arrays with the base in the target's place, plus the
 * floor and the best passing probe's powers per link - 76 or 84 bytes per link and 4 per RB - which must fit
 * D2D_BALANCE_MAX_LDS_BYTES.  1 <= n_links <= D2D_BALANCE_MAX_LINKS, 1 <= n_rbs <= D2D_BALANCE_MAX_RBS, 1 <= pow_k <= 8 with
 * D2D_BALANCE_LAW_POW_K, n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_balance_last_error().      */
#ifndef D2D_BALANCE_H
#define D2D_BALANCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_powerctl.h */
#define D2D_BALANCE_LAW_INV_SQUARE 0
#define D2D_BALANCE_LAW_POWER 1
#define D2D_BALANCE_LAW_POW_K 2

#define D2D_BALANCE_MAX_LINKS 2048
#define D2D_BALANCE_MAX_RBS 8192
#define D2D_BALANCE_MAX_MARGINS 4096
#define D2D_BALANCE_MAX_LDS_BYTES 163840

int d2d_balance_sinr(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                     const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                     int32_t n_links, int32_t n_rbs, const float* base_db, const float* floor_db, const float* margins_db,
                     int32_t n_margins, const int32_t* p_min, const int32_t* p_max, const uint8_t* adjustable, int32_t max_iters,
                     const uint8_t* env_mask, int32_t* power_dbm, float* sinr_db, float* margin_db, int32_t* level, int32_t* probes,
                     void* hip_stream);
const char* d2d_balance_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_BALANCE_H */
