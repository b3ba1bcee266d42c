/* libd2d_powerctl.so - target-SINR power control (gym_d2d_amd.envs.VecD2DEnv.power_control, power_control_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_power_control runs, per env b, the constrained target-SINR iteration (Foschini-Miljanic / Yates) on the integer dBm
 * alphabet, with positions and RBs as the last step left them.  Jacobi: every link updates from the same old vector.
 *
 *   p0[i]   = p_min[i] (adjustable link on an RB)      p0[i] = pwr_dbm[b][i] (every other link)
 *   s[i]    = the sinr_db the step kernel writes for link i under the powers p^t, bit for bit
 *   need    = ceilf((float)p^t[i] + (target_db[i] - s[i]))                       float32, exactly this expression
 *   p^t+1[i] = max(p^t[i], min(p_max[i], max(p_min[i], (int)need)))              never lowered; NaN need: unchanged
 *   stop when a sweep changed no link (converged) or after max_iters sweeps that each changed one
 *
 * Powers only rise inside a finite alphabet, so the iteration ends; it reaches the least fixed point, which is the componentwise
 * power-minimal assignment that meets the targets when they are feasible.  A link whose rb is outside [0, n_rbs) is on no RB: it
 * keeps pwr_dbm[b][i], interferes with nobody and its sinr_db is NaN.  A link that is not adjustable keeps pwr_dbm[b][i] and
 * interferes.  Sums are taken in ascending j in the step's precision without atomics: two calls on the same state give the same bits.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_sense_rb takes them (include/d2d_sense.h; dev_cols f32 [6][n_dev] as gym_d2d_amd.sensing.fold_columns
 *                      folds them)
 *   target_db          f32 [n_links]: every link's target SINR in dB
 *   p_min, p_max       i32 [n_links]: the link's power bounds in dBm, |p| < 4096
 *   adjustable         u8 [n_links] or NULL: 0 - the link keeps pwr_dbm and only interferes.  NULL: every link is adjustable
 *   max_iters          >= 1: the cap on the sweeps
 *   env_mask           u8 [n_envs] or NULL: the workgroup of an env whose byte is 0 returns at once and that env's rows of the
 *                      four outputs stay as they were.  NULL: every env
 *   power_dbm          i32 [n_envs][n_links]: the powers when the iteration stopped
 *   sinr_db            f32 [n_envs][n_links]: every link's SINR at power_dbm, evaluated behind the last update (valid at the cap too)
 *   iters              i32 [n_envs]: the sweeps that changed at least one link; max_iters when the cap was hit
 *   converged          u8 [n_envs]: 1 - a sweep changed nothing (the fixed point); 0 - the cap was hit
 *
 * One workgroup per env keeps the env's links in LDS across all sweeps: 1 <= n_links <= 2048 (D2D_MAX_LINKS of d2d_hip.h),
 * 1 <= n_rbs <= D2D_POWERCTL_MAX_RBS, and 68 (inverse square) or 76 (power laws) bytes per link plus 4 per RB must fit 160 KiB;
 * 1 <= pow_k <= 8 with D2D_POWERCTL_LAW_POW_K, n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in
 * d2d_powerctl_last_error().                                                                                                    */
#ifndef D2D_POWERCTL_H
#define D2D_POWERCTL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_sense.h */
#define D2D_POWERCTL_LAW_INV_SQUARE 0
#define D2D_POWERCTL_LAW_POWER 1
#define D2D_POWERCTL_LAW_POW_K 2

#define D2D_POWERCTL_MAX_LINKS 2048
#define D2D_POWERCTL_MAX_RBS 8192

int d2d_power_control(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                      const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                      int32_t n_links, int32_t n_rbs, const float* target_db, const int32_t* p_min, const int32_t* p_max,
                      const uint8_t* adjustable, int32_t max_iters, const uint8_t* env_mask, int32_t* power_dbm, float* sinr_db,
                      int32_t* iters, uint8_t* converged, void* hip_stream);
const char* d2d_powerctl_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_POWERCTL_H */
