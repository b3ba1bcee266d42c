/* libd2d_mobility.so - device mobility: Gauss-Markov velocities, a hard cell wall and a tethered D2D receiver, one launch per step
 * (gym_d2d_amd.envs.VecD2DEnv(mobility=GaussMarkovMobility(...))).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.  It
 * writes the planes a handle has bound as D2D_BUF_POS_X / D2D_BUF_POS_Y: call d2d_positions_changed on that handle after it.
 *
 * Devices of one env, as d2d_reset_positions places them: 0 the base station, 1 .. n_cues the CUEs, then n_due_pairs pairs
 * (transmitter n_cues + 1 + 2k, its receiver right behind it); n_dev = 1 + n_cues + 2 n_due_pairs.
 *
 * d2d_mobility_move, per env b, with the env's clock (episode e, step t, see below):
 *
 *   t == 0, the start of episode e:   v_d = speed_std * n(e, 0, d); positions are not touched (they are the reset sampler's)
 *   t >= 1, step t of episode e:      v_d <- memory * v_d + noise_scale * n(e, t, d)       one fma per axis
 *                                     p_d <- p_d + v_d * dt_s                              one fma per axis
 *                                     then, in this order:
 *     1  the base station and every device with fixed_mask[d] != 0 are not moved at all; their velocity is 0 (written at t == 0)
 *     2  a DUE receiver, AFTER its transmitter's move, against the transmitter's new position: if |rx - tx| > d2d_radius_m it is
 *        pulled onto the circle around tx, rx = tx + (rx - tx) * r / |rx - tx|, and its velocity is negated.  (A pair whose receiver
 *        is fixed and whose transmitter is not: the transmitter is tethered to the receiver in the same way.)
 *     3  a moved device with |p| > cell_radius_m is pulled onto the cell circle, p *= cell_radius_m / |p|, and its velocity is negated
 *        (twice negated: as it was)
 *     The circle of step 2 has the radius r = d2d_radius_m - ulp(cell_radius_m), one float32 grid step at the cell's edge inside
 *     d2d_radius_m, so that the ROUNDED coordinates, whose grid is up to ulp(cell_radius_m) wide, stand within d2d_radius_m; and a
 *     tethered device that step 3 moved is tested and pulled once more as in step 2 (velocity untouched), because step 3's own
 *     rounding - up to 2.5 ulp(cell_radius_m) - can push the pair apart again.  Afterwards |p| <= cell_radius_m (1 + 2^-22) and
 *     |rx - tx| <= d2d_radius_m (1 + 2^-22) for the float32 values as they stand in memory.
 *
 *   n(e, t, d) = (n_x, n_y), two independent standard normals: the Box-Muller Gaussian of libd2d_plugin.so and of the step's
 *   shadowing (philox_normal, csrc/d2d_step_device.h) at the Philox4x32-10 counter and key
 *
 *       counter word 0   the GLOBAL env index first_env + b (< 2^32)
 *       counter word 1   e, the episode index the env's current positions were drawn at (d2d_reset_positions' episode)
 *       counter word 2   t, the step in the episode; 0 is the start-of-episode draw
 *       counter word 3   2 d + axis, d the device index in the env, axis 0 for x and 1 for y
 *       key              seed, low word then high word
 *
 *   Nothing of launch geometry or of how a batch is sharded enters: shards given their first_env draw what the whole batch draws.
 *   `seed` is the MOBILITY seed - keep it apart from the shadowing seed, whose stream has the same generator and word layout.
 *
 * The clock.  In lockstep (reset_env == NULL) every env stands at the scalars `episode` and `step`.  With per-env episodes
 * (reset_env != NULL; the three arrays beside it then must not be NULL, `step` and `episode` are ignored):
 *
 *   reset_env[b] != 0   the env is being reset in this step (D2D_BUF_RESET_PENDING): start of episode e = episode_env[b], t = 0;
 *                       its positions are left to d2d_reset_positions; start_env[b] = 0 is written
 *   reset_env[b] == 0   the env moves: e = episode_env[b] - 1, t = elapsed_env[b] - start_env[b] + 1
 *
 *   episode_env  u32 [n_envs]  D2D_BUF_EPISODE: the index an env's NEXT reset draws at, hence one more than the episode it stands in
 *   elapsed_env  i32 [n_envs]  steps the env has taken in its episode (d2d_episode_advance's elapsed), read before that step's advance
 *   start_env    i32 [n_envs]  what elapsed_env[b] was when the env's velocities were drawn: the stagger of a first episode, 0 later
 *
 *   pos_x, pos_y, vel_x, vel_y   f32 [n_envs][n_dev], updated in place (t == 0 reads none of them and writes the velocities)
 *   fixed_mask                   u8 [n_dev] or NULL (no device is pinned): d2d_reset_positions' fixed_mask
 *   memory in [0, 1), noise_scale = speed_std * sqrt(1 - memory^2) and dt_s are the caller's float32 roundings of double values
 *
 * n_envs >= 0 (0: nothing to do), n_cues, n_due_pairs >= 0, first_env + n_envs <= 2^32, cell_radius_m > 0,
 * d2d_radius_m > ulp(cell_radius_m).  Returns 0, or non-zero with a message in d2d_mobility_last_error().                        */
#ifndef D2D_MOBILITY_H
#define D2D_MOBILITY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int d2d_mobility_move(float* pos_x, float* pos_y, float* vel_x, float* vel_y, const uint8_t* fixed_mask, int64_t n_envs,
                      int32_t n_cues, int32_t n_due_pairs, uint64_t first_env, uint64_t seed, float memory, float noise_scale,
                      float speed_std, float dt_s, float cell_radius_m, float d2d_radius_m, uint32_t step, uint32_t episode,
                      const int32_t* elapsed_env, int32_t* start_env, const uint32_t* episode_env, const int32_t* reset_env,
                      void* hip_stream);
const char* d2d_mobility_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_MOBILITY_H */
