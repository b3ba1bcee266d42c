/* libd2d_episode.so - device-side episode bookkeeping for per-env autoreset (gym_d2d_amd.envs.VecD2DEnv(autoreset=True)).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).  Nothing here
 * synchronises, so the host never learns which envs are done; the decision lives in the [B] arrays below.  One step of a
 * client that autoresets, all on the handle's stream (DESIGN.md / INTEGRATION.md, "Autoreset"):
 *
 *   d2d_reset_positions(h, seed, D2D_EPISODE_PER_ENV, NULL, NULL)      the pending envs get new positions
 *   d2d_episode_merge_actions(actions, D2D_BUF_ACTIONS, ...)            ... and their reset's random actions
 *   d2d_step(h, NULL)
 *   d2d_episode_advance(...)                                            counters, done, the next step's pending set
 *
 * d2d_episode_merge_actions: actions_out[b][c] = pending[b] ? draw(seed, episode[b], first_env + b, c) % high[c]
 *                                                           : actions_in[b][c]
 *   draw is the splitmix64 stream of gym_d2d_amd/envs/_rng.py (uniform_ints_numpy): x = key + (env * n_cols + c + 1) * golden,
 *   key = mix(mix(seed) ^ (episode + 1) * golden), value (mix(x) >> 11) % high[c] - bit-identical to the random actions a full
 *   reset at that episode draws.  actions_in / actions_out int32 [n_envs][n_cols] (distinct), high int32 [n_cols] (> 0),
 *   pending int32 [n_envs], episode uint32 [n_envs].
 *
 * d2d_episode_advance, per env b:
 *   pending[b] != 0:  elapsed = 0, episode += 1, pending = 0, reset_out = 1, done = 0, and its reward is zeroed:
 *                     reward[b][0 .. reward_cols) (reward may be NULL: nothing to zero)
 *   else:             elapsed += 1, done = elapsed >= episode_length, pending = done, reset_out = 0
 *   done and reset_out are uint8 [n_envs] (0 / 1: a bool tensor aliases them).
 *
 * Returns 0, or non-zero with a message in d2d_episode_last_error().                                                           */
#ifndef D2D_EPISODE_H
#define D2D_EPISODE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int d2d_episode_merge_actions(const int32_t* actions_in, int32_t* actions_out, const int32_t* pending, const uint32_t* episode,
                              const int32_t* high, int64_t n_envs, int32_t n_cols, uint64_t first_env, uint64_t seed,
                              void* hip_stream);
int d2d_episode_advance(int32_t* pending, uint32_t* episode, int32_t* elapsed, uint8_t* done, uint8_t* reset_out, float* reward,
                        int32_t reward_cols, int64_t n_envs, int32_t episode_length, void* hip_stream);
const char* d2d_episode_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_EPISODE_H */
