/* libd2d_brdyn.so - sequential best-response RB dynamics (gym_d2d_amd.envs.VecD2DEnv.best_response_dynamics,
 * best_response_dynamics_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_best_response_dynamics runs, per env b, Gauss-Seidel best response on the RB half of the action, with positions and powers
 * as the last step left them.  One link moves, the next link sees the move:
 *
 *   rb^0 = rb[b]
 *   round t = 1, 2, ...:
 *     for i = 0 .. n_links - 1 in ascending link index, movable links only:
 *       s[r]  = the sinr_db the step kernel would write for link i on RB r with every OTHER link where it is NOW (the moves of
 *               this round included), for the allowed r and for the link's own RB: a value of d2d_sense_rb's block for that state
 *       best  = the allowed r of the highest s[r]; strictly greater in ascending r, so equal values keep the lowest r (d2d_best_rb)
 *       gain  = s[best] - s[rb_i]                                                float32, exactly this subtraction
 *       if gain > min_gain_db: rb_i = best, at once
 *     stop after a round that moved nobody: converged = 1, rounds = the rounds that moved a link
 *     stop after max_rounds rounds that each moved one: converged = 0, rounds = max_rounds
 *
 * Never moved: a link whose movable byte is 0, a link on no RB (rb outside [0, n_rbs)), a link with no allowed RB, a link whose
 * gain is NaN.  Links that do not move still interfere, unless they are on no RB.  Selfish SINR response is no potential game: at
 * min_gain_db 0 envs can cycle until the cap; converged is a result, not a promise.  Sums are taken in ascending j in the step's
 * precision without atomics: two calls on the same state give the same bits.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_sense_rb takes them (include/d2d_sense.h; dev_cols f32 [6][n_dev] as gym_d2d_amd.sensing.fold_columns
 *                      folds them)
 *   allowed            u32 [n_links][ceil(n_rbs / 32)] or NULL: bit r & 31 of word r / 32 of row i - link i may choose RB r
 *                      (gym_d2d_amd.best_response.pack_allowed).  NULL: every RB
 *   movable            u8 [n_links] or NULL: 0 - the link stays where it is and only interferes.  NULL: every link is movable
 *   min_gain_db        >= 0, not NaN: a link moves only for a gain above it
 *   max_rounds         in [0, D2D_BRDYN_MAX_ROUNDS]: the cap on the rounds; 0 returns rb with converged = 0
 *   env_mask           u8 [n_envs] or NULL: the workgroup of an env whose byte is 0 returns at once and that env's rows of the
 *                      five outputs stay as they were.  NULL: every env
 *   rb_out             i32 [n_envs][n_links]: the RBs when the dynamics stopped (a link on no RB keeps the value it had)
 *   sinr_db            f32 [n_envs][n_links]: the step's sinr_db for rb_out, bit for bit; NaN for a link on no RB
 *   rounds             i32 [n_envs]: the rounds that moved at least one link; max_rounds when the cap was hit
 *   moves              i32 [n_envs]: the moves made
 *   converged          u8 [n_envs]: 1 - a round moved nobody; 0 - the cap was hit
 *
 * One workgroup per env keeps the env's links, the allowed words and the RB membership bitset in LDS across all rounds:
 * 1 <= n_links <= 2048 (D2D_MAX_LINKS of d2d_hip.h), 1 <= n_rbs <= D2D_BRDYN_MAX_RBS, and 44 (inverse square) or 52 (power laws)
 * bytes per link, 4 * ceil(n_rbs / 32) more per link with an allowed mask, and 4 * ceil(n_links / 32) per RB must fit
 * D2D_BRDYN_MAX_LDS_BYTES; 1 <= pow_k <= 8 with D2D_BRDYN_LAW_POW_K, n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero
 * with a message in d2d_brdyn_last_error().                                                                                     */
#ifndef D2D_BRDYN_H
#define D2D_BRDYN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_sense.h */
#define D2D_BRDYN_LAW_INV_SQUARE 0
#define D2D_BRDYN_LAW_POWER 1
#define D2D_BRDYN_LAW_POW_K 2

#define D2D_BRDYN_MAX_LINKS 2048
#define D2D_BRDYN_MAX_RBS 8192
#define D2D_BRDYN_MAX_ROUNDS 1024
/* the LDS one workgroup can get on gfx950 (160 KiB): what the links, the allowed words and the membership bitset must fit */
#define D2D_BRDYN_MAX_LDS_BYTES 163840

int d2d_best_response_dynamics(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm,
                               const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k,
                               int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const uint32_t* allowed,
                               const uint8_t* movable, float min_gain_db, int32_t max_rounds, const uint8_t* env_mask,
                               int32_t* rb_out, float* sinr_db, int32_t* rounds, int32_t* moves, uint8_t* converged,
                               void* hip_stream);
const char* d2d_brdyn_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_BRDYN_H */
