/* libd2d_bestrb.so - best-response RB selection (gym_d2d_amd.envs.VecD2DEnv.best_rb, best_response_actions, BestRbObsFunction).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_best_rb, per env b and link i, with the state as the last step left it and sinr[b][i][r] exactly the value
 * include/d2d_sense.h defines (the SINR link i would get if it alone moved to RB r at its current power; d2d_sense_rb with
 * D2D_SENSE_SINR_DB writes the same bits):
 *
 *   best_rb[b][i]      = argmax over the allowed r of sinr[b][i][r]; equal values go to the lowest r, so among RBs nobody else
 *                        uses (sinr == snr on each of them) the lowest one wins.  -1 for a link with no allowed RB.  A NaN value
 *                        (coinciding devices) is never preferred to a number
 *   best_sinr_db[b][i] = that maximum; NaN where best_rb == -1
 *   gain_db[b][i]      = best_sinr_db[b][i] - sinr[b][i][rb[b][i]], one float subtraction: what the move would gain.  0.0 exactly
 *                        when the link already sits on its best RB, >= 0 whenever its own RB is allowed (an own RB that is not
 *                        allowed still counts as where the link stands: the gain is finite and may be negative).  NaN when
 *                        rb[b][i] is outside [0, n_rbs) or best_rb == -1
 *
 * No [n_envs][n_links][n_rbs] block is written or read.  Sums are taken in ascending j in the step's precision without atomics:
 * two calls on the same state give the same bits.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_sense_rb takes them (include/d2d_sense.h; dev_cols f32 [6][n_dev] as gym_d2d_amd.sensing.fold_columns
 *                      folds them; an rb outside [0, n_rbs) puts the link on no RB: it interferes with nobody)
 *   allowed            u32 [n_links][ceil(n_rbs / 32)] or NULL: bit (r & 31) of word r / 32 of row i says that link i may choose
 *                      RB r (bits past n_rbs are ignored).  NULL: every link may choose every RB
 *   env_mask           u8 [n_envs] or NULL: the workgroups of an env whose byte is 0 return at once and that env's rows of the
 *                      three outputs stay as they were.  NULL: every env
 *   best_rb            i32 [n_envs][n_links]
 *   best_sinr_db       f32 [n_envs][n_links]
 *   gain_db            f32 [n_envs][n_links]
 *
 * 1 <= n_links <= 2048 (D2D_MAX_LINKS of d2d_hip.h), 1 <= n_rbs <= D2D_BESTRB_MAX_RBS, 1 <= pow_k <= 8 with D2D_BESTRB_LAW_POW_K,
 * n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_bestrb_last_error().                          */
#ifndef D2D_BESTRB_H
#define D2D_BESTRB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_sense.h */
#define D2D_BESTRB_LAW_INV_SQUARE 0
#define D2D_BESTRB_LAW_POWER 1
#define D2D_BESTRB_LAW_POW_K 2

#define D2D_BESTRB_MAX_LINKS 2048
#define D2D_BESTRB_MAX_RBS 8192

int d2d_best_rb(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                int32_t n_links, int32_t n_rbs, const uint32_t* allowed, const uint8_t* env_mask, int32_t* best_rb,
                float* best_sinr_db, float* gain_db, void* hip_stream);
const char* d2d_bestrb_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_BESTRB_H */
