/* libd2d_ascent.so - sum-capacity power ascent with SINR floors (gym_d2d_amd.envs.VecD2DEnv.power_ascent, power_ascent_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_power_ascent raises, per env b, the total capacity of every RB group by coordinate ascent on the integer dBm alphabet, with
 * positions and RBs as they are.  A link is ON AN RB iff 0 <= rb < n_rbs; the GROUP of RB r is the set of links on r in ascending
 * link index; groups do not interact.  A link is ADJUSTABLE iff it is on an RB, adjustable[i] != 0 (NULL: every link), p_min[i] <=
 * p_max[i] with at most D2D_ASCENT_MAX_LEVELS levels between them, and (start = HELD) p_min[i] <= pwr_dbm[b][i] <= p_max[i]; every
 * other link keeps pwr_dbm[b][i] throughout and takes no turn.  An adjustable link begins at pwr_dbm[b][i] (D2D_ASCENT_START_HELD),
 * p_min[i] (_MIN) or p_max[i] (_MAX).
 *
 * A TURN of the adjustable link i on RB r, at the current power vector p.  For every level q in p_min[i] .. p_max[i] let p^q be p
 * with p[i] = q, and sinr_m(q), cap_m(q) the float32 sinr_db and capacity_mbps d2d_evaluate (include/d2d_evaluate.h) gives the
 * member m of r's group for (rb, p^q), bit for bit: the same operands in the same order, float products into a double accumulator
 * over the group in ascending link index, the receiver's own slot adding 0.0.
 *
 *   T(q)         the sum, in double, in ascending link index, of (double)cap_m(q) over the group
 *   admissible   q == p[i], or every member m (i included) with floor_db[m] > -inf has sinr_m(q) >= floor_db[m] or
 *                sinr_m(p[i]) < floor_db[m]: float32 comparisons, NaN compares false.  A member already under its floor constrains
 *                nothing; a member that meets its floor is never pushed under it
 *   best         the lowest admissible level whose T is maximal among the admissible levels; a NaN T is never chosen
 *   the move     p[i] = best, at once, iff T(best) - T(p[i]) > min_gain_mbps (a double subtraction and comparison)
 *
 * ROUNDS.  The adjustable links of a group take turns in ascending link index, each seeing the moves made before its turn.  A round
 * that moves nobody ends the group's ascent (it has converged; its rounds = the rounds that moved a link); max_rounds rounds that
 * each moved a link end it too (not converged, rounds = max_rounds).  Per env: rounds = the largest per-group count, moves = the
 * sum of the groups' moves, converged = 1 iff every group saw a quiet round - what ONE sequential pass over all adjustable links
 * of the env in ascending link index gives, since a group that has converged repeats its quiet round.  Every move strictly raises
 * its group's T, a function of the group's power vector alone, so no state repeats; max_rounds bounds the launch all the same.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, cap_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_evaluate takes them, with rb and pwr_dbm i32 [n_envs][n_links]
 *   p_min, p_max       i32 [n_links]: the power alphabet of every link, dBm; |p| < 4096 is the caller's promise
 *   adjustable         u8 [n_links] or NULL (every link)
 *   floor_db           f32 [n_links] or NULL (no floors): the SINR a member that meets it keeps, dB; -inf: none for that link
 *   start              D2D_ASCENT_START_HELD, _MIN or _MAX
 *   min_gain_mbps      finite, >= 0
 *   max_rounds         1 .. D2D_ASCENT_MAX_ROUNDS
 *   env_mask           u8 [n_envs] or NULL: the workgroup of an env whose byte is 0 returns at once and that env's rows of the six
 *                      outputs stay as they were
 *   power_dbm          i32 [n_envs][n_links]: the powers the ascent ended at
 *   sinr_db            f32 [n_envs][n_links]: d2d_evaluate's plane for (rb, power_dbm), every link, bit for bit
 *   capacity_mbps      f32 [n_envs][n_links]: likewise
 *   rounds, moves      i32 [n_envs]
 *   converged          u8 [n_envs]
 *
 * One workgroup of 256 threads per env runs the whole ascent out of LDS: a wave owns an RB group (wave w takes the RBs w, w + 4,
 * ... in that order), its 64 lanes own the levels of the link whose turn it is.  No global access, no workgroup barrier and no
 * atomics inside the ascent; no scratch memory.  A group of G links costs G^2 pair evaluations per turn on one wave: one long group
 * is not balanced across the waves.  LDS bytes, with round16(x) = x rounded up to 16 and n4 = n_links rounded up to 4:
 *
 *   48 n_links + has_power_law round16(8 n_links) + 20 n4 + round16(4 (n_rbs + 1)) + 64
 *
 * (has_power_law = law != D2D_ASCENT_LAW_INV_SQUARE) - 68 or 76 bytes per link and 4 per RB - which must fit
 * D2D_ASCENT_MAX_LDS_BYTES.  1 <= n_links <= D2D_ASCENT_MAX_LINKS, 1 <= n_rbs <= D2D_ASCENT_MAX_RBS, 1 <= pow_k <= 8 with
 * D2D_ASCENT_LAW_POW_K, n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_ascent_last_error().       */
#ifndef D2D_ASCENT_H
#define D2D_ASCENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_evaluate.h */
#define D2D_ASCENT_LAW_INV_SQUARE 0
#define D2D_ASCENT_LAW_POWER 1
#define D2D_ASCENT_LAW_POW_K 2

#define D2D_ASCENT_START_HELD 0
#define D2D_ASCENT_START_MIN 1
#define D2D_ASCENT_START_MAX 2

#define D2D_ASCENT_MAX_LINKS 2048
#define D2D_ASCENT_MAX_RBS 8192
#define D2D_ASCENT_MAX_LEVELS 64
#define D2D_ASCENT_MAX_ROUNDS 4096
#define D2D_ASCENT_MAX_LDS_BYTES 163840

int d2d_power_ascent(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                     const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k, int64_t n_envs,
                     int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max,
                     const uint8_t* adjustable, const float* floor_db, int32_t start, double min_gain_mbps, int32_t max_rounds,
                     const uint8_t* env_mask, int32_t* power_dbm, float* sinr_db, float* capacity_mbps, int32_t* rounds,
                     int32_t* moves, uint8_t* converged, void* hip_stream);
const char* d2d_ascent_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_ASCENT_H */
