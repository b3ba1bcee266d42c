/* libd2d_tabascent.so - sum-capacity RB ascent with SINR floors on a path-loss TABLE
 * (gym_d2d_amd.envs.VecD2DEnv.rb_ascent_table, rb_ascent_table_actions).  d2d_rb_ascent (include/d2d_rbascent.h) with the pair path
 * loss read from a dB table by (tx link, rx link) instead of evaluated from positions and a law.
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation - the
 * work space is the caller's.
 *
 * d2d_table_rb_ascent raises, per env b, the total capacity by cooperative local search on the RB half of the action: a link moves
 * to the RB where the TOTAL capacity gains most.  The table and the powers are as given; only rb changes.
 *
 * A link is ON AN RB iff 0 <= rb < n_rbs.  The GROUP of RB r is the set of links on r, in ascending link index.  A link is MOVABLE
 * iff it is on an RB, movable[i] != 0 (NULL: every link) and it has at least one allowed RB (allowed NULL: every RB).
 *
 * A TURN of the movable link i, currently on RB c, at the current assignment rb:
 *
 *   1. For an RB r, rb^r is rb with rb[i] = r.
 *   2. sinr^r_m and cap^r_m are the float32 sinr_db and capacity_mbps d2d_evaluate_table (include/d2d_evaltab.h) gives link m for
 *      (rb^r, pwr_dbm) on table[b], bit for bit: every entry converted as (float)exp2(-log2(10)/10 * (double)x), float products
 *      into one double accumulator over the group in ascending link index, the receiver's own slot adding 0.0, then
 *      d2d_evaluate_table's closing operations.
 *   3. Groups do not interact.  For r != c, cap^c_m of a member of r is its value "without i", and cap^r_m of a member of c is its
 *      value "with i gone".
 *   4. With(r) is the sum, in double, in ascending link index, of (double)cap^r_m over group(r) u {i}.
 *   5. Without(r) is the same sum over group(r) \ {i} with i not on r: for r != c of cap^c_m, for r == c of cap^r'_m for any
 *      r' != c; an empty sum is 0.0.
 *   6. D(r) = With(r) - Without(r), one double subtraction: what link i's presence on r is worth to the total.
 *   7. r is a CANDIDATE iff r != c, allowed[i][r] and r is admissible.  r is ADMISSIBLE iff every m in group(r) u {i} with
 *      floor_db[m] > -inf passes one of these float32 comparisons (NaN compares false): sinr^r_m >= floor_db[m], or
 *      sinr^c_m < floor_db[m].  A link already under its floor constrains nothing; a link that meets its floor is never pushed
 *      under it.  Leaving c constrains nothing.
 *   8. best is the lowest candidate r whose D(r) is maximal among the candidates.  A NaN D is never chosen.
 *   9. Link i moves to best, at once, iff D(best) - D(c) > min_gain_mbps (a double subtraction and comparison; a NaN does not
 *      move).
 *
 * ROUNDS.  The movable links take turns in ascending link index, each seeing the moves made before its turn.  A round that moves
 * nobody ends the ascent: converged = 1, rounds = the rounds that moved a link.  max_rounds rounds that each moved a link end it
 * too: converged = 0, rounds = max_rounds.  TERMINATION is the property include/d2d_rbascent.h states: each group sum is a pure
 * function of the group's membership, so the exact sum of the group totals strictly rises on every move.
 *
 *   table              f32 or f64 [n_envs][table_rows][n_links], dB by (tx link, rx link); table_dtype D2D_TABASCENT_F32 / _F64;
 *                      table_rows n_links or n_links + 1 (the live table's layout: row n_links, the SNR's row, is never read)
 *   rb, pwr_dbm        i32 [n_envs][n_links]: the start state, in the units of D2D_BUF_RB / D2D_BUF_PWR
 *   link_tx, link_rx   i32 [n_links]: device index of every link's transmitter and receiver, in [0, n_dev) (not checked on the
 *                      device: the caller's link list)
 *   dev_cols           f32 [3][n_dev]: tx_lin, rx_lin, noise_mw - d2d_evaluate_table's
 *   cap_cols           f32 [2][n_dev]: bw_mhz at a link's TRANSMITTER, sens_db at its RECEIVER - d2d_evaluate_table's
 *   allowed            u32 [n_links][ceil(n_rbs / 32)] or NULL: bit r & 31 of word r / 32 of row i - link i may move to RB r
 *   movable            u8 [n_links] or NULL (every link)
 *   floor_db           f32 [n_links] or NULL (no floors): the SINR a link that meets it keeps, dB; -inf: none for that link
 *   min_gain_mbps      finite, >= 0
 *   max_rounds         1 .. D2D_TABASCENT_MAX_ROUNDS
 *   env_mask           u8 [n_envs] or NULL: an env whose byte is 0 is skipped by both launches: its rows of the seven outputs
 *                      stay as they were (and its block of the work space is not written)
 *   gains              f32 [n_envs][n_links][n_links]: the WORK SPACE, 4 n_envs n_links^2 bytes, overwritten by every call.  Its
 *                      layout is private to this library
 *   rb_out             i32 [n_envs][n_links]: the RBs the ascent ended at (a link on no RB keeps the value it had)
 *   sinr_db            f32 [n_envs][n_links]: d2d_evaluate_table's plane for (rb_out, pwr_dbm), every link, bit for bit
 *   capacity_mbps      f32 [n_envs][n_links]: likewise
 *   rounds, moves      i32 [n_envs]
 *   converged          u8 [n_envs]
 *   domain             i32 [n_envs]: 1 iff any entry [j][i] with j, i < n_links of the env's block fails x > -inf (a NaN or -inf),
 *                      else 0.  The whole block, not "where read": which pairs a trajectory reads is no part of the contract.
 *                      +inf is a legal entry: gain 0.  The other outputs of a flagged env are whatever the arithmetic gives (a NaN
 *                      D is never chosen, a NaN gain does not move)
 *
 * TWO launches on hip_stream.  (1) The conversion: one workgroup of 256 threads per env turns the env's n_links x n_links dB block,
 * tile by tile through LDS, into float32 linear gains in the work space, RECEIVER-major - G[b][rx i][tx j] - so that the ascent's
 * walk over the transmitters of one receiver runs along one row; it raises the env's domain word, written once by one thread, no
 * atomics.  (2) The ascent: one workgroup of at most 256 threads per env runs every turn of every round out of LDS as
 * d2d_rb_ascent does - lanes own RBs (a lane with several loops), membership is a bitset in LDS, one walk over group(r) u {i}
 * gives With, Without, both SINRs of the floor test and D(r) - with the pair term tz[o] * G[m][o], one float load from the work
 * space (L2) where d2d_rb_ascent evaluates a law.  No global writes and no atomics inside the turn loop, no scratch, nothing that
 * depends on scheduling: two calls give the same words.  A lane with a long group does G^2 pair loads while the others wait: that
 * is the known limit.  With one RB nobody has a candidate: moves = 0, converged = 1.  LDS bytes of the ascent, with round16(x) = x
 * rounded up to 16 and n4 = n_links rounded up to 4:
 *
 *   16 n_links + 2 round16(4 n_links) + 8 n4 + has_allowed round16(4 n_links ceil(n_rbs / 32))
 *     + round16(4 ceil(n_links / 32) n_rbs) + 112
 *
 * (has_allowed = allowed != NULL), which must fit D2D_TABASCENT_MAX_LDS_BYTES.  1 <= n_links <= D2D_TABASCENT_MAX_LINKS,
 * 1 <= n_rbs <= D2D_TABASCENT_MAX_RBS, n_dev >= 1, n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in
 * d2d_tabascent_last_error().                                                                                                   */
#ifndef D2D_TABASCENT_H
#define D2D_TABASCENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the entry types of include/d2d_evaltab.h */
#define D2D_TABASCENT_F32 0
#define D2D_TABASCENT_F64 1

#define D2D_TABASCENT_MAX_LINKS 2048
#define D2D_TABASCENT_MAX_RBS 8192
#define D2D_TABASCENT_MAX_ROUNDS 4096
/* the LDS one workgroup can get on gfx950 (160 KiB) */
#define D2D_TABASCENT_MAX_LDS_BYTES 163840

int d2d_table_rb_ascent(const void* table, int32_t table_dtype, int32_t table_rows, const int32_t* rb, const int32_t* pwr_dbm,
                        const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int64_t n_envs,
                        int32_t n_dev, int32_t n_links, int32_t n_rbs, const uint32_t* allowed, const uint8_t* movable,
                        const float* floor_db, double min_gain_mbps, int32_t max_rounds, const uint8_t* env_mask, float* gains,
                        int32_t* rb_out, float* sinr_db, float* capacity_mbps, int32_t* rounds, int32_t* moves, uint8_t* converged,
                        int32_t* domain, void* hip_stream);
const char* d2d_tabascent_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_TABASCENT_H */
