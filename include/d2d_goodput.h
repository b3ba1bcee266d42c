/* libd2d_goodput.so - queue-aware goodput ascent over RBs and powers (gym_d2d_amd.envs.VecD2DEnv.goodput_ascent,
 * goodput_ascent_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_goodput_ascent raises, per env b, the weighted number of bits the links can deliver out of their backlogs in one step, by
 * local search that moves one coordinate per turn: a link's RB or its power.  Positions are as the last step left them.  Every
 * decision compares integers, so the solver is exact: no float ordering enters any choice.
 *
 * A link is ON AN RB iff 0 <= rb < n_rbs.  The GROUP of RB r is the set of links on r, in ascending link index.  For a state
 * s = (rb, pwr):
 *
 *   cap_m(s)     d2d_evaluate's float32 capacity_mbps of link m for s (include/d2d_evaluate.h), bit for bit: float products into
 *                one double accumulator over the group in ascending link index, the receiver's own slot adding 0.0, then
 *                d2d_evaluate's closing operations.  sinr_m(s) is its sinr_db.
 *   budget(c)    rule 5 of include/d2d_queue.h, word for word: floor((double)c * bits_per_mbps) clipped to [0, 2^31 - 1]; a NaN,
 *                negative or zero capacity gives 0, +inf gives 2^31 - 1.
 *   served_m(s)  min(budget(cap_m(s)), demand_m), demand_m = max(demand_bits[b][m], 0) (NULL: 2^31 - 1, uncapped).
 *   term_m(s)    (int64)weight_m * served_m(s), weight_m = min(weight[b][m], 2^20) (NULL: 1).
 *   V(s)         the sum of term_m(s) over ALL links, those that never move and those on no RB included.  V < 2^62 for at most
 *                2048 links, so int64 sums are exact and order-free.
 *
 * A link TAKES TURNS iff it is on an RB, movable[i] != 0 (NULL: every link) and, when move_mask is 1 (RBs only), it has at least
 * one allowed RB (allowed NULL: every RB).  A TURN of link i, on RB c at power p, works on the candidate states s' that differ
 * from s in link i alone:
 *
 *   1. RB candidates, if bit 0 of move_mask is set: (r, p) for every r != c with allowed[i][r].
 *   2. Power candidates, if bit 1 is set: (c, q) for every q in [p_min[i], p_max[i]] with q != p.  A link whose class is no
 *      alphabet of 1 .. D2D_GOODPUT_MAX_LEVELS levels inside (-4096, 4096), or whose held power lies outside it, has none.
 *   3. A turn changes the RB or the power, never both.
 *   4. Delta(s') = V(s') - V(s).  Only the members of group(c), of group(r) and link i contribute.
 *   5. s' is ADMISSIBLE iff every such member m with floor_db[m] > -inf passes one of these float32 comparisons (NaN compares
 *      false): sinr_m(s') >= floor_db[m], or sinr_m(s) < floor_db[m].  A link already under its floor constrains nothing; a link
 *      that meets its floor is never pushed under it (the rule of d2d_power_ascent and d2d_rb_ascent, for both kinds of candidate).
 *   6. best is the admissible candidate of maximal Delta; ties go to the lowest power, then to the lowest RB.
 *   7. Link i moves to best, at once, iff Delta(best) > min_gain.
 *
 * ROUNDS.  The links that take turns do so in ascending link index, each seeing the moves made before its turn.  A round that
 * moves nobody ends the ascent: converged = 1, rounds = the rounds that moved a link.  max_rounds rounds that each moved a link end
 * it too: converged = 0, rounds = max_rounds.
 *
 * TERMINATION.  Every move raises the integer V by at least 1 (min_gain >= 0) and V is bounded, so no state repeats.  max_rounds
 * only bounds the launch.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, cap_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_evaluate takes them, with rb and pwr_dbm i32 [n_envs][n_links]: the held state
 *   p_min, p_max       i32 [n_links]: the power alphabet of every link, as d2d_power_ascent takes them
 *   weight             u32 [n_envs][n_links] or NULL (1): values in [0, 2^20]; a larger word counts as 2^20
 *   demand_bits        i32 [n_envs][n_links] or NULL (2^31 - 1): a negative value counts as 0
 *   bits_per_mbps      double, finite, > 0: what 1 Mbps carries in one step (d2d_queue_step's bits_per_mbps_step)
 *   allowed            u32 [n_links][ceil(n_rbs / 32)] or NULL: bit r & 31 of word r / 32 of row i - link i may move to RB r
 *   movable            u8 [n_links] or NULL (every link)
 *   floor_db           f32 [n_links] or NULL (no floors): the SINR a link that meets it keeps, dB; -inf: none for that link
 *   move_mask          bit 0: RBs may move, bit 1: powers may move; 1, 2 or 3
 *   min_gain           i64 in [0, 2^62), weighted bits
 *   max_rounds         1 .. D2D_GOODPUT_MAX_ROUNDS
 *   env_mask           u8 [n_envs] or NULL: the workgroup of an env whose byte is 0 returns at once and that env's rows of the nine
 *                      outputs stay as they were
 *   rb_out, power_dbm  i32 [n_envs][n_links]: the state the ascent ended at (a link that never moves keeps what it held)
 *   sinr_db            f32 [n_envs][n_links]: d2d_evaluate's plane for (rb_out, power_dbm), every link, bit for bit
 *   capacity_mbps      f32 [n_envs][n_links]: likewise
 *   served_bits        i32 [n_envs][n_links]: served_m of the final state
 *   value              i64 [n_envs]: V of the final state
 *   rounds, moves      i32 [n_envs]
 *   converged          u8 [n_envs]
 *
 * One workgroup of at most 256 threads per env runs every turn of every round in ONE launch out of LDS.  The candidates of a
 * turn are dealt over the threads as one flat list, RB candidates first and then power candidates.  A candidate's walk takes the
 * members of the affected group as receivers in ascending index and, per receiver, the same set as transmitters into one double
 * accumulator per state; what link i's leaving does to group(c) is computed once per turn, not per candidate.  The choice is a
 * reduction of two 64-bit keys: Delta with its sign bit flipped (0: no admissible candidate), then the complement of
 * (q - p_min) << 16 | r.  Inside the turn loop there is no global access; there are no atomics on global memory, no scratch, and
 * nothing that depends on scheduling: two calls give the same words.  Every loop is bounded.  A thread with a long group does G^2
 * pair evaluations while the others wait: that is the known limit.  LDS bytes, with round16(x) = x rounded up to 16:
 *
 *   96 n_links + has_allowed round16(4 n_links ceil(n_rbs / 32)) + round16(4 ceil(n_links / 32) n_rbs) + 208
 *
 * (has_allowed = allowed != NULL), which must fit D2D_GOODPUT_MAX_LDS_BYTES: 1600 links on up to 50 RBs, 512 links
 * on up to 1788; no shape of more than 1702 links fits.
 * 1 <= n_links <= D2D_GOODPUT_MAX_LINKS, 1 <= n_rbs <= D2D_GOODPUT_MAX_RBS, 1 <= pow_k <= 8 with D2D_GOODPUT_LAW_POW_K,
 * n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_goodput_last_error().                            */
#ifndef D2D_GOODPUT_H
#define D2D_GOODPUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_evaluate.h */
#define D2D_GOODPUT_LAW_INV_SQUARE 0
#define D2D_GOODPUT_LAW_POWER 1
#define D2D_GOODPUT_LAW_POW_K 2

#define D2D_GOODPUT_MOVE_RB 1
#define D2D_GOODPUT_MOVE_POWER 2

#define D2D_GOODPUT_MAX_LINKS 2048
#define D2D_GOODPUT_MAX_RBS 8192
#define D2D_GOODPUT_MAX_LEVELS 64
#define D2D_GOODPUT_MAX_ROUNDS 4096
#define D2D_GOODPUT_MAX_WEIGHT 1048576
/* the LDS one workgroup can get on gfx950 (160 KiB) */
#define D2D_GOODPUT_MAX_LDS_BYTES 163840

int d2d_goodput_ascent(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                       const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k, int64_t n_envs,
                       int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max,
                       const uint32_t* weight, const int32_t* demand_bits, double bits_per_mbps, const uint32_t* allowed,
                       const uint8_t* movable, const float* floor_db, int32_t move_mask, int64_t min_gain, int32_t max_rounds,
                       const uint8_t* env_mask, int32_t* rb_out, int32_t* power_dbm, float* sinr_db, float* capacity_mbps,
                       int32_t* served_bits, int64_t* value, int32_t* rounds, int32_t* moves, uint8_t* converged, void* hip_stream);
const char* d2d_goodput_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_GOODPUT_H */
