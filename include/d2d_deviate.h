/* libd2d_deviate.so - unilateral-deviation gains over every (RB, power) action (gym_d2d_amd.envs.VecD2DEnv.deviation_gains,
 * best_deviation, best_deviation_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.
 *
 * The counterfactual row of every selected link: what the env's total capacity would gain if link i ALONE had taken the action
 * (RB r, power q), for every r and every q of its alphabet - the product neighbourhood, where an RB and a power change in one
 * move.  Nothing is solved and nothing is sequential: n_envs x n_sel x n_rbs x n_levels independent entries.
 *
 * The state s = (rb, pwr_dbm) is what the last step left.  A link is ON AN RB iff 0 <= rb < n_rbs.  The GROUP of RB r is the set of
 * links on r, in ascending link index.  links is an ascending list of n_sel distinct link indices.  L_i = p_max[i] - p_min[i] + 1
 * is the number of levels of link i, 1 <= L_i <= n_levels <= D2D_DEVIATE_MAX_LEVELS for every selected link (the caller's to
 * hold, with |p| < 4096: the kernel takes a link whose bounds break it as a link of min(max(L_i, 0), n_levels) levels).
 *
 * For a selected link i on RB c at power p, an RB r and a level q = p_min[i] + l:
 *
 *   1. s^(r,q) is s with rb[i] = r, pwr[i] = q.  cap_m(.) and sinr_m(.) are the float32 capacity_mbps and sinr_db d2d_evaluate
 *      (include/d2d_evaluate.h) gives link m for that state, bit for bit: float products into one double accumulator over the
 *      group in ascending link index, the receiver's own slot adding 0.0, then d2d_evaluate's closing operations.
 *   2. With(r,q) is the sum, in double, in ascending link index, of (double)cap_m(s^(r,q)) over group(r) u {i}.
 *   3. Without(r) is the same sum over group(r) \ {i} with i on no RB; an empty sum is 0.0.
 *   4. D(r,q) = With(r,q) - Without(r).  gain(r,q) = D(r,q) - D(c,p).  Each is one double subtraction; gain(c,p) is +0.0 exactly.
 *      Groups do not interact, so in exact arithmetic gain(r,q) is the change of the env's total capacity when link i alone plays
 *      (r,q).
 *   5. (r,q) is ADMISSIBLE iff (r,q) == (c,p), or every m in group(r) u {i} with floor_db[m] > -inf passes one of these float32
 *      comparisons (NaN compares false): sinr_m(s^(r,q)) >= floor_db[m], or sinr_m(s) < floor_db[m].  A link already under its
 *      floor constrains nothing; a link that meets its floor is never pushed under it (the rule of d2d_rb_ascent and
 *      d2d_goodput_ascent).  Leaving c constrains nothing.
 *   6. The entry (r,l) is OPEN iff l < L_i, allowed[i][r] (allowed NULL: every RB; the held RB c is open whatever allowed says),
 *      (r,q) is admissible and link i is on an RB.
 *
 *   pos_x, pos_y, rb, pwr_dbm, link_tx, link_rx, dev_cols, cap_cols, law, pow_k, n_envs, n_dev, n_links, n_rbs
 *                      as d2d_evaluate takes them, with rb and pwr_dbm i32 [n_envs][n_links]: the held state
 *   p_min, p_max       i32 [n_links]: the power alphabet of every link, as d2d_goodput_ascent takes them
 *   links              i32 [n_sel], device memory: the selected links, ascending and distinct, each in [0, n_links) (an index
 *                      outside that range is read as a link on no RB: its entries are closed, nothing of it is written elsewhere)
 *   n_sel              1 .. n_links
 *   n_levels           1 .. D2D_DEVIATE_MAX_LEVELS: the innermost extent of the table, the largest L_i of the selected links
 *   allowed            u32 [n_links][ceil(n_rbs / 32)] or NULL: bit r & 31 of word r / 32 of row i - link i may play RB r
 *   floor_db           f32 [n_links] or NULL (no floors): the SINR a link that meets it keeps, dB; -inf: none for that link
 *   env_mask           u8 [n_envs] or NULL: the workgroups of an env whose byte is 0 return at once and that env's rows of every
 *                      output stay as they were
 *
 * d2d_deviation_gains writes the table:
 *
 *   gain_out           f32 [n_envs][n_sel][n_rbs][n_levels]: -inf for a closed entry, else gain(r,q) rounded once to float32; a
 *                      NaN stays NaN.  The innermost two axes are the step's action order rb * levels + level.
 *
 * d2d_best_deviation writes no table.  Per selected link i, best is the open entry other than (c,p) of maximal double gain; ties go
 * to the lowest power, then to the lowest RB (d2d_goodput_ascent's rule); a NaN gain is never chosen.
 *
 *   min_gain_mbps      finite, >= 0
 *   rb_out, pwr_out    i32 [n_envs][n_links]: best, iff gain(best) > min_gain_mbps; else the held (c,p).  A link that is not
 *                      selected keeps (rb, pwr_dbm)
 *   gain_link          f64 [n_envs][n_links]: gain(best) where best was written, else 0.0
 *   regret             f64 [n_envs]: the largest gain_link of the env (0.0: nobody would move)
 *   leader             i32 [n_envs]: the lowest link that has it, -1 when nobody would move
 *
 * Grid: (env, chunk of selected links), 256 threads at most, so one env is served by several workgroups.  Each stages the env's
 * per-link constants (one 80-byte record per link) and the membership bitset bits[w][r] of d2d_rb_ascent into LDS once and
 * evaluates the held state s once: cap_m(s) of every link, and the floor of a link that is under it in s set aside.  What link i's
 * leaving does to group(c) - Without(c), D(c,p) - is walked once per link; then the workgroup deals its (link, r, l) entries flat
 * over its threads, consecutive lanes owning consecutive (r, l), so that the table leaves in full contiguous rows.  An entry walks
 * one state, s^(r,q); Without(r) is a sum of the stored cap_m(s).  The levels of one (r) sit in adjacent lanes and run one walk in
 * lockstep.  d2d_best_deviation keeps the running best as two 64-
 * bit keys per thread - the order-preserving image of the double gain, then the complement of l << 16 | r - combined across the
 * wave by data-parallel primitives and across the waves by one LDS pass; regret and leader come from a second, tiny kernel of one
 * workgroup per env that also writes the rows of the links that are not selected.  No atomics, no scratch, nothing that depends on
 * scheduling: two calls give the same words.  An entry with a long group costs G^2 pair evaluations: that is the known limit.
 * LDS bytes of one workgroup, with round16(x) = x rounded up to 16:
 *
 *   80 n_links + has_allowed round16(4 n_links ceil(n_rbs / 32)) + round16(4 ceil(n_links / 32) n_rbs) + 5216
 *
 * (has_allowed = allowed != NULL), which must fit D2D_DEVIATE_MAX_LDS_BYTES.  This bound binds before D2D_DEVIATE_MAX_LINKS does:
 * 80 x 2048 is the whole 163840 and the 5216 come on top, so 2048 links never fit - with n_rbs = 1 and no mask the largest shape
 * taken is 1979 links (163792 bytes; 1980 need 163872).
 * 1 <= n_links <= D2D_DEVIATE_MAX_LINKS, 1 <= n_rbs <= D2D_DEVIATE_MAX_RBS, 1 <= pow_k <= 8 with D2D_DEVIATE_LAW_POW_K,
 * n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_deviate_last_error().                            */
#ifndef D2D_DEVIATE_H
#define D2D_DEVIATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_evaluate.h */
#define D2D_DEVIATE_LAW_INV_SQUARE 0
#define D2D_DEVIATE_LAW_POWER 1
#define D2D_DEVIATE_LAW_POW_K 2

#define D2D_DEVIATE_MAX_LINKS 2048
#define D2D_DEVIATE_MAX_RBS 8192
#define D2D_DEVIATE_MAX_LEVELS 64
/* the LDS one workgroup can get on gfx950 (160 KiB) */
#define D2D_DEVIATE_MAX_LDS_BYTES 163840

int d2d_deviation_gains(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                        const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k, int64_t n_envs,
                        int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max, const int32_t* links,
                        int32_t n_sel, int32_t n_levels, const uint32_t* allowed, const float* floor_db, const uint8_t* env_mask,
                        float* gain_out, void* hip_stream);
int d2d_best_deviation(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                       const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k, int64_t n_envs,
                       int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* p_min, const int32_t* p_max, const int32_t* links,
                       int32_t n_sel, int32_t n_levels, const uint32_t* allowed, const float* floor_db, double min_gain_mbps,
                       const uint8_t* env_mask, int32_t* rb_out, int32_t* pwr_out, double* gain_link, double* regret, int32_t* leader,
                       void* hip_stream);
const char* d2d_deviate_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_DEVIATE_H */
