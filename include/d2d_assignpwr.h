/* libd2d_assignpwr.so - joint RB and power matching with SINR floors: the best admissible power of every movable link on every RB
 * and the weight it has there (gym_d2d_amd.envs.VecD2DEnv.joint_assignment_weights / assign_rbs_power).  The matching itself is
 * d2d_assign_solve of include/d2d_assign.h, which takes any weights.
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.
 *
 * Definitions, per env.  Movable and background links as in include/d2d_assign.h: row a is movable_links[a]; every other link is
 * BACKGROUND and stays on its current rb and pwr; the movable links are taken off the air, and neither their current RB nor their
 * current power plays a part.  For movable link a, RB r and power level p in [p_min[a], p_max[a]] (whole dBm, ascending):
 *
 *   own(a,r,p)   = link a's capacity (Mbps) at power p with the background members of r as its interferers, formed by the step's
 *                  operations in the step's order with the transmit term pow10_tenth(p) * dev_cols[0][tx]
 *   harm(a,r,p)  = the sum over the background members k of r, in ascending link index, of the float32 loss d2d_assign_weights
 *                  computes - bw log2(1 + S t rx_pl / (den (den' + S))), or k's whole capacity when a pushes it under its
 *                  sensitivity - accumulated in double
 *   w(a,r,p)     = (float)((double)own - harm), one rounding
 *
 * With floor_db NULL, w(a,r,p) is bit for bit the weight d2d_assign_weights (D2D_ASSIGN_OBJECTIVE_TOTAL) gives with pwr_dbm of link
 * a set to p.
 *
 * Floors.  floor_db[i] is link i's minimum SINR in dB; -inf (or NaN): no floor for that link.  (a,r,p) is ADMISSIBLE iff
 *   - link a's own test:   sinr_db(a,r,p) >= floor_db[a], where sinr_db = 3.01029995663981195f * log2f(sinr_lin) is the float32 value
 *                          own(a,r,p) is formed from (the value compared with the sensitivity), and
 *   - the victims' test:   for every background member k of r that is CONSTRAINED, (float)sinr_with >= floor_db[k], where
 *                          sinr_with = 3.01029995663981195f * log2f((float)(S_k / den')) and den' is the double denominator
 *                          fma(I_k + t, rx_pl, noise) with link a's term t added - d2d_assign_weights's `ok_with` expression with
 *                          the floor in place of the sensitivity and >= in place of >.
 *   Member k is constrained iff floor_db[k] > -inf and its background-only float32 sinr_db (the step's expression, formed with the
 *   background members of its RB alone) is >= floor_db[k].  A victim the background alone already holds under its floor constrains
 *   nothing: the movable link cannot repair it.  The victims' test reads every member, whether over its sensitivity or not.
 *
 * Outputs.  weights[b][a][r] = the maximum of w(a,r,p) over the admissible p, scanned in ascending p with a strict > from -inf, so
 * equal values go to the lowest power; power_dbm[b][a][r] is that p.  Where allowed forbids, or no p is admissible: -inf and
 * D2D_ASSIGNPWR_NO_POWER.  A movable entry outside [0, n_links) gives a row of -inf / D2D_ASSIGNPWR_NO_POWER and touches nothing
 * else.
 *
 * Under a one-to-one placement a background link sees at most one movable link, so both its loss and its floor depend on that one
 * link's (r, p) alone: for every injective a -> r_a and every choice of powers the total capacity is exactly G_background + the sum of
 * w(a, r_a, p_a), and the floors hold iff every (a, r_a, p_a) is admissible.  The maximum-weight matching of `weights` is therefore the
 * optimum over (one-to-one placement) x (one power per movable link) subject to the floors.
 *
 * d2d_assign_power_weights: one workgroup of 256 threads per env.  The background is sorted by (rb, link index) into LDS; phase 1
 * parks every slot's interference sum, capacity and effective floor; phase 2 takes one movable link per wave, lanes across r.  An
 * item walks the members of r once for link a's own interference, then once per chunk of D2D_ASSIGNPWR_CHUNK power levels held in
 * registers: the gain a -> victim is evaluated once per chunk, each level's harm is summed in ascending member order.  No atomics;
 * every output word is written once by its owner; two calls give the same bits.
 *
 *   pos_x .. cap_cols, law, pow_k, n_envs .. n_rbs, movable_links, n_movable, allowed    as d2d_assign_weights takes them
 *   p_min, p_max       i32 [n_links], DEVICE memory as d2d_power_control takes them: the alphabet of every link in the dBm the step
 *                      transmits, |p| < 4096, p_min <= p_max, at most D2D_ASSIGNPWR_MAX_LEVELS levels.  The entries of links that
 *                      are not movable are not read.  The arrays are device memory, which a host entry point cannot read without
 *                      synchronising: a movable link whose alphabet is outside this contract (p_min > p_max, more than
 *                      D2D_ASSIGNPWR_MAX_LEVELS levels, |p| >= 4096) gets a row of -inf / D2D_ASSIGNPWR_NO_POWER from the kernel,
 *                      and nothing else is touched.  A caller that holds the bounds on the host refuses them by name before the
 *                      upload, as gym_d2d_amd.joint_assignment.check_alphabet does.
 *   floor_db           f32 [n_links] or NULL (no floors)
 *   weights            f32 [n_envs][n_movable][n_rbs], required
 *   power_dbm          i32 [n_envs][n_movable][n_rbs], required, a plane of its own
 *
 * 1 <= n_links <= D2D_ASSIGNPWR_MAX_LINKS, 1 <= n_rbs <= D2D_ASSIGNPWR_MAX_RBS, 1 <= n_movable <= n_links, n_dev >= 1, n_envs >= 0
 * (0: accepted, nothing is launched).  LDS of one workgroup, d2d_assign_weights's:
 *   48 n_links + round16(8 n4) + 3 round16(4 n_links) + round16(4 (n_rbs + 1)), n4 = n_links rounded up to 4,
 *   + round16(8 n_links) with a power law;
 * more than D2D_ASSIGNPWR_MAX_LDS_BYTES is refused by name, in bytes.  No scratch memory; at most 128 VGPRs per kernel (asserted in
 * tests/test_assignpwr_cpu.py).  Returns 0, or non-zero with a message in d2d_assignpwr_last_error().                         */
#ifndef D2D_ASSIGNPWR_H
#define D2D_ASSIGNPWR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the law ids and limits of include/d2d_assign.h */
#define D2D_ASSIGNPWR_LAW_INV_SQUARE 0
#define D2D_ASSIGNPWR_LAW_POWER 1
#define D2D_ASSIGNPWR_LAW_POW_K 2

#define D2D_ASSIGNPWR_MAX_LINKS 2048
#define D2D_ASSIGNPWR_MAX_RBS 8192
#define D2D_ASSIGNPWR_MAX_LDS_BYTES 163840
#define D2D_ASSIGNPWR_MAX_LEVELS 64
#define D2D_ASSIGNPWR_CHUNK 8
#define D2D_ASSIGNPWR_NO_POWER (-32768)

int d2d_assign_power_weights(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                             const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                             int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* movable_links,
                             int32_t n_movable, const uint32_t* allowed, const int32_t* p_min, const int32_t* p_max,
                             const float* floor_db, float* weights, int32_t* power_dbm, void* hip_stream);
const char* d2d_assignpwr_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_ASSIGNPWR_H */
