/* libd2d_evaluate.so - what-if evaluation: the SINR and capacity planes K candidate joint assignments of (RB, tx power) would give
 * in every env, at the env's current positions (gym_d2d_amd.envs.VecD2DEnv.evaluate / evaluate_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.
 *
 * d2d_evaluate, per env b and candidate k, with rb = rb[b][k], pwr = pwr_dbm[b][k]:
 *
 *   I_j           = sum over links i != j with rb[i] == rb[j] of  lin(eirp_i - PL(tx_i -> rx_j))                    [mW]
 *   sinr_db[j]    = dB(S_j / (I_j + noise_j))
 *   capacity[j]   = sinr_db[j] > sens_db[rx_j] ? bw_mhz[tx_j] * log2(1 + S_j / (I_j + noise_j)) : 0                 [Mbps]
 *   total[b][k]   = sum over j of capacity[j]
 *
 * eirp, S, noise and PL are d2d_sense.h's (the step's own terms).  I_j is the step's sum - float products in ascending link index i
 * into a double accumulator - and sinr_db / capacity are formed from it by the step's own operations, so both planes are, bit for
 * bit, what a step with that assignment exports at these positions.  total is accumulated in double over the float capacities in a
 * fixed order (no floating-point atomics) and rounded once: two calls give the same bits.  A candidate's results do not depend on
 * which other candidates the call holds.
 *
 *   pos_x, pos_y       f32 [n_envs][n_dev]              device positions (D2D_BUF_POS_X / D2D_BUF_POS_Y)
 *   rb, pwr_dbm        i32 [n_envs][n_cand][n_links]    the decoded planes of every candidate, in the units of D2D_BUF_RB /
 *                                                       D2D_BUF_PWR.  An rb outside [0, n_rbs) is outside the contract; it puts
 *                                                       the link ON NO RB, as in d2d_marginal_capacity: nobody interferes with it,
 *                                                       it interferes with nobody, nothing is written out of bounds
 *   link_tx, link_rx   i32 [n_links]                    device index of every link's transmitter and receiver, in [0, n_dev) (not
 *                                                       checked on the device: the caller's link list)
 *   dev_cols           f32 [6][n_dev]                   d2d_sense_rb's per-device columns (tx_lin, rx_pl, rx_lin, noise_mw, law columns)
 *   cap_cols           f32 [2][n_dev]                   d2d_marginal_capacity's: bw_mhz at a link's TRANSMITTER, sens_db at its RECEIVER
 *   law, pow_k         D2D_EVALUATE_LAW_*, as d2d_sense_rb's
 *   sinr_db, capacity_mbps   f32 [n_envs][n_cand][n_links] each; either may be NULL: that plane is not written
 *   total_mbps         f32 [n_envs][n_cand], required
 *
 * 1 <= n_links <= D2D_EVALUATE_MAX_LINKS, 1 <= n_rbs <= D2D_EVALUATE_MAX_RBS, 1 <= n_cand <= D2D_EVALUATE_MAX_CANDIDATES (one
 * workgroup serves D2D_EVALUATE_CHUNK candidates of one env; the grid's second dimension holds 65535 of them), 1 <= pow_k <= 8 with
 * D2D_EVALUATE_LAW_POW_K, n_dev >= 1, n_envs >= 0 (0: nothing to do).  One workgroup keeps an env's per-link constants and one
 * candidate's sorted lists in LDS: 64 bytes per link (80 with a power law) + 4 (n_rbs + 1) + 32; a shape that needs more than
 * D2D_EVALUATE_MAX_LDS_BYTES is refused.  Returns 0, or non-zero with a message in d2d_evaluate_last_error().                 */
#ifndef D2D_EVALUATE_H
#define D2D_EVALUATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_EVALUATE_LAW_INV_SQUARE 0
#define D2D_EVALUATE_LAW_POWER 1
#define D2D_EVALUATE_LAW_POW_K 2

#define D2D_EVALUATE_MAX_LINKS 2048
#define D2D_EVALUATE_MAX_RBS 8192
#define D2D_EVALUATE_CHUNK 8
#define D2D_EVALUATE_MAX_CANDIDATES 524280
#define D2D_EVALUATE_MAX_LDS_BYTES 163840

int d2d_evaluate(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                 const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k, int64_t n_envs,
                 int32_t n_cand, int32_t n_dev, int32_t n_links, int32_t n_rbs, float* sinr_db, float* capacity_mbps,
                 float* total_mbps, void* hip_stream);
const char* d2d_evaluate_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_EVALUATE_H */
