/* libd2d_marginal.so - per-agent difference rewards: what the system capacity loses when one link alone is taken out
 * (gym_d2d_amd.envs.VecD2DEnv.marginal_capacity, DifferenceRewardFunction).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.
 *
 * d2d_marginal_capacity, per env b, with the state as the last step left it and cap_k the step's capacity_mbps:
 *
 *   I_j        = sum over links k != j with rb[b][k] == rb[b][j] of  lin(eirp_k - PL(tx_k -> rx_j))               [mW]
 *   cap_j(I)   = sinr_db_j(I) > sens_db[rx_j] ? bw_mhz[tx_j] * log2(1 + S_j / (I + noise_j)) : 0                  [Mbps]
 *   harm[b][i] = sum over links j != i with rb[b][j] == rb[b][i] of  cap_j(I_j - t_ij) - cap_j(I_j),
 *                t_ij = lin(eirp_i - PL(tx_i -> rx_j)): what link i's transmitter puts into link j's receiver
 *   difference[b][i] = cap_i - harm[b][i]                 ( = G - G without link i,  G = sum over k of cap_k )
 *
 * eirp, S, noise and PL are d2d_sense.h's (the step's own terms); j != i and k != j are by link index.  I_j is the step's sum
 * (float products in ascending k into a double accumulator); I_j - t_ij is formed in double with the identical float t_ij that was
 * added, and every pair contributes one log2(1 + x) term of relative accuracy, summed in double in ascending j: no floating-point
 * atomics, two calls on the same state give the same bits.  harm >= 0; a link alone on its RB has harm == 0.0 exactly and
 * difference == cap_i, whose bits are the step's capacity plane.  difference is the float subtraction cap_i - harm[b][i].
 *
 *   pos_x, pos_y       f32 [n_envs][n_dev]     device positions (D2D_BUF_POS_X / D2D_BUF_POS_Y)
 *   rb, pwr_dbm        i32 [n_envs][n_links]   the decoded planes (D2D_BUF_RB / D2D_BUF_PWR).  An rb outside [0, n_rbs) puts a link
 *                                              ON NO RB, as in d2d_sense_rb: it harms nobody, nobody harms it, nothing is written
 *                                              out of bounds
 *   link_tx, link_rx   i32 [n_links]           device index of every link's transmitter and receiver, in [0, n_dev) (not checked
 *                                              on the device: the caller's link list)
 *   dev_cols           f32 [6][n_dev]          d2d_sense_rb's per-device columns (tx_lin, rx_pl, rx_lin, noise_mw, law columns)
 *   cap_cols           f32 [2][n_dev]          0  bw_mhz  = 1e-6 * bandwidth in Hz, read at a link's TRANSMITTER
 *                                              1  sens_db = the threshold sinr_db must exceed, read at a link's RECEIVER
 *   law, pow_k         D2D_MARGINAL_LAW_*, as d2d_sense_rb's
 *   harm_mbps, difference_mbps   f32 [n_envs][n_links] each
 *
 * 1 <= n_links <= D2D_MARGINAL_MAX_LINKS, 1 <= n_rbs <= D2D_MARGINAL_MAX_RBS, 1 <= pow_k <= 8 with D2D_MARGINAL_LAW_POW_K,
 * n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_marginal_last_error().                         */
#ifndef D2D_MARGINAL_H
#define D2D_MARGINAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_MARGINAL_LAW_INV_SQUARE 0
#define D2D_MARGINAL_LAW_POWER 1
#define D2D_MARGINAL_LAW_POW_K 2

#define D2D_MARGINAL_MAX_LINKS 2048
#define D2D_MARGINAL_MAX_RBS 8192

int d2d_marginal_capacity(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                          const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                          int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, float* harm_mbps, float* difference_mbps,
                          void* hip_stream);
const char* d2d_marginal_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_MARGINAL_H */
