/* libd2d_evaltab.so - what-if evaluation on a path-loss TABLE: the SINR and capacity planes K candidate joint assignments of
 * (RB, tx power) would give in every env when the step reads the given dB table by (tx link, rx link)
 * (gym_d2d_amd.envs.VecD2DEnv.evaluate_table / evaluate_table_actions).  d2d_evaluate (include/d2d_evaluate.h) with the pair path
 * loss read from memory instead of evaluated from positions and a law.
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream), no allocation.
 *
 * d2d_evaluate_table, per env b and candidate k, with rb = rb[b][k], pwr = pwr_dbm[b][k], T = table[b]:
 *
 *   I_i           = sum over links j != i with rb[j] == rb[i] of  lin(eirp_j - T[j][i])                              [mW]
 *   sinr_db[i]    = dB(lin(eirp_i - T[i][i] + rx_off_i) / (I_i + noise_i))
 *   capacity[i]   = sinr_db[i] > sens_db[rx_i] ? bw_mhz[tx_i] * log2(1 + sinr_i) : 0                                [Mbps]
 *   total[b][k]   = sum over i of capacity[i]
 *   domain[b][k]  = 1 if an entry READ for this candidate - T[i][i] of every link, T[j][i] of every same-RB pair - is NaN or -inf
 *                   (the step's D2D_FLAG_PATH_LOSS_DOMAIN, raised only where read), else 0.  +inf is a legal entry: gain 0.
 *
 * Every entry is converted where it is read, as the step's live-table mode converts it: (float)exp2(-log2(10)/10 * (double)x).
 * I_i is the step's sum - float products in ascending link index j into a double accumulator - and sinr_db / capacity are formed
 * from it by the step's own operations, so both planes are, bit for bit, what a step with that assignment exports when it reads
 * that table.  total is accumulated in double over the float capacities in d2d_evaluate's fixed order (no floating-point atomics)
 * and rounded once: two calls give the same bits.  A candidate's results do not depend on which other candidates the call holds.
 * The planes of a flagged candidate are whatever the arithmetic gives.
 *
 *   table              f32 or f64 [n_envs][table_rows][n_links], dB by (tx link, rx link); table_dtype D2D_EVALTAB_F32 / _F64;
 *                      table_rows n_links or n_links + 1 (the live table's layout: row n_links, the SNR's row, is never read)
 *   rb, pwr_dbm        i32 [n_envs][n_cand][n_links]    the decoded planes of every candidate, in the units of D2D_BUF_RB /
 *                                                       D2D_BUF_PWR.  An rb outside [0, n_rbs) puts the link ON NO RB, as in
 *                                                       d2d_evaluate: nobody interferes with it, it interferes with nobody, its own
 *                                                       entry is still read, nothing is written out of bounds
 *   link_tx, link_rx   i32 [n_links]                    device index of every link's transmitter and receiver, in [0, n_dev) (not
 *                                                       checked on the device: the caller's link list)
 *   dev_cols           f32 [3][n_dev]                   tx_lin (the EIRP offset, linear), rx_lin, noise_mw: the step's columns in its
 *                                                       table modes, where the path loss carries no per-device constant
 *   cap_cols           f32 [2][n_dev]                   d2d_marginal_capacity's: bw_mhz at a link's TRANSMITTER, sens_db at its RECEIVER
 *   sinr_db, capacity_mbps   f32 [n_envs][n_cand][n_links] each; either may be NULL: that plane is not written
 *   total_mbps         f32 [n_envs][n_cand], required
 *   domain             i32 [n_envs][n_cand], required
 *
 * 1 <= n_links <= D2D_EVALTAB_MAX_LINKS, 1 <= n_rbs <= D2D_EVALTAB_MAX_RBS, 1 <= n_cand <= D2D_EVALTAB_MAX_CANDIDATES (one
 * workgroup serves D2D_EVALTAB_CHUNK candidates of one env; the grid's second dimension holds 65535 of them), n_dev >= 1,
 * n_envs >= 0 (0: nothing to do).  One workgroup keeps an env's per-link constants and one candidate's sorted lists in LDS: 36
 * bytes per link + 4 (n_rbs + 1) + 48, each array rounded up to 16; a shape that needs more than D2D_EVALTAB_MAX_LDS_BYTES is
 * refused.  Returns 0, or non-zero with a message in d2d_evaltab_last_error().                                                    */
#ifndef D2D_EVALTAB_H
#define D2D_EVALTAB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_EVALTAB_F32 0
#define D2D_EVALTAB_F64 1

#define D2D_EVALTAB_MAX_LINKS 2048
#define D2D_EVALTAB_MAX_RBS 8192
#define D2D_EVALTAB_CHUNK 8
#define D2D_EVALTAB_MAX_CANDIDATES 524280
#define D2D_EVALTAB_MAX_LDS_BYTES 163840

int d2d_evaluate_table(const void* table, int32_t table_dtype, int32_t table_rows, const int32_t* rb, const int32_t* pwr_dbm,
                       const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int64_t n_envs,
                       int32_t n_cand, int32_t n_dev, int32_t n_links, int32_t n_rbs, float* sinr_db, float* capacity_mbps,
                       float* total_mbps, int32_t* domain, void* hip_stream);
const char* d2d_evaltab_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_EVALTAB_H */
