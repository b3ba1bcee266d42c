/* libd2d_graph.so - the interference graph (gym_d2d_amd.envs.VecD2DEnv.coupling / neighbors, NeighborObsFunction).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).  Arguments are checked
 * before any launch.
 *
 * Per env b, RECEIVER link i, TRANSMITTER link j, with the step's own terms (interferer terms omit the receiver's gains, as the step
 * does):
 *
 *   coupling_db[b][i][j] = eirp_off_db[tx_j] - PL(tx_j -> rx_i)          dBm received at rx_i per 0 dBm of tx power of link j
 *
 * PL(tx -> rx) = a_tx_db[tx] + a_rx_db[rx] + 10 exponent[tx] log10(d), so the step's interference on link i is the sum over
 * j != i with rb_j == rb_i of lin(pwr_j + coupling_db[b][i][j]).  INDEX ORDER: [b][i][j] is receiver-major, one agent's row
 * contiguous; the path-loss tables of include/d2d_hip.h are [b][j][i].  The diagonal holds the same formula (own transmitter into
 * own receiver, no receiver gains).  Every kernel here evaluates a pair by the same operations in the same order (the step's
 * fmaf(dx, dx, dy * dy) and pair_gain, then (tx_lin * gain) * rx_pl; the dB with the exponent taken exactly), without
 * floating-point atomics: the selection's values are entries of the dense matrix bit for bit, and two calls on the same state give
 * the same bits.
 *
 * Common inputs, as d2d_sense_rb takes them (include/d2d_sense.h):
 *   pos_x, pos_y       f32 [n_envs][n_dev]     device positions (D2D_BUF_POS_X / D2D_BUF_POS_Y)
 *   link_tx, link_rx   i32 [n_links]           device index of every link's transmitter and receiver, in [0, n_dev) (not checked on
 *                                              the device: the caller's link list)
 *   dev_cols           f32 [6][n_dev]          the folded per-device columns of d2d_sense_rb (rows 0, 1, 4, 5 are read here)
 *   law, pow_k         D2D_SENSE_LAW_* of include/d2d_sense.h, 1 <= pow_k <= 8 with D2D_SENSE_LAW_POW_K
 *
 * d2d_graph_coupling       out f32 [n_envs][n_links][n_links]: the dense matrix.
 * d2d_graph_neighbors      for every (b, i) the k links j != i with the largest coupling_db[b][i][j], strongest first; equal values
 *                          in ascending j.  idx i32 [n_envs][n_links][k], coupling_db f32 [n_envs][n_links][k],
 *                          1 <= k <= min(n_links - 1, D2D_GRAPH_MAX_K).  env_mask u8 [n_envs] or NULL (= all): the rows of an env
 *                          whose byte is 0 are left untouched.  Depends on positions and the model only, never on actions.
 * d2d_graph_neighbor_obs   the per-step gather, out f32 [n_envs][n_links][k + 1][4]:
 *                            [0]      own       (rb, pwr_dbm, sinr_db, snr_db) of link i
 *                            [1 + m]  rank m    (coupling_db[b][i][m], rb[b][j], pwr_dbm[b][j], sinr_db[b][j]), j = idx[b][i][m]
 *                          rb, pwr_dbm i32 and sinr_db, snr_db f32 [n_envs][n_links] are the step's planes (D2D_BUF_RB, D2D_BUF_PWR,
 *                          D2D_BUF_SINR_DB, D2D_BUF_SNR_DB).  An idx entry outside [0, n_links) reads nothing: its three gathered
 *                          values are NaN.  0 <= k <= D2D_GRAPH_MAX_K.
 *
 * 1 <= n_links <= 2048, n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_graph_last_error().       */
#ifndef D2D_GRAPH_H
#define D2D_GRAPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_GRAPH_MAX_LINKS 2048
#define D2D_GRAPH_MAX_K 64

int d2d_graph_coupling(const float* pos_x, const float* pos_y, const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols,
                       int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links, float* out, void* hip_stream);
int d2d_graph_neighbors(const float* pos_x, const float* pos_y, const int32_t* link_tx, const int32_t* link_rx, const float* dev_cols,
                        int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t k,
                        const uint8_t* env_mask, int32_t* idx, float* coupling_db, void* hip_stream);
int d2d_graph_neighbor_obs(const int32_t* idx, const float* coupling_db, const int32_t* rb, const int32_t* pwr_dbm,
                           const float* sinr_db, const float* snr_db, int64_t n_envs, int32_t n_links, int32_t k, float* out,
                           void* hip_stream);
const char* d2d_graph_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_GRAPH_H */
