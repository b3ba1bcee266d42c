/* libd2d_sense.so - per-RB interference sensing (gym_d2d_amd.envs.VecD2DEnv.sense, RbSensingObsFunction).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_sense_rb, per env b, link i, resource block r, with the state as the last step left it:
 *
 *   I[b][i][r]    = sum over links j != i with rb[b][j] == r of  lin(eirp_j - PL(tx_j -> rx_i))                  [mW]
 *   sinr[b][i][r] = sig_i - dB(I[b][i][r] + lin(noise_i))                                                         [dB]
 *
 * eirp_j = pwr_dbm[b][j] + eirp_off_db[tx_j], sig_i = eirp_i - PL(tx_i -> rx_i) + rx_off_db[rx_i], noise_i = noise_dbm[rx_i],
 * PL(tx -> rx) = a_tx_db[tx] + a_rx_db[rx] + 10 exponent[tx] log10(d): the step's own terms (interferer terms omit the receiver's
 * gains, as the step does).  j != i is by link index.  sinr[b][i][r] is the SINR link i would get if it alone moved to RB r at
 * its current power; column r == rb[b][i] is the step's sinr_db; an RB nobody else uses gives I == 0.0 exactly and sinr == snr.
 * Sums are taken in ascending j in the step's precision (float products, double accumulator) without floating-point atomics: two
 * calls on the same state give the same bits.
 *
 *   pos_x, pos_y       f32 [n_envs][n_dev]     device positions (D2D_BUF_POS_X / D2D_BUF_POS_Y)
 *   rb, pwr_dbm        i32 [n_envs][n_links]   the decoded planes (D2D_BUF_RB / D2D_BUF_PWR).  An rb outside [0, n_rbs) puts link j
 *                                              ON NO RB: it interferes with nobody, nothing is written out of bounds, and its own
 *                                              row is still sensed (on every RB it meets that RB's other links)
 *   link_tx, link_rx   i32 [n_links]           device index of every link's transmitter and receiver, in [0, n_dev) (not checked
 *                                              on the device: the caller's link list)
 *   dev_cols           f32 [6][n_dev]          per-device columns, folded by the host in double precision:
 *                        0  tx_lin   = 10^((eirp_off_db - a_tx_db) / 10)        1  rx_pl    = 10^(-a_rx_db / 10)
 *                        2  rx_lin   = 10^(rx_off_db / 10)                      3  noise_mw = 10^(noise_dbm / 10)
 *                        4, 5  by law:  D2D_SENSE_LAW_INV_SQUARE  unused (every exponent is 2: gain = 1 / d^2)
 *                                       D2D_SENSE_LAW_POWER       head and tail of -exponent / 2: the head keeps the 12 leading
 *                                                                 mantissa bits of the float, the tail is the rest of the double
 *                                       D2D_SENSE_LAW_POW_K       -(exponent - pow_k) / 2 in [-1/4, 1/4], and 0: every link
 *                                                                 transmitter's exponent lies within 1/2 of the integer pow_k
 *   what               D2D_SENSE_SINR_DB or D2D_SENSE_INTERFERENCE_MW
 *   out                f32 [n_envs][n_links][n_rbs]
 *
 * 1 <= n_links <= 2048 (D2D_MAX_LINKS of d2d_hip.h), 1 <= n_rbs <= D2D_SENSE_MAX_RBS, 1 <= pow_k <= 8 with D2D_SENSE_LAW_POW_K,
 * n_envs >= 0 (0: nothing to do).  Returns 0, or non-zero with a message in d2d_sense_last_error().                            */
#ifndef D2D_SENSE_H
#define D2D_SENSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_SENSE_SINR_DB 0
#define D2D_SENSE_INTERFERENCE_MW 1

#define D2D_SENSE_LAW_INV_SQUARE 0
#define D2D_SENSE_LAW_POWER 1
#define D2D_SENSE_LAW_POW_K 2

#define D2D_SENSE_MAX_LINKS 2048
#define D2D_SENSE_MAX_RBS 8192

int d2d_sense_rb(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                 const int32_t* link_rx, const float* dev_cols, int32_t law, int32_t pow_k, int64_t n_envs, int32_t n_dev,
                 int32_t n_links, int32_t n_rbs, int32_t what, float* out, void* hip_stream);
const char* d2d_sense_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_SENSE_H */
