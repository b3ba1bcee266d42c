/* libd2d_plugin.so - device-side helpers for array-native path-loss plugins (gym_d2d_amd.path_loss.ArrayPathLoss).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle.
 *
 * d2d_plugin_normal fills out_dev with standard normals from the SAME counter-based stream the step kernel's built-in
 * shadowing draws (d2d_set_path_loss_shadowing, csrc/d2d_step_device.h: philox_normal): Box-Muller of Philox4x32-10 with
 * counter (first_env + b, step, j | i << 16, kind) and key seed.  A plugin that adds chi * z where the built-in model would
 * therefore reproduces it, and the values do not depend on how envs are chunked or sharded.
 *
 *   out_dev   device memory of this process's current HIP device, float32 (dtype 0) or float64 (dtype 1), contiguous
 *             [n_envs][n_rows][n_cols]
 *   kind 0    element [b][j][i] uses j | i << 16 (tx link j -> rx link i: the SINR's signal and interferer evaluations)
 *   kind 1    n_rows must be 1: element [b][0][i] uses i | i << 16 (the SNR's own evaluation of link i's signal path)
 *   n_rows, n_cols <= 65536; first_env + n_envs <= 2^32
 *
 * Asynchronous on hip_stream (NULL: the null stream).  Returns 0, or non-zero with a message in d2d_plugin_last_error().    */
#ifndef D2D_PLUGIN_H
#define D2D_PLUGIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_PLUGIN_F32 0
#define D2D_PLUGIN_F64 1

int d2d_plugin_normal(void* out_dev, int32_t dtype, int64_t n_envs, uint64_t first_env, int32_t n_rows, int32_t n_cols,
                      uint64_t step, int32_t kind, uint64_t seed, void* hip_stream);
const char* d2d_plugin_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_PLUGIN_H */
