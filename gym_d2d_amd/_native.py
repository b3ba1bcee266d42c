"""ctypes binding of libd2d_hip.so (include/d2d_hip.h) and of the side libraries `SIDE`, `SOLVERS`, `ADDONS`, `FAMILIES`, `EXTRAS`, `EXACT`, `GROWING` and `LATER` list
(libd2d_<name>.so, include/d2d_<name>.h).
There is no CPU fallback: if a library or a gfx950 GPU is missing, the calls below raise."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / 'lib' / 'libd2d_hip.so'
ABI_VERSION = 7
MAX_LINKS = 2048

# d2d_status
OK, ERR_INVALID, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED, ERR_NO_MEMORY = 0, 1, 2, 3, 4, 5
# d2d_link_type
UPLINK, DOWNLINK, SIDELINK = 1, 2, 3
# d2d_reward_fn
REWARD_NONE, REWARD_SYSTEM_CAPACITY, REWARD_SHANNON, REWARD_CUE_SINR_SHANNON = 0, 1, 2, 3
# d2d_obs_mode
OBS_NONE, OBS_TABLE, OBS_LINEAR = 0, 1, 2
# d2d_buffer
(BUF_POS_X, BUF_POS_Y, BUF_ACTIONS, BUF_RB, BUF_PWR, BUF_SINR_DB, BUF_SNR_DB, BUF_RATE_BPS, BUF_CAPACITY,
 BUF_REWARD, BUF_OBS_TABLE, BUF_OBS, BUF_ENV_FLAGS, BUF_LINK_POS, BUF_REWARD_ENV, BUF_RESET_PENDING, BUF_EPISODE,
 BUF_COUNT) = range(18)
FLAG_ZERO_DISTANCE, FLAG_RB_OUT_OF_RANGE, FLAG_NON_FINITE, FLAG_PATH_LOSS_DOMAIN = 1, 2, 4, 8
# d2d_set_path_loss_link_table_dev's per_env: 0 [N,N], 1 [B,N,N] (converted once), PL_TABLE_LIVE [B,N+1,N] (bound, read every step)
PL_TABLE_LIVE = 2
# d2d_reset_positions's episode: reset the envs BUF_RESET_PENDING marks, each at its BUF_EPISODE entry
EPISODE_PER_ENV = (1 << 64) - 1
# d2d_tuning (TUNE_OBS_VARIANT, TUNE_STEP_ABLATE, TUNE_OBS_STAGGER: include/d2d_hip_diag.h, diagnostic builds only)
(TUNE_OBS_ROWS_PER_WG, TUNE_OBS_NONTEMPORAL, TUNE_OBS_XCD_REMAP, TUNE_OBS_BLOCK, TUNE_OBS_VARIANT,
 TUNE_STEP_THREADS, TUNE_STEP_ENVS_PER_WG, TUNE_STEP_BLOCK, TUNE_STEP_FUSE_OBS, TUNE_STEP_ABLATE,
 TUNE_STEP_WALK, TUNE_STEP_PREFETCH, TUNE_STEP_LPT, TUNE_STEP_NT_RESULTS, TUNE_STEP_SCALAR_RECORDS,
 TUNE_STEP_OBS_ROTATE, TUNE_OBS_STAGGER) = range(17)
# d2d_reward_layout
REWARD_PER_AGENT, REWARD_PER_ENV = 0, 1
# d2d_dtype
F32, F64 = 0, 1
UNIQUE_ID_BYTES = 128
# d2d_sense_rb's what / law (include/d2d_sense.h)
SENSE_SINR_DB, SENSE_INTERFERENCE_MW = 0, 1
SENSE_LAW_INV_SQUARE, SENSE_LAW_POWER, SENSE_LAW_POW_K = 0, 1, 2
SENSE_MAX_RBS = 8192
# d2d_graph_neighbors's largest k (include/d2d_graph.h)
GRAPH_MAX_K = 64
# d2d_marginal_capacity's law / limits (include/d2d_marginal.h): the sensing kernel's
MARGINAL_LAW_INV_SQUARE, MARGINAL_LAW_POWER, MARGINAL_LAW_POW_K = 0, 1, 2
MARGINAL_MAX_RBS = 8192
# d2d_channel_fill's fading (include/d2d_channel.h)
CHANNEL_FADING_NONE, CHANNEL_FADING_RAYLEIGH, CHANNEL_FADING_RICIAN = 0, 1, 2
# d2d_queue_step's limits (include/d2d_queue.h)
QUEUE_MAX_DEADLINE, QUEUE_TABLE = 32, 64
# d2d_best_rb's law / limits (include/d2d_bestrb.h): the sensing kernel's
BESTRB_LAW_INV_SQUARE, BESTRB_LAW_POWER, BESTRB_LAW_POW_K = 0, 1, 2
BESTRB_MAX_RBS = 8192
# d2d_power_control's law / limits (include/d2d_powerctl.h): the sensing kernel's
POWERCTL_LAW_INV_SQUARE, POWERCTL_LAW_POWER, POWERCTL_LAW_POW_K = 0, 1, 2
POWERCTL_MAX_RBS = 8192
# d2d_best_response_dynamics's law / limits (include/d2d_brdyn.h): the sensing kernel's, and the LDS of one workgroup
BRDYN_LAW_INV_SQUARE, BRDYN_LAW_POWER, BRDYN_LAW_POW_K = 0, 1, 2
BRDYN_MAX_RBS = 8192
BRDYN_MAX_ROUNDS = 1024
BRDYN_MAX_LDS_BYTES = 163840
# d2d_evaluate's law / limits (include/d2d_evaluate.h): the sensing kernel's, the candidates one workgroup serves and one launch holds
EVALUATE_LAW_INV_SQUARE, EVALUATE_LAW_POWER, EVALUATE_LAW_POW_K = 0, 1, 2
EVALUATE_MAX_RBS = 8192
EVALUATE_CHUNK = 8
EVALUATE_MAX_CANDIDATES = 65535 * EVALUATE_CHUNK
EVALUATE_MAX_LDS_BYTES = 163840
# d2d_assign_weights's law / objective / limits (include/d2d_assign.h): the sensing kernel's, and the LDS of one workgroup
ASSIGN_LAW_INV_SQUARE, ASSIGN_LAW_POWER, ASSIGN_LAW_POW_K = 0, 1, 2
ASSIGN_OBJECTIVE_TOTAL, ASSIGN_OBJECTIVE_OWN = 0, 1
ASSIGN_MAX_RBS = 8192
ASSIGN_MAX_LDS_BYTES = 163840
# d2d_assign_power_weights's law / limits (include/d2d_assignpwr.h): d2d_assign_weights's, and the power alphabet of a movable link
ASSIGNPWR_LAW_INV_SQUARE, ASSIGNPWR_LAW_POWER, ASSIGNPWR_LAW_POW_K = 0, 1, 2
ASSIGNPWR_MAX_RBS = 8192
ASSIGNPWR_MAX_LDS_BYTES = 163840
ASSIGNPWR_MAX_LEVELS = 64
ASSIGNPWR_CHUNK = 8
ASSIGNPWR_NO_POWER = -32768
# d2d_color_graph's limits (include/d2d_color.h): the links and RBs an env may have, and the LDS of one workgroup
COLOR_MAX_LINKS = 2048
COLOR_MAX_RBS = 8192
COLOR_MAX_LDS_BYTES = 163840
# d2d_balance_sinr's law / limits (include/d2d_balance.h): d2d_power_control's, the levels of the grid and the LDS of one workgroup
BALANCE_LAW_INV_SQUARE, BALANCE_LAW_POWER, BALANCE_LAW_POW_K = 0, 1, 2
BALANCE_MAX_LINKS = 2048
BALANCE_MAX_RBS = 8192
BALANCE_MAX_MARGINS = 4096
BALANCE_MAX_LDS_BYTES = 163840
# d2d_stable_match's limits (include/d2d_stable.h): the rows and columns an env may have, and the LDS of one workgroup
STABLE_MAX_LINKS = 2048
STABLE_MAX_RBS = 8192
STABLE_MAX_LDS_BYTES = 163840
# d2d_share_values's law / limits (include/d2d_share.h): the sensing kernel's, the movable links of one call, the background members
# of an RB that takes movable links, the LDS of one workgroup and the bytes of the value block and the choice words together
SHARE_LAW_INV_SQUARE, SHARE_LAW_POWER, SHARE_LAW_POW_K = 0, 1, 2
SHARE_MAX_LINKS = 2048
SHARE_MAX_RBS = 8192
SHARE_MAX_MOVABLE = 12
SHARE_MAX_BACKGROUND = 64
SHARE_MAX_LDS_BYTES = 163840
SHARE_MAX_BLOCK_BYTES = 8 << 30
# d2d_power_ascent's law / start / limits (include/d2d_ascent.h): d2d_evaluate's, the levels of a link's power alphabet (one lane
# each), the rounds of one launch and the LDS of one workgroup
ASCENT_LAW_INV_SQUARE, ASCENT_LAW_POWER, ASCENT_LAW_POW_K = 0, 1, 2
ASCENT_START_HELD, ASCENT_START_MIN, ASCENT_START_MAX = 0, 1, 2
ASCENT_MAX_LINKS = 2048
ASCENT_MAX_RBS = 8192
ASCENT_MAX_LEVELS = 64
ASCENT_MAX_ROUNDS = 4096
ASCENT_MAX_LDS_BYTES = 163840
# d2d_rb_ascent's law / limits (include/d2d_rbascent.h): d2d_evaluate's, the rounds of one launch and the LDS of one workgroup
RBASCENT_LAW_INV_SQUARE, RBASCENT_LAW_POWER, RBASCENT_LAW_POW_K = 0, 1, 2
RBASCENT_MAX_LINKS = 2048
RBASCENT_MAX_RBS = 8192
RBASCENT_MAX_ROUNDS = 4096
RBASCENT_MAX_LDS_BYTES = 163840
# d2d_goodput_ascent's law / move bits / limits (include/d2d_goodput.h): d2d_rb_ascent's, the levels of a link's power alphabet and
# the largest weight
GOODPUT_LAW_INV_SQUARE, GOODPUT_LAW_POWER, GOODPUT_LAW_POW_K = 0, 1, 2
GOODPUT_MOVE_RB, GOODPUT_MOVE_POWER = 1, 2
GOODPUT_MAX_LINKS = 2048
GOODPUT_MAX_RBS = 8192
GOODPUT_MAX_LEVELS = 64
GOODPUT_MAX_ROUNDS = 4096
GOODPUT_MAX_WEIGHT = 1 << 20
GOODPUT_MAX_LDS_BYTES = 163840
# d2d_deviation_gains' / d2d_best_deviation's law / limits (include/d2d_deviate.h): d2d_goodput_ascent's, and the bytes of one table
DEVIATE_LAW_INV_SQUARE, DEVIATE_LAW_POWER, DEVIATE_LAW_POW_K = 0, 1, 2
DEVIATE_MAX_LINKS = 2048
DEVIATE_MAX_RBS = 8192
DEVIATE_MAX_LEVELS = 64
DEVIATE_MAX_LDS_BYTES = 163840
DEVIATE_MAX_TABLE_BYTES = 8 << 30
# d2d_evaluate_table's entry types / limits (include/d2d_evaltab.h): the entry types are F32 / F64 above, the limits d2d_evaluate's
EVALTAB_F32, EVALTAB_F64 = 0, 1
EVALTAB_MAX_LINKS = 2048
EVALTAB_MAX_RBS = 8192
EVALTAB_CHUNK = 8
EVALTAB_MAX_CANDIDATES = 65535 * EVALTAB_CHUNK
EVALTAB_MAX_LDS_BYTES = 163840
# d2d_table_rb_ascent's entry types / limits (include/d2d_tabascent.h): d2d_evaluate_table's entry types, d2d_rb_ascent's limits
TABASCENT_F32, TABASCENT_F64 = 0, 1
TABASCENT_MAX_LINKS = 2048
TABASCENT_MAX_RBS = 8192
TABASCENT_MAX_ROUNDS = 4096
TABASCENT_MAX_LDS_BYTES = 163840
# d2d_table_marginal's entry types / limits (include/d2d_tabmarg.h): d2d_evaluate_table's entry types, d2d_marginal_capacity's limits
TABMARG_F32, TABMARG_F64 = 0, 1
TABMARG_MAX_LINKS = 2048
TABMARG_MAX_RBS = 8192
TABMARG_MAX_LDS_BYTES = 163840

BUFFER_DTYPES = {BUF_ACTIONS: np.int32, BUF_RB: np.int32, BUF_PWR: np.int32, BUF_ENV_FLAGS: np.int32, BUF_RESET_PENDING: np.int32,
                 BUF_EPISODE: np.uint32}


class Config(C.Structure):
    _fields_ = [
        ('abi_version', C.c_int32), ('device_ordinal', C.c_int32), ('num_envs', C.c_int32),
        ('num_rbs', C.c_int32), ('num_cues', C.c_int32), ('num_due_pairs', C.c_int32),
        ('max_links', C.c_int32), ('pwr_levels_due', C.c_int32), ('pwr_levels_cue', C.c_int32),
        ('pwr_levels_mbs', C.c_int32), ('cell_radius_m', C.c_float), ('d2d_radius_m', C.c_float),
    ]


class HostLayout(C.Structure):
    """d2d_host_layout: byte offsets of every result inside the pinned block d2d_step_host returns."""
    _fields_ = [(name, C.c_size_t) for name in ('sinr_db', 'snr_db', 'rate_bps', 'capacity', 'reward', 'rb', 'pwr',
                                                 'obs_table', 'env_flags', 'obs', 'total_bytes')]


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f'libd2d_hip error {code}: {message}')
        self.code = code
        self.message = message


_P = C.c_void_p
_I = C.c_int32
_DP = C.POINTER(C.c_double)
_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int32)

# every symbol include/d2d_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    'd2d_create': (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    'd2d_destroy': (C.c_int, [_P]),
    'd2d_last_error': (C.c_char_p, []),
    'd2d_abi_version': (C.c_int, []),
    'd2d_set_stream': (C.c_int, [_P, _P]),
    'd2d_synchronize': (C.c_int, [_P]),
    'd2d_set_device_table': (C.c_int, [_P, _I, _DP, _DP, _DP, _DP, _DP]),
    'd2d_set_path_loss_power_law': (C.c_int, [_P, _I, _DP, _DP, _DP]),
    'd2d_set_path_loss_table': (C.c_int, [_P, _DP, _I]),
    'd2d_set_path_loss_link_table': (C.c_int, [_P, _DP, _I, _I]),
    'd2d_set_path_loss_link_table_dev': (C.c_int, [_P, _P, _I, _I, _I]),
    'd2d_set_path_loss_shadowing': (C.c_int, [_P, _I, _DP, _DP, _DP, C.c_double, C.c_double, C.c_uint64]),
    'd2d_set_links': (C.c_int, [_P, _I, _IP, _IP, _IP]),
    'd2d_set_fixed_actions': (C.c_int, [_P, _I, _IP, _IP, _IP]),
    'd2d_positions_changed': (C.c_int, [_P]),
    'd2d_set_reward': (C.c_int, [_P, _I, C.c_float]),
    'd2d_set_obs_mode': (C.c_int, [_P, _I]),
    'd2d_set_reward_layout': (C.c_int, [_P, _I]),
    'd2d_set_obs_dtype': (C.c_int, [_P, _I]),
    'd2d_set_bucketing': (C.c_int, [_P, _I]),
    'd2d_set_export_actions': (C.c_int, [_P, _I]),
    'd2d_set_tuning': (C.c_int, [_P, _I, _I]),
    'd2d_get_buffer': (C.c_int, [_P, _I, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    'd2d_bind_buffer': (C.c_int, [_P, _I, _P, C.c_size_t]),
    'd2d_upload': (C.c_int, [_P, _I, _P, C.c_size_t, C.c_size_t]),
    'd2d_download': (C.c_int, [_P, _I, _P, C.c_size_t, C.c_size_t]),
    'd2d_set_positions': (C.c_int, [_P, _FP, _FP, _I, _I]),
    'd2d_set_positions_f64': (C.c_int, [_P, _DP, _DP, _I, _I]),
    'd2d_reset_positions': (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint8), _FP]),
    'd2d_set_env_offset': (C.c_int, [_P, C.c_uint64]),
    'd2d_step': (C.c_int, [_P, _P]),
    'd2d_step_rb_pwr': (C.c_int, [_P, _P, _P]),
    'd2d_expand_table': (C.c_int, [_P, _P, _I, _I, _P]),
    'd2d_step_host': (C.c_int, [_P, _IP, _IP, C.POINTER(_P), C.POINTER(HostLayout)]),
    'd2d_status_flags': (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    'd2d_comm_unique_id': (C.c_int, [_P]),
    'd2d_comm_init': (C.c_int, [_P, _I, _I, _P]),
    'd2d_comm_destroy': (C.c_int, [_P]),
    'd2d_allgather': (C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    'd2d_profile_enable': (C.c_int, [_P, _I]),
    'd2d_profile_read': (C.c_int, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'd2d_profile_reset': (C.c_int, [_P]),
    'd2d_profile_median': (C.c_int, [_P, _I, C.POINTER(C.c_double)]),
}

# every symbol include/d2d_plugin.h declares
PLUGIN_SIGNATURES = {
    'd2d_plugin_normal': (C.c_int, [_P, _I, C.c_int64, C.c_uint64, _I, _I, C.c_uint64, _I, C.c_uint64, _P]),
    'd2d_plugin_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_episode.h declares
EPISODE_SIGNATURES = {
    'd2d_episode_merge_actions': (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _I, C.c_uint64, C.c_uint64, _P]),
    'd2d_episode_advance': (C.c_int, [_P, _P, _P, _P, _P, _P, _I, C.c_int64, _I, _P]),
    'd2d_episode_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_sense.h declares
SENSE_SIGNATURES = {
    'd2d_sense_rb': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _I, _P, _P]),
    'd2d_sense_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_graph.h declares
GRAPH_SIGNATURES = {
    'd2d_graph_coupling': (C.c_int, [_P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _P, _P]),
    'd2d_graph_neighbors': (C.c_int, [_P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _P]),
    'd2d_graph_neighbor_obs': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _P, _P]),
    'd2d_graph_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_marginal.h declares
MARGINAL_SIGNATURES = {
    'd2d_marginal_capacity': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P]),
    'd2d_marginal_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_mobility.h declares
MOBILITY_SIGNATURES = {
    'd2d_mobility_move': (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _I, _I, C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    'd2d_mobility_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_channel.h declares
CHANNEL_SIGNATURES = {
    'd2d_channel_fill': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, C.c_uint64, _I, C.c_float, C.c_double, _I, C.c_float,
                                   C.c_float, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _I, _P]),
    'd2d_channel_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_queue.h declares
QUEUE_SIGNATURES = {
    'd2d_queue_step': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, C.c_int64, C.c_int64, C.c_double,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    'd2d_queue_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_bestrb.h declares
BESTRB_SIGNATURES = {
    'd2d_best_rb': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    'd2d_bestrb_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_powerctl.h declares
POWERCTL_SIGNATURES = {
    'd2d_power_control': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    'd2d_powerctl_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_brdyn.h declares
BRDYN_SIGNATURES = {
    'd2d_best_response_dynamics': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, C.c_float, _I, _P, _P, _P, _P,
                                             _P, _P, _P]),
    'd2d_brdyn_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_evaluate.h declares
EVALUATE_SIGNATURES = {
    'd2d_evaluate': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _I, _P, _P, _P, _P]),
    'd2d_evaluate_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_assign.h declares
ASSIGN_SIGNATURES = {
    'd2d_assign_weights': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P]),
    'd2d_assign_solve': (C.c_int, [_P, C.c_int64, _I, _I, _P, _P, _P, _P]),
    'd2d_assign_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_assignpwr.h declares
ASSIGNPWR_SIGNATURES = {
    'd2d_assign_power_weights': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P,
                                           _P]),
    'd2d_assignpwr_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_color.h declares
COLOR_SIGNATURES = {
    'd2d_color_graph': (C.c_int, [_P, _P, _P, _P, C.c_int64, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P]),
    'd2d_color_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_balance.h declares
BALANCE_SIGNATURES = {
    'd2d_balance_sinr': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P,
                                   _P, _P, _P]),
    'd2d_balance_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_stable.h declares
STABLE_SIGNATURES = {
    'd2d_stable_match': (C.c_int, [_P, _P, _P, C.c_int64, _I, _I, _P, _P, _P, _P, _P]),
    'd2d_stable_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_share.h declares
SHARE_SIGNATURES = {
    'd2d_share_values': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    'd2d_share_solve': (C.c_int, [_P, _P, C.c_int64, _I, _I, _P, _P, _P, _P, _P]),
    'd2d_share_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_ascent.h declares
ASCENT_SIGNATURES = {
    'd2d_power_ascent': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _P, _I, C.c_double, _I, _P, _P,
                                   _P, _P, _P, _P, _P, _P]),
    'd2d_ascent_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_rbascent.h declares
RBASCENT_SIGNATURES = {
    'd2d_rb_ascent': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, C.c_double, _I, _P, _P, _P, _P,
                                _P, _P, _P, _P]),
    'd2d_rbascent_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_goodput.h declares
GOODPUT_SIGNATURES = {
    'd2d_goodput_ascent': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _P, C.c_double, _P, _P, _P, _I,
                                     C.c_int64, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'd2d_goodput_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_deviate.h declares
DEVIATE_SIGNATURES = {
    'd2d_deviation_gains': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    'd2d_best_deviation': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_int64, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P, C.c_double, _P,
                                     _P, _P, _P, _P, _P, _P]),
    'd2d_deviate_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_evaltab.h declares
EVALTAB_SIGNATURES = {
    'd2d_evaluate_table': (C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    'd2d_evaltab_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_tabascent.h declares
TABASCENT_SIGNATURES = {
    'd2d_table_rb_ascent': (C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _P, _P, _P, C.c_double, _I, _P, _P, _P, _P,
                                      _P, _P, _P, _P, _P, _P]),
    'd2d_tabascent_last_error': (C.c_char_p, []),
}

# every symbol include/d2d_tabmarg.h declares
TABMARG_SIGNATURES = {
    'd2d_table_marginal': (C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _P, _P, _P, _P]),
    'd2d_tabmarg_last_error': (C.c_char_p, []),
}

# the side libraries: name -> every symbol include/d2d_<name>.h declares; libd2d_<name>.so, its error text in d2d_<name>_last_error
SIDE = {'plugin': PLUGIN_SIGNATURES, 'episode': EPISODE_SIGNATURES, 'sense': SENSE_SIGNATURES, 'graph': GRAPH_SIGNATURES,
        'marginal': MARGINAL_SIGNATURES, 'mobility': MOBILITY_SIGNATURES, 'channel': CHANNEL_SIGNATURES, 'queue': QUEUE_SIGNATURES,
        'bestrb': BESTRB_SIGNATURES, 'powerctl': POWERCTL_SIGNATURES, 'brdyn': BRDYN_SIGNATURES, 'evaluate': EVALUATE_SIGNATURES}
# build.SOLVERS' libraries: opened, typed and reported by the same loader
SOLVERS = {'assign': ASSIGN_SIGNATURES}
# build.ADDONS' libraries, likewise: the table later add-on kernel families join
ADDONS = {'assignpwr': ASSIGNPWR_SIGNATURES, 'color': COLOR_SIGNATURES}
# build.FAMILIES' libraries, likewise: the table the kernel families since then join
FAMILIES = {'balance': BALANCE_SIGNATURES}
# build.EXTRAS' libraries, likewise: what joined behind the families
EXTRAS = {'stable': STABLE_SIGNATURES}
# build.EXACT's libraries, likewise: what joined behind the extras
EXACT = {'share': SHARE_SIGNATURES}
# build.GROWING's libraries, likewise: what joined behind the exact solvers
GROWING = {'ascent': ASCENT_SIGNATURES}
# build.LATER's libraries, likewise: what joined behind the power ascent, and the table the next library joins
LATER = {'rbascent': RBASCENT_SIGNATURES, 'deviate': DEVIATE_SIGNATURES, 'tabmarg': TABMARG_SIGNATURES, 'evaltab': EVALTAB_SIGNATURES,
         'tabascent': TABASCENT_SIGNATURES, 'goodput': GOODPUT_SIGNATURES}

_lib: Optional[C.CDLL] = None
_side: dict = {}                    # name -> the opened, typed side library
# launches made through the wrappers below in this process
sense_launches = 0                  # d2d_sense_rb calls made through sense_rb()
graph_launches = {'coupling': 0, 'neighbors': 0, 'neighbor_obs': 0}     # launches made through the graph_*() wrappers
marginal_launches = 0               # d2d_marginal_capacity calls made through marginal_capacity()
bestrb_launches = 0                 # d2d_best_rb calls made through best_rb()
powerctl_launches = 0               # d2d_power_control launches made through power_control()
brdyn_launches = 0                  # d2d_best_response_dynamics launches made through best_response_dynamics()
evaluate_launches = 0               # d2d_evaluate launches made through evaluate()
assign_weights_launches = 0         # d2d_assign_weights launches made through assign_weights()
assign_solve_launches = 0           # d2d_assign_solve launches made through assign_solve()
assign_power_weights_launches = 0   # d2d_assign_power_weights launches made through assign_power_weights()
color_launches = 0                  # d2d_color_graph launches made through color_graph()
balance_launches = 0                # d2d_balance_sinr launches made through balance_sinr()
stable_launches = 0                 # d2d_stable_match launches made through stable_match()
share_values_launches = 0           # d2d_share_values launches made through share_values()
share_solve_launches = 0            # d2d_share_solve launches made through share_solve()
ascent_launches = 0                 # d2d_power_ascent launches made through power_ascent()
rbascent_launches = 0               # d2d_rb_ascent launches made through rb_ascent()
goodput_launches = 0                # d2d_goodput_ascent launches made through goodput_ascent()
deviate_launches = 0                # d2d_deviation_gains / d2d_best_deviation calls made through deviation_gains() / best_deviation()
evaltab_launches = 0                # d2d_evaluate_table launches made through evaluate_table()
tabascent_launches = 0              # d2d_table_rb_ascent calls made through table_rb_ascent() (two kernel launches each)
tabmarg_launches = 0                # d2d_table_marginal launches made through table_marginal()
mobility_launches = 0               # d2d_mobility_move calls made through mobility_move()
channel_launches = 0                # d2d_channel_fill calls made through channel_fill()
queue_launches = 0                  # d2d_queue_step calls made through queue_step()


def load_library() -> C.CDLL:
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f'{LIB_PATH} is missing - build it with `python -m gym_d2d_amd.build` '
                          '(gym_d2d_amd has no CPU fallback for the simulation path)')
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.d2d_abi_version() != ABI_VERSION:
        raise ImportError('libd2d_hip.so ABI version mismatch - rebuild it')
    _lib = lib
    return lib


def side_path(name: str) -> Path:
    return Path(__file__).resolve().parent / 'lib' / f'libd2d_{name}.so'


def side_library(name: str) -> C.CDLL:
    """dlopen libd2d_<name>.so once and type the entry points SIDE[name] (or SOLVERS[name], ADDONS[name], FAMILIES[name], EXTRAS[name], EXACT[name], GROWING[name], LATER[name]) lists.  Raises if it has not been built."""
    lib = _side.get(name)
    if lib is None:
        path = side_path(name)
        if not path.exists():
            raise ImportError(f'{path} is missing - build it with `python -m gym_d2d_amd.build`')
        lib = C.CDLL(str(path))
        for symbol, (res, args) in (SIDE.get(name) or SOLVERS.get(name) or ADDONS.get(name) or FAMILIES.get(name) or EXTRAS.get(name)
                                    or EXACT.get(name) or GROWING.get(name) or LATER[name]).items():
            fn = getattr(lib, symbol)
            fn.restype = res
            fn.argtypes = args
        _side[name] = lib
    return lib


def _check_side(name: str, rc: int) -> None:
    if rc != 0:
        raise NativeError(rc, getattr(side_library(name), f'd2d_{name}_last_error')().decode(errors='replace'))


# the public loaders: a caller that wants a missing library to fail early calls one (mobility.py, queues.py); the wrappers below
# go through them too, so replacing one intercepts every use of its library
def load_plugin_library() -> C.CDLL: return side_library('plugin')
def load_episode_library() -> C.CDLL: return side_library('episode')
def load_sense_library() -> C.CDLL: return side_library('sense')
def load_graph_library() -> C.CDLL: return side_library('graph')
def load_marginal_library() -> C.CDLL: return side_library('marginal')
def load_mobility_library() -> C.CDLL: return side_library('mobility')
def load_channel_library() -> C.CDLL: return side_library('channel')
def load_queue_library() -> C.CDLL: return side_library('queue')
def load_bestrb_library() -> C.CDLL: return side_library('bestrb')
def load_powerctl_library() -> C.CDLL: return side_library('powerctl')
def load_brdyn_library() -> C.CDLL: return side_library('brdyn')
def load_evaluate_library() -> C.CDLL: return side_library('evaluate')
def load_assign_library() -> C.CDLL: return side_library('assign')
def load_assignpwr_library() -> C.CDLL: return side_library('assignpwr')
def load_color_library() -> C.CDLL: return side_library('color')
def load_balance_library() -> C.CDLL: return side_library('balance')
def load_stable_library() -> C.CDLL: return side_library('stable')
def load_share_library() -> C.CDLL: return side_library('share')
def load_ascent_library() -> C.CDLL: return side_library('ascent')
def load_rbascent_library() -> C.CDLL: return side_library('rbascent')
def load_goodput_library() -> C.CDLL: return side_library('goodput')
def load_deviate_library() -> C.CDLL: return side_library('deviate')
def load_evaltab_library() -> C.CDLL: return side_library('evaltab')
def load_tabascent_library() -> C.CDLL: return side_library('tabascent')
def load_tabmarg_library() -> C.CDLL: return side_library('tabmarg')


# Pointer arguments are passed as the ints they are: every argtype is c_void_p, which takes 0 as the null pointer and any int up to
# 2^64 - 1 as that address.  The c_uint64(... & (2 ** 64 - 1)) and & 0xFFFFFFFF maskings define the wrap-around and stay.
def plugin_normal(out_ptr: int, dtype: int, n_envs: int, first_env: int, n_rows: int, n_cols: int, step: int, kind: int,
                  seed: int, stream_ptr: int = 0) -> None:
    """d2d_plugin_normal: standard normals of the built-in shadowing stream into device memory [n_envs, n_rows, n_cols]."""
    _check_side('plugin', load_plugin_library().d2d_plugin_normal(
        out_ptr, dtype, n_envs, C.c_uint64(first_env), n_rows, n_cols, C.c_uint64(step & (2 ** 64 - 1)), kind,
        C.c_uint64(seed & (2 ** 64 - 1)), stream_ptr))


def episode_merge_actions(in_ptr: int, out_ptr: int, pending_ptr: int, episode_ptr: int, high_ptr: int, n_envs: int, n_cols: int,
                          first_env: int, seed: int, stream_ptr: int = 0) -> None:
    """d2d_episode_merge_actions: out[b] = pending[b] ? the reset's random actions at episode[b] : in[b] (device pointers)."""
    _check_side('episode', load_episode_library().d2d_episode_merge_actions(
        in_ptr, out_ptr, pending_ptr, episode_ptr, high_ptr, n_envs, n_cols, C.c_uint64(first_env), C.c_uint64(seed & (2 ** 64 - 1)),
        stream_ptr))


def episode_advance(pending_ptr: int, episode_ptr: int, elapsed_ptr: int, done_ptr: int, reset_ptr: int, reward_ptr: int,
                    reward_cols: int, n_envs: int, episode_length: int, stream_ptr: int = 0) -> None:
    """d2d_episode_advance: per-env counters after a step; zeroes the reward rows of the envs that were reset (reward_ptr 0: none)."""
    _check_side('episode', load_episode_library().d2d_episode_advance(
        pending_ptr, episode_ptr, elapsed_ptr, done_ptr, reset_ptr, reward_ptr, reward_cols, n_envs, episode_length, stream_ptr))


def sense_rb(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int, law: int,
             pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, what: int, out_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_sense_rb: every link's SINR (dB) or interference (mW) on every RB into out [n_envs, n_links, n_rbs] (device pointers)."""
    global sense_launches
    _check_side('sense', load_sense_library().d2d_sense_rb(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, n_rbs, what,
        out_ptr, stream_ptr))
    sense_launches += 1


def graph_coupling(pos_x_ptr: int, pos_y_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int, law: int, pow_k: int,
                   n_envs: int, n_dev: int, n_links: int, out_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_graph_coupling: coupling_db [n_envs, n_links (receiver i), n_links (transmitter j)] into out (device pointers)."""
    _check_side('graph', load_graph_library().d2d_graph_coupling(
        pos_x_ptr, pos_y_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, out_ptr, stream_ptr))
    graph_launches['coupling'] += 1


def graph_neighbors(pos_x_ptr: int, pos_y_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int, law: int, pow_k: int,
                    n_envs: int, n_dev: int, n_links: int, k: int, env_mask_ptr: int, idx_ptr: int, coupling_ptr: int,
                    stream_ptr: int = 0) -> None:
    """d2d_graph_neighbors: every receiver's k strongest interferers, idx / coupling_db [n_envs, n_links (receiver i), k] (device
    pointers; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte is 0 keep their rows)."""
    _check_side('graph', load_graph_library().d2d_graph_neighbors(
        pos_x_ptr, pos_y_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, k, env_mask_ptr, idx_ptr,
        coupling_ptr, stream_ptr))
    graph_launches['neighbors'] += 1


def graph_neighbor_obs(idx_ptr: int, coupling_ptr: int, rb_ptr: int, pwr_ptr: int, sinr_ptr: int, snr_ptr: int, n_envs: int,
                       n_links: int, k: int, out_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_graph_neighbor_obs: the per-step gather, out [n_envs, n_links (receiver i), k + 1, 4] (device pointers)."""
    _check_side('graph', load_graph_library().d2d_graph_neighbor_obs(
        idx_ptr, coupling_ptr, rb_ptr, pwr_ptr, sinr_ptr, snr_ptr, n_envs, n_links, k, out_ptr, stream_ptr))
    graph_launches['neighbor_obs'] += 1


def marginal_capacity(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                      cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, harm_ptr: int,
                      diff_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_marginal_capacity: every link's harm and difference reward (Mbps) into two planes [n_envs, n_links] (device pointers)."""
    global marginal_launches
    _check_side('marginal', load_marginal_library().d2d_marginal_capacity(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, harm_ptr, diff_ptr, stream_ptr))
    marginal_launches += 1


def best_rb(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int, law: int,
            pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, allowed_ptr: int, env_mask_ptr: int, best_rb_ptr: int,
            best_sinr_ptr: int, gain_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_best_rb: every link's best RB (int32), the SINR there and the gain over its own RB (dB) into three planes [n_envs, n_links]
    (device pointers; allowed_ptr 0: every RB, else uint32 [n_links, ceil(n_rbs / 32)]; env_mask_ptr 0: every env, else uint8
    [n_envs] and the envs whose byte is 0 keep their rows)."""
    global bestrb_launches
    _check_side('bestrb', load_bestrb_library().d2d_best_rb(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, n_rbs,
        allowed_ptr, env_mask_ptr, best_rb_ptr, best_sinr_ptr, gain_ptr, stream_ptr))
    bestrb_launches += 1


def power_control(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                  law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, target_ptr: int, p_min_ptr: int,
                  p_max_ptr: int, adjustable_ptr: int, max_iters: int, env_mask_ptr: int, power_ptr: int, sinr_ptr: int,
                  iters_ptr: int, converged_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_power_control: the target-SINR power iteration of every env in one launch - power_dbm int32 and sinr_db float32
    [n_envs, n_links], iters int32 and converged uint8 [n_envs] (device pointers; target float32, p_min / p_max int32 [n_links];
    adjustable_ptr 0: every link, else uint8 [n_links]; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte is 0
    keep their rows)."""
    global powerctl_launches
    _check_side('powerctl', load_powerctl_library().d2d_power_control(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, n_rbs,
        target_ptr, p_min_ptr, p_max_ptr, adjustable_ptr, max_iters, env_mask_ptr, power_ptr, sinr_ptr, iters_ptr, converged_ptr,
        stream_ptr))
    if n_envs:
        powerctl_launches += 1


def best_response_dynamics(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                           law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, allowed_ptr: int, movable_ptr: int,
                           min_gain_db: float, max_rounds: int, env_mask_ptr: int, rb_out_ptr: int, sinr_ptr: int, rounds_ptr: int,
                           moves_ptr: int, converged_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_best_response_dynamics: sequential best response on the RBs of every env in one launch - rb int32 and sinr_db float32
    [n_envs, n_links], rounds / moves int32 and converged uint8 [n_envs] (device pointers; allowed_ptr 0: every RB, else uint32
    [n_links, ceil(n_rbs / 32)]; movable_ptr 0: every link, else uint8 [n_links]; env_mask_ptr 0: every env, else uint8 [n_envs]
    and the envs whose byte is 0 keep their rows)."""
    global brdyn_launches
    _check_side('brdyn', load_brdyn_library().d2d_best_response_dynamics(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, n_rbs,
        allowed_ptr, movable_ptr, min_gain_db, max_rounds, env_mask_ptr, rb_out_ptr, sinr_ptr, rounds_ptr, moves_ptr, converged_ptr,
        stream_ptr))
    if n_envs:
        brdyn_launches += 1


def evaluate(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
             cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_cand: int, n_dev: int, n_links: int, n_rbs: int, sinr_ptr: int,
             capacity_ptr: int, total_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_evaluate: the planes n_cand candidate assignments per env would give - sinr_db and capacity_mbps float32 [n_envs, n_cand,
    n_links] (either pointer 0: not written) and total_mbps float32 [n_envs, n_cand] (device pointers; rb_ptr / pwr_ptr int32
    [n_envs, n_cand, n_links])."""
    global evaluate_launches
    _check_side('evaluate', load_evaluate_library().d2d_evaluate(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_cand, n_dev,
        n_links, n_rbs, sinr_ptr, capacity_ptr, total_ptr, stream_ptr))
    if n_envs:
        evaluate_launches += 1


def evaluate_table(table_ptr: int, table_dtype: int, table_rows: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int,
                   cols_ptr: int, cap_cols_ptr: int, n_envs: int, n_cand: int, n_dev: int, n_links: int, n_rbs: int, sinr_ptr: int,
                   capacity_ptr: int, total_ptr: int, domain_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_evaluate_table: the planes n_cand candidate assignments per env would give on the dB table at table_ptr (EVALTAB_F32 /
    EVALTAB_F64 entries, [n_envs, table_rows, n_links] by (tx link, rx link), table_rows = n_links or n_links + 1) - sinr_db and
    capacity_mbps float32 [n_envs, n_cand, n_links] (either pointer 0: not written), total_mbps float32 and domain int32 [n_envs,
    n_cand] (device pointers; rb_ptr / pwr_ptr int32 [n_envs, n_cand, n_links]; cols_ptr float32 [3, n_dev]: tx_lin, rx_lin,
    noise_mw)."""
    global evaltab_launches
    _check_side('evaltab', load_evaltab_library().d2d_evaluate_table(
        table_ptr, table_dtype, table_rows, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, n_envs, n_cand, n_dev,
        n_links, n_rbs, sinr_ptr, capacity_ptr, total_ptr, domain_ptr, stream_ptr))
    if n_envs:
        evaltab_launches += 1


def table_marginal(table_ptr: int, table_dtype: int, table_rows: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int,
                   cols_ptr: int, cap_cols_ptr: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, harm_ptr: int, diff_ptr: int,
                   domain_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_table_marginal: every link's harm and difference reward (Mbps) on the dB table at table_ptr (TABMARG_F32 / TABMARG_F64
    entries, [n_envs, table_rows, n_links] by (tx link, rx link), table_rows = n_links or n_links + 1) into two float32 planes
    [n_envs, n_links], and domain int32 [n_envs] (device pointers; rb_ptr / pwr_ptr int32 [n_envs, n_links]; cols_ptr float32
    [3, n_dev]: tx_lin, rx_lin, noise_mw)."""
    global tabmarg_launches
    _check_side('tabmarg', load_tabmarg_library().d2d_table_marginal(
        table_ptr, table_dtype, table_rows, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, n_envs, n_dev, n_links,
        n_rbs, harm_ptr, diff_ptr, domain_ptr, stream_ptr))
    if n_envs:
        tabmarg_launches += 1


def table_rb_ascent(table_ptr: int, table_dtype: int, table_rows: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int,
                    cols_ptr: int, cap_cols_ptr: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, allowed_ptr: int, movable_ptr: int,
                    floor_ptr: int, min_gain_mbps: float, max_rounds: int, env_mask_ptr: int, gains_ptr: int, rb_out_ptr: int,
                    sinr_ptr: int, capacity_ptr: int, rounds_ptr: int, moves_ptr: int, converged_ptr: int, domain_ptr: int,
                    stream_ptr: int = 0) -> None:
    """d2d_table_rb_ascent: the sum-capacity RB ascent of every env on the dB table at table_ptr (TABASCENT_F32 / TABASCENT_F64
    entries, [n_envs, table_rows, n_links] by (tx link, rx link), table_rows = n_links or n_links + 1) - rb int32, sinr_db and
    capacity_mbps float32 [n_envs, n_links], rounds and moves int32, converged uint8, domain int32 [n_envs] (device pointers; rb_ptr /
    pwr_ptr int32 [n_envs, n_links]: the start state; cols_ptr float32 [3, n_dev]: tx_lin, rx_lin, noise_mw; gains_ptr: the float32
    work space [n_envs, n_links, n_links]; allowed_ptr 0: every RB, else uint32 [n_links, ceil(n_rbs / 32)]; movable_ptr 0: every link,
    else uint8 [n_links]; floor_ptr 0: no floors, else float32 [n_links], -inf: none for that link; env_mask_ptr 0: every env, else
    uint8 [n_envs] and the envs whose byte is 0 keep their rows)."""
    global tabascent_launches
    _check_side('tabascent', load_tabascent_library().d2d_table_rb_ascent(
        table_ptr, table_dtype, table_rows, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, n_envs, n_dev, n_links,
        n_rbs, allowed_ptr, movable_ptr, floor_ptr, min_gain_mbps, max_rounds, env_mask_ptr, gains_ptr, rb_out_ptr, sinr_ptr,
        capacity_ptr, rounds_ptr, moves_ptr, converged_ptr, domain_ptr, stream_ptr))
    if n_envs:
        tabascent_launches += 1


def assign_weights(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                   cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, movable_links_ptr: int,
                   n_movable: int, allowed_ptr: int, objective: int, weights_ptr: int, harm_ptr: int = 0, stream_ptr: int = 0) -> None:
    """d2d_assign_weights: the matching weights of every movable link on every RB, float32 [n_envs, n_movable, n_rbs], and the
    harm plane of the same shape (harm_ptr 0: not written) - device pointers; movable_links_ptr int32 [n_movable], ascending link
    indices; allowed_ptr 0: every RB, else uint32 [n_links, ceil(n_rbs / 32)]; objective ASSIGN_OBJECTIVE_*."""
    global assign_weights_launches
    _check_side('assign', load_assign_library().d2d_assign_weights(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, movable_links_ptr, n_movable, allowed_ptr, objective, weights_ptr, harm_ptr, stream_ptr))
    if n_envs:
        assign_weights_launches += 1


def assign_solve(weights_ptr: int, n_envs: int, n_rows: int, n_cols: int, col_ptr: int, value_ptr: int, feasible_ptr: int,
                 stream_ptr: int = 0) -> None:
    """d2d_assign_solve: the maximum-weight one-to-one matching of float32 weights [n_envs, n_rows, n_cols] - col int32
    [n_envs, n_rows], value float32 and feasible uint8 [n_envs] (device pointers)."""
    global assign_solve_launches
    _check_side('assign', load_assign_library().d2d_assign_solve(
        weights_ptr, n_envs, n_rows, n_cols, col_ptr, value_ptr, feasible_ptr, stream_ptr))
    if n_envs:
        assign_solve_launches += 1


def assign_power_weights(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                         cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int,
                         movable_links_ptr: int, n_movable: int, allowed_ptr: int, p_min_ptr: int, p_max_ptr: int, floor_ptr: int,
                         weights_ptr: int, power_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_assign_power_weights: every movable link's best admissible power on every RB and its weight there - weights float32 and
    power_dbm int32 [n_envs, n_movable, n_rbs], two planes (device pointers; movable_links_ptr, allowed_ptr as assign_weights()
    takes them; p_min_ptr / p_max_ptr int32 [n_links] on the device; floor_ptr 0: no floors, else float32 [n_links], -inf: none for
    that link)."""
    global assign_power_weights_launches
    _check_side('assignpwr', load_assignpwr_library().d2d_assign_power_weights(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, movable_links_ptr, n_movable, allowed_ptr, p_min_ptr, p_max_ptr, floor_ptr, weights_ptr, power_ptr, stream_ptr))
    if n_envs:
        assign_power_weights_launches += 1


def color_graph(score_ptr: int, tx_bias_ptr: int, rx_thr_ptr: int, rb_ptr: int, n_envs: int, n_links: int, n_rbs: int, allowed_ptr: int,
                movable_ptr: int, pack: bool, rb_out_ptr: int, conflicts_ptr: int, rbs_used_ptr: int, proper_ptr: int,
                stream_ptr: int = 0) -> None:
    """d2d_color_graph: the DSATUR colouring of every env's conflict graph in one launch - rb int32 [n_envs, n_links], conflicts /
    rbs_used int32 and proper uint8 [n_envs] (device pointers; score float32 [n_envs, n_links, n_links], receiver-major; tx_bias_ptr
    0: no bias, else float32 [n_envs, n_links]; rx_thr float32 [n_envs, n_links]; allowed_ptr 0: every RB, else uint32 [n_links,
    ceil(n_rbs / 32)]; movable_ptr 0: every link, else uint8 [n_links])."""
    global color_launches
    _check_side('color', load_color_library().d2d_color_graph(
        score_ptr, tx_bias_ptr, rx_thr_ptr, rb_ptr, n_envs, n_links, n_rbs, allowed_ptr, movable_ptr, 1 if pack else 0, rb_out_ptr,
        conflicts_ptr, rbs_used_ptr, proper_ptr, stream_ptr))
    if n_envs:
        color_launches += 1


def balance_sinr(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int, law: int,
                 pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, base_ptr: int, floor_ptr: int, margins_ptr: int,
                 n_margins: int, p_min_ptr: int, p_max_ptr: int, adjustable_ptr: int, max_iters: int, env_mask_ptr: int, power_ptr: int,
                 sinr_ptr: int, margin_ptr: int, level_ptr: int, probes_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_balance_sinr: the max-min SINR search of every env in one launch - power_dbm int32 and sinr_db float32 [n_envs, n_links],
    margin_db float32, level and probes int32 [n_envs] (device pointers; base float32 [n_links]; floor_ptr 0: no floors, else float32
    [n_links], -inf: none for that link; margins float32 [n_margins], ascending; p_min / p_max int32 [n_links]; adjustable_ptr 0:
    every link, else uint8 [n_links]; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte is 0 keep their
    rows)."""
    global balance_launches
    _check_side('balance', load_balance_library().d2d_balance_sinr(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, law, pow_k, n_envs, n_dev, n_links, n_rbs,
        base_ptr, floor_ptr, margins_ptr, n_margins, p_min_ptr, p_max_ptr, adjustable_ptr, max_iters, env_mask_ptr, power_ptr,
        sinr_ptr, margin_ptr, level_ptr, probes_ptr, stream_ptr))
    if n_envs:
        balance_launches += 1


def stable_match(link_pref_ptr: int, rb_pref_ptr: int, quota_ptr: int, n_envs: int, n_links: int, n_rbs: int, col_ptr: int, load_ptr: int,
                 proposals_ptr: int, unmatched_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_stable_match: the link-optimal stable matching of every env in one launch - col int32 [n_envs, n_links] (-1: unmatched),
    load int32 [n_envs, n_rbs], proposals and unmatched int32 [n_envs] (device pointers; link_pref and rb_pref float32 [n_envs,
    n_links, n_rbs], higher is better, a pair with an entry that is not finite is unacceptable; quota int32 [n_rbs])."""
    global stable_launches
    _check_side('stable', load_stable_library().d2d_stable_match(
        link_pref_ptr, rb_pref_ptr, quota_ptr, n_envs, n_links, n_rbs, col_ptr, load_ptr, proposals_ptr, unmatched_ptr, stream_ptr))
    if n_envs:
        stable_launches += 1


def share_values(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                 cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, movable_links_ptr: int,
                 n_movable: int, allowed_ptr: int, values_ptr: int, closed_rb_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_share_values: the total capacity of every RB under every subset of the movable links - values float64 [n_envs, n_rbs,
    2^n_movable] and closed_rb int32 [n_envs, n_rbs] (device pointers; movable_links_ptr int32 [n_movable], ascending link indices;
    allowed_ptr 0: every RB, else uint32 [n_links, ceil(n_rbs / 32)])."""
    global share_values_launches
    _check_side('share', load_share_library().d2d_share_values(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, movable_links_ptr, n_movable, allowed_ptr, values_ptr, closed_rb_ptr, stream_ptr))
    if n_envs:
        share_values_launches += 1


def share_solve(values_ptr: int, quota_ptr: int, n_envs: int, n_rbs: int, n_movable: int, choice_ptr: int, col_ptr: int, value_ptr: int,
                feasible_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_share_solve: the max-plus subset convolution of float64 values [n_envs, n_rbs, 2^n_movable] over the RBs - col int32
    [n_envs, n_movable], value float64 and feasible int32 [n_envs] (device pointers; quota_ptr 0: no limit, else int32 [n_rbs];
    choice_ptr uint16 [n_envs, n_rbs, 2^n_movable], the kernel's own)."""
    global share_solve_launches
    _check_side('share', load_share_library().d2d_share_solve(
        values_ptr, quota_ptr, n_envs, n_rbs, n_movable, choice_ptr, col_ptr, value_ptr, feasible_ptr, stream_ptr))
    if n_envs:
        share_solve_launches += 1


def power_ascent(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                 cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, p_min_ptr: int, p_max_ptr: int,
                 adjustable_ptr: int, floor_ptr: int, start: int, min_gain_mbps: float, max_rounds: int, env_mask_ptr: int, power_ptr: int,
                 sinr_ptr: int, capacity_ptr: int, rounds_ptr: int, moves_ptr: int, converged_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_power_ascent: the sum-capacity power ascent of every env in one launch - power_dbm int32, sinr_db and capacity_mbps
    float32 [n_envs, n_links], rounds and moves int32, converged uint8 [n_envs] (device pointers; p_min / p_max int32 [n_links];
    adjustable_ptr 0: every link, else uint8 [n_links]; floor_ptr 0: no floors, else float32 [n_links], -inf: none for that link;
    start: ASCENT_START_HELD / _MIN / _MAX; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte is 0 keep their
    rows)."""
    global ascent_launches
    _check_side('ascent', load_ascent_library().d2d_power_ascent(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, p_min_ptr, p_max_ptr, adjustable_ptr, floor_ptr, start, min_gain_mbps, max_rounds, env_mask_ptr, power_ptr, sinr_ptr,
        capacity_ptr, rounds_ptr, moves_ptr, converged_ptr, stream_ptr))
    if n_envs:
        ascent_launches += 1


def rb_ascent(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
              cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, allowed_ptr: int, movable_ptr: int,
              floor_ptr: int, min_gain_mbps: float, max_rounds: int, env_mask_ptr: int, rb_out_ptr: int, sinr_ptr: int, capacity_ptr: int,
              rounds_ptr: int, moves_ptr: int, converged_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_rb_ascent: the sum-capacity RB ascent of every env in one launch - rb int32, sinr_db and capacity_mbps float32
    [n_envs, n_links], rounds and moves int32, converged uint8 [n_envs] (device pointers; allowed_ptr 0: every RB, else uint32
    [n_links, ceil(n_rbs / 32)]; movable_ptr 0: every link, else uint8 [n_links]; floor_ptr 0: no floors, else float32 [n_links],
    -inf: none for that link; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte is 0 keep their rows)."""
    global rbascent_launches
    _check_side('rbascent', load_rbascent_library().d2d_rb_ascent(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, allowed_ptr, movable_ptr, floor_ptr, min_gain_mbps, max_rounds, env_mask_ptr, rb_out_ptr, sinr_ptr, capacity_ptr,
        rounds_ptr, moves_ptr, converged_ptr, stream_ptr))
    if n_envs:
        rbascent_launches += 1


def goodput_ascent(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                   cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, p_min_ptr: int, p_max_ptr: int,
                   weight_ptr: int, demand_ptr: int, bits_per_mbps: float, allowed_ptr: int, movable_ptr: int, floor_ptr: int,
                   move_mask: int, min_gain: int, max_rounds: int, env_mask_ptr: int, rb_out_ptr: int, power_ptr: int, sinr_ptr: int,
                   capacity_ptr: int, served_ptr: int, value_ptr: int, rounds_ptr: int, moves_ptr: int, converged_ptr: int,
                   stream_ptr: int = 0) -> None:
    """d2d_goodput_ascent: the queue-aware goodput ascent of every env in one launch - rb and power_dbm int32, sinr_db and
    capacity_mbps float32, served_bits int32 [n_envs, n_links], value int64, rounds and moves int32, converged uint8 [n_envs]
    (device pointers; p_min / p_max int32 [n_links]; weight_ptr 0: 1, else uint32 [n_envs, n_links] in [0, 2^20]; demand_ptr 0:
    uncapped, else int32 [n_envs, n_links]; allowed_ptr 0: every RB, else uint32 [n_links, ceil(n_rbs / 32)]; movable_ptr 0: every
    link, else uint8 [n_links]; floor_ptr 0: no floors, else float32 [n_links], -inf: none for that link; move_mask: GOODPUT_MOVE_RB |
    GOODPUT_MOVE_POWER; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte is 0 keep their rows)."""
    global goodput_launches
    _check_side('goodput', load_goodput_library().d2d_goodput_ascent(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, p_min_ptr, p_max_ptr, weight_ptr, demand_ptr, bits_per_mbps, allowed_ptr, movable_ptr, floor_ptr, move_mask, min_gain,
        max_rounds, env_mask_ptr, rb_out_ptr, power_ptr, sinr_ptr, capacity_ptr, served_ptr, value_ptr, rounds_ptr, moves_ptr,
        converged_ptr, stream_ptr))
    if n_envs:
        goodput_launches += 1


def deviation_gains(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                    cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, p_min_ptr: int, p_max_ptr: int,
                    links_ptr: int, n_sel: int, n_levels: int, allowed_ptr: int, floor_ptr: int, env_mask_ptr: int, gain_ptr: int,
                    stream_ptr: int = 0) -> None:
    """d2d_deviation_gains: what the total capacity gains when one selected link alone plays (RB, level), every entry of float32
    [n_envs, n_sel, n_rbs, n_levels] in one launch, -inf where the entry is closed (device pointers; p_min / p_max int32 [n_links];
    links int32 [n_sel], ascending and distinct; allowed_ptr 0: every RB, else uint32 [n_links, ceil(n_rbs / 32)]; floor_ptr 0: no
    floors, else float32 [n_links], -inf: none for that link; env_mask_ptr 0: every env, else uint8 [n_envs] and the envs whose byte
    is 0 keep their rows)."""
    global deviate_launches
    _check_side('deviate', load_deviate_library().d2d_deviation_gains(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, p_min_ptr, p_max_ptr, links_ptr, n_sel, n_levels, allowed_ptr, floor_ptr, env_mask_ptr, gain_ptr, stream_ptr))
    if n_envs:
        deviate_launches += 1


def best_deviation(pos_x_ptr: int, pos_y_ptr: int, rb_ptr: int, pwr_ptr: int, link_tx_ptr: int, link_rx_ptr: int, cols_ptr: int,
                   cap_cols_ptr: int, law: int, pow_k: int, n_envs: int, n_dev: int, n_links: int, n_rbs: int, p_min_ptr: int, p_max_ptr: int,
                   links_ptr: int, n_sel: int, n_levels: int, allowed_ptr: int, floor_ptr: int, min_gain_mbps: float, env_mask_ptr: int,
                   rb_out_ptr: int, pwr_out_ptr: int, gain_link_ptr: int, regret_ptr: int, leader_ptr: int, stream_ptr: int = 0) -> None:
    """d2d_best_deviation: every selected link's best unilateral deviation and the env's regret, no table - rb and power_dbm int32,
    gain_mbps float64 [n_envs, n_links], regret_mbps float64 and leader int32 [n_envs] (device pointers; the inputs as
    deviation_gains() takes them)."""
    global deviate_launches
    _check_side('deviate', load_deviate_library().d2d_best_deviation(
        pos_x_ptr, pos_y_ptr, rb_ptr, pwr_ptr, link_tx_ptr, link_rx_ptr, cols_ptr, cap_cols_ptr, law, pow_k, n_envs, n_dev, n_links,
        n_rbs, p_min_ptr, p_max_ptr, links_ptr, n_sel, n_levels, allowed_ptr, floor_ptr, min_gain_mbps, env_mask_ptr, rb_out_ptr,
        pwr_out_ptr, gain_link_ptr, regret_ptr, leader_ptr, stream_ptr))
    if n_envs:
        deviate_launches += 1


def mobility_move(pos_x_ptr: int, pos_y_ptr: int, vel_x_ptr: int, vel_y_ptr: int, fixed_mask_ptr: int, n_envs: int, n_cues: int,
                  n_due_pairs: int, first_env: int, seed: int, memory: float, noise_scale: float, speed_std: float, dt_s: float,
                  cell_radius_m: float, d2d_radius_m: float, step: int = 0, episode: int = 0, elapsed_ptr: int = 0, start_ptr: int = 0,
                  episode_ptr: int = 0, reset_ptr: int = 0, stream_ptr: int = 0) -> None:
    """d2d_mobility_move: one Gauss-Markov move of the position / velocity planes [n_envs, n_dev] in place (device pointers), or the
    start-of-episode velocities (step 0); reset_ptr != 0: the per-env clock of the four [n_envs] arrays."""
    global mobility_launches
    _check_side('mobility', load_mobility_library().d2d_mobility_move(
        pos_x_ptr, pos_y_ptr, vel_x_ptr, vel_y_ptr, fixed_mask_ptr, n_envs, n_cues, n_due_pairs, C.c_uint64(first_env),
        C.c_uint64(seed & (2 ** 64 - 1)), memory, noise_scale, speed_std, dt_s, cell_radius_m, d2d_radius_m, step & 0xFFFFFFFF,
        episode & 0xFFFFFFFF, elapsed_ptr, start_ptr, episode_ptr, reset_ptr, stream_ptr))
    mobility_launches += 1


def channel_fill(pos_x_ptr: int, pos_y_ptr: int, link_tx_ptr: int, link_rx_ptr: int, a_tx_ptr: int, a_rx_ptr: int, exponent_ptr: int,
                 n_envs: int, n_dev: int, n_links: int, first_env: int, num_sinusoids: int, shadow_amp_db: float, wave_scale: float,
                 fading: int, rician_mu: float, rician_s: float, shadow_seed: int, fading_seed: int, scratch_ptr: int, table_ptr: int,
                 table_dtype: int = F64, step: int = 0, episode: int = 0, elapsed_ptr: int = 0, start_ptr: int = 0, episode_ptr: int = 0, reset_ptr: int = 0,
                 stream_ptr: int = 0) -> None:
    """d2d_channel_fill: the spatial channel's live dB table [n_envs, n_links + 1, n_links] of table_dtype (F32 / F64; device pointers) at the clock
    (episode, step); reset_ptr != 0: the per-env clock of the four [n_envs] arrays."""
    global channel_launches
    u64 = 2 ** 64 - 1
    _check_side('channel', load_channel_library().d2d_channel_fill(
        pos_x_ptr, pos_y_ptr, link_tx_ptr, link_rx_ptr, a_tx_ptr, a_rx_ptr, exponent_ptr, n_envs, n_dev, n_links, C.c_uint64(first_env),
        num_sinusoids, shadow_amp_db, wave_scale, fading, rician_mu, rician_s, C.c_uint64(shadow_seed & u64),
        C.c_uint64(fading_seed & u64), step & 0xFFFFFFFF, episode & 0xFFFFFFFF, elapsed_ptr, start_ptr, episode_ptr, reset_ptr,
        scratch_ptr, table_ptr, table_dtype, stream_ptr))
    channel_launches += 1


def queue_step(capacity_ptr: int, ring_ptr: int, arrived_ptr: int, served_ptr: int, expired_ptr: int, overflow_ptr: int, backlog_ptr: int,
               hol_age_ptr: int, mean_delay_ptr: int, on_ptr: int, thresholds: np.ndarray, n_envs: int, n_cues: int, n_due_pairs: int,
               deadline_steps: int, packet_bits: int, buffer_bits: int, bits_per_mbps_step: float, p_on_to_off: int, p_off_to_on: int,
               p_start_on: int, first_env: int, seed: int, step: int = 0, episode: int = 0, elapsed_ptr: int = 0, start_ptr: int = 0,
               episode_ptr: int = 0, reset_ptr: int = 0, stream_ptr: int = 0) -> None:
    """d2d_queue_step: one step of the packet queues behind the capacity plane [n_envs, n_links] (device pointers; `thresholds` is a
    host uint32 [2, 64] array), or the start of an episode (step 0); reset_ptr != 0: the per-env clock of the four [n_envs] arrays."""
    global queue_launches
    lib = load_queue_library()
    tab = np.ascontiguousarray(thresholds, dtype=np.uint32)
    if tab.shape != (2, QUEUE_TABLE):
        raise ValueError(f'thresholds must be uint32 [2, {QUEUE_TABLE}], got {tab.shape}')
    _check_side('queue', lib.d2d_queue_step(
        capacity_ptr, ring_ptr, arrived_ptr, served_ptr, expired_ptr, overflow_ptr, backlog_ptr, hol_age_ptr, mean_delay_ptr, on_ptr,
        tab.ctypes.data, n_envs, n_cues, n_due_pairs, deadline_steps, packet_bits, buffer_bits, bits_per_mbps_step, p_on_to_off,
        p_off_to_on, p_start_on, C.c_uint64(first_env), C.c_uint64(seed & (2 ** 64 - 1)), step & 0xFFFFFFFF, episode & 0xFFFFFFFF,
        elapsed_ptr, start_ptr, episode_ptr, reset_ptr, stream_ptr))
    queue_launches += 1


def _check(rc: int) -> None:
    if rc == ERR_NO_MEMORY:         # std::bad_alloc caught at the C boundary
        raise MemoryError(load_library().d2d_last_error().decode(errors='replace'))
    if rc != OK:
        raise NativeError(rc, load_library().d2d_last_error().decode(errors='replace'))


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(_DP)


class Handle:
    """Thin RAII wrapper over d2d_handle*.  Array arguments are NumPy (host) unless named *_ptr (device)."""

    def __init__(self, *, num_envs: int, num_rbs: int, num_cues: int, num_due_pairs: int, pwr_levels_due: int,
                 pwr_levels_cue: int, pwr_levels_mbs: int, max_links: int = 0, device_ordinal: int = 0,
                 cell_radius_m: float = 500.0, d2d_radius_m: float = 20.0):
        self._lib = load_library()
        self._h = _P()
        cfg = Config(ABI_VERSION, device_ordinal, num_envs, num_rbs, num_cues, num_due_pairs, max_links,
                     pwr_levels_due, pwr_levels_cue, pwr_levels_mbs, cell_radius_m, d2d_radius_m)
        _check(self._lib.d2d_create(C.byref(cfg), C.byref(self._h)))
        self.num_envs = num_envs
        self.num_devices = 1 + num_cues + 2 * num_due_pairs
        self.max_links = max_links or (num_cues + num_due_pairs)
        self.num_links = 0
        self.num_fixed = 0
        self.env_offset = 0

    # -- lifetime
    def close(self) -> None:
        if getattr(self, '_h', None):
            self._lib.d2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int) -> None:
        _check(self._lib.d2d_set_stream(self._h, _P(stream_ptr)))

    def synchronize(self) -> None:
        _check(self._lib.d2d_synchronize(self._h))

    # -- tables
    def set_device_table(self, eirp_off_db, rx_off_db, noise_dbm, sens_dbm, bw_hz) -> None:
        cols = [np.ascontiguousarray(c, dtype=np.float64) for c in (eirp_off_db, rx_off_db, noise_dbm, sens_dbm, bw_hz)]
        _check(self._lib.d2d_set_device_table(self._h, len(cols[0]), *[_dptr(c) for c in cols]))

    def set_path_loss_power_law(self, a_tx_db, a_rx_db, exponent) -> None:
        cols = [np.ascontiguousarray(c, dtype=np.float64) for c in (a_tx_db, a_rx_db, exponent)]
        _check(self._lib.d2d_set_path_loss_power_law(self._h, len(cols[0]), *[_dptr(c) for c in cols]))

    def set_path_loss_shadowing(self, a_tx_db, a_rx_db, exponent, d0_m: float, chi_db: float, seed: int) -> None:
        cols = [np.ascontiguousarray(c, dtype=np.float64) for c in (a_tx_db, a_rx_db, exponent)]
        _check(self._lib.d2d_set_path_loss_shadowing(self._h, len(cols[0]), *[_dptr(c) for c in cols],
                                                     float(d0_m), float(chi_db), C.c_uint64(seed)))

    def set_path_loss_table(self, pl_db: np.ndarray) -> None:
        t = np.ascontiguousarray(pl_db, dtype=np.float64)        # dB as the plugin returned them; rounded once, as linear gains
        d = self.num_devices
        if t.shape not in ((d, d), (self.num_envs, d, d)):
            raise ValueError(f'path-loss table must be [{d},{d}] or [{self.num_envs},{d},{d}], got {t.shape}')
        _check(self._lib.d2d_set_path_loss_table(self._h, _dptr(t), int(t.ndim == 3)))

    def set_path_loss_link_table(self, pl_db: np.ndarray) -> None:
        """pl_db[(e,) j, i] = PathLoss(tx of link j, rx of link i) of the CURRENT link list, float64 dB: [N,N] or [B,N,N]."""
        t = np.ascontiguousarray(pl_db, dtype=np.float64)
        n = t.shape[-1]
        if t.shape not in ((n, n), (self.num_envs, n, n)):
            raise ValueError(f'link path-loss table must be [N,N] or [{self.num_envs},N,N], got {t.shape}')
        _check(self._lib.d2d_set_path_loss_link_table(self._h, _dptr(t), n, int(t.ndim == 3)))

    def set_path_loss_link_table_dev(self, dev_ptr: int, dtype: int, n_links: int, per_env) -> None:
        """The link table from DEVICE memory (float32 / float64 dB, [N,N] or [B,N,N]): converted to gains by a kernel, no host copy.
        per_env = PL_TABLE_LIVE binds a [B,N+1,N] table instead, read in place by every later step."""
        _check(self._lib.d2d_set_path_loss_link_table_dev(self._h, _P(dev_ptr), dtype, n_links, int(per_env)))

    def set_links(self, tx_dev, rx_dev, link_type) -> None:
        a = [np.ascontiguousarray(c, dtype=np.int32) for c in (tx_dev, rx_dev, link_type)]
        n = len(a[0])
        _check(self._lib.d2d_set_links(self._h, n, *[c.ctypes.data_as(_IP) for c in a]))
        self.num_links = n
        self.num_fixed = 0

    def set_fixed_actions(self, link_idx, rb, pwr_dbm) -> None:
        """Links driven by the traffic model: d2d_step then takes actions for the other links only."""
        a = [np.ascontiguousarray(c, dtype=np.int32) for c in (link_idx, rb, pwr_dbm)]
        n = len(a[0])
        if len(a[1]) != n or len(a[2]) != n:
            raise ValueError('link_idx, rb and pwr_dbm must have the same length')
        _check(self._lib.d2d_set_fixed_actions(self._h, n, *[c.ctypes.data_as(_IP) for c in a]))
        self.num_fixed = n

    def positions_changed(self) -> None:
        _check(self._lib.d2d_positions_changed(self._h))

    def set_reward(self, reward_fn: int, param: float = 0.0) -> None:
        _check(self._lib.d2d_set_reward(self._h, reward_fn, param))

    def set_obs_mode(self, mode: int) -> None:
        _check(self._lib.d2d_set_obs_mode(self._h, mode))

    def set_obs_dtype(self, dtype: int) -> None:
        """F64: D2D_BUF_OBS is float64 [B,N,6N], widened by the expansion kernel itself (the reference's dtype, obs_fn.py:51)."""
        _check(self._lib.d2d_set_obs_dtype(self._h, dtype))
        self.obs_f64 = dtype == F64

    def set_reward_layout(self, layout: int) -> None:
        """REWARD_PER_ENV: SystemCapacity's scalar once per env (BUF_REWARD_ENV [B]) instead of N copies (BUF_REWARD [B,N])."""
        _check(self._lib.d2d_set_reward_layout(self._h, layout))

    def set_bucketing(self, enabled: bool) -> None:
        _check(self._lib.d2d_set_bucketing(self._h, int(enabled)))

    def set_export_actions(self, enabled: bool) -> None:
        _check(self._lib.d2d_set_export_actions(self._h, int(enabled)))

    def set_tuning(self, key: int, value: int) -> None:
        _check(self._lib.d2d_set_tuning(self._h, key, value))

    # -- buffers
    def buffer_shape(self, which: int):
        b, n, d = self.num_envs, self.num_links, self.num_devices
        if which in (BUF_POS_X, BUF_POS_Y):
            return (b, d)
        if which == BUF_OBS_TABLE:
            return (b, n, 6)
        if which == BUF_OBS:
            return (b, n, 6 * n)
        if which in (BUF_ENV_FLAGS, BUF_REWARD_ENV, BUF_RESET_PENDING, BUF_EPISODE):
            return (b,)
        if which == BUF_LINK_POS:
            return (b, n, 4)
        if which == BUF_ACTIONS:
            return (b, n - self.num_fixed)
        return (b, n)

    def get_buffer(self, which: int):
        ptr, size = _P(), C.c_size_t()
        _check(self._lib.d2d_get_buffer(self._h, which, C.byref(ptr), C.byref(size)))
        return ptr.value, size.value

    def bind_buffer(self, which: int, dev_ptr: int, nbytes: int) -> None:
        _check(self._lib.d2d_bind_buffer(self._h, which, _P(dev_ptr), nbytes))

    def upload(self, which: int, array: np.ndarray, offset_bytes: int = 0) -> None:
        a = np.ascontiguousarray(array, dtype=BUFFER_DTYPES.get(which, np.float32))
        _check(self._lib.d2d_upload(self._h, which, a.ctypes.data_as(_P), a.nbytes, offset_bytes))

    def download(self, which: int, env_begin: int = 0, env_count: Optional[int] = None) -> np.ndarray:
        shape = self.buffer_shape(which)
        env_count = self.num_envs - env_begin if env_count is None else env_count
        dtype = np.float64 if which == BUF_OBS and getattr(self, 'obs_f64', False) else BUFFER_DTYPES.get(which, np.float32)
        out = np.empty((env_count,) + shape[1:], dtype=dtype)
        per_env = out.nbytes // max(env_count, 1)
        if out.nbytes:
            _check(self._lib.d2d_download(self._h, which, out.ctypes.data_as(_P), out.nbytes, env_begin * per_env))
        return out

    def set_positions(self, x: np.ndarray, y: np.ndarray, env_begin: int = 0) -> None:
        """x, y [envs, D].  float64 arrays go through d2d_set_positions_f64 - the reference's own precision (position.py:7-12), kept
        as (hi, lo) float32 pairs on the device; anything else is uploaded as float32."""
        exact = getattr(x, 'dtype', None) == np.float64 and getattr(y, 'dtype', None) == np.float64
        dtype = np.float64 if exact else np.float32
        x = np.ascontiguousarray(x, dtype=dtype); y = np.ascontiguousarray(y, dtype=dtype)
        if x.shape != y.shape or x.ndim != 2 or x.shape[1] != self.num_devices:
            raise ValueError(f'positions must be [envs, {self.num_devices}]')
        if exact:
            _check(self._lib.d2d_set_positions_f64(self._h, _dptr(x), _dptr(y), env_begin, x.shape[0]))
        else:
            _check(self._lib.d2d_set_positions(self._h, x.ctypes.data_as(_FP), y.ctypes.data_as(_FP), env_begin, x.shape[0]))

    def reset_positions(self, seed: int, episode: int = 0, fixed_mask=None, fixed_xy=None) -> None:
        """episode = EPISODE_PER_ENV: only the envs BUF_RESET_PENDING marks, each at its BUF_EPISODE entry (asynchronous)."""
        m = xy = None
        if fixed_mask is not None:
            m = np.ascontiguousarray(fixed_mask, dtype=np.uint8)
            xy = np.ascontiguousarray(fixed_xy, dtype=np.float32)
            if m.shape != (self.num_devices,) or xy.shape != (self.num_devices, 2):
                raise ValueError('fixed_mask [D] / fixed_xy [D,2] expected')
        _check(self._lib.d2d_reset_positions(
            self._h, C.c_uint64(seed), C.c_uint64(episode),
            m.ctypes.data_as(C.POINTER(C.c_uint8)) if m is not None else None,
            xy.ctypes.data_as(_FP) if xy is not None else None))

    def set_env_offset(self, first_env: int) -> None:
        _check(self._lib.d2d_set_env_offset(self._h, C.c_uint64(first_env)))
        self.env_offset = int(first_env)

    # -- hot path
    def step(self, actions_ptr: int = 0) -> None:
        _check(self._lib.d2d_step(self._h, _P(actions_ptr or None)))

    def step_rb_pwr(self, rb_ptr: int = 0, pwr_ptr: int = 0) -> None:
        _check(self._lib.d2d_step_rb_pwr(self._h, _P(rb_ptr or None), _P(pwr_ptr or None)))

    def expand_table(self, table_ptr: int, n_envs: int, n_links: int, obs_ptr: int) -> None:
        _check(self._lib.d2d_expand_table(self._h, _P(table_ptr), n_envs, n_links, _P(obs_ptr)))

    def step_host(self, rb: np.ndarray, pwr: np.ndarray) -> dict:
        """One step with host (rb, pwr) [B,N] in and every result back in one pinned block.  The returned arrays are
        VIEWS into library-owned pinned memory, valid until the next step_host on this handle."""
        b, n = self.num_envs, self.num_links
        r = np.ascontiguousarray(rb, dtype=np.int32); p = np.ascontiguousarray(pwr, dtype=np.int32)
        if r.shape != (b, n) or p.shape != (b, n):
            raise ValueError(f'rb/pwr must be [{b},{n}]')
        out, lay = _P(), HostLayout()
        _check(self._lib.d2d_step_host(self._h, r.ctypes.data_as(_IP), p.ctypes.data_as(_IP), C.byref(out), C.byref(lay)))
        key = (out.value, lay.total_bytes, lay.obs, b, n)
        cached = getattr(self, '_host_views', None)
        if cached is not None and cached[0] == key:           # same pinned block, same layout: the views still hold
            return cached[1]
        raw = (C.c_char * lay.total_bytes).from_address(out.value)

        def view(off, dtype, shape):
            count = 1
            for d in shape:
                count *= d
            return np.frombuffer(raw, dtype=dtype, count=count, offset=off).reshape(shape)
        res = {name: view(getattr(lay, name), np.float32, (b, n))
               for name in ('sinr_db', 'snr_db', 'rate_bps', 'capacity', 'reward')}
        res['rb'] = view(lay.rb, np.int32, (b, n)); res['pwr'] = view(lay.pwr, np.int32, (b, n))
        res['obs_table'] = view(lay.obs_table, np.float32, (b, n, 6))
        res['env_flags'] = view(lay.env_flags, np.int32, (b,))
        if lay.total_bytes > lay.obs:
            res['obs'] = view(lay.obs, np.float32, (b, n, 6 * n))
        self._host_views = (key, res)
        return res

    # -- multi-GPU (RCCL behind the C ABI)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        _check(load_library().d2d_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, world_size: int, rank: int, unique_id: bytes) -> None:
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError(f'unique_id must be {UNIQUE_ID_BYTES} bytes')
        _check(self._lib.d2d_comm_init(self._h, world_size, rank, C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)))

    def comm_destroy(self) -> None:
        _check(self._lib.d2d_comm_destroy(self._h))

    def allgather(self, send_ptr: int, recv_ptr: int, bytes_per_rank: int, stream_ptr: int = 0) -> None:
        _check(self._lib.d2d_allgather(self._h, _P(send_ptr), _P(recv_ptr), bytes_per_rank, _P(stream_ptr or None)))

    def status_flags(self) -> int:
        f = C.c_uint32()
        _check(self._lib.d2d_status_flags(self._h, C.byref(f)))
        return f.value

    # -- measurement
    def profile_enable(self, on: bool) -> None:
        _check(self._lib.d2d_profile_enable(self._h, int(on)))

    def profile_read(self, kernel: int):
        ms, n = C.c_double(), C.c_int64()
        _check(self._lib.d2d_profile_read(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_median(self, kernel: int) -> float:
        """Median launch duration (ms) of kernel 0 (step) / 1 (LinearObs expansion) since the last profile_reset()."""
        ms = C.c_double()
        _check(self._lib.d2d_profile_median(self._h, kernel, C.byref(ms)))
        return ms.value

    def profile_reset(self) -> None:
        _check(self._lib.d2d_profile_reset(self._h))

