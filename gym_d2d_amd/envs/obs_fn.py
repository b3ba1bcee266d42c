"""Observation plugins (mirrors gym_d2d/envs/obs_fn.py).

Two levels:
  * `ObsFunction` - the reference's ABC, dict-in / dict-out, for single-env drop-in use.  Built-ins are executed
    by the HIP obs kernel; their get_state() only re-keys the kernel's output.  A user subclass that overrides
    get_state() runs as ordinary Python on dict views of the GPU results.
  * `ArrayObsFunction` - array-native variant for the batched env: receives the step's arrays (device tensors when
    torch is available) and returns an array; `native_mode` tells the kernel what to materialise for it.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Dict

import numpy as np

from .. import _native
from ..spaces import Box, Space


class ObsFunction(ABC):
    native_mode = _native.OBS_TABLE     # what a Python-side get_state needs from the GPU: the base table

    @abstractmethod
    def get_obs_space(self, env_config) -> Space:
        """Observation space of one agent."""

    @abstractmethod
    def get_state(self, actions, state: dict, devices) -> Dict[str, np.ndarray]:
        """Observations per 'tx:rx' agent id for the step described by `actions` / `state`."""


class LinearObsFunction(ObsFunction):
    """Every agent sees the whole network: its own (tx_x, tx_y, rx_x, rx_y, sinr_dB, snr_dB) first, then every other
    link's six values in agent order (obs_fn.py:43-61).  Materialised by csrc/d2d_obs.hip."""
    native_mode = _native.OBS_LINEAR
    FEATURES = 6

    def get_obs_space(self, env_config) -> Space:
        r = env_config.cell_radius_m
        width = self.FEATURES * (env_config.num_cues + env_config.num_due_pairs)
        return Box(low=-r, high=r, shape=(width,))

    def get_state(self, actions, state, devices) -> Dict[str, np.ndarray]:
        obs = getattr(state, 'linear_obs', None)
        if obs is None:
            raise RuntimeError('LinearObsFunction is evaluated by the HIP obs kernel; `state` must be the NativeState '
                               'returned by gym_d2d_amd.Simulator.step (there is no host implementation)')
        return dict(zip(map(':'.join, getattr(actions, 'data', actions).keys()), obs))     # rows of the [N, 6N] block


class ArrayObsFunction(ABC):
    """Batched plugin: compute(view) -> [B, N, width] array/tensor.  `view` has pos_x/pos_y [B,D], rb, pwr, sinr_db,
    snr_db, rate_bps, capacity_mbps [B,N], table [B,N,6], link_tx/link_rx/link_type [N].  A subclass that sets
    `needs_rb_sensing = True` also gets rb_sinr_db [B,N,R]: VecD2DEnv runs the sensing kernel (VecD2DEnv.sense) after every step
    for it; without the attribute nothing is launched or allocated.  A subclass that sets `needs_neighbors = k` (1 .. min(N - 1, 64))
    also gets neighbor_idx int32 [B,N,k] and neighbor_coupling_db float32 [B,N,k], every link's k strongest interferers
    (VecD2DEnv.neighbors: receiver-major, row [b, i] belongs to the RECEIVING link i, strongest first): selected at reset() and for
    the envs an autoreset step reset, never per step; without the attribute nothing is built, allocated or launched.  A subclass that
    sets `needs_best_rb = True` also gets best_rb int32, best_sinr_db and gain_db float32 [B,N] (VecD2DEnv.best_rb: one launch of
    csrc/d2d_bestrb.hip behind every step and reset); without the attribute nothing is loaded, allocated or launched.  A subclass
    that sets `needs_table_marginal = True` also gets difference_mbps and harm_mbps float32 [B,N] on the path-loss table the step
    just read (VecD2DEnv.marginal_capacity_table: one launch of csrc/d2d_tabmarg.hip behind every step and reset; table routes
    only, refused at construction elsewhere)."""
    native_mode = _native.OBS_TABLE
    needs_rb_sensing = False
    needs_neighbors = 0
    needs_best_rb = False

    @abstractmethod
    def get_obs_space(self, env_config) -> Space:
        pass

    @abstractmethod
    def compute(self, view):
        pass


class OwnLinkObsFunction(ArrayObsFunction):
    """Example custom plugin (BASELINE.json config 4): each agent observes only its own six values."""

    def get_obs_space(self, env_config) -> Space:
        r = env_config.cell_radius_m
        return Box(low=-r, high=r, shape=(6,))

    def compute(self, view):
        return view.table


class SignalPlanesObsFunction(ArrayObsFunction):
    """No observation array is materialised at all (D2D_OBS_NONE: the step writes neither the [B,N,6N] block nor the
    compact [B,N,6] table): a learner that builds its own features reads the step's (sinr_dB, snr_dB) planes - the only
    columns of the table that change within an episode (obs_fn.py:57-60) - and takes the four position columns once per
    reset from `VecD2DEnv.link_positions()` ([B,N,4], simulator.py:61-75 only moves devices in reset()).  compute()
    returns the pair of planes; `distributed.StepGatherer(mode='planes')` ships exactly these across GPUs."""
    native_mode = _native.OBS_NONE

    def get_obs_space(self, env_config) -> Space:
        return Box(low=-np.inf, high=np.inf, shape=(2,))

    def compute(self, view):
        return view.sinr_db, view.snr_db


class RbSensingObsFunction(ArrayObsFunction):
    """Each agent observes the SINR (dB) it would get on every resource block at its current power, everything else as the last
    step left it: [B, N, R] = VecD2DEnv.sense('sinr_db'), evaluated by csrc/d2d_sense.hip after every step.  Column rb[b, i] is the
    step's own sinr_db; an RB nobody else uses shows the link's SNR.  Width R instead of LinearObs's 6N.  The tensor is the env's
    own sensing block, rewritten by every step (clone it to keep a step's values)."""
    native_mode = _native.OBS_NONE
    needs_rb_sensing = True

    def get_obs_space(self, env_config) -> Space:
        return Box(low=-np.inf, high=np.inf, shape=(env_config.num_rbs,))

    def compute(self, view):
        return view.rb_sinr_db


class BestRbObsFunction(ArrayObsFunction):
    """Each agent observes where it would be best off and by how much, width 3: [B, N, 3] float32 = (best_rb, best_sinr_dB, gain_dB) of
    VecD2DEnv.best_rb(), evaluated by csrc/d2d_bestrb.hip behind every step - the RB on which the link would see the highest SINR if it
    alone moved there, that SINR, and what the move would gain over its own RB (0.0: it already sits there).  Width 3 instead of
    RbSensingObsFunction's R, and no [B, N, R] block behind it.  A fresh tensor per call."""
    native_mode = _native.OBS_NONE
    needs_best_rb = True

    def get_obs_space(self, env_config) -> Space:
        return Box(low=-np.inf, high=np.inf, shape=(3,))

    def compute(self, view):
        import torch
        return torch.stack([view.best_rb.to(torch.float32), view.best_sinr_db, view.gain_db], dim=-1)


class NeighborObsFunction(ArrayObsFunction):
    """Each agent observes its own link and its k strongest interferers - the interference graph, width 4 (k + 1) whatever N is:
    [B, N, 4 (k + 1)] float32 = own (rb, pwr_dBm, sinr_dB, snr_dB), then for each neighbour in rank order (coupling_dB, rb_j, pwr_dBm_j,
    sinr_dB_j).  The neighbours of link i are the k links j != i whose transmitters couple most strongly into link i's RECEIVER
    (VecD2DEnv.neighbors(k): receiver-major [b, i, m]; the path-loss tables elsewhere are [b, j, i]), strongest first, ties in
    ascending j.  The lists depend on positions only: the env selects them at reset() and, under autoreset=True, for the envs a step
    reset; every step is one gather kernel (csrc/d2d_graph.hip).  A subclass sets another `k` (1 .. min(N - 1, 64)).  The tensor is
    the env's own block, rewritten by every step (clone it to keep a step's values)."""
    native_mode = _native.OBS_NONE
    native_neighbor_obs = True          # the env runs d2d_graph_neighbor_obs and hands the block over as view.neighbor_obs
    k = 8

    @property
    def needs_neighbors(self) -> int:
        return self.k

    def get_obs_space(self, env_config) -> Space:
        return Box(low=-np.inf, high=np.inf, shape=(4 * (self.k + 1),))

    def compute(self, view):
        return view.neighbor_obs


class QueueObsFunction(ArrayObsFunction):
    """Each agent observes its own link and its own packet queue (VecD2DEnv(traffic=PacketTraffic(...)), csrc/d2d_queue.hip), width 6:
    [B, N, 6] float32 = (sinr_dB, snr_dB, capacity_mbps, backlog_bits / buffer_bits, hol_age_steps / deadline_steps, on).  The two
    ratios are formed in float64 and rounded once.  `needs_traffic` makes an env without traffic= refuse it at construction."""
    native_mode = _native.OBS_NONE
    needs_traffic = True

    def get_obs_space(self, env_config) -> Space:
        return Box(low=-np.inf, high=np.inf, shape=(6,))

    def compute(self, view):
        m = view.traffic
        import torch
        f32 = torch.float32
        fill = (view.backlog_bits.to(torch.float64) / float(max(m.buffer_bits, 1))).to(f32)
        age = (view.hol_age_steps.to(torch.float64) / float(m.deadline_steps)).to(f32)
        return torch.stack([view.sinr_db, view.snr_db, view.capacity_mbps, fill, age, view.on.to(f32)], dim=-1)
