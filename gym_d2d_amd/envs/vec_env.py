"""VecD2DEnv - the batched, array-native face of D2DEnv: B independent environments stepped by one kernel launch.

The reference has no batched API (dicts of ~2M Python objects per step are not viable); this class keeps D2DEnv's
semantics per env (reset = new positions + one step with random CUE/DUE actions, 10-step episodes, same decode,
same reward / obs definitions) but speaks arrays:

    env = VecD2DEnv({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, num_envs=4096)
    obs = env.reset(seed=1234)                        # [B, N, 6N] float32 (LinearObsFunction)
    obs, rewards, dones, info = env.step(actions)     # actions int32 [B, N]; rewards [B, N]; dones [B] bool

    env = VecD2DEnv(config, num_envs=4096, autoreset=True)  # done envs start their next episode inside step(), on the GPU
    obs = env.reset(seed=1234, elapsed=np.arange(4096) % 10)  # staggered: env b's first episode is 10 - elapsed[b] steps

With PyTorch-ROCm present all arrays are CUDA tensors that alias the library's HBM buffers (zero copy: the tensors are
allocated by torch and bound into the handle, kernels run on torch's current stream).  Without torch they are NumPy
copies.  Agent order along N: all CUE uplinks, then all DUE sidelinks (d2d_env.py:54-60).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np

from .. import _native, assignment, balance, best_response, best_response_dynamics, coloring, deviation, goodput_ascent, graph, joint_assignment, marginal, power_ascent, power_control, rb_ascent, sensing, sharing, stable_matching
from .. import evaluate as evaluate_mod
from .. import mobility as mobility_mod
from .. import queues as queues_mod
from .. import table_evaluate as table_evaluate_mod
from .. import table_marginal as table_marginal_mod
from .. import table_rb_ascent as table_rb_ascent_mod
from ..path_loss_table import CHANNEL, PER_STEP, positions_move_unserved
from ..simulator import BASE_STATION_ID, Simulator
from ..traffic_model import DownlinkTrafficModel
from . import _rng
from .d2d_env import EPISODE_LENGTH
from .obs_fn import ArrayObsFunction, LinearObsFunction, ObsFunction
from .reward_fn import SystemCapacityRewardFunction

try:
    import torch
except Exception:       # pragma: no cover
    torch = None

_OUTPUTS = (('sinr_db', _native.BUF_SINR_DB), ('snr_db', _native.BUF_SNR_DB), ('rate_bps', _native.BUF_RATE_BPS),
            ('capacity_mbps', _native.BUF_CAPACITY), ('reward', _native.BUF_REWARD))


class VecD2DEnv:
    def __init__(self, env_config: Optional[dict] = None, num_envs: Optional[int] = None, *,
                 cue_actions: str = 'agent', use_torch: Optional[bool] = None, first_env: int = 0,
                 export_actions: bool = True, reward_per_env: bool = False, placement_trials: int = 0,
                 placement_budget_bytes: int = 1 << 30, autoreset: bool = False, mobility=None,
                 neighbor_refresh: int = 1, traffic=None) -> None:
        """cue_actions: 'agent' - step() takes actions for CUEs and DUEs [B, C+P] (reference behaviour);
        'traffic' - CUE links follow the env's traffic model (round-robin RB at max power,
        traffic_model.py:15-22): their (rb, pwr) are constants of the kernel's link records
        (d2d_set_fixed_actions) and step() takes DUE actions only [B, P] - the CUE half of the action
        traffic does not exist.
        first_env: global index of env 0 when one logical batch is sharded over several GPUs (positions AND the
        random actions of reset() are keyed by global env index, so a sharded run reproduces the single-GPU run).

        export_actions: False - the kernel does not write the decoded (rb, tx power) planes behind info['rb'] /
        info['tx_pwr_dbm'] (d2d_set_export_actions: 8 of the step's 72 bytes per link; a rollout knows its own actions);
        the two info entries are then None.

        reward_per_env: True - SystemCapacityRewardFunction's reward is ONE scalar per env handed to every agent
        (reward_fn.py:42-44); step() then returns it as [B] instead of N copies [B, N] (d2d_set_reward_layout: 4 bytes per
        link and step less).  Only with the native SystemCapacity reward.

        placement_trials (default 0 = off; opt-in): where the step's dominant output block sits physically decides how fast the
        kernel streams it - the same 61 MB obs block of BASELINE config 2 runs 13.2, 13.9 or 15.1 us per step depending on the
        allocation it landed in, reproducibly per allocation (profiles/r4_obs_block_placement_candidates.jsonl; TLB and
        L2-channel counters are equal, so it is how the block's pages spread over the memory channels).  K > 1: the first
        reset() times a few hundred steps on up to K candidate blocks for the fused LinearObs step's obs block (or the table of a
        compact-obs env), allocated one by one behind paddings of 2 - 22 MB, and keeps the fastest; it stops early once a
        candidate is 7 % faster than the slowest seen.  Bounded and private: candidates + paddings never exceed
        placement_budget_bytes (default 1 GiB) at once, each comes from a torch MemPool of its own that is dropped with the
        loser (nothing is released from - or left in - the caller's caching allocator: no torch.cuda.empty_cache()), and the
        obs tensor step() returns MOVES once, at that first reset (a tensor taken from an earlier reset() of the same env does
        not exist - the trials run inside the first).  A lottery with better odds, not a cure: off unless asked for.

        step()'s `dones` on the torch path is one of two preallocated CONSTANT tensors (all False / all True), shared by
        every call: treat it as read-only (clone it before an in-place update).

        autoreset: True - next-step autoreset (gymnasium's NEXT_STEP): the step() after the one that returned dones[b] = True
        ignores env b's action row and resets env b on the device instead - new positions at its own episode index, the reset's
        uniformly random actions, one step with them - and returns that step's obs and planes, reward 0, done False and
        info['reset'][b] = True.  From each env's side the sequence is the reference loop `obs = reset() if done else step(a)`;
        episode k of env b draws what the k-th reset() of a lockstep env draws (same seed, same global env index).  Nothing is
        synchronised: `dones` and info['reset'] are bool [B] device tensors the library writes every step - the SAME two tensor
        objects on every call, like the other aliased outputs (clone them to keep a step's values).  reset(elapsed=...) staggers
        the first episodes; request_reset(mask) resets chosen envs at the next step.  Needs the torch path and a path-loss model
        the kernels evaluate per step (the native laws, ShadowingPathLoss, SpatialChannelPathLoss, a per-step ArrayPathLoss): a table evaluated once per
        reset, or pinned device_config coordinates float32 cannot hold, would need the host between steps (ValueError).

        mobility: a gym_d2d_amd.mobility.GaussMarkovMobility - devices move before every step (csrc/d2d_mobility.hip, one launch):
        reset() draws start-of-episode velocities behind the sampler (its positions, obs and planes are those of a mobility-less env
        with the same seed, bit for bit), step() moves every device, tells the handle (d2d_positions_changed) and then steps, so the
        step, the obs table's columns 0 - 3, link_positions(), sense(), coupling() and marginal_capacity() all see the new positions.
        Under autoreset=True an env that is reset inside a step is not moved in that step and gets its new episode's velocities.  The
        draws are keyed by (global env index, episode, step in the episode, device, axis): sharding and autoreset reproduce the
        lockstep single-GPU trajectories.  velocities() returns the planes; the view carries them as vel_x / vel_y.  None (default):
        nothing is loaded, allocated or launched.  Needs the torch path and what autoreset needs of the path-loss model (ValueError).
        neighbor_refresh: with mobility, an obs function's neighbour lists (needs_neighbors) are selected again after the move of
        every neighbor_refresh-th step() call since reset() (default 1: every step; between refreshes the lists are the last
        refresh's, and under autoreset the envs a step reset still get theirs at once).
        One d2d_graph_neighbors launch per refresh - profiles/mobility_cost.jsonl has its cost.

        traffic: a gym_d2d_amd.queues.PacketTraffic - finite-buffer packet traffic with deadlines behind every link
        (csrc/d2d_queue.hip, one launch per step, right after the step kernel): an on/off source with Poisson arrivals, tail drop, a
        deadline of D steps and oldest-first service by what this step's capacity_mbps carries in dt_s.  reset() starts the episode
        behind the reset's own step (cleared rings, zero planes; that step serves nothing), step() queues behind d2d_step; under
        autoreset=True an env that is reset inside a step shows zero planes and a cleared ring in that step.  The draws are keyed by
        (global env index, episode, step in the episode, link): sharding and autoreset reproduce the lockstep single-GPU run bit for
        bit.  queues() returns the planes; the view carries them (view.backlog_bits, ...) and the model (view.traffic), and info
        gains served_bits, backlog_bits, expired_bits and overflow_bits.  A link whose buffer is empty still transmits: the step
        kernel has no off state.  None (default): nothing is loaded, allocated or launched.  Needs the torch path (ValueError); any
        path-loss route serves it, since it only reads capacity_mbps.

        env_config['obs_dtype'] = 'float64' returns observations in the reference's dtype (obs_fn.py:51 builds float64
        arrays); the default float32 is the kernels' own block, zero copy.

        reset() checks the status flags once and raises ValueError('math domain error') if two interacting devices
        coincide (what the reference's log10(0) does, path_loss.py:66) or a per-step ArrayPathLoss returned NaN / -inf dB for a
        pair the step used; step() does not synchronise - poll status_flags() for FLAG_ZERO_DISTANCE / FLAG_NON_FINITE /
        FLAG_PATH_LOSS_DOMAIN if positions are written from outside."""
        env_config = dict(env_config or {})
        self.export_actions = bool(export_actions)
        obs_cls = env_config.pop('obs_fn', LinearObsFunction)
        rew_cls = env_config.pop('reward_fn', SystemCapacityRewardFunction)
        if num_envs is not None:
            env_config['num_envs'] = num_envs
        self.obs_fn = obs_cls()
        self.reward_fn = rew_cls()
        if isinstance(self.obs_fn, ObsFunction) and type(self.obs_fn).get_state is not LinearObsFunction.get_state:
            raise TypeError('dict-style ObsFunction subclasses work with D2DEnv; VecD2DEnv takes LinearObsFunction or '
                            'an ArrayObsFunction')
        rid = getattr(self.reward_fn, 'native_id', _native.REWARD_NONE)
        if rid == _native.REWARD_NONE and not hasattr(self.reward_fn, 'compute'):
            raise TypeError('VecD2DEnv takes a built-in reward function or an object with compute(view) -> [B,N]')

        n_links = int(env_config.get('num_cues', 25)) + int(env_config.get('num_due_pairs', 25))
        self.simulator = Simulator(env_config, max_links=n_links)     # link set is fixed: no spare capacity needed
        sim, cfg = self.simulator, self.simulator.config
        self.num_envs = sim.num_envs
        self.config = cfg
        self.observation_space = self.obs_fn.get_obs_space(cfg)
        self.num_pwr_actions = cfg.num_pwr_actions
        # CUE links: uplinks cueXX -> mbs (what reset() builds, d2d_env.py:54-60), unless the CUEs are driven by a
        # DownlinkTrafficModel, whose links are mbs -> cueXX (traffic_model.py:25-32)
        self._cue_kind = 'cue'
        if cue_actions == 'traffic' and isinstance(sim.traffic_model, DownlinkTrafficModel):
            self._cue_kind = 'mbs'
            sim.set_links([(BASE_STATION_ID, c) for c in sim.devices.cues.keys()] + list(sim.devices.dues.keys()))
        else:
            sim.set_links(sim.default_link_keys())
        self.num_cues, self.num_due_pairs = cfg.num_cues, cfg.num_due_pairs
        self.num_links = self.num_cues + self.num_due_pairs
        if cue_actions not in ('agent', 'traffic'):
            raise ValueError("cue_actions must be 'agent' or 'traffic'")
        self.cue_actions = cue_actions
        self.num_agents = self.num_links if cue_actions == 'agent' else self.num_due_pairs

        h = sim.handle
        self.first_env = int(first_env)
        if cue_actions == 'traffic' and self.num_cues:
            # (rb, pwr) exactly as TrafficModel.get_traffic would hand them to the simulator: no a // P encode /
            # decode round trip, so a device_config_file max_tx_power_dBm above the action alphabet stays legal
            rb, pwr = sim.traffic_model.assignments(sim.devices)
            h.set_fixed_actions(np.arange(self.num_cues), rb, pwr)
        h.set_env_offset(first_env)
        h.set_export_actions(self.export_actions)
        self._obs64 = cfg.obs_dtype == 'float64'
        h.set_obs_mode(self.obs_fn.native_mode)
        # float64 observations of the native LinearObs: the expansion kernel writes them as float64 itself (no cast pass)
        self._native_obs64 = self._obs64 and self.obs_fn.native_mode == _native.OBS_LINEAR and not isinstance(self.obs_fn, ArrayObsFunction)
        if self._native_obs64:
            h.set_obs_dtype(_native.F64)
        h.set_reward(rid, float(getattr(self.reward_fn, 'native_param', 0.0)))
        self._native_reward = bool(rid)
        self.reward_per_env = bool(reward_per_env)
        if self.reward_per_env:
            if rid != _native.REWARD_SYSTEM_CAPACITY:
                raise ValueError('reward_per_env needs the native SystemCapacityRewardFunction (the per-agent rewards differ per link)')
            h.set_reward_layout(_native.REWARD_PER_ENV)
        self._array_obs = isinstance(self.obs_fn, ArrayObsFunction)
        self.use_torch = (torch is not None and torch.cuda.is_available()) if use_torch is None else use_torch
        self._channel = sim.path_loss_table.route == CHANNEL      # SpatialChannelPathLoss: the table is filled at this env's clock
        if self._channel and not self.use_torch:
            raise ValueError('path_loss_model=SpatialChannelPathLoss needs the torch path (use_torch): its table is filled on the '
                             "device, on torch's stream, before every step - the NumPy path has no such hook")
        if mobility is not None:                       # refusals surface here, before anything is allocated
            if not isinstance(mobility, mobility_mod.GaussMarkovMobility):
                raise TypeError(f'mobility must be a GaussMarkovMobility or None, got {type(mobility).__name__}')
            why = mobility_mod.refusal(sim, self.use_torch)
            if why:
                raise ValueError(why)
        if traffic is not None:
            if not isinstance(traffic, queues_mod.PacketTraffic):
                raise TypeError(f'traffic must be a PacketTraffic or None, got {type(traffic).__name__}')
            why = queues_mod.refusal(self.use_torch)
            if why:
                raise ValueError(why)
        else:
            for fn, what in ((self.obs_fn, 'obs function'), (self.reward_fn, 'reward function')):
                if getattr(fn, 'needs_traffic', False):
                    raise ValueError(f'{type(fn).__name__} needs traffic=: this env has no packet queues for the {what} to read '
                                     '(VecD2DEnv(traffic=PacketTraffic(...)))')
        self._t = {}
        if self.use_torch:
            self._bind_torch_buffers()
        self.num_steps = 0
        self._episode = 0
        self._seed = cfg.seed if cfg.seed is not None else 0
        # which block the trials move: the obs block of the fused LinearObs step, or the table of the compact-obs step
        mode = self.obs_fn.native_mode
        fused = mode == _native.OBS_LINEAR and self.num_links <= 128 and not getattr(self, '_native_obs64', False)
        self._placement_target = ('obs', _native.BUF_OBS) if fused else (('table', _native.BUF_OBS_TABLE) if mode == _native.OBS_TABLE else None)
        if placement_trials in ('auto', None):             # the default of rounds 3 - 4; since round 5 the trials are opt-in
            placement_trials = 0
        if not isinstance(placement_trials, int) or isinstance(placement_trials, bool) or placement_trials < 0:
            raise ValueError("placement_trials must be a non-negative int (0 = off; 'auto' is accepted as 0)")
        self._placement_trials = placement_trials if self.use_torch and self._placement_target is not None else 0
        self._placement_budget = int(placement_budget_bytes)
        self.placement = None                      # after the trials: {'buffer': ..., 'us_per_step': [...], 'chosen': k}
        self.autoreset = bool(autoreset)
        if self.autoreset:
            self._setup_autoreset()
        # device mobility: nothing is loaded, allocated or launched unless a model is given
        self._mobility = None
        if isinstance(neighbor_refresh, bool) or not isinstance(neighbor_refresh, (int, np.integer)) or neighbor_refresh < 1:
            raise ValueError(f'neighbor_refresh must be an int >= 1, got {neighbor_refresh!r}')
        if neighbor_refresh != 1 and mobility is None:
            raise ValueError('neighbor_refresh needs mobility=: without it the neighbour lists are selected at reset and stay valid '
                             'until the next one')
        self._neighbor_refresh = int(neighbor_refresh)
        if mobility is not None:
            sim.path_loss_table.device_resets = True           # a per-step ArrayPathLoss gathers the coordinates before every step
            self._mobility = mobility_mod.Mobility(mobility, sim, torch, self.device, self.first_env, self.autoreset)
            self._t['vel_x'], self._t['vel_y'] = self._mobility.vel_x, self._mobility.vel_y
            self._view_cache = None
        # packet traffic: likewise nothing is loaded, allocated or launched unless a model is given
        self._queues = None
        if traffic is not None:
            self._queues = queues_mod.Queues(traffic, self.num_envs, self.num_cues, self.num_due_pairs, torch, self.device,
                                             self.first_env, self.autoreset)
            for name in queues_mod.PLANES:
                self._t[name] = getattr(self._queues, name)
            self._t['traffic'] = traffic
            self._view_cache = None
        # per-RB sensing (sense()): nothing is built, allocated or launched unless sense() is called or the obs function asks
        self._sensor = None
        self._senses = bool(getattr(self.obs_fn, 'needs_rb_sensing', False))
        if self._senses:
            self._rb_sensor()                      # refusals surface here, not inside the first step
        # the neighbour graph (coupling(), neighbors()): likewise nothing unless one of them is called or the obs function asks
        self._graph = None
        self._neighbors = None                     # (idx, coupling_db) of the obs function's k: selected at reset, constant between
        k = getattr(self.obs_fn, 'needs_neighbors', 0)
        self._neighbors_k = graph.check_k(k, self.num_links) if k is not False and k != 0 else 0
        if self._neighbors_k:
            self._neighbor_graph()
        # difference rewards (marginal_capacity()): likewise nothing unless it is called or the reward / obs function asks
        self._marginal = None
        self._obs_marginal = bool(getattr(self.obs_fn, 'needs_marginal', False)) and self._array_obs
        self._wants_marginal = self._obs_marginal or bool(getattr(self.reward_fn, 'needs_marginal', False))
        if self._wants_marginal:
            self._marginal_kernel()                # refusals surface here, not inside the first step
        # best-response RB selection (best_rb()): likewise nothing unless it is called or the obs / reward function asks
        self._bestrb = None
        self._action_levels = None                 # best_response_actions(): the power levels of every agent link's class
        self._obs_best_rb = bool(getattr(self.obs_fn, 'needs_best_rb', False)) and self._array_obs
        self._wants_best_rb = self._obs_best_rb or bool(getattr(self.reward_fn, 'needs_best_rb', False))
        if self._wants_best_rb:
            self._best_rb_kernel()                 # refusals surface here, not inside the first step
        # target-SINR power control (power_control()): nothing is loaded, allocated or launched unless it is called
        self._powerctl = None
        self._power_levels = None                  # power_control_actions(): (lowest power, power levels) of every agent link's class
        # sequential best-response dynamics (best_response_dynamics()): likewise nothing unless it is called
        self._brdyn = None
        # what-if evaluation of candidate joint actions (evaluate()): likewise nothing unless it is called
        self._evaluate = None
        # optimal one-to-one RB matching (assign_rbs()): likewise nothing unless it is called
        self._assign = None
        # joint RB and power matching with SINR floors (assign_rbs_power()): likewise
        self._joint = None
        # conflict-graph RB colouring (color_graph(), color_rbs()): likewise
        self._color = None
        # max-min SINR balancing (balance_sinr()): likewise
        self._balance = None
        # stable RB matching with quotas (solve_stable_matching(), stable_rbs()): likewise
        self._stable = None
        # exact optimal RB sharing (sharing_values(), solve_sharing(), share_rbs()): likewise
        self._share = None
        # sum-capacity power ascent with SINR floors (power_ascent()): likewise
        self._ascent = None
        # sum-capacity RB ascent with SINR floors (rb_ascent()): likewise
        self._rbascent = None
        # queue-aware goodput ascent over RBs and powers (goodput_ascent()): likewise
        self._goodput = None
        # unilateral-deviation gains over every (RB, power) action (deviation_gains(), best_deviation()): likewise
        self._deviation = None
        # what-if evaluation on a path-loss table (evaluate_table()): likewise
        self._table_evaluate = None
        # sum-capacity RB ascent on a path-loss table (rb_ascent_table()): likewise
        self._table_rbascent = None
        # difference rewards on a path-loss table (marginal_capacity_table()): likewise nothing unless it is called or the reward /
        # obs function asks
        self._table_marginal = None
        self._obs_table_marginal = bool(getattr(self.obs_fn, 'needs_table_marginal', False)) and self._array_obs
        self._wants_table_marginal = self._obs_table_marginal or bool(getattr(self.reward_fn, 'needs_table_marginal', False))
        if self._wants_table_marginal:             # refusals surface here, not inside the first step
            who = self.reward_fn if getattr(self.reward_fn, 'needs_table_marginal', False) else self.obs_fn
            why = table_marginal_mod.reward_refusal(sim, self.export_actions, self.use_torch, type(who).__name__)
            if why:
                raise ValueError(why)
            self._table_marginal_kernel()

    def _setup_autoreset(self) -> None:
        """Refuse what a device-side per-env reset cannot serve, then allocate the per-env bookkeeping: pending / episode are bound
        into the handle (D2D_BUF_RESET_PENDING / D2D_BUF_EPISODE), elapsed / done / reset belong to libd2d_episode.so's kernels."""
        sim = self.simulator
        kind, route = positions_move_unserved(sim, self.use_torch) or (None, '')
        if kind == 'numpy':
            raise ValueError('autoreset=True needs the torch path (use_torch): the per-env bookkeeping lives in device tensors')
        if kind == 'route':
            raise ValueError(f"autoreset=True cannot serve the '{route}' path-loss route: its table is evaluated once per reset, "
                             'which a device-side reset inside step() cannot follow without the host (use a per-step ArrayPathLoss '
                             'or a native model)')
        if kind == 'pinned':
            raise ValueError('autoreset=True cannot pin device_config coordinates that float32 cannot hold: they need the host '
                             'upload of a full reset')
        sim.path_loss_table.device_resets = True
        h, b, dev = sim.handle, self.num_envs, self.device
        for name, which in (('pending', _native.BUF_RESET_PENDING), ('episode', _native.BUF_EPISODE)):
            t = torch.zeros(b, dtype=torch.int32, device=dev)
            h.bind_buffer(which, t.data_ptr(), t.numel() * t.element_size())
            self._t[name] = t
        self._t['elapsed'] = torch.zeros(b, dtype=torch.int32, device=dev)
        self._t['done'] = torch.zeros(b, dtype=torch.bool, device=dev)
        self._t['reset'] = torch.zeros(b, dtype=torch.bool, device=dev)
        self._t['high'] = torch.as_tensor(np.asarray(self._initial_action_highs(), dtype=np.int32), device=dev)
        self._view_cache = None

    # ------------------------------------------------------------------ buffers
    def _bind_torch_buffers(self) -> None:
        h = self.simulator.handle
        dev = torch.device('cuda', self.config.device_ordinal)
        self.device = dev
        b, n, d = self.num_envs, self.num_links, h.num_devices
        cap = h.max_links

        def alloc(which, shape, dtype):
            # capacity follows the handle's max_links so re-linking never outgrows the binding
            t = torch.empty(shape, dtype=dtype, device=dev)
            h.bind_buffer(which, t.data_ptr(), t.numel() * t.element_size())
            return t

        self._t['pos_x'] = alloc(_native.BUF_POS_X, (b, d), torch.float32)
        self._t['pos_y'] = alloc(_native.BUF_POS_Y, (b, d), torch.float32)
        self._t['actions'] = alloc(_native.BUF_ACTIONS, (b * cap,), torch.int32)[:b * self.num_agents].view(b, self.num_agents)
        for name, which in (('rb', _native.BUF_RB), ('pwr', _native.BUF_PWR)):
            self._t[name] = alloc(which, (b * cap,), torch.int32)[:b * n].view(b, n)
        for name, which in _OUTPUTS:
            if name == 'reward' and self.reward_per_env:
                self._t[name] = alloc(_native.BUF_REWARD_ENV, (b,), torch.float32)
                continue
            self._t[name] = alloc(which, (b * cap,), torch.float32)[:b * n].view(b, n)
        if self.obs_fn.native_mode != _native.OBS_NONE:
            self._t['table'] = alloc(_native.BUF_OBS_TABLE, (b * cap * 6,), torch.float32)[:b * n * 6].view(b, n, 6)
        else:
            self._t['table'] = None                        # D2D_OBS_NONE: no table exists; positions: link_positions()
        self._t['env_flags'] = alloc(_native.BUF_ENV_FLAGS, (b,), torch.int32)
        if self.obs_fn.native_mode == _native.OBS_LINEAR:
            self._t['obs'] = alloc(_native.BUF_OBS, (b, n, 6 * n), torch.float64 if self._native_obs64 else torch.float32)
        self._stream_ptr = None
        # the raw current-stream query (one C call, no Stream object) when this torch has it
        raw = getattr(torch._C, '_cuda_getCurrentRawStream', None)
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        self._current_stream_ptr = (lambda: raw(index)) if raw is not None else \
            (lambda: torch.cuda.current_stream(self.device).cuda_stream)
        self._follow_torch_stream()
        # per-step constants of the torch path: the buffers do not move (the opt-in placement trials re-bind ONE block once, inside
        # the first reset, and drop this cache), so the view, the info dict and the two possible `dones` vectors are built once
        self._view_cache = None
        self._dones = (torch.zeros(b, dtype=torch.bool, device=dev), torch.ones(b, dtype=torch.bool, device=dev))

    def _follow_torch_stream(self) -> None:
        """Run the library's kernels on torch's CURRENT stream (the null stream by default) so they are ordered with
        the torch ops that produce actions / consume results.  Re-bound only when the caller switches streams."""
        ptr = self._current_stream_ptr()
        if ptr != self._stream_ptr:
            self.simulator.set_stream(ptr)
            self._stream_ptr = ptr

    def _view(self) -> SimpleNamespace:
        sim = self.simulator
        if self.use_torch:
            if self._view_cache is not None:
                return self._view_cache
            v = dict(self._t)
        else:
            v = {name: sim.fetch(_native.BUF_REWARD_ENV if name == 'reward' and self.reward_per_env else which)
                 for name, which in _OUTPUTS if name != 'reward' or getattr(self.reward_fn, 'native_id', 0)}
            if self.export_actions:                        # otherwise the two planes are stale / never written
                v['rb'] = sim.fetch(_native.BUF_RB); v['pwr'] = sim.fetch(_native.BUF_PWR)
            v['table'] = sim.fetch(_native.BUF_OBS_TABLE) if self.obs_fn.native_mode != _native.OBS_NONE else None
            v['pos_x'] = sim.fetch(_native.BUF_POS_X); v['pos_y'] = sim.fetch(_native.BUF_POS_Y)
            if self.obs_fn.native_mode == _native.OBS_LINEAR:
                v['obs'] = sim.fetch(_native.BUF_OBS)
        v.update(link_tx=sim.link_tx, link_rx=sim.link_rx, link_type=sim.link_type)
        if not self.export_actions:
            v['rb'] = v['pwr'] = None
        view = SimpleNamespace(**v)
        if self.use_torch:
            self._view_cache = view
            self._info = {'rb': view.rb, 'tx_pwr_dbm': view.pwr, 'snr_db': view.snr_db, 'sinr_db': view.sinr_db,
                          'rate_bps': view.rate_bps, 'capacity_mbps': view.capacity_mbps}
            if self._queues is not None:
                self._info.update({k: v[k] for k in ('served_bits', 'backlog_bits', 'expired_bits', 'overflow_bits')})
        return view

    # ------------------------------------------------------------------ gym-like API
    def _initial_action_highs(self):
        n_cue = self.config.num_rbs * self.num_pwr_actions[self._cue_kind]
        n_due = self.config.num_rbs * self.num_pwr_actions['due']
        return ([n_cue] * self.num_cues if self.cue_actions == 'agent' else []) + [n_due] * self.num_due_pairs

    def reset(self, seed: Optional[int] = None, *, elapsed=None):
        """New positions for every env (device-side sampler), then one step with uniformly random actions on every
        agent-driven link to produce the initial SINRs (d2d_env.py:45-60).  Both draws are counter-based and keyed
        by global env index (first_env + b).

        elapsed (autoreset only): int [B] in [0, EPISODE_LENGTH) - env b's first episode then ends after EPISODE_LENGTH -
        elapsed[b] steps.  Without a seed, the episode index continues after the largest one any env has drawn."""
        if elapsed is not None:
            if not self.autoreset:
                raise ValueError('elapsed staggers the episodes of autoreset=True; a lockstep env has one episode clock')
            elapsed = np.asarray(elapsed.cpu() if torch is not None and torch.is_tensor(elapsed) else elapsed)
            if elapsed.shape != (self.num_envs,) or elapsed.dtype.kind not in 'iu' or \
                    (elapsed.size and (elapsed.min() < 0 or elapsed.max() >= EPISODE_LENGTH)):
                raise ValueError(f'elapsed must be ints [{self.num_envs}] in [0, {EPISODE_LENGTH})')
        if seed is not None:
            self._seed, self._episode = int(seed), 0
        elif self.autoreset:
            # per-env resets drew episodes up to (not including) the largest counter: continue after them (reset() syncs anyway)
            self._episode = max(self._episode, int(self._t['episode'].max()))
        self.num_steps = 0
        if self.use_torch:
            self._follow_torch_stream()
        self.simulator.reset_device(self._seed, self._episode)
        highs = self._initial_action_highs()
        if self.use_torch:
            if self.num_agents:
                self._t['actions'].copy_(_rng.uniform_ints_torch(torch, self._seed, self._episode, self.first_env,
                                                                  self.num_envs, self.num_agents, highs, self.device))
            if self._channel:
                self.simulator.path_loss_table.set_channel_clock(self._seed, self._episode, 0)
            self.simulator.prepare_step()
            self.simulator.handle.step()
        else:
            a = _rng.uniform_ints_numpy(self._seed, self._episode, self.first_env, self.num_envs, self.num_agents, highs) \
                if self.num_agents else np.zeros((self.num_envs, 0), np.int32)
            self.simulator.step_arrays(a)
        self._episode += 1
        if self.autoreset:
            self._t['episode'].fill_(self._episode)
            self._t['pending'].zero_()
            self._t['done'].zero_()
            self._t['reset'].zero_()
            if elapsed is None:
                self._t['elapsed'].zero_()
            else:
                self._t['elapsed'].copy_(torch.as_tensor(elapsed.astype(np.int32), device=self.device))
            if self._channel:
                self.simulator.path_loss_table.channel.start_episode(self._t['elapsed'])
        if self._mobility is not None:                        # behind the sampler; the reset's own step did not see a move
            self._mobility.start_episode(self._t, self._seed, self._episode - 1, self._stream_ptr)
        if self._queues is not None:                          # t = 0 behind the reset's step, which serves nothing
            self._queues.start_episode(self._t, self._seed, self._episode - 1, self._stream_ptr)
        self.simulator.check_flags()
        if self._placement_trials > 1 and self.placement is None:
            self._choose_obs_placement(self._placement_trials)
        if self._neighbors_k:
            self._select_neighbors()
        view = self._view()
        if self._obs_marginal:
            view = self._with_marginal(view)
        if self._obs_table_marginal:
            view = self._with_table_marginal(view)
        if self._obs_best_rb:
            view = self._with_best_rb(view)
        return self._observe(view)

    def _choose_obs_placement(self, trials: int, warm_ms: float = 15.0, steps: int = 256) -> None:
        """Time the step on up to `trials` candidate blocks for the dominant output (all held until the choice, hence distinct
        physical ranges), keep the fastest.  The step repeated here is the reset's own (same positions, same actions in the
        bound action buffer: same outputs), so the env's state after the trials is what reset() produced; only the shadowing
        model's step counter would advance, so that model keeps the block it has."""
        import time
        h = self.simulator.handle
        if self.simulator.shadowing_seed is not None:
            self.placement = {'skipped': 'ShadowingPathLoss draws per step'}
            return
        if self.simulator.path_loss_table.route == PER_STEP:
            self.placement = {'skipped': 'a per-step ArrayPathLoss is evaluated before every step'}
            return
        if self._channel:
            self.placement = {'skipped': 'SpatialChannelPathLoss is evaluated before every step'}
            return
        key, which = self._placement_target
        base = self._t[key]                                     # a view of the bound allocation (capacity may exceed the active part)
        first = base._base if base._base is not None else base
        nbytes = first.numel() * first.element_size()

        def timed(n):
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            for _ in range(n):
                h.step()
            torch.cuda.synchronize(self.device)
            return (time.perf_counter() - t0) / n * 1e6
        t_end = time.perf_counter() + warm_ms * 1e-3            # past the clock ramp behind the idle stretch of building the env
        while time.perf_counter() < t_end:
            timed(64)
        # every candidate (and the padding in front of it) lives in a MemPool of its own: dropping a loser's pool gives its memory
        # back to the driver without touching the caching allocator the caller's tensors live in
        def alloc_private(nbytes_, like=None):
            pool = torch.cuda.MemPool() if hasattr(torch.cuda, 'MemPool') else None
            if pool is None:
                return None, (torch.empty_like(like) if like is not None else torch.empty(nbytes_, dtype=torch.uint8, device=self.device))
            # use_mem_pool routes the allocations of ONE device: name the env's, which need not be the current one
            with torch.cuda.device(self.device), torch.cuda.use_mem_pool(pool, device=self.device):
                t = torch.empty_like(like) if like is not None else torch.empty(nbytes_, dtype=torch.uint8, device=self.device)
            return pool, t
        cands, pools, pads, times = [first], [None], [], []
        held = 0
        for k in range(trials):
            if k:
                # neighbouring allocations tend to share a speed class: a padding of varying size in front of every candidate
                pad = ((k * 7) % 11 + 1) * (2 << 20) + (k % 3) * 4096
                if held + pad + nbytes > self._placement_budget:
                    break
                try:
                    pads.append(alloc_private(pad))
                    pool, t = alloc_private(0, like=first)
                except torch.cuda.OutOfMemoryError:             # a crowded GPU: choose among what there is
                    break
                cands.append(t); pools.append(pool)
                held += pad + nbytes
            h.bind_buffer(which, cands[k].data_ptr(), nbytes)
            timed(32)
            times.append(timed(steps))
            if k >= 3 and min(times) < 0.93 * max(times):
                break
        best = min(range(len(times)), key=times.__getitem__)
        chosen = cands[best]
        h.bind_buffer(which, chosen.data_ptr(), nbytes)
        self._t[key] = chosen[:base.numel()].view(base.shape) if chosen.shape != base.shape else chosen
        self._placement_pool = pools[best]                      # the winner's pool lives as long as the env
        h.step()                                                # the reset's step once more, into the block that stays
        self._view_cache = None
        self.placement = {'buffer': key, 'us_per_step': [round(t, 2) for t in times], 'chosen': best,
                          'transient_bytes': held, 'private_pools': pools[-1] is not None or len(pools) == 1}
        # the losers and the paddings: tensors first, then their pools (a pool without live tensors returns its blocks to the driver)
        torch.cuda.synchronize(self.device)
        del cands, pads, first, base, chosen, pools

    def step(self, actions):
        """actions: int [B, num_agents] (torch CUDA tensor, or NumPy).  Returns (obs, rewards[B,N], dones[B], info).
        Asynchronous on the torch path: nothing here waits for the GPU, so error flags are NOT checked per step -
        see status_flags()."""
        sim = self.simulator
        if self.autoreset:
            return self._step_autoreset(actions)
        if self.use_torch:
            self._follow_torch_stream()
            src = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions), device=self.device)
            if tuple(src.shape) != (self.num_envs, self.num_agents):
                raise ValueError(f'actions must be [{self.num_envs},{self.num_agents}], got {tuple(src.shape)}')
            if self._mobility is not None:
                self._move_devices()
            if self._channel:
                sim.path_loss_table.set_channel_clock(self._seed, self._episode - 1, self.num_steps + 1)
            sim.prepare_step()                                # a per-step ArrayPathLoss or the spatial channel: this step's table
            if src.dtype == torch.int32 and src.is_contiguous() and src.device == self.device:
                sim.handle.step(src.data_ptr())               # zero copy: the kernel reads the caller's tensor
            else:
                self._t['actions'].copy_(src)
                sim.handle.step()
            if self._queues is not None:
                self._queues.step(self._t, self._seed, self.num_steps + 1, self._episode - 1, self._stream_ptr)
        else:
            src = np.asarray(actions, dtype=np.int32)
            if src.shape != (self.num_envs, self.num_agents):
                raise ValueError(f'actions must be [{self.num_envs},{self.num_agents}], got {src.shape}')
            sim.step_arrays(src)
        self.num_steps += 1
        if self._mobility is not None and self._neighbors_k and self.num_steps % self._neighbor_refresh == 0:
            self._select_neighbors()                          # the lists of the moved positions
        view = self._view()
        if self._wants_marginal:
            view = self._with_marginal(view)
        if self._wants_table_marginal:
            view = self._with_table_marginal(view)            # one launch behind the step, on the table the step just read
        if self._wants_best_rb:
            view = self._with_best_rb(view)
        obs = self._observe(view)
        rewards = view.reward if self._native_reward else self.reward_fn.compute(view)
        done = self.num_steps >= EPISODE_LENGTH
        if self.use_torch:
            return obs, rewards, self._dones[done], dict(self._info)
        info = {'rb': view.rb, 'tx_pwr_dbm': view.pwr, 'snr_db': view.snr_db, 'sinr_db': view.sinr_db,
                'rate_bps': view.rate_bps, 'capacity_mbps': view.capacity_mbps}
        return obs, rewards, np.full(self.num_envs, done), info

    def _step_autoreset(self, actions):
        """One step of autoreset=True, enqueued on torch's current stream: the pending envs' positions (masked reset) -> a per-step
        path-loss table for the step -> the action rows, pending envs' replaced by their reset's random actions, into the bound
        action buffer -> d2d_step -> the per-env counters, dones and next pending set (libd2d_episode.so).  No synchronisation."""
        sim, t = self.simulator, self._t
        h = sim.handle
        self._follow_torch_stream()
        src = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions), device=self.device)
        if tuple(src.shape) != (self.num_envs, self.num_agents):
            raise ValueError(f'actions must be [{self.num_envs},{self.num_agents}], got {tuple(src.shape)}')
        if src.dtype != torch.int32 or not src.is_contiguous() or src.device != self.device:
            src = src.to(device=self.device, dtype=torch.int32).contiguous()
        stream = self._stream_ptr
        h.reset_positions(self._seed, _native.EPISODE_PER_ENV)
        if self._mobility is not None:
            self._move_devices()                              # the envs that are not pending; the pending ones get new velocities
        if self._channel:
            sim.path_loss_table.set_channel_clock(self._seed, per_env=t)
        sim.prepare_step()                                    # a per-step ArrayPathLoss: this step's table, at the new positions
        if self.num_agents:
            _native.episode_merge_actions(src.data_ptr(), t['actions'].data_ptr(), t['pending'].data_ptr(), t['episode'].data_ptr(),
                                          t['high'].data_ptr(), self.num_envs, self.num_agents, self.first_env, self._seed, stream)
        h.step()
        if self._queues is not None:                          # before episode_advance: the clock is the move's
            self._queues.step_per_env(t, self._seed, stream)
        self.num_steps += 1
        view = self._view()
        native = self._native_reward
        reward = view.reward if native else None
        _native.episode_advance(t['pending'].data_ptr(), t['episode'].data_ptr(), t['elapsed'].data_ptr(), t['done'].data_ptr(),
                                t['reset'].data_ptr(), reward.data_ptr() if native else 0,
                                1 if self.reward_per_env else self.num_links, self.num_envs, EPISODE_LENGTH, stream)
        if self._neighbors_k:
            refresh = self._mobility is not None and self.num_steps % self._neighbor_refresh == 0
            self._select_neighbors(None if refresh else t['reset'])   # the envs this step reset stand at new positions; moved: all
        if self._wants_marginal:
            view = self._with_marginal(view)                  # after the step: the envs it reset at their new positions and actions
        if self._wants_table_marginal:
            view = self._with_table_marginal(view)            # likewise: the table is the last fill, the reset envs' new blocks included
        if self._wants_best_rb:
            view = self._with_best_rb(view)                   # likewise: one launch behind the step serves every env
        obs = self._observe(view)
        if native:
            rewards = view.reward
        else:
            rewards = self.reward_fn.compute(view)
            reset = t['reset'].view((-1,) + (1,) * (rewards.dim() - 1))
            rewards = torch.where(reset, torch.zeros((), dtype=rewards.dtype, device=rewards.device), rewards)
        info = dict(self._info)
        info['reset'] = t['reset']
        return obs, rewards, t['done'], info

    def _move_devices(self) -> None:
        """One move of every device before the step about to be enqueued, then the handle's and the path-loss table's notice."""
        m, sim = self._mobility, self.simulator
        if self.autoreset:
            m.move_per_env(self._t, self._seed, self._stream_ptr)
        else:
            m.move(self._t, self._seed, self.num_steps + 1, self._episode - 1, self._stream_ptr)
        sim.handle.positions_changed()
        sim.path_loss_table.positions_changed()

    def velocities(self):
        """(vel_x, vel_y), float32 [B, D] in m/s: the env's own planes, updated in place by every step (mobility= only)."""
        if self._mobility is None:
            raise ValueError('velocities() needs mobility=: this env\'s devices stand still between resets')
        return self._mobility.vel_x, self._mobility.vel_y

    def queues(self):
        """The packet queues' planes as a namespace (traffic= only): arrived_bits, served_bits, expired_bits, overflow_bits,
        backlog_bits, hol_age_steps int32, mean_delay_steps float32, on uint8, all [B, N], and ring int32 [D, B, N] - the env's own
        tensors, updated in place by every step (clone them to keep a step's values)."""
        if self._queues is None:
            raise ValueError('queues() needs traffic=: this env\'s links are full-buffer')
        return self._queues.planes()

    def request_reset(self, mask) -> None:
        """Reset the envs mask marks (bool [B], tensor or ndarray) at the next step() instead of stepping them - device-side and
        asynchronous (autoreset=True only)."""
        if not self.autoreset:
            raise ValueError('request_reset needs autoreset=True')
        m = torch.as_tensor(mask, device=self.device)
        if tuple(m.shape) != (self.num_envs,) or m.dtype != torch.bool:
            raise ValueError(f'mask must be bool [{self.num_envs}]')
        self._follow_torch_stream()
        self._t['pending'].masked_fill_(m, 1)

    # ------------------------------------------------------------------ the add-on kernels' objects
    def _kernel(self, slot: str, module, cls, extra=tuple, torch_only: bool = True):
        """The add-on kernel object in self.<slot>, opened on first use: module.refusal() says why this env cannot have one
        (ValueError), else cls(simulator, num_links, *extra(), torch, device) - torch / device None on the NumPy path."""
        if getattr(self, slot) is None:
            why = module.refusal(self.simulator, self.export_actions, *((self.use_torch,) if torch_only else ()))
            if why:
                raise ValueError(why)
            where = (torch, self.device) if self.use_torch else (None, None)
            setattr(self, slot, cls(self.simulator, self.num_links, *extra(), *where))
        return getattr(self, slot)

    def _agent_links(self):
        """bool [N]: the links that have an action column (links on fixed actions come first and have none)."""
        return np.arange(self.num_links) >= self.num_links - self.num_agents

    def _due_links(self):
        """bool [N]: the DUE-pair links (the last ones of the link list)."""
        return np.arange(self.num_links) >= self.num_links - self.num_due_pairs

    def _agent_levels(self):
        """int32 [num_agents] on the device: the power levels of every agent link's class, what the encode_actions / decode_actions
        functions take.  self._action_levels, made by the first *_actions call that needs it."""
        if self._action_levels is None:
            p = self.num_pwr_actions
            levels = ([p[self._cue_kind]] * self.num_cues if self.cue_actions == 'agent' else []) + [p['due']] * self.num_due_pairs
            self._action_levels = torch.as_tensor(np.asarray(levels, dtype=np.int32), device=self.device)
        return self._action_levels

    # ------------------------------------------------------------------ per-RB sensing
    def _rb_sensor(self):
        return self._kernel('_sensor', sensing, sensing.RbSensor, torch_only=False)

    def sense(self, what: str = 'sinr_db', out=None):
        """What every link would see on every resource block, with everything else as the last step left it: float32 [B, N, R].

        what='sinr_db': sense[b, i, r] is the SINR (dB) link i would get if it alone moved to RB r at its current power - column
        rb[b, i] is the step's own sinr_db, an RB nobody else uses gives the link's SNR.  what='interference_mw': the sum, in mW, of
        what the other links on RB r put into link i's receiver (0.0 exactly on an RB nobody else uses).  One kernel launch
        (csrc/d2d_sense.hip).  Valid after reset() and after every step(), autoreset steps included: an env that was reset inside
        the step is sensed at its new positions and its reset's random actions.  With mobility= the position planes it reads are the
        moved ones: current after every step.

        torch path: enqueued on torch's current stream, nothing is synchronised; the result is ONE tensor the env owns and
        rewrites on every call (clone it to keep it), or `out` (contiguous float32 [B, N, R] on the env's device) if given.
        NumPy path: a fresh array, or `out`.

        Serves the native power-law models (LogDistance with any exponent, FreeSpace, COST-Hata, per-device overrides, uplink
        and downlink CUE links).  ValueError for what it cannot serve: export_actions=False (it reads the decoded planes),
        ShadowingPathLoss, every table route (device_table, link_table, array, per_step), pinned device_config coordinates
        float32 cannot hold."""
        if what not in sensing.WHAT:
            raise ValueError("what must be 'sinr_db' or 'interference_mw'")
        sensor = self._rb_sensor()
        if self.use_torch:
            self._follow_torch_stream()
            return sensor.sense_torch(self._t, sensing.WHAT[what], out, self._stream_ptr)
        return sensor.sense_numpy(sensing.WHAT[what], out)

    # ------------------------------------------------------------------ the neighbour graph
    def _neighbor_graph(self):
        return self._kernel('_graph', graph, graph.NeighborGraph, torch_only=False)

    def coupling(self, out=None):
        """The dense interference graph, float32 [B, N, N]: coupling[b, i, j] = eirp_off_db[tx_j] - PL(tx_j -> rx_i), the dBm link
        i's receiver gets per 0 dBm of link j's tx power, so that the step's interference on link i is the sum over j != i with
        rb_j == rb_i of lin(pwr_j + coupling[b, i, j]).  INDEX ORDER: [b, i, j] is receiver-major - i receives, j transmits, one
        agent's row contiguous; the path-loss tables elsewhere in the project are [b, j, i].  The diagonal holds the same formula
        (own transmitter into own receiver, no receiver gains).  Positions and the model only: constant between resets - unless the
        env has mobility=, where every call reads the position planes as the last move left them.  One kernel
        launch (csrc/d2d_graph.hip); 4 B N^2 bytes - 4.3 GB at 4096 x 512.

        torch path: enqueued on torch's current stream, nothing is synchronised; ONE tensor the env owns and rewrites on every call,
        or `out` (contiguous float32 [B, N, N] on the env's device).  NumPy path: a fresh array, or `out`.  Valid after reset() and
        after every step(), autoreset steps included.  ValueError for what sense() refuses too: export_actions=False,
        ShadowingPathLoss, every table route, pinned device_config coordinates float32 cannot hold."""
        g = self._neighbor_graph()
        if self.use_torch:
            self._follow_torch_stream()
            return g.coupling_torch(self._t, out, self._stream_ptr)
        return g.coupling_numpy(out)

    def neighbors(self, k: int, out=None):
        """Every link's k strongest interferers: (idx int32 [B, N, k], coupling_db float32 [B, N, k]).  Row [b, i] lists the k links
        j != i with the largest coupling()[b, i, j] - i is the RECEIVING link, receiver-major as coupling() ([b, i, j]; the path-loss
        tables elsewhere are [b, j, i]) - strongest first, equal values (a downlink base station transmits every CUE link) in
        ascending j; coupling_db[b, i, m] is coupling()[b, i, idx[b, i, m]] bit for bit.  1 <= k <= min(N - 1, 64).  Positions and
        the model only, never actions: constant between resets (with mobility=: current after every move; the lists an obs function
        sees are re-selected every neighbor_refresh-th step).  One kernel launch, no [B, N, N] cube.

        torch path: on torch's current stream, nothing is synchronised; the pair of tensors the env owns for this k, rewritten by
        every call, or `out` = (idx, coupling_db), contiguous int32 / float32 [B, N, k] on the env's device.  NumPy path: fresh
        arrays, or `out`.  Valid and refused as coupling() is."""
        k = graph.check_k(k, self.num_links)
        g = self._neighbor_graph()
        if self.use_torch:
            self._follow_torch_stream()
            return g.neighbors_torch(self._t, k, out, self._stream_ptr)
        return g.neighbors_numpy(k, out)

    def _select_neighbors(self, env_mask=None) -> None:
        """The obs function's neighbour lists: all envs (reset()), or the envs env_mask marks (bool [B]: the envs an autoreset step
        reset; the others keep their rows)."""
        g, k = self._graph, self._neighbors_k
        if self.use_torch:
            self._neighbors = g.neighbors_torch(self._t, k, None, self._stream_ptr, env_mask)
        else:
            self._neighbors = g.neighbors_numpy(k, None)

    # ------------------------------------------------------------------ difference rewards
    def _marginal_kernel(self):
        return self._kernel('_marginal', marginal, marginal.MarginalCapacity, torch_only=False)

    def marginal_capacity(self, out=None):
        """What every link costs the others, with everything as the last step left it: (difference_mbps, harm_mbps), float32 [B, N].

        harm_mbps[b, i] is the capacity the OTHER links of link i's RB would gain if link i alone went off the air - the sum over
        them of cap_j without i's transmitter minus cap_j with it, the `sinr > rx_sensitivity` threshold of the step included -
        and difference_mbps[b, i] = capacity_mbps[b, i] - harm_mbps[b, i] is the difference reward G(a) - G(a without link i) of
        the total capacity G.  harm >= 0; a link alone on its RB has harm == 0.0 and difference == capacity exactly.  One kernel
        launch (csrc/d2d_marginal.hip), no [B, N, N] cube.  Valid after reset() and after every step(), autoreset steps included:
        an env that was reset inside the step is evaluated at its new positions and its reset's random actions; with mobility= at the
        positions the step's own move left.

        torch path: enqueued on torch's current stream, nothing is synchronised; the pair of tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (difference_mbps, harm_mbps), two contiguous float32 [B, N] tensors on the
        env's device.  NumPy path: fresh arrays, or `out`.

        Serves what sense() serves; ValueError for export_actions=False, ShadowingPathLoss, every table route, pinned device_config
        coordinates float32 cannot hold."""
        m = self._marginal_kernel()
        if self.use_torch:
            self._follow_torch_stream()
            return m.torch_planes(self._t, out, self._stream_ptr)
        return m.numpy_planes(out)

    def _with_marginal(self, view):
        """The view plus difference_mbps / harm_mbps, as a namespace of its own: the cached view stays what every other consumer sees."""
        diff, harm = self.marginal_capacity()
        return SimpleNamespace(**vars(view), difference_mbps=diff, harm_mbps=harm)

    # ------------------------------------------------------------------ best-response RB selection
    def _best_rb_kernel(self):
        return self._kernel('_bestrb', best_response, best_response.BestRb)

    def best_rb(self, allowed=None, out=None):
        """Where every link would be best off, with everything else as the last step left it: (best_rb int32, best_sinr_db float32,
        gain_db float32), each [B, N].

        best_rb[b, i] is the RB on which link i would see the highest SINR if it alone moved there at its current power - the argmax
        over r of sense('sinr_db')[b, i, r], equal values (RBs nobody else uses) to the lowest r - best_sinr_db that SINR, a value
        of the sensed block bit for bit, and gain_db = best_sinr_db - sinr_db: what the move would gain, 0.0 exactly for a link that
        already sits on its best RB.  One kernel launch (csrc/d2d_bestrb.hip) that keeps a running best in registers: no [B, N, R]
        block is written or read.  Valid after reset() and after every step(), autoreset steps included, as sense() is.

        allowed: bool [N, R] (tensor or array), allowed[i, r] = link i may choose RB r; None: every RB.  A link with no allowed RB
        gets best_rb -1 and NaN values; a link whose own RB is not allowed still gets a finite (possibly negative) gain_db.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the three tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (best_rb, best_sinr_db, gain_db), contiguous int32 / float32 / float32
        [B, N] on the env's device.  Serves what sense() serves; ValueError for export_actions=False, ShadowingPathLoss, every table
        route, pinned device_config coordinates float32 cannot hold."""
        k = self._best_rb_kernel()
        self._follow_torch_stream()
        return k.planes(self._t, allowed, out, self._stream_ptr)

    def best_response_actions(self, allowed=None, min_gain_db: float = 0.0):
        """One round of best response as an action tensor, int32 [B, num_agents], ready for step(): every agent link whose
        gain_db > min_gain_db moves to its best_rb() at its current power level, every other one repeats its last action (as the
        decoded planes hold it), encoded rb * power levels + level.  Links on fixed actions (cue_actions='traffic') have no column
        and are never moved; `allowed` as best_rb() takes it.  All links moving at once can chase each other onto the same quiet
        RBs: a min_gain_db above 0, or an `allowed` mask that lets a part of the links move per round, damps that."""
        if not np.isfinite(min_gain_db) or min_gain_db < 0.0:
            raise ValueError(f'min_gain_db must be a finite number >= 0, got {min_gain_db!r}')
        best, _, gain = self.best_rb(allowed)
        return best_response.encode_actions(self._t['rb'], self._t['pwr'], best, gain, self._agent_levels(), float(min_gain_db),
                                            self.num_links - self.num_agents)

    def _with_best_rb(self, view):
        """The view plus best_rb / best_sinr_db / gain_db, as a namespace of its own: the cached view stays what every other consumer
        sees."""
        best, sinr, gain = self.best_rb()
        return SimpleNamespace(**vars(view), best_rb=best, best_sinr_db=sinr, gain_db=gain)

    # ------------------------------------------------------------------ target-SINR power control
    def _class_bounds(self):
        """(p_min, p_max) int32 [N] of every link's class, in the dBm the step transmits (power_control.class_bounds)."""
        return power_control.class_bounds(self.num_pwr_actions, self._cue_kind, self.num_cues, self.num_due_pairs)

    def _agent_power_levels(self):
        """(first agent link, lowest power [num_agents], power levels [num_agents]) for power_control.encode_actions: the two
        device tensors are made once."""
        first = self.num_links - self.num_agents
        if self._power_levels is None:
            p_min, p_max = self._class_bounds()
            self._power_levels = tuple(torch.as_tensor(a[first:], device=self.device) for a in (p_min, p_max - p_min + 1))
        return (first, *self._power_levels)

    def _power_control_kernel(self):
        return self._kernel('_powerctl', power_control, power_control.PowerControl,
                            lambda: (*self._class_bounds(), self._agent_links()))

    def power_control(self, target_sinr_db, adjustable=None, max_iters: int = 64, out=None, env_mask=None):
        """The least powers that meet a target SINR, with positions and RBs as the last step left them: (power_dbm int32 [B, N],
        sinr_db float32 [B, N], iters int32 [B], converged uint8 [B]), a tuple with those names.

        The constrained target-SINR iteration (Foschini-Miljanic / Yates) on the env's integer dBm alphabet: every adjustable link
        starts at the lowest power of its class and raises it, whole dBm at a time and all links at once from the same old vector,
        to ceil(power + target - sinr_db), never past its class maximum and never down.  It ends at the least fixed point - the
        componentwise power-minimal assignment that meets the targets when they are feasible; links whose target is out of reach
        end at their maximum - or after max_iters sweeps that each changed a link (converged 0, iters == max_iters).  sinr_db is
        the step's sinr_db for power_dbm bit for bit, valid at the cap too.  All sweeps of an env run in one workgroup of one kernel
        launch (csrc/d2d_powerctl.hip) out of LDS: no [B, N, N] pass per sweep.  Valid after reset() and after every step(),
        autoreset steps included, as sense() is.

        target_sinr_db: a number, {'cue': x, 'due': y}, or [N] values (array or tensor), dB.  adjustable: bool [N], the links that
        may move (array, or a tensor that is combined with the agent links on the device and never read on the host); None: every
        agent link.  Links on fixed actions (cue_actions='traffic') are never adjusted; a link that is not
        adjusted keeps its power and interferes; a link on no RB (rb outside [0, R)) keeps its power and has sinr_db NaN.  The
        bounds are the ones step() decodes: an agent's power is its action's level, 0 .. levels - 1 dBm (due_min_tx_power_dBm is
        not added back, as in d2d_env.py:94-96).  env_mask: bool / uint8 [B], envs whose entry is 0 keep their rows; None: all.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the four tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (power_dbm, sinr_db, iters, converged), contiguous int32 / float32 [B, N],
        int32 / uint8 [B] on the env's device.  Serves what sense() serves; ValueError for export_actions=False, ShadowingPathLoss,
        every table route, pinned device_config coordinates float32 cannot hold."""
        k = self._power_control_kernel()
        target, adj = k.target(target_sinr_db, self.num_cues), k.adjustable(adjustable)
        self._follow_torch_stream()
        return k.solve(self._t, target, adj, max_iters, out, self._stream_ptr, env_mask)

    def power_control_actions(self, target_sinr_db, adjustable=None, max_iters: int = 64):
        """power_control() as an action tensor, int32 [B, num_agents], ready for step(): every agent link stays on its RB (as the
        decoded planes hold it) at the solved power, encoded rb * power levels + level; an agent link that is not adjustable
        repeats its last action.  Links on fixed actions (cue_actions='traffic') have no column.  Composes with
        best_response_actions(): one call picks RBs, the other picks powers."""
        power = self.power_control(target_sinr_db, adjustable, max_iters)[0]
        first, p_min, levels = self._agent_power_levels()
        return power_control.encode_actions(self._t['rb'], power, p_min, levels, first)

    # ------------------------------------------------------------------ max-min SINR balancing
    def _balance_kernel(self):
        return self._kernel('_balance', balance, balance.SinrBalance, lambda: (*self._class_bounds(), self._agent_links()))

    def balance_sinr(self, base_sinr_db=0.0, margins_db=None, floor_sinr_db=None, adjustable=None, max_iters: int = 64, out=None,
                     env_mask=None):
        """The largest SINR level every adjustable link can be given at once with the protected links kept above their floors, and the
        least powers that give it, with positions and RBs as the last step left them: (power_dbm int32 [B, N], sinr_db float32
        [B, N], margin_db float32 [B], level int32 [B], probes int32 [B]), a tuple with those names.

        Level k of the grid margins_db asks every adjustable link i for base_sinr_db[i] + margins_db[k].  Probe k is power_control()
        for that target - cold from the lowest powers, at most max_iters sweeps - and its powers, SINRs and converged flag are what
        power_control() returns for it, bit for bit.  It passes iff it converged, no adjustable link on an RB sits at its class
        maximum with sinr_db below its target, and no link on an RB has sinr_db below floor_sinr_db (float32 comparisons; NaN
        compares false).  The search is fixed: probe 0 first - if it fails the env is infeasible (level -1, margin_db -inf, the
        planes of probe 0, probes 1) - then lo = 0, hi = K and, while hi - lo > 1, probe (lo + hi) // 2: a pass raises lo, a fail
        lowers hi.  level = lo: it passes, and level + 1 is K or fails.  At most 13 probes.  The whole search of an env runs in one
        workgroup of ONE kernel launch (csrc/d2d_balance.hip) out of LDS.  Valid after reset() and after every step(), as
        power_control() is.

        base_sinr_db, floor_sinr_db: a number, {'cue': x, 'due': y}, or [N] values (array or tensor), dB; floor None or -inf: no
        floor.  margins_db: 1 to 4096 finite, strictly ascending values, checked on the host when given as an array; a float32
        tensor [K] on the env's device is taken as it is (its order is the caller's promise); None: -20, -19, ..., 40.
        adjustable, max_iters, env_mask: as power_control() takes them - None adjusts every agent link, links on fixed actions
        (cue_actions='traffic') never move, a link that is not adjusted keeps its power, interferes and is still held to its floor.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the five tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (power_dbm, sinr_db, margin_db, level, probes), contiguous int32 / float32
        [B, N], float32 / int32 / int32 [B] on the env's device.  Serves what power_control() serves; ValueError for
        export_actions=False, ShadowingPathLoss, every table route, pinned device_config coordinates float32 cannot hold."""
        k = self._balance_kernel()
        base, floor = k.base(base_sinr_db, self.num_cues), k.floor(floor_sinr_db, self.num_cues)
        margins, adj = k.margins(margins_db), k.adjustable(adjustable)
        self._follow_torch_stream()
        return k.solve(self._t, base, margins, floor, adj, max_iters, out, self._stream_ptr, env_mask)

    def balance_sinr_actions(self, base_sinr_db=0.0, margins_db=None, floor_sinr_db=None, adjustable=None, max_iters: int = 64):
        """balance_sinr() as an action tensor, int32 [B, num_agents], ready for step(): every agent link stays on its RB (as the
        decoded planes hold it) at the balanced power, encoded rb * power levels + level (power_control.encode_actions); an agent
        link that is not adjustable repeats its last action.  Links on fixed actions (cue_actions='traffic') have no column.
        Composes with color_rbs_actions() or best_response_dynamics_actions(): one call picks RBs, the other picks powers."""
        power = self.balance_sinr(base_sinr_db, margins_db, floor_sinr_db, adjustable, max_iters)[0]
        first, p_min, levels = self._agent_power_levels()
        return power_control.encode_actions(self._t['rb'], power, p_min, levels, first)

    # ------------------------------------------------------------------ sum-capacity power ascent
    def _power_ascent_kernel(self):
        return self._kernel('_ascent', power_ascent, power_ascent.PowerAscent, lambda: (*self._class_bounds(), self._agent_links()))

    def power_ascent(self, adjustable=None, floor_sinr_db=None, start: str = 'held', min_gain_mbps: float = 0.0, max_rounds: int = 16,
                     out=None, env_mask=None):
        """The powers a coordinate ascent on the total capacity ends at, with the protected links kept above their SINR floors and
        positions and RBs as the last step left them: (power_dbm int32 [B, N], sinr_db float32 [B, N], capacity_mbps float32 [B, N],
        rounds int32 [B], moves int32 [B], converged uint8 [B]), a tuple with those names.

        A link is on an RB iff 0 <= rb < R; the group of RB r is the set of links on r in ascending link index; groups do not
        interact.  An adjustable link on an RB begins at its held power (start='held'), the lowest (start='min') or the highest
        (start='max') power of its class; every other link keeps its held power throughout.

        A turn of the adjustable link i on RB r, at the current power vector p: for every level q of i's class let p^q be p with
        p[i] = q, and sinr_m(q), cap_m(q) the float32 values evaluate() gives the member m of r's group for (rb, p^q), bit for bit.
        T(q) is the sum, in double, in ascending link index, of cap_m(q) over the group.  q is admissible iff q == p[i], or every
        member m of the group (i included) with a floor above -inf has sinr_m(q) >= floor[m] or sinr_m(p[i]) < floor[m] (float32
        comparisons, NaN compares false): a member already under its floor constrains nothing, as in assign_rbs_power(), and a
        member that meets its floor is never pushed under it.  best is the lowest admissible level whose T is maximal among the
        admissible levels (a NaN T is never chosen), and link i moves to best, at once, iff T(best) - T(p[i]) > min_gain_mbps.

        The adjustable links take turns in ascending link index, each seeing the moves made before its turn (Gauss-Seidel).  A
        round that moves nobody ends the ascent (converged 1, rounds = the rounds that moved a link); so do max_rounds rounds that
        each moved a link (converged 0, rounds == max_rounds).  moves counts the moves.  Groups are independent: rounds is the
        largest per-group count, moves the sum over the groups, converged 1 iff every group saw a quiet round.  Every move strictly
        raises its group's T, which is a function of the group's power vector alone, so no state repeats: termination is a
        property, and max_rounds only bounds the launch.  sinr_db and capacity_mbps are evaluate()'s planes for (rb, power_dbm), for
        every link.  All turns of an env run in one workgroup of ONE kernel launch (csrc/d2d_ascent.hip) out of LDS: a wave owns an
        RB group, its 64 lanes the power levels of the link whose turn it is.  One long group runs on one wave (G^2 pair
        evaluations per turn): that is the known limit.  Valid after reset() and after every step(), autoreset steps included, as
        power_control() is; with mobility= at the current positions.

        adjustable: bool [N], the links that take turns; None: every agent link.  Links on fixed actions (cue_actions='traffic')
        never move; neither does a link on no RB.  floor_sinr_db: None (no floors), a number, {'cue': x, 'due': y} or [N] values
        (array or tensor), dB; -inf: no floor for that link.  min_gain_mbps: finite, >= 0.  max_rounds: 1 .. 4096.  The bounds are
        the ones step() decodes, as in power_control(); a class of more than 64 power levels is refused.  env_mask: bool / uint8
        [B], envs whose entry is 0 keep their rows; None: all.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the six tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (power_dbm, sinr_db, capacity_mbps, rounds, moves, converged), contiguous
        int32 / float32 / float32 [B, N], int32 / int32 / uint8 [B] on the env's device.  Serves what power_control() serves, as far
        as an env fits the LDS of one workgroup; ValueError for export_actions=False, ShadowingPathLoss, every table route, pinned
        device_config coordinates float32 cannot hold."""
        k = self._power_ascent_kernel()
        adj, floor = k.adjustable(adjustable), k.floor(floor_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.solve(self._t, adj, floor, start, min_gain_mbps, max_rounds, out, self._stream_ptr, env_mask)

    def power_ascent_actions(self, adjustable=None, floor_sinr_db=None, start: str = 'held', min_gain_mbps: float = 0.0,
                             max_rounds: int = 16):
        """power_ascent() as an action tensor, int32 [B, num_agents], ready for step(): every agent link stays on its RB (as the
        decoded planes hold it) at the solved power, encoded rb * power levels + level (power_control.encode_actions); an agent
        link that is not adjustable repeats its last action.  Links on fixed actions (cue_actions='traffic') have no column.
        Composes with color_rbs_actions(), stable_rbs_actions() and best_response_dynamics_actions(): one call picks RBs, this one
        picks powers."""
        power = self.power_ascent(adjustable, floor_sinr_db, start, min_gain_mbps, max_rounds)[0]
        first, p_min, levels = self._agent_power_levels()
        return power_control.encode_actions(self._t['rb'], power, p_min, levels, first)

    # ------------------------------------------------------------------ sum-capacity RB ascent
    def _rb_ascent_kernel(self):
        return self._kernel('_rbascent', rb_ascent, rb_ascent.RbAscent, lambda: (self._agent_links(),))

    def rb_ascent(self, allowed=None, movable=None, floor_sinr_db=None, min_gain_mbps: float = 0.0, max_rounds: int = 16, out=None,
                  env_mask=None):
        """The RBs a cooperative local search on the total capacity ends at - a link moves to the RB where the TOTAL capacity gains
        most - with the protected links kept above their SINR floors and positions and powers as the last step left them: (rb int32
        [B, N], sinr_db float32 [B, N], capacity_mbps float32 [B, N], rounds int32 [B], moves int32 [B], converged uint8 [B]), a
        tuple with those names.  Only rb changes.

        A link is on an RB iff 0 <= rb < R; the group of RB r is the set of links on r in ascending link index.  A link is movable
        iff it is on an RB, `movable` marks it (None: the agent links; links on cue_actions='traffic' never move) and it has at
        least one allowed RB.

        A turn of the movable link i, currently on RB c, at the current assignment rb.  For an RB r let rb^r be rb with rb[i] = r,
        and sinr^r_m, cap^r_m the float32 values evaluate() gives link m for (rb^r, pwr), bit for bit.  Groups do not interact: for
        r != c, cap^c_m of a member of r is its value "without i", and cap^r_m of a member of c is its value "with i gone".  With(r)
        is the sum, in double, in ascending link index, of cap^r_m over group(r) and i; Without(r) is the same sum over group(r)
        less i with i not on r (for r != c of cap^c_m, for r == c of cap^r'_m for any r' != c; an empty sum is 0.0).  D(r) =
        With(r) - Without(r), one double subtraction, is what link i's presence on r is worth to the total.  r is a candidate iff
        r != c, allowed[i][r] and r is admissible; r is admissible iff every m of group(r) and i with a floor above -inf has
        sinr^r_m >= floor[m] or sinr^c_m < floor[m] (float32 comparisons, NaN compares false): a link already under its floor
        constrains nothing, a link that meets its floor is never pushed under it - the rule of power_ascent() and
        assign_rbs_power() - and leaving c constrains nothing.  best is the lowest candidate r whose D(r) is maximal among the
        candidates (a NaN D is never chosen), and link i moves to best, at once, iff D(best) - D(c) > min_gain_mbps (a double
        subtraction and comparison; a NaN does not move).

        The movable links take turns in ascending link index, each seeing the moves made before its turn.  A round that moves
        nobody ends the ascent (converged 1, rounds = the rounds that moved a link); so do max_rounds rounds that each moved a link
        (converged 0, rounds == max_rounds).  Termination is a property: rounding is monotone, so a move implies With(best) -
        Without(best) > With(c) - Without(c) in exact arithmetic over the double group sums; each group sum is a pure function of
        the group's membership, so the exact sum of the group totals strictly rises on every move and no assignment repeats.
        max_rounds only bounds the launch.  sinr_db and capacity_mbps are evaluate(rb, pwr)'s planes for every link, a link on no
        RB included.  All turns of an env run in one workgroup of ONE kernel launch (csrc/d2d_rbascent.hip) out of LDS: lanes own
        RBs, membership is a bitset.  A lane with a long group does G^2 pair evaluations while the others wait: that is the known
        limit.  With one RB nobody has a candidate: moves 0, converged 1.  Alternate with power_ascent() to move RBs and powers in
        turn.  Valid after reset() and after every step(), autoreset steps included, as best_response_dynamics() is.

        allowed: bool [N, R] (tensor or array) as best_rb() takes it; None: every RB.  movable: bool [N]; None: every agent link.
        floor_sinr_db: None (no floors), a number, {'cue': x, 'due': y} or [N] values (array or tensor), dB; -inf: no floor for
        that link.  min_gain_mbps: finite, >= 0.  max_rounds: 1 .. 4096.  env_mask: bool / uint8 [B], envs whose entry is 0 keep
        their rows; None: all.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the six tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (rb, sinr_db, capacity_mbps, rounds, moves, converged), contiguous int32 /
        float32 / float32 [B, N], int32 / int32 / uint8 [B] on the env's device.  Serves what power_ascent() serves, as far as an
        env's links, allowed words and RB membership fit the LDS of one workgroup; ValueError for export_actions=False,
        ShadowingPathLoss, every table route, pinned device_config coordinates float32 cannot hold."""
        k = self._rb_ascent_kernel()
        mov, floor = k.movable(movable), k.floor(floor_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.solve(self._t, allowed, mov, floor, min_gain_mbps, max_rounds, out, self._stream_ptr, env_mask)

    def rb_ascent_actions(self, allowed=None, movable=None, floor_sinr_db=None, min_gain_mbps: float = 0.0, max_rounds: int = 16):
        """rb_ascent() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its solved RB at its
        current power level (as the decoded planes hold it), encoded rb * power levels + level
        (best_response_dynamics.encode_actions).  Links on fixed actions (cue_actions='traffic') have no column.  Composes with
        power_ascent_actions(): one call picks RBs, the other picks powers."""
        rb = self.rb_ascent(allowed, movable, floor_sinr_db, min_gain_mbps, max_rounds)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    # ------------------------------------------------------------------ queue-aware goodput ascent
    def _goodput_ascent_kernel(self):
        return self._kernel('_goodput', goodput_ascent, goodput_ascent.GoodputAscent, lambda: (*self._class_bounds(), self._agent_links()))

    def goodput_ascent(self, demand_bits=None, weight=None, bits_per_mbps=None, move=('rb', 'power'), allowed=None, movable=None,
                       floor_sinr_db=None, min_gain_bits: int = 0, max_rounds: int = 16, out=None, env_mask=None):
        """The RBs and powers a local search on the weighted bits the links can DELIVER ends at - the baseline of
        GoodputRewardFunction, and with backlog weights the max-weight scheduler - with the protected links kept above their SINR
        floors and positions as the last step left them: (rb int32 [B, N], power_dbm int32 [B, N], sinr_db float32 [B, N],
        capacity_mbps float32 [B, N], served_bits int32 [B, N], value int64 [B], rounds int32 [B], moves int32 [B], converged uint8
        [B]), a tuple with those names.  Every decision compares integers: no float ordering enters any choice.

        For a state s = (rb, pwr): cap_m(s) and sinr_m(s) are the float32 values evaluate() gives link m, bit for bit.  budget(c) is
        the packet queues' rule (include/d2d_queue.h, rule 5): floor(double(c) * bits_per_mbps) clipped to [0, 2^31 - 1]; a NaN,
        negative or zero capacity gives 0, +inf gives 2^31 - 1.  served_m(s) = min(budget(cap_m(s)), demand_m), term_m(s) =
        int64(weight_m) * served_m(s), and V(s) is the sum of term_m(s) over ALL links - those that never move and those on no RB
        included.  V stays below 2^62, so int64 sums are exact and order-free.

        A link takes turns iff it is on an RB (0 <= rb < R), `movable` marks it (None: the agent links; links on
        cue_actions='traffic' never move) and, with move=('rb',) only, it has an allowed RB.  A turn of link i, on RB c at power p,
        works on the candidate states s' that differ from s in link i alone: with 'rb' in move, (r, p) for every r != c with
        allowed[i][r]; with 'power' in move, (c, q) for every level q != p of the link's class.  A turn changes the RB or the
        power, never both.  Delta(s') = V(s') - V(s); only the members of c's group, of r's group and link i contribute.  s' is
        admissible iff every such member m with a floor above -inf has sinr_m(s') >= floor[m] or sinr_m(s) < floor[m] (float32
        comparisons, NaN compares false) - the rule of power_ascent() and rb_ascent(), for both kinds of candidate.  best is the
        admissible candidate of maximal Delta, ties to the lowest power, then to the lowest RB, and link i moves to best, at once,
        iff Delta(best) > min_gain_bits.

        The links take turns in ascending link index, each seeing the moves made before its turn.  A round that moves nobody ends
        the ascent (converged 1, rounds = the rounds that moved a link); so do max_rounds rounds that each moved a link (converged
        0, rounds == max_rounds).  Every move raises the integer V by at least 1 and V is bounded, so no state repeats: max_rounds
        only bounds the launch.  sinr_db and capacity_mbps are evaluate(rb, power_dbm)'s planes for every link; value is V of the
        final state.  All turns of an env run in one workgroup of ONE kernel launch (csrc/d2d_goodput.hip) out of LDS: the
        candidates of a turn are one flat list dealt over the threads, RBs first, then levels.  A thread with a long group does G^2
        pair evaluations while the others wait: that is the known limit.  Valid after reset() and after every step(), autoreset
        steps included, as rb_ascent() is.

        demand_bits, weight: ints - a scalar, [N] or [B, N] values (array or tensor), broadcast.  demand_bits None: on an env with
        traffic= the live backlog_bits plane of queues(), as it is when the launch runs; a negative value counts as 0.  weight
        None: 1; values in [0, 2^20] (host values are checked; a tensor is not read on the host, and the kernel takes a larger
        word as 2^20).  bits_per_mbps None: traffic.bits_per_mbps_step.  On an env without traffic= both demand_bits and
        bits_per_mbps must be given.  move: 'rb', 'power' or both.  allowed: bool [N, R] as best_rb() takes it; None: every RB.
        movable: bool [N]; None: every agent link.  floor_sinr_db: None (no floors), a number, {'cue': x, 'due': y} or [N]
        values, dB; -inf: no floor for that link.  min_gain_bits: an int in [0, 2^62), in weighted bits.  max_rounds: 1 .. 4096.
        The power bounds are the ones step() decodes; a class of more than 64 power levels is refused.  env_mask: bool / uint8
        [B], envs whose entry is 0 keep their rows; None: all.

        Recipes.  The goodput baseline: the defaults on a traffic env - weight 1, demand the backlog.  Classic max-weight
        scheduling: weight = backlog_bits >> k, scaled into [0, 2^20], with demand_bits = 2^31 - 1 (uncapped).

        Two limits.  The prediction uses the backlog as it is now: bits that arrive or expire before the next service are not in
        it.  A link with nothing to send still transmits, because the step has no off state: "muting" a link means its lowest
        power level, which is where ties send it.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the nine tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (rb, power_dbm, sinr_db, capacity_mbps, served_bits, value, rounds, moves,
        converged), contiguous int32 / int32 / float32 / float32 / int32 [B, N], int64 / int32 / int32 / uint8 [B] on the env's
        device.  Serves what rb_ascent() serves, as far as an env fits the LDS of one workgroup (96 bytes per link and the RB
        membership); ValueError for export_actions=False, ShadowingPathLoss, every table route, pinned device_config coordinates
        float32 cannot hold."""
        k = self._goodput_ascent_kernel()
        if self._queues is None and (demand_bits is None or bits_per_mbps is None):
            raise ValueError('goodput_ascent() on an env without traffic= needs demand_bits and bits_per_mbps: there is no backlog '
                             'plane and no step length to take them from')
        if demand_bits is None:
            demand_bits = self._queues.backlog_bits
        if bits_per_mbps is None:
            bits_per_mbps = self._t['traffic'].bits_per_mbps_step
        mov, floor = k.movable(movable), k.floor(floor_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.solve(self._t, demand_bits, weight, bits_per_mbps, move, allowed, mov, floor, min_gain_bits, max_rounds, out,
                       self._stream_ptr, env_mask)

    def goodput_ascent_actions(self, demand_bits=None, weight=None, bits_per_mbps=None, move=('rb', 'power'), allowed=None, movable=None,
                               floor_sinr_db=None, min_gain_bits: int = 0, max_rounds: int = 16):
        """goodput_ascent() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its solved RB at its
        solved power, encoded rb * power levels + level (power_control.encode_actions, the encoder of power_ascent_actions(), on
        the solved RBs where rb_ascent_actions() puts them).  Links on fixed actions (cue_actions='traffic') have no column.  One
        call picks RBs and powers: no alternation of rb_ascent_actions() and power_ascent_actions() through step()."""
        res = self.goodput_ascent(demand_bits, weight, bits_per_mbps, move, allowed, movable, floor_sinr_db, min_gain_bits, max_rounds)
        first, p_min, levels = self._agent_power_levels()
        return power_control.encode_actions(res[0], res[1], p_min, levels, first)

    # ------------------------------------------------------------------ unilateral-deviation gains
    def _deviation_kernel(self):
        return self._kernel('_deviation', deviation, deviation.Deviation, lambda: (*self._class_bounds(), self._agent_links()))

    def deviation_gains(self, links=None, allowed=None, floor_sinr_db=None, out=None, env_mask=None):
        """The whole counterfactual row of every selected link: what the env's total capacity would gain if link i ALONE had taken
        the action (RB r, power level l), for every r and every l of its alphabet, with positions and every other link as the last
        step left them: (gain_mbps float32 [B, M, R, Lmax], links int32 [M], levels int32 [M]).  It is the COMA / aristocrat-utility
        baseline, the table behind exploitability and regret (the joint action is a Nash point of the team game iff no row holds a
        positive entry) and, under SINR floors, an exact safe-action mask: a closed entry is -inf.  It is also the product
        neighbourhood, where an RB and a power change in one move, which no ascent of this package searches.

        A link is on an RB iff 0 <= rb < R; the group of RB r is the set of links on r in ascending link index.  For a selected link
        i on RB c at power p, an RB r and a power q = p_min[i] + l: s^(r,q) is the held state with rb[i] = r, pwr[i] = q, and
        cap_m(.), sinr_m(.) are the float32 values evaluate() gives link m for a state, bit for bit.  With(r,q) is the sum, in
        double, in ascending link index, of cap_m(s^(r,q)) over group(r) and i; Without(r) is the same sum over group(r) less i
        with i on no RB (an empty sum is 0.0).  D(r,q) = With(r,q) - Without(r) is what link i's presence on r at q is worth to
        the total, and gain(r,q) = D(r,q) - D(c,p), each one double subtraction: gain(c,p) is +0.0 exactly, and because groups do
        not interact gain(r,q) is, in exact arithmetic, the change of the env's total capacity when link i alone plays (r,q).
        (r,q) is admissible iff it is (c,p), or every m of group(r) and i with a floor above -inf has sinr_m(s^(r,q)) >= floor[m]
        or sinr_m(s) < floor[m] (float32 comparisons, NaN compares false): a link already under its floor constrains nothing, a
        link that meets its floor is never pushed under it - the rule of rb_ascent() and goodput_ascent() - and leaving c
        constrains nothing.  An entry is open iff l < L_i (the levels of link i's class), allowed[i][r] (the held RB c is open
        whatever `allowed` says), it is admissible and link i is on an RB.  A closed entry is -inf, an open one gain(r,q) rounded
        once to float32; a NaN stays NaN.

        The innermost two axes are in step()'s action order rb * levels + level: where the selected links share one class,
        gain_mbps.view(B, M, R * Lmax) is indexed by the action itself.  Lmax is the largest L_i of the selection; a link of fewer
        levels has its last Lmax - L_i columns closed.  `levels` is L_i per selected link, `links` the selection.

        Every entry is independent: B M R Lmax of them in ONE kernel launch (csrc/d2d_deviate.hip), one env served by several
        workgroups that each stage it in LDS, the entries dealt flat over the threads so that the table leaves in full rows.  An
        entry with a long group costs G^2 pair evaluations: that is the known limit.  Valid after reset() and after every step(),
        autoreset steps included, as rb_ascent() is.

        links: None (every agent link), or ascending, distinct link indices (a list or an array of ints); links on fixed actions
        (cue_actions='traffic') are never selected and may not be named.  allowed: bool [N, R] (tensor or array) as best_rb()
        takes it; None: every RB.  floor_sinr_db: None (no floors), a number, {'cue': x, 'due': y} or [N] values (array or
        tensor), dB; -inf: no floor for that link.  env_mask: bool / uint8 [B], envs whose entry is 0 keep their rows; None: all.
        The power bounds are the ones step() decodes; a class of more than 64 power levels is refused, and so is a table of more
        than 8 GiB (4 B M R Lmax bytes; the text names the count): select fewer links, or take best_deviation().

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the table the env owns, rewritten by every
        call (clone it to keep it), or `out`, a contiguous float32 [B, M, R, Lmax] tensor on the env's device.  Serves what
        rb_ascent() serves, as far as an env's links, allowed words and RB membership fit the LDS of one workgroup (80 bytes per
        link); ValueError for export_actions=False, ShadowingPathLoss, every table route, pinned device_config coordinates float32
        cannot hold."""
        k = self._deviation_kernel()
        floor = k.floor(floor_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.gains(self._t, links, allowed, floor, out, self._stream_ptr, env_mask)

    def best_deviation(self, links=None, allowed=None, floor_sinr_db=None, min_gain_mbps: float = 0.0, out=None, env_mask=None):
        """Every selected link's best unilateral deviation and the env's regret, without the table of deviation_gains(): (rb int32
        [B, N], power_dbm int32 [B, N], gain_mbps float64 [B, N], regret_mbps float64 [B], leader int32 [B]), a tuple with those
        names.

        With gain(r,q) and "open" as deviation_gains() words them: best is the open entry other than the held (c,p) of maximal
        double gain, ties to the lowest power, then to the lowest RB (goodput_ascent()'s rule); a NaN is never chosen.  If
        gain(best) > min_gain_mbps, (rb, power_dbm)[b, i] = best and gain_mbps[b, i] = gain(best), the double, not rounded to
        float32; else the held (c,p) with 0.0.  A link that is not selected keeps (rb, pwr) with 0.0.  regret_mbps[b] is the
        largest gain_mbps of the env - 0.0 at a Nash point of the team game, as far as min_gain_mbps and the floors let a link
        move - and leader[b] the lowest link that has it, -1 when nobody would move.  Every choice is a reduction of integer keys:
        two calls give the same words.

        links, allowed, floor_sinr_db, env_mask: as deviation_gains() takes them.  min_gain_mbps: finite, >= 0.

        Torch path only: two launches (csrc/d2d_deviate.hip: the entries, then one workgroup per env for regret and leader) on
        torch's current stream, nothing is synchronised; the five tensors the env owns, rewritten by every call (clone them to
        keep them), or `out` = (rb, power_dbm, gain_mbps, regret_mbps, leader), contiguous int32 / int32 / float64 [B, N], float64
        / int32 [B] on the env's device.  Serves what deviation_gains() serves."""
        k = self._deviation_kernel()
        floor = k.floor(floor_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.best(self._t, links, allowed, floor, min_gain_mbps, out, self._stream_ptr, env_mask)

    def best_deviation_actions(self, links=None, allowed=None, floor_sinr_db=None, min_gain_mbps: float = 0.0):
        """One STEEPEST-ASCENT step as an action tensor, int32 [B, num_agents], ready for step(): in every env only the `leader` of
        best_deviation() takes its best (rb, power) and every other agent link repeats its current action (as the decoded planes
        hold it), encoded rb * power levels + level (power_control.encode_actions).  An env whose leader is -1 repeats its
        actions.  On an env without mobility the step raises the total capacity by regret_mbps; repeated, it ends at regret 0.
        Links on fixed actions (cue_actions='traffic') have no column."""
        res = self.best_deviation(links, allowed, floor_sinr_db, min_gain_mbps)
        moves = torch.arange(self.num_links, device=self.device, dtype=torch.int32)[None, :] == res.leader[:, None]
        rb = torch.where(moves, res.rb, self._t['rb'])
        power = torch.where(moves, res.power_dbm, self._t['pwr'])
        first, p_min, levels = self._agent_power_levels()
        return power_control.encode_actions(rb, power, p_min, levels, first)

    # ------------------------------------------------------------------ sequential best-response dynamics
    def _best_response_dynamics_kernel(self):
        return self._kernel('_brdyn', best_response_dynamics, best_response_dynamics.BestResponseDynamics,
                            lambda: (self._agent_links(),))

    def best_response_dynamics(self, allowed=None, movable=None, min_gain_db: float = 3.0, max_rounds: int = 16, out=None,
                               env_mask=None):
        """Sequential (Gauss-Seidel) best response on the RBs, with positions and powers as the last step left them: (rb int32
        [B, N], sinr_db float32 [B, N], rounds int32 [B], moves int32 [B], converged uint8 [B]), a tuple with those names.

        Round after round the movable links take turns in ascending link index.  A link evaluates the SINR it would have on every
        allowed RB with every other link where it is NOW - the moves of this round included - picks the best one as best_rb() does
        (equal values to the lowest r) and moves there at once if that gains more than min_gain_db over its own RB.  A round that
        moves nobody ends the dynamics (converged 1, rounds = the rounds that moved a link); so do max_rounds rounds that each moved
        one (converged 0, rounds == max_rounds; max_rounds = 0 returns the RBs as they are).  Every value is a value of sense() for
        that state bit for bit, so the whole trajectory is what a loop of best_rb() and step() per link would give; sinr_db is the
        step's sinr_db for rb, NaN for a link on no RB.  Selfish SINR response is no potential game: without hysteresis envs can
        cycle until the cap, and converged is a result, not a promise.  All turns of an env run in one workgroup of one kernel
        launch (csrc/d2d_brdyn.hip) out of LDS.  Valid after reset() and after every step(), autoreset steps included, as sense() is.

        allowed: bool [N, R] (tensor or array) as best_rb() takes it; None: every RB.  movable: bool [N], the links that take
        turns; None: every agent link.  Links on fixed actions (cue_actions='traffic') never move; neither does a link on no RB
        (rb outside [0, R)), a link with no allowed RB, or a link whose gain is NaN; links that do not move still interfere, unless
        they are on no RB.  min_gain_db >= 0.  env_mask: bool / uint8 [B], envs whose entry is 0 keep their rows; None: all.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the five tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (rb, sinr_db, rounds, moves, converged), contiguous int32 / float32 [B, N],
        int32 / int32 / uint8 [B] on the env's device.  Serves what sense() serves, as far as an env's links, allowed words and RB
        membership fit the LDS of one workgroup; ValueError for export_actions=False, ShadowingPathLoss, every table route, pinned
        device_config coordinates float32 cannot hold."""
        k = self._best_response_dynamics_kernel()
        mov = k.movable(movable)
        self._follow_torch_stream()
        return k.solve(self._t, allowed, mov, min_gain_db, max_rounds, out, self._stream_ptr, env_mask)

    def best_response_dynamics_actions(self, allowed=None, movable=None, min_gain_db: float = 3.0, max_rounds: int = 16):
        """best_response_dynamics() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its solved RB
        at its current power level (as the decoded planes hold it), encoded rb * power levels + level.  Links on fixed actions
        (cue_actions='traffic') have no column.  Composes with power_control_actions() the way best_response_actions() does: one
        call picks RBs, the other picks powers."""
        rb = self.best_response_dynamics(allowed, movable, min_gain_db, max_rounds)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    # ------------------------------------------------------------------ what-if evaluation of candidate joint actions
    def _evaluate_kernel(self):
        return self._kernel('_evaluate', evaluate_mod, evaluate_mod.Evaluate)

    def evaluate(self, rb, power_dbm, planes=('sinr_db', 'capacity_mbps'), out=None):
        """What K complete joint assignments per env would give, at the current positions: a dict with 'total_mbps' float32 [B, K]
        and the requested planes float32 [B, K, N].

        rb, power_dbm: contiguous int32 [B, K, N] tensors on the env's device, candidate k of env b as the decoded planes step()
        exports (info['rb'], info['pwr']) would hold it; K >= 1 is free and may change from call to call.  sinr_db[b, k] and
        capacity_mbps[b, k] are, bit for bit, the planes a step() with that assignment exports at these positions, and
        total_mbps[b, k] is the sum of capacity_mbps[b, k] over the links, accumulated in double in a fixed order (two calls give
        the same bits).  One kernel launch (csrc/d2d_evaluate.hip): a workgroup stages an env once and evaluates a chunk of its
        candidates out of LDS.  planes: which of 'sinr_db', 'capacity_mbps' to write; () gives the totals only and writes no
        [B, K, N] block.  An rb outside [0, num_rbs) is outside the contract (the link is on no RB, as in marginal_capacity()).

        The env is left untouched: no counter, plane, queue, position or reward changes.  Valid after reset() and after every
        step(), autoreset steps included.  With mobility= the evaluation is at the CURRENT positions, whereas the next step() moves
        the devices first: equality with the next step's planes holds without mobility only.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the tensors the env owns, reallocated when K
        changes and rewritten by every call (clone them to keep them), or `out`, a dict of contiguous float32 tensors with exactly
        the returned keys and shapes.  Serves what best_rb() serves; ValueError for export_actions=False, ShadowingPathLoss, every
        table route, pinned device_config coordinates float32 cannot hold."""
        k = self._evaluate_kernel()
        self._follow_torch_stream()
        return k.planes(self._t, rb, power_dbm, planes, out, self._stream_ptr)

    def evaluate_actions(self, actions, planes=('sinr_db', 'capacity_mbps')):
        """evaluate() of K candidate action sets: actions is an integer tensor [B, K, num_agents], every [:, k] in the layout step()
        takes (rb * power levels + level).  Links on fixed actions (cue_actions='traffic') have no column and keep their current
        rb / power in every candidate.  Decoded by evaluate.decode_actions; the result and its validity are evaluate()'s."""
        k = self._evaluate_kernel()
        if not torch.is_tensor(actions) or actions.ndim != 3 or tuple(actions.shape[::2]) != (self.num_envs, self.num_agents) \
                or actions.device != self.device:
            raise ValueError(f'actions must be an integer tensor [{self.num_envs}, K, {self.num_agents}] (env, candidate, agent) on '
                             f'{self.device}')
        levels = self._agent_levels()
        first = self.num_links - self.num_agents
        self._follow_torch_stream()
        fixed = (self._t['rb'][:, :first], self._t['pwr'][:, :first]) if first else (None, None)
        rb, pwr = evaluate_mod.decode_actions(actions, levels, *fixed)
        return k.planes(self._t, rb, pwr, planes, None, self._stream_ptr)

    # ------------------------------------------------------------------ what-if evaluation on a path-loss table
    def _table_evaluate_kernel(self):
        return self._kernel('_table_evaluate', table_evaluate_mod, table_evaluate_mod.TableEvaluate)

    def evaluate_table(self, rb, power_dbm, table=None, planes=('sinr_db', 'capacity_mbps'), out=None):
        """evaluate() for the envs whose step reads a path-loss TABLE: what K complete joint assignments per env would give when
        the step reads `table` - a dict with 'total_mbps' float32 [B, K], 'domain' int32 [B, K] and the requested planes float32
        [B, K, N].

        rb, power_dbm, planes: as evaluate() takes them (contiguous int32 [B, K, N] in the units of info['rb'] / info['tx_pwr_dbm'];
        K >= 1 is free per call; an rb outside [0, num_rbs) puts the link on no RB).  sinr_db[b, k] and capacity_mbps[b, k] are,
        bit for bit, the planes a step() with that assignment exports when it reads that table; total_mbps[b, k] is evaluate()'s
        total, the sum of capacity_mbps[b, k] accumulated in double in a fixed order (two calls give the same bits).  domain[b, k]
        is 1 iff an entry read for that candidate - every link's own entry [i, i] and entry [j, i] of every pair on one RB - is NaN
        or -inf (the step's D2D_FLAG_PATH_LOSS_DOMAIN, raised only where read); +inf is a legal entry (gain 0); the planes of a
        flagged candidate are whatever the arithmetic gives.  One kernel launch (csrc/d2d_evaltab.hip).

        table=None: the env's live table AS IT STANDS, that is, the channel realisation of the last step() (or of reset()'s own
        step).  Served on every route that has one: 'channel' (SpatialChannelPathLoss), 'per_step' (a per-step ArrayPathLoss), and
        'array' when compute() returned the SNR row; ValueError on any other route, which names table=.  "As it stands" means:
        with fading the next step() draws again, with mobility= the next step() moves the devices first, and after an autoreset
        step the block of an env that was reset is its NEW layout's - in each of these the next step's planes are another
        realisation's.  With fading=None and nothing moving the table IS the next step's and the prediction is exact.

        table=: a contiguous float32 or float64 tensor [B, N, N] or [B, N+1, N] on the env's device, in dB by (tx link, rx link).
        Works on every route, native models included, and with export_actions=False: the hook for Monte-Carlo over fading draws
        of one's own and for scoring under a measured channel.  Row N is never read (it feeds snr_db only); SINR and capacity use
        the signal entry [i, i].

        The env is left untouched: no counter, plane, queue, position or table word changes.  Torch path only: enqueued on torch's
        current stream, nothing is synchronised; the tensors the env owns, reallocated when K changes and rewritten by every call
        (clone them to keep them), or `out`, a dict of contiguous tensors with exactly the returned keys and shapes (float32,
        domain int32)."""
        k = self._table_evaluate_kernel()
        self._follow_torch_stream()
        return k.planes(rb, power_dbm, table, planes, out, self._stream_ptr)

    def evaluate_table_actions(self, actions, table=None, planes=('sinr_db', 'capacity_mbps')):
        """evaluate_table() of K candidate action sets: actions is an integer tensor [B, K, num_agents], every [:, k] in the layout
        step() takes (rb * power levels + level).  Links on fixed actions (cue_actions='traffic') have no column and keep their
        current rb / power in every candidate: with such links - and only then - the env must export its decoded planes
        (export_actions=True), ValueError otherwise.  Decoded by evaluate.decode_actions; the result and its validity are
        evaluate_table()'s."""
        k = self._table_evaluate_kernel()
        if not torch.is_tensor(actions) or actions.ndim != 3 or tuple(actions.shape[::2]) != (self.num_envs, self.num_agents) \
                or actions.device != self.device:
            raise ValueError(f'actions must be an integer tensor [{self.num_envs}, K, {self.num_agents}] (env, candidate, agent) on '
                             f'{self.device}')
        first = self.num_links - self.num_agents
        if first:
            why = table_evaluate_mod.fixed_links_refusal(self.simulator, self.export_actions)
            if why:
                raise ValueError(why)
        levels = self._agent_levels()
        self._follow_torch_stream()
        fixed = (self._t['rb'][:, :first], self._t['pwr'][:, :first]) if first else (None, None)
        rb, pwr = evaluate_mod.decode_actions(actions, levels, *fixed)
        return k.planes(rb, pwr, table, planes, None, self._stream_ptr)

    # ------------------------------------------------------------------ sum-capacity RB ascent on a path-loss table
    def _table_rb_ascent_kernel(self):
        return self._kernel('_table_rbascent', table_rb_ascent_mod, table_rb_ascent_mod.TableRbAscent, lambda: (self._agent_links(),))

    def rb_ascent_table(self, table=None, rb=None, power_dbm=None, allowed=None, movable=None, floor_sinr_db=None,
                        min_gain_mbps: float = 0.0, max_rounds: int = 16, out=None, env_mask=None):
        """rb_ascent() for the envs whose step reads a path-loss TABLE: the RBs a cooperative local search on the total capacity ends
        at when the step reads `table` - (rb int32 [B, N], sinr_db float32 [B, N], capacity_mbps float32 [B, N], rounds int32 [B],
        moves int32 [B], converged uint8 [B], domain int32 [B]), a tuple with those names.  Only rb changes.

        The statement is rb_ascent()'s, steps and round rule, with one substitution: sinr^r_m and cap^r_m are the float32 values
        evaluate_table() gives link m for (rb^r, pwr) on `table`, bit for bit.  A link is on an RB iff 0 <= rb < R; the group of RB r
        is the set of links on r in ascending link index; a link is movable iff it is on an RB, `movable` marks it (None: the agent
        links; links on cue_actions='traffic' never move) and it has at least one allowed RB.  In the turn of the movable link i on
        RB c, With(r) is the sum, in double, in ascending link index, of cap^r_m over group(r) and i, Without(r) the same sum over
        group(r) less i with i not on r, D(r) = With(r) - Without(r); r is a candidate iff r != c, allowed[i][r] and every m of
        group(r) and i with a floor above -inf has sinr^r_m >= floor[m] or sinr^c_m < floor[m] (float32, NaN compares false); best is
        the lowest candidate whose D is maximal (a NaN D is never chosen) and link i moves to it, at once, iff D(best) - D(c) >
        min_gain_mbps (a NaN does not move).  The movable links take turns in ascending link index; a round that moves nobody ends
        the ascent (converged 1), and so do max_rounds rounds that each moved a link (converged 0).  Termination is rb_ascent()'s
        property.  sinr_db and capacity_mbps are evaluate_table(rb, pwr, table)'s planes for every link, a link on no RB included.

        table: exactly what evaluate_table() takes.  None: the env's live table AS IT STANDS, the channel realisation of the last
        step() - served on the 'channel' and 'per_step' routes and on 'array' with an SNR row, ValueError on any other route, which
        names table=; with fading the next step() draws again, with mobility= it moves first (see evaluate_table()).  A tensor:
        contiguous float32 or float64 [B, N, N] or [B, N+1, N] on the env's device, in dB by (tx link, rx link), on every route,
        native models and ShadowingPathLoss included; row N is never read.

        rb, power_dbm: the start state, contiguous int32 [B, N] in the units of info['rb'] / info['tx_pwr_dbm'].  None: the decoded
        planes of the last step, which needs export_actions=True (ValueError otherwise, naming rb= and power_dbm=); given
        explicitly they work with export_actions=False.

        domain[b] is 1 iff ANY entry [j, i] with j, i < N of env b's block is NaN or -inf - the whole block, not "where read": a
        trajectory may read any pair.  +inf is a legal entry (gain 0).  The other outputs of a flagged env are whatever the
        arithmetic gives.

        allowed, movable, floor_sinr_db, min_gain_mbps, max_rounds, env_mask (envs whose entry is 0 keep all seven rows), out:
        rb_ascent()'s meaning, checks and limits.  Two kernel launches (csrc/d2d_tabascent.hip): the table is converted once into
        float32 linear gains, receiver-major, in a work space the env owns - 4 B N N bytes, allocated by the first call and kept:
        4.3 GB at 4096 envs x 512 links - and all turns of an env then run in one workgroup out of LDS, the pair gains read from
        that block.  A lane with a long group does G^2 pair loads while the others wait: that is the known limit.

        The env is left untouched.  Torch path only: enqueued on torch's current stream, nothing is synchronised; the seven tensors
        the env owns, rewritten by every call (clone them to keep them), or `out` = (rb, sinr_db, capacity_mbps, rounds, moves,
        converged, domain), contiguous int32 / float32 / float32 [B, N], int32 / int32 / uint8 / int32 [B] on the env's device.
        ValueError for shapes whose links, allowed words and RB membership exceed the LDS of one workgroup, with the byte count."""
        k = self._table_rb_ascent_kernel()
        if (rb is None or power_dbm is None) and not self.export_actions:
            raise ValueError(table_rb_ascent_mod.no_start_state())
        rb = self._t['rb'] if rb is None else k.start(rb, 'rb')
        pwr = self._t['pwr'] if power_dbm is None else k.start(power_dbm, 'power_dbm')
        mov, floor = k.movable(movable), k.floor(floor_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.solve(table, rb, pwr, allowed, mov, floor, min_gain_mbps, max_rounds, out, self._stream_ptr, env_mask)

    def rb_ascent_table_actions(self, table=None, allowed=None, movable=None, floor_sinr_db=None, min_gain_mbps: float = 0.0,
                                max_rounds: int = 16):
        """rb_ascent_table() from the decoded planes of the last step as an action tensor, int32 [B, num_agents], ready for step():
        every agent link on its solved RB at its current power level (as the decoded planes hold it), encoded rb * power levels +
        level (best_response_dynamics.encode_actions).  Links on fixed actions (cue_actions='traffic') have no column.  Needs
        export_actions=True."""
        if not self.export_actions and self.use_torch:
            raise ValueError(table_rb_ascent_mod.no_start_state('rb_ascent_table_actions()'))
        rb = self.rb_ascent_table(table, None, None, allowed, movable, floor_sinr_db, min_gain_mbps, max_rounds)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    # ------------------------------------------------------------------ difference rewards on a path-loss table
    def _table_marginal_kernel(self):
        return self._kernel('_table_marginal', table_marginal_mod, table_marginal_mod.TableMarginal)

    def marginal_capacity_table(self, table=None, rb=None, power_dbm=None, out=None):
        """marginal_capacity() for the envs whose step reads a path-loss TABLE: what every link costs the others when the step reads
        `table` - (difference_mbps float32 [B, N], harm_mbps float32 [B, N], domain int32 [B]), a tuple with those names.

        harm_mbps[b, i] is the capacity the OTHER links of link i's RB would gain if link i alone went off the air - the sum over
        them of cap_j without i's transmitter minus cap_j with it, the `sinr > rx_sensitivity` threshold of the step included - and
        difference_mbps[b, i] = capacity_mbps[b, i] - harm_mbps[b, i], where capacity_mbps is evaluate_table()'s plane for (rb,
        power_dbm) on `table`, bit for bit (with the defaults: the last step's own capacity_mbps).  harm >= 0; a link alone on its
        RB, or on no RB (rb outside [0, num_rbs)), has harm == 0.0 and difference == capacity exactly.  domain[b] is 1 iff an entry
        read for env b's state - every link's own entry [i, i] and entry [j, i] of every pair on one RB - is NaN or -inf
        (evaluate_table()'s rule, per env); +inf is a legal entry (gain 0, harm 0); the planes of a flagged env are whatever the
        arithmetic gives.  One kernel launch (csrc/d2d_tabmarg.hip) that reads the table in place: no [B, N, N] work space.

        table: exactly what rb_ascent_table() takes.  None: the env's live table AS IT STANDS, the channel realisation of the last
        step() - served on the 'channel' and 'per_step' routes and on 'array' with an SNR row, ValueError on any other route, which
        names table=.  A tensor: contiguous float32 or float64 [B, N, N] or [B, N+1, N] on the env's device, in dB by (tx link, rx
        link), on every route, native models and ShadowingPathLoss included; row N is never read.

        rb, power_dbm: contiguous int32 [B, N] in the units of info['rb'] / info['tx_pwr_dbm'].  None: the decoded planes of the
        last step, which needs export_actions=True (ValueError otherwise, naming rb= and power_dbm=); given explicitly they work with
        export_actions=False.

        The env is left untouched.  Torch path only: enqueued on torch's current stream, nothing is synchronised; the three tensors
        the env owns, rewritten by every call (clone them to keep them), or `out` = (difference_mbps, harm_mbps, domain), contiguous
        float32 / float32 [B, N] and int32 [B] on the env's device that do not share memory.  marginal_capacity() itself keeps
        refusing the table routes."""
        k = self._table_marginal_kernel()
        if (rb is None or power_dbm is None) and not self.export_actions:
            raise ValueError(table_marginal_mod.no_start_state())
        rb = self._t['rb'] if rb is None else k.start(rb, 'rb')
        pwr = self._t['pwr'] if power_dbm is None else k.start(power_dbm, 'power_dbm')
        self._follow_torch_stream()
        return k.marginal(table, rb, pwr, out, self._stream_ptr)

    def _with_table_marginal(self, view):
        """The view plus difference_mbps / harm_mbps on the table the step just read, as a namespace of its own (_with_marginal's
        form): the cached view stays what every other consumer sees."""
        diff, harm, _ = self.marginal_capacity_table()
        return SimpleNamespace(**vars(view), difference_mbps=diff, harm_mbps=harm)

    # ------------------------------------------------------------------ optimal one-to-one RB matching
    def _assignment_kernel(self):
        return self._kernel('_assign', assignment, assignment.Assignment,
                            lambda: (self._agent_links(), self._due_links()))

    def assignment_weights(self, movable=None, allowed=None, objective: str = 'total', harm: bool = False, out=None):
        """What every movable link is worth on every RB, with the background as the last step left it: (weights float32 [B, M, R],
        links int32 [M]), and harm float32 [B, M, R] behind them if harm=True.

        movable: bool [N] (tensor or array), the same for every env; None: the DUE-pair links.  Row a is the a-th movable link in
        ascending link index, links[a].  A movable TENSOR is read on the host, here and in every call that takes `movable` as this
        one does (assign_rbs(), stable_rbs(), sharing_values(), share_rbs(), joint_assignment_weights(), assign_rbs_power() and
        their *_actions forms): the number of movable links shapes the outputs, so that form waits for what is queued before it.  Every other link is background: it stays on its current RB and power (an rb outside
        [0, R) is on no RB).  The movable links are taken off the air: their current RB plays no part, their current power is the
        power they are placed with.  own[b, a, r] is link a's capacity (Mbps, the step's definition) alone with the background
        members of r; harm[b, a, r] what those members lose to it, 0.0 exactly on an RB without them, a victim pushed under its
        sensitivity losing its whole capacity.  weights = own - harm under objective='total', own under objective='own' (bit for
        bit evaluate()'s capacity_mbps of link a for the candidate that puts a on r and every other movable link on rb -1);
        -inf where allowed (bool [N, R], as best_rb() takes it) forbids.  Movable links on DISTINCT RBs do not interfere with each
        other, so the total capacity of a one-to-one placement is evaluate(background) + the sum of its 'total' weights.

        One kernel launch (csrc/d2d_assign.hip).  The env is left untouched.  Valid after reset() and after every step(), autoreset
        and mobility included, as sense() is.  Torch path only: enqueued on torch's current stream, nothing is synchronised; the
        tensors the env owns (4 B M R bytes each, rewritten by every call), or `out`: one contiguous float32 [B, M, R] tensor, or
        (weights, harm) with harm=True.  ValueError for a `movable` that marks a link without an action column, and for what
        evaluate() refuses."""
        k = self._assignment_kernel()
        self._follow_torch_stream()
        return k.weights(self._t, movable, allowed, objective, harm, out, self._stream_ptr)

    def solve_assignment(self, weights, out=None):
        """The maximum-weight one-to-one matching of ANY float32 [B, M, R] tensor on the env's device, M <= R: (col int32 [B, M],
        value_mbps float32 [B], feasible uint8 [B]).  col[b, a] is the column row a takes, value_mbps[b] the matched weights summed
        in double in ascending row.  Entries that are not finite are never matched; an env without a complete matching is
        infeasible - feasible 0, every col -1, value 0.0 - and does not disturb the others.  One kernel launch (csrc/d2d_assign.hip):
        the shortest-augmenting-path method in double, one workgroup per env.  The env's own tensors, rewritten by every call, or
        `out` = (col, value_mbps, feasible).  M > R is a ValueError."""
        k = self._assignment_kernel()
        self._follow_torch_stream()
        return k.solve(weights, out, self._stream_ptr)

    def assign_rbs(self, movable=None, allowed=None, objective: str = 'total', out=None):
        """The one-to-one placement of the movable links that maximises the TOTAL capacity of the env (objective='total'; 'own':
        the movable links' own capacities), the background staying where it is: (rb int32 [B, N], value_mbps float32 [B],
        feasible uint8 [B]), a tuple with those names.

        rb is the current plane with every movable link on its matched RB, all distinct; an infeasible env (allowed leaves some
        link no RB of its own) keeps its row, with value 0.0.  Because the weights separate exactly over one-to-one placements
        (assignment_weights()), evaluate(rb)['total_mbps'] = evaluate(background) + value_mbps and no other such placement gives
        more: a certificate, not a heuristic.  Two kernel launches, assignment_weights() and solve_assignment(), and the scatter
        of the columns; the weights block, 4 B M R bytes, is owned by the env.  movable, allowed, validity and refusals as
        assignment_weights(); more movable links than RBs is a ValueError.  `out` = (rb, value_mbps, feasible)."""
        k = self._assignment_kernel()
        self._follow_torch_stream()
        return k.assign(self._t, movable, allowed, objective, out, self._stream_ptr)

    def assign_rbs_actions(self, movable=None, allowed=None, objective: str = 'total'):
        """assign_rbs() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its RB of assign_rbs() at
        its current power level, encoded rb * power levels + level.  Links on fixed actions (cue_actions='traffic') have no
        column.  Composes with power_control_actions() the way best_response_dynamics_actions() does."""
        rb = self.assign_rbs(movable, allowed, objective)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    # ------------------------------------------------------------------ stable RB matching with quotas
    def _stable_kernel(self):
        return self._kernel('_stable', stable_matching, stable_matching.StableMatching, lambda: (self._assignment_kernel(),))

    def solve_stable_matching(self, link_pref, rb_pref, quota=1, out=None):
        """The link-optimal stable matching of ANY pair of contiguous float32 [B, M, R] tensors (env, row = link, column = RB; higher
        is better) on the env's device, by Gale-Shapley deferred acceptance with the links proposing: (col int32 [B, M], load int32
        [B, R], proposals int32 [B], unmatched int32 [B]), a tuple with those names.

        A pair (a, r) is acceptable iff both its entries are finite.  Link a ranks its acceptable RBs by (link_pref descending, r
        ascending), RB r the links by (rb_pref descending, a ascending), in float32 comparisons (+0.0 ties with -0.0).  quota: the
        links an RB can hold - an int for every RB, [R] ints each in [0, M] (0: closed), or an int32 [R] tensor on the device.  col[b,
        a] is the RB of row a, -1 for an unmatched row; load[b, r] <= quota[r] the rows on r.  No acceptable pair blocks the result
        (a prefers r to its match, and r is under quota or prefers a to its worst holder), every link weakly prefers it to every
        other stable matching, and it is unique: any order of proposals reaches it and makes the same proposals, whose number is
        proposals[b].  An env without an acceptable pair has every col -1 and does not disturb the others.

        One kernel launch (csrc/d2d_stable.hip), one workgroup per env, every round inside it; integers only behind the
        comparisons: two calls give the same words.  Enqueued on torch's current stream, nothing is synchronised.  The env's own
        tensors, rewritten by every call, or `out` = (col, load, proposals, unmatched).  Refused as stable_rbs() is."""
        k = self._stable_kernel()
        self._follow_torch_stream()
        return k.solve(link_pref, rb_pref, quota, out, self._stream_ptr)

    def stable_rbs(self, movable=None, allowed=None, quota=1, rb_pref: str = 'harm', out=None):
        """The stable-matching baseline of the D2D-underlay literature: the movable links and the RBs (the base station acting for
        the background on each RB) rank each other, and the links are placed by solve_stable_matching(): (rb int32 [B, N],
        unmatched int32 [B], proposals int32 [B]), a tuple with those names.

        The preferences are the planes of ONE assignment_weights(objective='own', harm=True) launch: link_pref = own, what a link
        gets on an RB beside its background; rb_pref = -harm under rb_pref='harm' (the RB prefers whoever hurts its background
        least) or own - harm under 'total' (one float32 subtraction, assignment_weights(objective='total')).  A pair `allowed`
        forbids arrives as -inf and is unacceptable.  Then the matching launch and one scatter: a matched movable link goes to its
        RB, an unmatched one keeps its current RB and unmatched[b] counts it, background rows are copied through.  More movable
        links than RBs is no error: quota > 1 serves them, or they stay unmatched.

        What stability means here.  With quota = 1 the movable links end on distinct RBs and do not interfere with each other, so
        the preferences are the true capacities and stability is a statement about the env: no link and RB would both rather be
        together.  With quota > 1 the links that share an RB interfere with each other, which the fixed preferences ignore:
        stability then holds with respect to the stated tensors only, and evaluate() gives the truth.  Unlike assign_rbs() nothing
        is maximised; unlike best_response_dynamics() it always ends.  movable, allowed, validity and refusals as
        assignment_weights(), whose env-owned planes are rewritten, under the name stable_rbs().  `out` = (rb, unmatched,
        proposals)."""
        k = self._stable_kernel()
        self._follow_torch_stream()
        return k.rbs(self._t, movable, allowed, quota, rb_pref, out, self._stream_ptr)

    def stable_rbs_actions(self, movable=None, allowed=None, quota=1, rb_pref: str = 'harm'):
        """stable_rbs() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its RB of stable_rbs() at
        its current power level, encoded rb * power levels + level, as assign_rbs_actions() does."""
        rb = self.stable_rbs(movable, allowed, quota, rb_pref)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    # ------------------------------------------------------------------ exact optimal RB sharing for small link groups
    def _share_kernel(self):
        return self._kernel('_share', sharing, sharing.Sharing, lambda: (self._assignment_kernel(),))

    def sharing_values(self, movable=None, allowed=None, power_dbm=None, out=None):
        """What every RB is worth under every subset of the movable links, with the background as the last step left it: (values
        float64 [B, R, 2^M], links int32 [M], closed int32 [B]), a tuple with those names.

        movable: bool [N], the same for every env; None: the DUE-pair links, as assign_rbs() has it.  links holds them in ascending
        link index and bit a of a subset mask S is links[a]; M must be in 1 .. 12 (D2D_SHARE_MAX_MOVABLE).  Every other link is
        background: it stays on its RB (an rb outside [0, R) is on no RB and in no value) at its power.  power_dbm: int32 [B, N] on
        the env's device, in the decoded plane's units, replaces the powers of ALL links, as color_rbs() takes it; None: the
        decoded plane.  values[b, r, S] is the total capacity of RB r when exactly the movable links of S join r's background: the
        sum, in double, in ascending link index, of the float32 capacities of all those members, each of them bit for bit
        evaluate()'s - and so the step's - for that state.  values[b, r, 0] is the background of r alone.  allowed: bool [N, R] as
        best_rb() takes it; a subset with a link that is not allowed on r is -inf.  An RB whose background has more than 64
        members (D2D_SHARE_MAX_BACKGROUND) is closed: its S != 0 entries are -inf, its S = 0 entry is still its background's
        capacity, and closed[b] counts such RBs.

        Links on different RBs do not interfere, so the total capacity of ANY placement of the movable links, several per RB
        included, is the sum over the RBs of values[b, r, S_r], S_r the movable links placed on r.

        One kernel launch (csrc/d2d_share.hip), grid (env, RB), and one torch sum.  The env is left untouched.  Valid after reset()
        and after every step(), autoreset and mobility included.  Torch path only: enqueued on torch's current stream, nothing is
        synchronised; the block the env owns (8 B R 2^M bytes, rewritten by every call), or `out`, a contiguous float64 tensor of
        that shape.  ValueError for M outside 1 .. 12, for a block that with solve_sharing()'s choice words would exceed 8 GiB
        (D2D_SHARE_MAX_BLOCK_BYTES), and for what assign_rbs() refuses, under the name share_rbs()."""
        k = self._share_kernel()
        self._follow_torch_stream()
        return k.values(self._t, movable, allowed, power_dbm, out, self._stream_ptr)

    def solve_sharing(self, values, quota=None, out=None):
        """The optimal many-to-one placement under ANY contiguous float64 [B, R, 2^M] tensor on the env's device (env, RB, subset of
        the M rows): (col int32 [B, M], value float64 [B], feasible int32 [B]), a tuple with those names.

        The total of a placement is the sum over the RBs of values[b, r, S_r], S_r the rows placed on r.  The optimum is the
        max-plus subset convolution over the RBs: g[T] = max over S in T of g'[T - S] + values[b, r, S], RB after RB from g[0] = 0.
        An entry that is not finite (-inf, +inf, NaN) is never chosen.  quota: None (no limit), an int, [R] ints or an int32 [R]
        tensor; S may sit on r iff popcount(S) <= quota[r], 0 closes r to the rows.  Equal sums go to the numerically lowest S.
        col[b, a] is the RB of mask bit a.  An env that has no admissible placement is infeasible - every col -1, value 0.0, feasible
        0 - and does not disturb the others.  Every candidate is one double addition and max is exact: the result does not depend on
        the order of evaluation, two calls give the same words, and quota 1 gives solve_assignment()'s optimum.

        One kernel launch (csrc/d2d_share.hip), one workgroup per env, every RB inside it out of LDS, which is why M stops at 12.
        The choice words, 2 B R 2^M bytes, are owned by the env.  Enqueued on torch's current stream, nothing is synchronised.  The
        env's own tensors, rewritten by every call, or `out` = (col, value, feasible).  Refused as share_rbs() is."""
        k = self._share_kernel()
        self._follow_torch_stream()
        return k.solve(values, quota, out, self._stream_ptr)

    def share_rbs(self, movable=None, allowed=None, quota=None, power_dbm=None, out=None):
        """The placement of the movable links, SEVERAL PER RB ALLOWED, that maximises the total capacity of the env, the background
        staying where it is: (rb int32 [B, N], value_mbps float32 [B], feasible int32 [B], closed int32 [B]), a tuple with those
        names.

        Exact: sharing_values() holds the capacity of every RB under every subset of the movable links, mutual interference of the
        links that share it included, and solve_sharing() takes the best of all R^M placements - a certificate for color_rbs(),
        stable_rbs(quota > 1) and best_response_dynamics(), and an optimal "re-place these M <= 12 links" move.  rb is the current
        plane with every movable link on its optimal RB; an infeasible env (allowed, quota or closed RBs leave no placement) keeps
        its row, with value 0.0.  value_mbps is the env's TOTAL capacity under rb, float32 of the double optimum, comparable with
        evaluate(rb, power)['total_mbps'] (a background link on no RB is in neither).  Two kernel launches and the gather and
        scatter of the columns.  movable, allowed, power_dbm and closed as sharing_values(); quota as solve_sharing().  `out` =
        (rb, value_mbps, feasible, closed)."""
        k = self._share_kernel()
        self._follow_torch_stream()
        return k.rbs(self._t, movable, allowed, quota, power_dbm, out, self._stream_ptr)

    def share_rbs_actions(self, movable=None, allowed=None, quota=None, power_dbm=None):
        """share_rbs() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its RB of share_rbs() at
        its current power level, encoded rb * power levels + level, as assign_rbs_actions() does.  Composes with
        power_control_actions() the same way."""
        rb = self.share_rbs(movable, allowed, quota, power_dbm)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    # ------------------------------------------------------------------ joint RB and power matching with SINR floors
    def _joint_assignment_kernel(self):
        return self._kernel('_joint', joint_assignment, joint_assignment.JointAssignment,
                            lambda: (self._agent_links(), self._due_links(), *self._class_bounds()))

    def joint_assignment_weights(self, movable=None, allowed=None, min_sinr_db=None, out=None):
        """What every movable link is worth on every RB at its BEST admissible power, with the background as the last step left
        it: (weights float32 [B, M, R], power_dbm int32 [B, M, R], links int32 [M]).

        movable, allowed, the background and the rows as assignment_weights() has them, except that a movable link's current power
        plays no part either: every level p of its class (power_control()'s bounds, the ones step() decodes) is tried.
        w(a, r, p) = own - harm as assignment_weights(objective='total') defines them at power p - bit for bit that call's weight
        with the link's power set to p.  min_sinr_db: a number, {'cue': x, 'due': y} or [N] values (array or tensor), dB, -inf: no
        floor for that link; None: no floors.  (a, r, p) is admissible iff link a's SINR there is >= its floor and no background
        member of r that meets its floor without link a falls below it with link a present; a member the background alone already
        holds under its floor constrains nothing.  weights[b, a, r] is the largest w over the admissible p - equal values to the
        lowest power - and power_dbm[b, a, r] that p; -inf and -32768 where allowed forbids or no p is admissible.

        Under a one-to-one placement a background link sees at most one movable link, so the capacity it loses and whether it keeps
        its floor depend on that link's RB and power alone: total = evaluate(background) + the sum of w(a, r_a, p_a) for every
        one-to-one placement and every choice of powers, and the floors hold iff every (a, r_a, p_a) is admissible.

        One kernel launch (csrc/d2d_assignpwr.hip): sorts, background sums and pair gains are shared across the levels.  The env is
        left untouched.  Valid after reset() and after every step(), autoreset and mobility included.  Torch path only: enqueued on
        torch's current stream, nothing is synchronised; the two tensors the env owns (4 B M R bytes each, rewritten by every call),
        or `out` = (weights, power_dbm).  Refusals as assignment_weights(), under the name assign_rbs_power()."""
        k = self._joint_assignment_kernel()
        floors = k.floors(min_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.power_weights(self._t, movable, allowed, floors, out, self._stream_ptr)

    def assign_rbs_power(self, movable=None, allowed=None, min_sinr_db=None, out=None):
        """The one-to-one placement of the movable links AND the power of each that maximise the total capacity of the env subject
        to the SINR floors, the background staying where it is: (rb int32 [B, N], power_dbm int32 [B, N], value_mbps float32 [B],
        feasible uint8 [B]), a tuple with those names.

        rb / power_dbm are the current planes with every movable link on its matched RB, all distinct, at the best admissible power
        of that entry.  evaluate(rb, power_dbm)['total_mbps'] = evaluate(background) + value_mbps, every constrained link keeps
        min_sinr_db, and no other (one-to-one placement, powers) that keeps the floors gives more (joint_assignment_weights()): the
        Hungarian optimum of max over p of w[a, r, p] is the joint optimum.  An env in which the floors or `allowed` leave some
        movable link no RB of its own is infeasible: it keeps its rb and power rows, with value 0.0 and feasible 0.  The joint
        launch, then solve_assignment(), then the gather of the matched powers and the two scatters.  More movable links than RBs
        is a ValueError.  `out` = (rb, power_dbm, value_mbps, feasible)."""
        k = self._joint_assignment_kernel()
        floors = k.floors(min_sinr_db, self.num_cues)
        self._follow_torch_stream()
        return k.assign_power(self._t, movable, allowed, floors, out, self._stream_ptr)

    def assign_rbs_power_actions(self, movable=None, allowed=None, min_sinr_db=None):
        """assign_rbs_power() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its RB at its power
        of assign_rbs_power(), encoded rb * power levels + level (power_control.encode_actions).  Links on fixed actions
        (cue_actions='traffic') have no column."""
        res = self.assign_rbs_power(movable, allowed, min_sinr_db)
        first, p_min, levels = self._agent_power_levels()
        return power_control.encode_actions(res.rb, res.power_dbm, p_min, levels, first)

    # ------------------------------------------------------------------ conflict-graph RB colouring
    def _color_kernel(self):
        return self._kernel('_color', coloring, coloring.Coloring, lambda: (self._agent_links(),))

    def color_graph(self, score, rx_thr, tx_bias=None, movable=None, allowed=None, pack: bool = False, out=None):
        """DSATUR colouring of a conflict graph with the RBs, several compatible links per RB: (rb int32 [B, N], conflicts int32 [B],
        rbs_used int32 [B], proper uint8 [B]), a tuple with those names.

        score: ANY contiguous float32 [B, N, N] tensor on the env's device, receiver-major as coupling() is (i receives, j
        transmits); rx_thr float32 [B, N]; tx_bias float32 [B, N] or None (0).  Link j conflicts with link i iff i != j and
        score[b, i, j] + tx_bias[b, j] >= rx_thr[b, i] - one float32 addition, a NaN on either side compares false, rx_thr +inf: never
        a victim - and {i, j} is an edge iff either direction conflicts.  A link takes a turn iff it is movable and has an allowed RB;
        every other link is background: it keeps its RB (as the decoded plane holds it) and is coloured from the start.  Turn after
        turn the uncoloured link with the most distinct RBs among its coloured neighbours (then the most neighbours, then the lowest
        index) takes the allowed RB with the fewest coloured neighbours on it, then - pack=False - the fewest links on it, then the
        lowest; pack=True leaves the load out: the lowest free RB, the classic minimum-colour greedy.  With no free RB the rule
        degrades to the least-conflicting one.  conflicts counts the same-RB edges with an end that took a turn, rbs_used the distinct
        RBs those links hold, proper is conflicts == 0.  A heuristic: nothing is claimed beyond those counts.

        movable: bool [N], the links that take turns; None: every agent link (links on cue_actions='traffic' never move).  allowed:
        bool [N, R] as best_rb() takes it; None: every RB.  All turns of an env run in one workgroup of one kernel launch
        (csrc/d2d_color.hip) out of LDS, in integers: two calls give the same words.  The env is left untouched.

        Torch path only: enqueued on torch's current stream, nothing is synchronised; the four tensors the env owns, rewritten by
        every call (clone them to keep them), or `out` = (rb, conflicts, rbs_used, proper), contiguous int32 [B, N], int32 / int32 /
        uint8 [B] on the env's device.  Refused as color_rbs() is."""
        k = self._color_kernel()
        mov = k.movable(movable)
        self._follow_torch_stream()
        return k.color(self._t['rb'], score, rx_thr, tx_bias, mov, allowed, pack, out, self._stream_ptr)

    def color_rbs(self, margin_db, movable=None, allowed=None, power_dbm=None, pack: bool = False, out=None):
        """The interference-graph colouring baseline: color_graph() on the SIR conflict graph of the current positions and powers.

        Link j conflicts with link i iff j alone, at its power, would hold i's signal-to-interference ratio under margin_db[i]:
        coupling()[b, i, j] + p[b, j] >= (coupling()[b, i, i] + p[b, i]) - margin_db[i], every operation in float32 in that
        association (the receiver gains are on both sides, which is why coupling() fits although it carries none).  p is the
        decoded power plane, or power_dbm (int32 [B, N] on the env's device) - power_control()'s powers, say.  margin_db: a number,
        {'cue': x, 'due': y} or [N] values (array or tensor), dB; -inf: that link is never a victim; NaN is a ValueError - which a
        margin_db TENSOR is read on the host for: that form waits for what is queued before it, every other one is enqueue-only.

        When proper is 1 every same-RB pair with an end that took a turn keeps those PAIRWISE margins.  Nothing is said about the
        aggregate SINR of several co-channel links, and there is no optimality certificate as assign_rbs() has one; several links
        may share an RB, so more movable links than RBs is no error here.  movable, allowed, pack, out and the result as
        color_graph() has them.  Two kernel launches, coupling() - whose env-owned tensor is rewritten - and the colouring, and three
        elementwise torch operations.  Valid after reset() and after every step(), autoreset and mobility included, as coupling()
        is.  Torch path only; ValueError for what coupling() refuses: export_actions=False, ShadowingPathLoss, every table route,
        pinned device_config coordinates float32 cannot hold."""
        k = self._color_kernel()
        margin, mov = k.margin(margin_db, self.num_cues), k.movable(movable)
        if power_dbm is None:
            power_dbm = self._t['pwr']
        elif not torch.is_tensor(power_dbm) or tuple(power_dbm.shape) != (self.num_envs, self.num_links) or power_dbm.dtype != torch.int32 \
                or power_dbm.device != self.device:
            raise ValueError(f'power_dbm must be an int32 tensor [{self.num_envs}, {self.num_links}] on {self.device} or None')
        c = self.coupling()
        p = power_dbm.to(torch.float32).contiguous()
        thr = coloring.sir_threshold(c, p, margin).contiguous()
        return k.color(self._t['rb'], c, thr, p, mov, allowed, pack, out, self._stream_ptr)

    def color_rbs_actions(self, margin_db, movable=None, allowed=None, power_dbm=None, pack: bool = False):
        """color_rbs() as an action tensor, int32 [B, num_agents], ready for step(): every agent link on its RB of color_rbs() at its
        current power level (as the decoded planes hold it), encoded rb * power levels + level.  Links on fixed actions
        (cue_actions='traffic') have no column.  Composes with power_control_actions() the way best_response_dynamics_actions()
        does: one call picks RBs, the other picks powers."""
        rb = self.color_rbs(margin_db, movable, allowed, power_dbm, pack)[0]
        return best_response_dynamics.encode_actions(rb, self._t['pwr'], self._agent_levels(), self.num_links - self.num_agents)

    def _observe(self, view):
        extra = {}
        if self._senses:
            extra['rb_sinr_db'] = self.sense('sinr_db')
        if self._neighbors_k:
            idx, cdb = self._neighbors
            extra.update(neighbor_idx=idx, neighbor_coupling_db=cdb)
            if getattr(self.obs_fn, 'native_neighbor_obs', False):
                g, k = self._graph, self._neighbors_k
                extra['neighbor_obs'] = g.obs_torch(self._t, k, idx, cdb, self._stream_ptr) if self.use_torch else g.obs_numpy(k)
        if extra:
            # a namespace of its own: the cached view stays what every other consumer sees
            view = SimpleNamespace(**vars(view), **extra)
        obs = self.obs_fn.compute(view) if self._array_obs else view.obs
        if self._obs64 and not self._native_obs64 and not isinstance(obs, tuple):   # the reference's dtype (obs_fn.py:51) for a custom array obs: cast here
            obs = obs.double() if self.use_torch else np.asarray(obs, dtype=np.float64)
        return obs

    def path_loss_db(self):
        """The live path-loss table of SpatialChannelPathLoss as the last step read it: [B, N + 1, N] dB, pl_db[b, j, i] from the
        transmitter of link j to the receiver of link i, row N the links' own paths (the diagonal); the model's table_dtype.  The
        route's own tensor, rewritten before every step (clone it to keep it).  ValueError for every other model."""
        if not self._channel:
            raise ValueError('path_loss_db() needs path_loss_model=SpatialChannelPathLoss: no other model keeps a table of every pair')
        return self.simulator.path_loss_table.live

    def link_positions(self):
        """[B, N, 4] float32 (tx_x, tx_y, rx_x, rx_y) of every link = columns 0-3 of the obs table (obs_fn.py:57-59), constant
        between resets (with mobility=: of the last move - call it after the step to bring the rows up to date).  torch path: a
        zero-copy view of the library's own rows (D2D_BUF_LINK_POS) - read-only, valid until close(), refreshed by the library on
        reset."""
        h = self.simulator.handle
        if not self.use_torch:
            return h.download(_native.BUF_LINK_POS)
        ptr, nbytes = h.get_buffer(_native.BUF_LINK_POS)           # also brings the rows up to date on the current stream
        if getattr(self, '_lpos_view', None) is None or self._lpos_view[0] != (ptr, nbytes):
            shape = (self.num_envs, self.num_links, 4)
            holder = SimpleNamespace(__cuda_array_interface__={'shape': shape, 'typestr': '<f4', 'data': (ptr, False), 'version': 2,
                                                              'strides': None})
            self._lpos_view = ((ptr, nbytes), torch.as_tensor(holder, device=self.device))
        return self._lpos_view[1]

    def action_buffer(self):
        """The bound int32 [B, num_agents] action tensor (step() with no copy also accepts any contiguous int32 CUDA
        tensor of that shape)."""
        return self._t.get('actions')

    def status_flags(self) -> int:
        return self.simulator.handle.status_flags()

    def close(self) -> None:
        if self._sensor is not None:
            self._sensor.close()
            self._sensor = None
        if self._graph is not None:
            self._graph.close()
            self._graph = None
        if self._marginal is not None:
            self._marginal.close()
            self._marginal = None
        if self._bestrb is not None:
            self._bestrb.close()
            self._bestrb = None
        if self._powerctl is not None:
            self._powerctl.close()
            self._powerctl = None
        if self._brdyn is not None:
            self._brdyn.close()
            self._brdyn = None
        if self._evaluate is not None:
            self._evaluate.close()
            self._evaluate = None
        if self._table_evaluate is not None:
            self._table_evaluate.close()
            self._table_evaluate = None
        if self._table_rbascent is not None:
            self._table_rbascent.close()
            self._table_rbascent = None
        if self._table_marginal is not None:
            self._table_marginal.close()
            self._table_marginal = None
        if self._assign is not None:
            self._assign.close()
            self._assign = None
        if self._joint is not None:
            self._joint.close()
            self._joint = None
        if self._color is not None:
            self._color.close()
            self._color = None
        if self._balance is not None:
            self._balance.close()
            self._balance = None
        if self._stable is not None:
            self._stable.close()
            self._stable = None
        if self._share is not None:
            self._share.close()
            self._share = None
        if self._ascent is not None:
            self._ascent.close()
            self._ascent = None
        if self._rbascent is not None:
            self._rbascent.close()
            self._rbascent = None
        if self._goodput is not None:
            self._goodput.close()
            self._goodput = None
        if self._deviation is not None:
            self._deviation.close()
            self._deviation = None
        self.simulator.handle.close()
