"""How a PathLoss reaches the kernels: one route per model, chosen when the simulator is built.

    native        power_law_columns: the kernels evaluate the law (d2d_set_path_loss_power_law / _shadowing)
    device_table  one env, per-object: [D, D] of the pairs the links read, topped up per link list (d2d_set_path_loss_table)
    link_table    a batch, per-object (an ArrayPathLoss too, without a GPU): [B, N, N] by (tx link, rx link), on the host
    array         a batch, an ArrayPathLoss: compute(view) on the GPU once per reset, [B, N, N] from device memory
                  (d2d_set_path_loss_link_table_dev), or a live [B, N+1, N] table when compute returns the SNR row
    per_step      ArrayPathLoss.per_step: compute(view) before every step into a live [B, N+1, N] table the step kernel reads
    channel       SpatialChannelPathLoss: libd2d_channel.so fills a live [B, N+1, N] table (float64, or float32 on request) before every step, at the clock
                  (episode, step in the episode) VecD2DEnv hands over
"""
from __future__ import annotations

import random
from contextlib import contextmanager
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _native
from .path_loss import ArrayPathLoss, PathLoss, PathLossView, SpatialChannelPathLoss, warn_if_stochastic
from .position import Position

NATIVE, DEVICE_TABLE, LINK_TABLE, ARRAY, PER_STEP, CHANNEL = 'native', 'device_table', 'link_table', 'array', 'per_step', 'channel'
PL_CHUNK_BYTES = 1 << 30            # ArrayPathLoss.env_chunk = None: envs per compute() call keep one [b,N,N] float64 within this


def _torch_cuda():
    """torch with a GPU, or a clear error: a per-step ArrayPathLoss has no host route to fall back to."""
    try:
        import torch
    except Exception as e:      # pragma: no cover - torch is part of the platform
        raise RuntimeError('ArrayPathLoss.per_step = True needs PyTorch with a GPU: its model is evaluated on the device before '
                           'every step (there is no frozen-table fallback)') from e
    if not torch.cuda.is_available():
        raise RuntimeError('ArrayPathLoss.per_step = True needs PyTorch with a GPU (torch.cuda.is_available() is False): its model '
                           'is evaluated on the device before every step (there is no frozen-table fallback)')
    return torch


def _write_live(torch, live, b0: int, b1: int, pl, snr) -> None:
    """Envs [b0, b1) of compute()'s result into the live [B, N+1, N] float64 table (row N: the SNR's row, else pl's diagonal)."""
    live[b0:b1, :-1].copy_(pl)
    live[b0:b1, -1].copy_(snr if snr is not None else torch.diagonal(pl, dim1=1, dim2=2))


def positions_move_unserved(sim, use_torch: bool):
    """What about this env positions that change on the device inside step() cannot serve, as (kind, detail), or None: 'numpy' (the
    bookkeeping lives in device tensors), 'route' (detail: the route's name - a table evaluated once per reset), 'pinned' (pinned
    device_config coordinates float32 cannot hold).  The one predicate behind autoreset's and mobility's refusals, each with texts of
    its own."""
    if not use_torch:
        return 'numpy', ''
    route = sim.path_loss_table.route
    if route not in (NATIVE, PER_STEP, CHANNEL):
        return 'route', route
    mask, xy = sim.fixed_positions()
    if mask.any() and (xy != xy.astype(np.float32)).any():
        return 'pinned', ''
    return None


class PathLossTable:
    def __init__(self, handle, model: PathLoss, devices, config) -> None:
        self.handle, self.model, self.devices = handle, model, devices      # devices: the Device objects in handle order
        self.num_envs, self.device_ordinal, self.config_seed = int(config.num_envs), config.device_ordinal, config.seed
        self.channel = None                         # channel: the route's device-side state (ChannelFill)
        spatial = isinstance(model, SpatialChannelPathLoss)
        # channel: the law is the MEDIAN's (ValueError: a median without columns, or a stochastic one)
        self.law = model.median_columns(devices) if spatial else model.power_law_columns(devices)
        if spatial:
            if len(devices) >= 65536:
                raise ValueError('SpatialChannelPathLoss: the env must have fewer than 65536 devices (the fading counter holds two '
                                 'device indices in one word)')
            self.route = CHANNEL
            self.channel = ChannelFill(self, model)
        elif self.law is not None:
            self.route = NATIVE
        elif isinstance(model, ArrayPathLoss) and model.per_step:
            _torch_cuda()
            self.route = PER_STEP
        else:                                       # one env: an ArrayPathLoss too, through its derived __call__
            self.route = DEVICE_TABLE if self.num_envs == 1 else ARRAY if isinstance(model, ArrayPathLoss) else LINK_TABLE
        self.check_stochastic = self.route in (DEVICE_TABLE, LINK_TABLE) and not isinstance(model, ArrayPathLoss)
        self.shadowing_seed = self.seed = None      # seed: PathLossView.seed of an ArrayPathLoss
        self.step = 0                               # steps enqueued since the model was installed (PathLossView.step)
        self.stream: Optional[int] = None           # the handle's stream when a caller put it on torch's (Simulator.set_stream)
        self.link_tx = self.link_rx = np.zeros(0, dtype=np.int32)
        self.positions_known, self.positions = False, None   # positions: [B, D, 2] float64 as last given, else None
        self.covered = (set(), set())               # device_table: the transmitters and receivers the bound table holds
        self.cols = self.live = None                # per_step: per-link coordinates; the live table, held while steps may read it
        self.live_bound = False                     # per_step: self.live is bound for the current link list
        # per_step: positions may move on the device between steps (VecD2DEnv(autoreset=True) resets envs inside step()): the
        # per-link coordinates are gathered from POS_X / POS_Y again before every step
        self.device_resets = False
        # per_step: what compute(view) would otherwise upload before every step - a synchronous copy each - is uploaded once per
        # link list: the link index tensors of _link_coordinates and the view's per-device columns (PathLossView._column)
        self.link_index = None
        self.columns = {}

    def install(self) -> None:
        """Hand the native route's law to the handle and draw the seeds (again: restarts the built-in shadowing's stream)."""
        law = self.law
        if self.route == CHANNEL:
            return                                  # the law is the fill kernel's; the keys derive from the env's seed per fill
        if law is not None and law.get('shadowing'):
            self.shadowing_seed = self.config_seed if self.config_seed is not None else random.getrandbits(63)
            self.handle.set_path_loss_shadowing(law['a_tx_db'], law['a_rx_db'], law['exponent'], law['shadowing']['d0_m'],
                                                law['shadowing']['chi_dB'], self.shadowing_seed)
        elif law is not None:
            self.handle.set_path_loss_power_law(law['a_tx_db'], law['a_rx_db'], law['exponent'])
        elif isinstance(self.model, ArrayPathLoss):
            # a per-step model follows the rule ShadowingPathLoss's seed follows above (same seed, same draws); a once-per-reset
            # model takes its unseeded default from the OS, leaving Python's random stream - the single env's layout - as it was
            draw = random.getrandbits if self.route == PER_STEP else random.SystemRandom().getrandbits
            self.seed = self.config_seed if self.config_seed is not None else draw(63)

    # ------------------------------------------------------------------ what the simulator reports
    def positions_changed(self, positions: Optional[np.ndarray] = None) -> None:
        """positions [B, D, 2] as the handle was given them, or None: the Device objects' (one env) or the handle's (a batch)."""
        if self.route == NATIVE:
            return
        if self.route == CHANNEL:
            self.channel.moved = True               # the fill reads POS_X / POS_Y where they are
            return
        self.positions_known, self.covered, self.cols = True, (set(), set()), None
        # a COPY: the caller may reuse its array before a later set_links re-evaluates the table from it
        self.positions = None if positions is None else np.array(positions, dtype=np.float64, copy=True)
        self._evaluate()

    def links_changed(self, link_tx: np.ndarray, link_rx: np.ndarray) -> None:
        self.link_tx, self.link_rx = link_tx, link_rx
        self.cols, self.live_bound = None, False    # d2d_set_links drops a table bound for the old list
        self.link_index, self.columns = None, {}
        if self.channel is not None:
            self.channel.links = None
        if self.positions_known:
            self._evaluate()                        # pairs the new link list reads that the table does not hold yet

    def before_step(self) -> None:
        """per_step: evaluate the model for the step about to be enqueued (view.step = the step's counter) into the live table
        the step kernel reads.  Ordered with the step: on the handle's stream when that is torch's current one (VecD2DEnv), else
        by synchronising both sides.  channel: libd2d_channel.so's fill for that step, on the handle's stream."""
        if self.route == CHANNEL:
            if len(self.link_tx):
                self.channel.fill()
            return
        if self.route == PER_STEP and len(self.link_tx):
            torch = _torch_cuda()
            dev, n = torch.device('cuda', self.device_ordinal), len(self.link_tx)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev)
                same = self.stream is not None and self.stream == stream.cuda_stream
                if self.cols is None or self.device_resets:
                    self.cols = self._link_coordinates(torch, dev, sync=not same)
                if not same and self.live is not None:
                    self.handle.synchronize()       # the last step still reads the table this evaluation overwrites
                if not self.live_bound:
                    self.live = torch.empty((self.num_envs, n + 1, n), dtype=torch.float64, device=dev)
                for b0, b1, pl, snr in self._compute(torch, self.cols):
                    _write_live(torch, self.live, b0, b1, pl, snr)
                if not (same and self.live_bound):
                    stream.synchronize()            # binding does not order, and the step may run on another stream
                if not self.live_bound:
                    self.handle.set_path_loss_link_table_dev(self.live.data_ptr(), _native.F64, n, _native.PL_TABLE_LIVE)
                    self.live_bound = True
        if self.seed is not None:
            self.step += 1                          # also the counter a once-per-reset ArrayPathLoss sees at its next evaluation

    def set_channel_clock(self, env_seed: int, episode: int = 0, step: int = 0, per_env: Optional[dict] = None) -> None:
        """channel: where the step about to be enqueued stands - lockstep (episode, step in the episode; 0 is the reset's own
        step), or per_env: VecD2DEnv's tensors 'episode', 'elapsed', 'pending' of an autoreset step.  A no-op for other routes."""
        if self.channel is not None:
            self.channel.clock = (int(env_seed), int(episode), int(step), per_env)

    # ------------------------------------------------------------------ the routes
    def _evaluate(self) -> None:
        if self.route == PER_STEP or not len(self.link_tx):
            return                                  # per_step: before the next step; no links, no pairs: the next list has them
        if self.route == ARRAY:
            try:
                torch = _torch_cuda()
            except RuntimeError:
                self.route = LINK_TABLE             # no GPU for compute(view): its per-object call on the host
            else:
                return self._evaluate_array(torch)
        txs, rxs = set(self.link_tx.tolist()), set(self.link_rx.tolist())
        # one env: the Device objects stand at the positions; a batch: as given, else as the handle holds them (float32)
        positions = None if self.route == DEVICE_TABLE else self.positions if self.positions is not None else \
            np.stack([self.handle.download(_native.BUF_POS_X), self.handle.download(_native.BUF_POS_Y)], axis=-1)
        if self.check_stochastic:
            # a per-object model is frozen into its table until the next reset: say so, once, if it draws per call
            self.check_stochastic = False
            with self._devices_at(None if positions is None else positions[0]):
                warn_if_stochastic(self.model, self.devices[int(self.link_tx[0])], self.devices[int(self.link_rx[0])])
        if self.route == DEVICE_TABLE:
            # a [D,D] DEVICE table survives the link list changing from step to step (D2DEnv steps whatever subset of links the
            # action dict names); same positions + a changed list: only the pairs not yet there are evaluated
            if not (txs <= self.covered[0] and rxs <= self.covered[1]):
                txs, rxs = txs | self.covered[0], rxs | self.covered[1]
                self.handle.set_path_loss_table(self.model.table_db(self.devices, txs, rxs))
                self.covered = (txs, rxs)
            return
        # a batch: [B,N,N] by (tx LINK, rx LINK) - exactly the pairs the step reads (d2d_set_path_loss_link_table), not the
        # dense [B,D,D] device cube (9.7 GB at 4096 x 769 devices).  Tied to the link list: re-evaluated when it changes.
        tables = np.empty((self.num_envs, len(self.link_tx), len(self.link_tx)), dtype=np.float64)
        for b in range(self.num_envs):
            with self._devices_at(positions[b]):
                tables[b] = self.model.table_db(self.devices, txs, rxs)[np.ix_(self.link_tx, self.link_rx)]
        self.handle.set_path_loss_link_table(tables)

    @contextmanager
    def _devices_at(self, xy):
        """The Device objects at one env's positions xy [D, 2] (None: where they are) for the block, then back where they were."""
        saved = [d.position for d in self.devices]
        try:
            for d, p in zip(self.devices, () if xy is None else xy):
                d.set_position(Position(float(p[0]), float(p[1])))
            yield
        finally:
            for d, p in zip(self.devices, saved):
                d.set_position(p)

    def _link_coordinates(self, torch, dev, sync: bool = True):
        """(tx_x, tx_y, rx_x, rx_y) [B, N] of every link as tensors on `dev`: host-supplied positions as given (float64 possible),
        the Device objects' float64 positions for one env, else POS_X / POS_Y where the device-side reset wrote them (sync = False:
        the handle runs on torch's current stream, which orders the gather after the reset)."""
        if self.link_index is None:
            self.link_index = tuple(torch.as_tensor(j.astype(np.int64), device=dev) for j in (self.link_tx, self.link_rx))
        jt, jr = self.link_index
        if self.positions is not None:
            p = torch.as_tensor(self.positions, device=dev)
        elif self.num_envs == 1 and not self.device_resets:
            # one env: the reference's own float64 coordinates (the kernels take them as exact (hi, lo) pairs)
            p = torch.as_tensor(np.array([d.position.as_tuple() for d in self.devices], dtype=np.float64)[None], device=dev)
        else:
            def plane(which):                       # device-side reset: POS_X / POS_Y where they are, gathered per link by torch
                cai = {'shape': (self.num_envs, len(self.devices)), 'typestr': '<f4', 'version': 2, 'strides': None,
                       'data': (self.handle.get_buffer(which)[0], False)}
                return torch.as_tensor(SimpleNamespace(__cuda_array_interface__=cai), device=dev)
            px, py = plane(_native.BUF_POS_X), plane(_native.BUF_POS_Y)
            if sync or not self.device_resets:
                self.handle.synchronize()           # the sampler wrote them on the handle's stream; torch reads on its own
            return (px[:, jt], py[:, jt], px[:, jr], py[:, jr])
        return (p[:, jt, 0], p[:, jt, 1], p[:, jr, 0], p[:, jr, 1])

    def _compute(self, torch, cols):
        """ArrayPathLoss.compute on env slices [b0, b1) (ArrayPathLoss.env_chunk), each result yielded as (b0, b1, pl, snr) as it
        comes: no chunk's [b,N,N] float64 temporaries exceed about PL_CHUNK_BYTES, whatever B."""
        n = len(self.link_tx)
        chunk = int(self.model.env_chunk) if self.model.env_chunk else max(1, PL_CHUNK_BYTES // max(1, n * n * 8))
        if chunk < 1:
            raise ValueError('ArrayPathLoss.env_chunk must be a positive int or None')
        txd, rxd = [self.devices[i] for i in self.link_tx], [self.devices[i] for i in self.link_rx]
        for b0 in range(0, self.num_envs, chunk):
            b1 = min(self.num_envs, b0 + chunk)
            part = cols if (b0, b1) == (0, self.num_envs) else tuple(c[b0:b1] for c in cols)
            res = self.model.compute(PathLossView(torch, *part, txd, rxd, like=cols[0], step=self.step,
                                                  first_env=self.handle.env_offset + b0, seed=self.seed,
                                                  columns=self.columns))
            pl, snr = res if isinstance(res, tuple) else (res, None)
            if tuple(pl.shape) != (b1 - b0, n, n):
                raise ValueError(f'ArrayPathLoss.compute must return [{b1 - b0},{n},{n}], got {tuple(pl.shape)}')
            if snr is not None and tuple(snr.shape) != (b1 - b0, n):
                raise ValueError(f'ArrayPathLoss.compute\'s SNR path loss must be [{b1 - b0},{n}], got {tuple(snr.shape)}')
            yield b0, b1, pl, snr

    def _evaluate_array(self, torch) -> None:
        """compute(view) on the GPU into one [B,N,N] dB table the handle converts from device memory; from the first chunk that
        returns the SNR's own evaluation on, a live [B,N+1,N] table instead (the chunks before it converted to that layout)."""
        dev, n = torch.device('cuda', self.device_ordinal), len(self.link_tx)
        live = table = None
        with torch.cuda.device(dev):
            for b0, b1, pl, snr in self._compute(torch, self._link_coordinates(torch, dev)):
                if snr is not None and live is None:
                    live = torch.empty((self.num_envs, n + 1, n), dtype=torch.float64, device=dev)
                    if table is not None:
                        _write_live(torch, live, 0, b0, table[:b0], None)
                        table = None
                if live is not None:
                    _write_live(torch, live, b0, b1, pl, snr)
                    continue
                dtype = pl.dtype if pl.dtype in (torch.float32, torch.float64) else torch.float64
                if (b0, b1) == (0, self.num_envs):
                    table = pl.to(dtype).contiguous()
                    continue
                if table is None:
                    table = torch.empty((self.num_envs, n, n), dtype=dtype, device=dev)
                table[b0:b1].copy_(pl)
            torch.cuda.current_stream(dev).synchronize()     # the conversion kernel runs on the handle's stream
            self.live = live                                 # held until the next evaluation
            out = live if live is not None else table
            self.handle.set_path_loss_link_table_dev(out.data_ptr(), _native.F64 if out.dtype == torch.float64 else _native.F32, n,
                                                     _native.PL_TABLE_LIVE if live is not None else True)


class ChannelFill:
    """The 'channel' route's device side: the live table (the model's table_dtype), the phase work space, the link lists and law columns as device
    tensors (allocated once per link list), and one d2d_channel_fill per step on the handle's stream.  With fading=None the table
    depends on the positions and the episode only: a fill is skipped when nothing moved since the last one (no mobility=, no
    device-side reset that step)."""

    def __init__(self, table: PathLossTable, model: SpatialChannelPathLoss) -> None:
        self.table, self.model, self.consts = table, model, model.constants()
        self.clock = None                           # (env seed, episode, step, per-env tensors or None): set_channel_clock
        self.links = None                           # (link_tx, link_rx) int32 device tensors of the current list
        self.cols = self.scratch = self.start = None
        self.moved = True
        self.fills = 0

    def start_episode(self, elapsed) -> None:
        """Autoreset: what `elapsed` is at reset() - the per-env clock's origin, as Mobility.start."""
        if self.start is None:
            self.start = elapsed.clone()
        else:
            self.start.copy_(elapsed)

    def fill(self) -> None:
        t = self.table
        if self.clock is None:
            raise ValueError('SpatialChannelPathLoss needs an episode clock (episode, step in the episode), which only VecD2DEnv '
                             'keeps: Simulator.step / step_arrays and the single-env D2DEnv cannot drive it')
        env_seed, episode, step, per_env = self.clock
        m, amp, wave_scale, fading, mu, s = self.consts
        if self.links is not None and per_env is None and not self.moved and fading == _native.CHANNEL_FADING_NONE:
            return                                  # same positions, same episode, no per-step draw: the table is still right
        torch = _torch_cuda()
        h, n, d = t.handle, len(t.link_tx), len(t.devices)
        dev = torch.device('cuda', t.device_ordinal)
        stream = t.stream if t.stream is not None else 0
        with torch.cuda.device(dev):
            if t.stream is None:
                raise ValueError("SpatialChannelPathLoss: the handle must run on torch's current stream (VecD2DEnv puts it there)")
            if self.cols is None:
                self.cols = tuple(torch.as_tensor(np.ascontiguousarray(t.law[k], dtype=np.float64), device=dev)
                                  for k in ('a_tx_db', 'a_rx_db', 'exponent'))
            if self.links is None:
                self.links = tuple(torch.as_tensor(np.ascontiguousarray(j, dtype=np.int32), device=dev) for j in (t.link_tx, t.link_rx))
                f64 = self.model.table_dtype == 'float64'
                t.live = torch.empty((t.num_envs, n + 1, n), dtype=torch.float64 if f64 else torch.float32, device=dev)
                self.scratch = torch.empty((t.num_envs, n, m, 4), dtype=torch.float32, device=dev) if m else None
                self.dtype = _native.F64 if f64 else _native.F32
                h.set_path_loss_link_table_dev(t.live.data_ptr(), self.dtype, n, _native.PL_TABLE_LIVE)
                t.live_bound = True
            shadow_seed, fading_seed = self.model.stream_seeds(env_seed)
            clock = dict(step=step, episode=episode)
            if per_env is not None:
                if self.start is None:
                    self.start = torch.zeros(t.num_envs, dtype=torch.int32, device=dev)
                clock = dict(elapsed_ptr=per_env['elapsed'].data_ptr(), start_ptr=self.start.data_ptr(),
                             episode_ptr=per_env['episode'].data_ptr(), reset_ptr=per_env['pending'].data_ptr())
            _native.channel_fill(h.get_buffer(_native.BUF_POS_X)[0], h.get_buffer(_native.BUF_POS_Y)[0], self.links[0].data_ptr(),
                                 self.links[1].data_ptr(), *(c.data_ptr() for c in self.cols), t.num_envs, d, n, h.env_offset, m, amp,
                                 wave_scale, fading, mu, s, shadow_seed, fading_seed,
                                 0 if self.scratch is None else self.scratch.data_ptr(), t.live.data_ptr(), self.dtype, stream_ptr=stream,
                                 **clock)
        self.moved = False
        self.fills += 1
